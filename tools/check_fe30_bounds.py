#!/usr/bin/env python3
"""Worst-case column sums of fe30.hip.h:f30_mul / f30_sqr for every modulus the engine uses: all must stay below 2^64.
Operand limbs 0..7 <= 2^30 - 1, limb 8 <= TOP - 1 (value < 2^258 -> TOP = 2^18); m_i <= 2^30 - 1; the modulus limbs are exact."""
MODULI = {
    "bn254_p": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
    "bn254_r": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "p_icc": 207 * 2**248 + 1,
}
# the ICC kernel of icc30.hip.h multiplies an UNREDUCED butterfly output (< 2^263: limb 8 < 2^23) by a twiddle (a product's result,
# in the table below p + 2^242; as an operand anything with limb 8 < 2^17, i.e. < 2^257) modulo p_icc, the BN254 group order and the
# secp256k1 group order.  The numbers of check_icc_chain are the ones tests/icc_vectors.py feeds.
ICC_MODULI = {
    "p_icc": 207 * 2**248 + 1,
    "bn254_r": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "secp256k1_n": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141,
}
MASK = 2**30 - 1
def check(name, p, top_bits=18, top_bits_b=None):
    P = [(p >> (30 * i)) & MASK for i in range(9)]
    amax = [MASK] * 8 + [2**top_bits - 1]
    bmax = [MASK] * 8 + [2**(top_bits_b or top_bits) - 1]
    carry = 0
    worst = 0
    for k in range(17):
        t = carry
        for i in range(9):
            j = k - i
            if 0 <= j <= 8:
                t += amax[i] * bmax[j]
                if not (k < 9 and i == k):
                    pass
        # reduction products m_i * P_{k-i}, i <= min(k, 8); for k < 9 this includes m_k * P_0
        for i in range(9):
            j = k - i
            if 0 <= j <= 8:
                t += MASK * P[j]
        worst = max(worst, t)
        carry = t >> 30
    ok = worst < 2**64
    print("%-8s worst column %.4f x 2^64  %s" % (name, worst / 2**64, "ok" if ok else "OVERFLOW"))
    return ok
MUL2_CHAIN = (6, 8)     # = tools/gen_fe30_asm.py:MUL2_CHAIN = fe30.hip.h:F30_MUL2_CHAIN_LO / _HI
def check_mul2(name, p, top_bits=18, chain=MUL2_CHAIN):
    """f30_mul2: t = a b + reduction (+ c d outside the chained columns, + one 30-bit digit of u inside them, + u's carry after them);
    u = the products of c d in the chained columns with its own carries"""
    k0, k1 = chain
    P = [(p >> (30 * i)) & MASK for i in range(9)]
    amax = [MASK] * 8 + [2**top_bits - 1]
    ct = cu = 0
    worst_t = worst_u = 0
    for k in range(17):
        ab = sum(amax[i] * amax[k - i] for i in range(9) if 0 <= k - i <= 8)
        mp = sum(MASK * P[k - i] for i in range(9) if 0 <= k - i <= 8)
        if k0 <= k <= k1:
            u = cu + ab
            worst_u, cu = max(worst_u, u), u >> 30
            t = ct + MASK + ab + mp
        else:
            t = ct + 2 * ab + mp + (cu if k == k1 + 1 else 0)
        worst_t, ct = max(worst_t, t), t >> 30
    ok = worst_t < 2**64 and worst_u < 2**64
    print("%-8s mul2: worst t column %.4f x 2^64, worst u column %.4f x 2^64  %s" % (name, worst_t / 2**64, worst_u / 2**64, "ok" if ok else "OVERFLOW"))
    return ok
PM_MUL2_CHAIN = 7        # = tools/gen_fe30_asm.py:PM_MUL2_CHAIN = fe30.hip.h:F30_PM_MUL2_CHAIN
def check_pm_mul2(top_bits=19, chain=PM_MUL2_CHAIN):
    """f30_mul2_pm (special-form modulus, no reduction terms in the columns): both products' terms in t, except the chained column,
    whose c d terms run in u; then the fold of a double-width value < 2^519: R[9] < 2^26"""
    amax = [MASK] * 8 + [2**top_bits - 1]
    ct = cu = 0
    worst = 0
    for k in range(17):
        ab = sum(amax[i] * amax[k - i] for i in range(9) if 0 <= k - i <= 8)
        if k == chain:
            cu = ab >> 30
            t = ct + ab + MASK
        else:
            t = ct + 2 * ab + (cu if k == chain + 1 else 0)
        worst, ct = max(worst, t), t >> 30
    unchained = max(2 * sum(amax[i] * amax[k - i] for i in range(9) if 0 <= k - i <= 8) for k in range(17)) + 2**35
    # the fold: hi = bits 270.. of the sum (< 2^519 / 2^270), times 2^14 (2^32 + FOLD) with FOLD < 2^16
    hi_max = (2 * (2**259 - 1) ** 2) >> 270
    r9_ok = (hi_max * (2**14 * (2**32 + 2**16)) + 2**270) >> 270 < 2**26
    ok = worst < 2**64 and r9_ok
    print("special-form mul2: worst column %.6f x 2^64 (a single accumulator would reach %.10f), fold R[9] < 2^26: %s  %s"
          % (worst / 2**64, unchained / 2**64, r9_ok, "ok" if ok else "OVERFLOW"))
    return ok
SECP_P = 2**256 - 2**32 - 977


def check_value_ranges():
    """the operand ranges the group law of ec30.hip.h leans on (comments there: X <= 5p, Y <= 4p, U = 2Y <= 8p in a doubling,
    D = Q - X3 + 6p <= 7p + eps in an addition) against what a product accepts: value < 2^258 (limb 8 < 2^18) for BN254,
    < 2^259 (limb 8 < 2^19) for secp256k1; and what the lazy MEMORY form can hold (256 bits: BN254 stores X <= 5p, Y <= 4p
    unreduced, secp256k1 reduces on the way out); eps = the slack of a product's result (2^247 / 2^50)"""
    ok = True
    bn = MODULI["bn254_p"]
    for name, p, budget, eps in (("bn254_p", bn, 2**258, 2**247), ("secp256k1_p", SECP_P, 2**259, 2**50)):
        worst = max(2 * (4 * p), 7 * p + 8 * eps, 5 * p + 4 * eps)       # U = 2 Y (Y <= 4p), D, X
        good = worst < budget
        print("%-12s largest product operand of the group law %.3f x budget  %s" % (name, worst / budget, "ok" if good else "TOO LARGE"))
        ok = ok and good
    mem = 5 * bn + 2**247 < 2**256 and 4 * bn < 2**256
    print("bn254_p      lazy memory form: X <= 5p + eps and Y <= 4p fit 256 bits: %s" % ("ok" if mem else "NO"))
    return ok and mem


def check_sub_tables():
    """borrow-free subtractions a + (K p' - b) of fe30.hip.h: every limb of the K p table of f30_sub exceeds a normal limb of b
    (limbs 0..7) and the top limb exceeds b's for b <= (K - 1) p + 2^247; f30_sub_twice (a - 2 b, allowance doubled) stays
    inside 32 bits per limb, carries included.  The ICC stream uses the same tables with wider operands (icc30.hip.h:icc30_sub):
    those are checked at the call sites' own bounds (icc_sub_operands)"""
    ok = True
    for name, p in (("bn254_p", MODULI["bn254_p"]), ("secp256k1_p", SECP_P)):
        for K in (2, 3, 4, 5, 6):
            kp = K * p
            T = [(kp >> (30 * i)) & MASK for i in range(8)] + [kp >> 240]
            T[0] += 2**30
            for i in range(1, 8):
                T[i] += 2**30 - 1
            T[8] -= 1
            assert sum(t << (30 * i) for i, t in enumerate(T)) == kp
            b_top = ((K - 1) * p + 2**247) >> 240
            good = all(T[i] >= MASK for i in range(8)) and T[8] >= b_top and max(T[:8]) + MASK + 3 < 2**32
            ok = ok and good
        # f30_sub_twice<3>: X3 = MM - 2 S + 3 p of a doubling
        kp = 3 * p
        T = [(kp >> (30 * i)) & MASK for i in range(8)] + [kp >> 240]
        T2 = [T[0] + 2**31] + [t + 2**31 - 2 for t in T[1:8]] + [T[8] - 2]
        assert sum(t << (30 * i) for i, t in enumerate(T2)) == kp
        two_b_top = (2 * (p + 2**247)) >> 240
        good = all(T2[i] >= 2 * MASK for i in range(8)) and T2[8] >= two_b_top and max(T2[:8]) + MASK + 3 < 2**32          # + a normal limb of a + a carry of at most 3
        print("%-12s subtraction tables (K = 2..6, and the doubled one of f30_sub_twice<3>): %s" % (name, "ok" if ok and good else "BAD"))
        ok = ok and good
    # the ICC stream (icc30.hip.h:icc30_sub, icc30_split.hip.h:icc30_bfly_plain): the three ICC moduli, K as the call sites use it,
    # b at the largest value each call site can hand over.  a is a symbol of the stream: limb 8 < 2^23, so the limb-wise sum
    # a + (K p' - b) stays far inside 32 bits
    for name, p in ICC_MODULI.items():
        good = True
        for K, b_max in icc_sub_operands(p).items():
            kp = K * p
            T = [(kp >> (30 * i)) & MASK for i in range(8)] + [kp >> 240]
            T[0] += 2**30
            for i in range(1, 8):
                T[i] += 2**30 - 1
            T[8] -= 1
            assert sum(t << (30 * i) for i, t in enumerate(T)) == kp
            good = good and all(T[i] >= MASK for i in range(8)) and T[8] >= b_max >> 240 and max(T[:8]) + MASK + 3 < 2**32 \
                and T[8] + 2**23 < 2**32
        print("icc:%-11s subtraction tables (K = 2, 3, 4, 7 at the call sites' operand bounds): %s" % (name, "ok" if good else "BAD"))
        ok = ok and good
    return ok


# ---------------------------------------------------------------- the ICC stream's bound chain
ICC_A_BITS, ICC_W_BITS, ICC_STAGES = 263, 257, 30    # a symbol: limb 8 < 2^23; a twiddle as an operand: limb 8 < 2^17; stages without a reduction


def icc_product_top(p):
    """exclusive bound of a product a w / 2^270 (+ m p / 2^270, m < 2^270) over the whole operand domain: p + 2^250"""
    return p + (((2**ICC_A_BITS - 1) * (2**ICC_W_BITS - 1)) >> 270) + 1


def icc_load_top(p):
    """exclusive bound the comments state for a load-step product (256-bit chunk times a table twiddle below p + 2^242)"""
    return p + 2**248


def icc_sub_operands(p):
    """K -> the largest b of a - b + K p at its call site"""
    return {2: icc_product_top(p) - 1,               # icc30_bfly, icc30_mix_elem: a product; icc30_bfly_plain<2>: a load-step product
            3: 2 * p - 1,                            # raw first round, pair (0, 2): icc30_reduce_top's result
            4: 2 * icc_load_top(p) - 1,              # scaled first round, pair (0, 2): the sum of two load-step products
            7: 2**256 - 1}                           # raw first round: a 256-bit chunk


def icc_reduce_top_ok(p, bits=ICC_A_BITS):
    """icc30.hip.h:icc30_reduce_top for EVERY v < 2^bits: qh = floor(v[8] MU / 2^40) depends on limb 8 alone and is monotone in it,
    so the extremes of v - qh p sit at the first and the last limb 8 of each qh"""
    MU = 2**88 // ((p >> 192) + 1)
    top8 = 2**(bits - 240) - 1
    if MU >= 2**32:
        return False
    for qh in range(((top8 * MU) >> 40) + 1):
        lo8 = -(-(qh << 40) // MU)
        hi8 = min(-(-((qh + 1) << 40) // MU) - 1, top8)
        if lo8 <= hi8 and not ((lo8 << 240) - qh * p >= 0 and ((hi8 + 1) << 240) - 1 - qh * p < 2 * p):
            return False
    return True


def check_icc_chain(stages=ICC_STAGES):
    """the symbol bound chain of icc30_split.hip.h closes: load step -> first round -> `stages` stages in all -> limb 8 < 2^23 (the
    operand range of a product and of icc30_reduce_top) -> [0, 2 p) (icc30_canonical's range), raw and scaled, all three moduli.
    Bounds are exclusive."""
    ok = True
    for name, p in ICC_MODULI.items():
        T = icc_product_top(p)
        grow = max(T, 2 * p)                         # X[k] + t < X[k] + T;  X[k] - t + 2 p <= X[k] + 2 p
        tw = p + 2**242                              # a table twiddle: icc30_from_elem's product of two values below 2^256
        good = p + (((2**256 - 1) ** 2) >> 270) + 1 <= tw and tw <= 2**ICC_W_BITS
        good = good and p + (((2**256 - 1) * (tw - 1)) >> 270) + 1 <= icc_load_top(p)                  # the scaled load step
        for form in ("raw", "scaled"):
            if form == "raw":
                # stage 1, K = 7: (a + b, a - b + 7 p) of two chunks; stage 2: pair (0, 2) = (2^257 sum, reduced to < 2 p) with K = 3,
                # pair (1, 3) an ordinary butterfly
                s1 = 2**256 + 7 * p
                s2 = max(2**257 + 3 * p, s1 + grow)
                good = good and icc_reduce_top_ok(p, 257)
            else:
                L = icc_load_top(p)
                s1 = L + 2 * p                                                             # K = 2: (2 L, L + 2 p)
                s2 = max(4 * L, 2 * L + 4 * p, s1 + grow)                                  # K = 4 on pair (0, 2)
            worst = s2 + (stages - 2) * grow
            good = good and s1 < 2**ICC_A_BITS and worst <= 2**ICC_A_BITS
            print("icc:%-11s %-6s stream: %.2f p after the first round, %.2f p = %.4f x 2^263 after %d stages  %s"
                  % (name, form, s2 / p, worst / p, worst / 2**ICC_A_BITS, stages, "ok" if worst <= 2**ICC_A_BITS else "TOO LARGE"))
        # the finish step: any v < 2^263 -> [0, 2 p) -> canonical; the second part's product (symbol times wt) is below T as well
        good = good and icc_reduce_top_ok(p) and T <= 2**ICC_A_BITS
        # the mix: two symbols of 512 bits enter below 2^258, the outputs stay below 2^258 + max(T, 2 p)
        good = good and (p + (((2**256 - 1) * (p - 1)) >> 270) + 1) + 2**256 <= 2**258 and 2**258 + grow <= 2**ICC_A_BITS
        print("icc:%-11s bound chain (load step, %d stages, icc30_reduce_top on every v < 2^263, icc30_canonical): %s"
              % (name, stages, "ok" if good else "BAD"))
        ok = ok and good
    return ok


ICC_DECODE_STAGES = 16


def check_icc_decode_chain(stages=ICC_DECODE_STAGES):
    """the symbol bound chain of icc_decode.hip.h closes for the three moduli: EVERY symbol of the stream is below 2 p.  In the decode
    a + b adds two unreduced symbols and row 0 of a tile is never multiplied, so the sum is reduced at every butterfly:
      load      64-byte symbol: hi C526 + lo < (p + 2^242) + 2^256, icc30_reduce_top -> [0, 2 p); 32-byte row: < 2^256 <= 2 p_icc
      butterfly a, b < 2 p:  a + b < 4 p -> icc30_reduce_top -> [0, 2 p);  d = a - b + 3 p < 5 p (icc30_sub<3>: the table takes b
                up to 2 p - 1, check_sub_tables);  d * inverse twiddle (a product's result, < T <= 2^257 as an operand) < T <= 2 p
      finish    products with n^-1 (< p) and wt^-1 (a table twiddle): < T; icc30_reduce_top on any v < 2^263, then icc30_canonical
    The walk carries the largest symbol through `stages` stages and checks every operand at its consumer.  Bounds are exclusive."""
    ok = True
    for name, p in ICC_MODULI.items():
        T = icc_product_top(p)                       # a product's result over the whole operand domain (a < 2^263, w < 2^257)
        good = T <= 2 * p and T <= 2**ICC_W_BITS     # ... is below 2 p, and fits a twiddle operand (the inverse table, the finish)
        good = good and icc_sub_operands(p)[3] == 2 * p - 1
        load64 = (p + 2**242) + 2**256               # hi * (2^256 in the 2^270 form) + the raw lower half
        good = good and load64 <= 2**ICC_A_BITS and icc_reduce_top_ok(p)
        sym = 2 * p                                  # after the load step's short reduction
        if name == "p_icc":
            good = good and 2**256 <= 2 * p          # a 32-byte row enters as it is
        worst_sum = worst_diff = 0
        for _ in range(stages):
            s, d = 2 * sym, sym + 3 * p              # a + b;  a - b + 3 p with b >= 0
            worst_sum, worst_diff = max(worst_sum, s), max(worst_diff, d)
            good = good and s <= 2**ICC_A_BITS and d <= 2**ICC_A_BITS and sym <= 2 * p
            sym = max(2 * p, T)                      # the reduced sum, the product
            good = good and sym <= 2 * p
        # the inverse table's entry: (v^-1 + k q < 4 q) * C540 / 2^270; the finish's factors
        good = good and 4 * p <= 2**ICC_A_BITS and p <= 2**ICC_W_BITS
        print("icc:%-11s decode stream: sums below %.2f p, differences below %.2f p = %.5f x 2^263, symbols below 2 p at each of %d stages  %s"
              % (name, worst_sum / p, worst_diff / p, worst_diff / 2**ICC_A_BITS, stages, "ok" if good else "BAD"))
        ok = ok and good
    return ok


if __name__ == "__main__":
    import sys
    ok = all([check(n, p) for n, p in MODULI.items()])
    ok = all([check_mul2(n, p) for n, p in MODULI.items() if n != "p_icc"]) and ok
    ok = check_pm_mul2() and ok
    ok = all([check("icc:" + n, p, 23, 17) for n, p in ICC_MODULI.items()]) and ok
    ok = check_value_ranges() and ok
    ok = check_sub_tables() and ok
    # result bound of the ICC product: a b / 2^270 + p < p + 2^250 for a < 2^263, b < 2^257: limb 8 stays far below 2^30
    ok = check_icc_chain() and ok
    ok = check_icc_decode_chain() and ok
    sys.exit(0 if ok else 1)

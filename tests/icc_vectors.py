"""Vectors and expected values for the per-operation checks of the ICC field layer (tools/icc30_check.hip; the helpers of
porla_amd/csrc/icc30.hip.h and icc30_split.hip.h): shared by tests/test_icc30_gpu.py and tests/test_icc30_vectors_cpu.py.

Every expected value is a Python integer computed here; oracle/icc_py.py supplies the constants (p_icc, the group orders, LCM,
the root of unity) and pins the finish step and the mix (tests/test_icc30_vectors_cpu.py).  Generation is deterministic (fixed
seeds) and reads nothing outside the repository.

FORM: a residue travels as 9 limbs of 30 bits, limbs 0..7 < 2^30 ("normal"), everything from bit 240 up in limb 8.  The symbols
of the ICC stream are PLAIN residues, the twiddles carry the factor 2^270; a product is a b / 2^270.

THE NUMBERS (the same ones the comments of icc30.hip.h, icc30_split.hip.h, fe30.hip.h and tools/check_fe30_bounds.py state):
  A_MAX   = 2^263 - 1          a symbol of the stream: limb 8 < 2^23
  W_MAX   = 2^257 - 1          a twiddle as a product takes it: limb 8 < 2^17
  TW_TOP  = p + 2^242 - 1      a twiddle of the table: icc30_from_elem's product of two values below 2^256
  product(a, w), a <= A_MAX, w <= W_MAX:  r = (a w + m p) / 2^270 with m = (-a w p^-1) mod 2^270 -- unique, so the comparison is
          exact -- and r < p + floor(amax wmax / 2^270) + 1 for the operand maxima amax, wmax of the record's family; over the whole
          domain that is PRODUCT_TOP + 1 = p + 2^250
  LOAD_TOP = p + 2^248 - 1     what the load step leaves (a product of a 256-bit chunk with a table twiddle is below p + 2^243)
  a - b + K p is borrow-free limb by limb iff limb 8 of K p, minus 1, is at least limb 8 of b (fe30.hip.h:KP30); the call sites:
          K = 2: b a product's result, <= PRODUCT_TOP = p + 2^250 - 1 (and p + 2^249 - 1, the bound the comments stated before)
          K = 3: b = icc30_reduce_top's result, <= 2 p - 1
          K = 4: b the sum of two load-step products, <= 2 (p + 2^248) - 1
          K = 7: b a raw 256-bit chunk, <= 2^256 - 1
"""
import os
import random
import subprocess
import tempfile

import numpy as np

from tests import common  # (puts oracle/ on sys.path)
import icc_py  # noqa: E402

EXE = os.path.join(common.ROOT, "porla_amd", "icc30_check")

# record layout of tools/icc30_check.hip
REC, A0, FO, O0 = 192, 16, 96, 112
F_TIMES, F_SCALED, F_FEED, F_OUTS, F_SCALAR_LE = range(5)
MAX_TIMES = 32
SENTINEL = 0xA5A5A5A5
MASK30 = (1 << 30) - 1
R = 1 << 270
RUN_TIMEOUT = 120             # seconds, per driver process

P_ICC = icc_py.P_ICC
MODULI = {"p_icc": P_ICC, "bn254_r": icc_py.Q_BN254, "secp256k1_n": icc_py.Q_SECP256K1}
CURVE_OF = {"bn254_r": "bn254", "secp256k1_n": "secp256k1"}
K_COUNT = {"p_icc": 158, "bn254_r": 677, "secp256k1_n": 128}      # floor(2^263 / p): the multiples of p a symbol can hold

A_MAX = (1 << 263) - 1
W_MAX = (1 << 257) - 1
CHUNK_MAX = (1 << 256) - 1
SUM2_MAX = (1 << 257) - 1     # a2 + a3 of two raw chunks: what icc30_reduce_top takes in the raw first round
STAGES = 30                   # the longest chain of unreduced stages icc30_split.hip.h:icc30_fetch bounds


def tw_top(p):
    return p + (1 << 242) - 1


def product_top(p):
    return p + (1 << 250) - 1


def load_top(p):
    return p + (1 << 248) - 1


def sub_b_tops(p, K):
    """the largest b of a - b + K p at the call sites (module docstring)"""
    return {2: [p + (1 << 249) - 1, product_top(p)], 3: [2 * p - 1], 4: [2 * (p + (1 << 248)) - 1], 7: [CHUNK_MAX]}[K]


# ---------------------------------------------------------------- limbs and words
def limbs(v):
    assert v >= 0
    return [(v >> (30 * i)) & MASK30 for i in range(8)] + [v >> 240]


def limbs_value(l):
    return sum(int(x) << (30 * i) for i, x in enumerate(l))


def words(v, n=8):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def words_value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def new_records(n):
    r = np.zeros((n, REC), dtype=np.uint32)
    r[:, FO:] = SENTINEL
    return r


# ---------------------------------------------------------------- the helpers on Python integers
def mont(a, b, p):
    """the Montgomery product of the 9 x 30-bit form: digit by digit it computes the unique m < 2^270 with a b + m p = 0 mod 2^270"""
    m = (-a * b * pow(p, -1, R)) % R
    return (a * b + m * p) >> 270


def product_bound(p, amax, bmax):
    """exclusive bound of mont(a, b) over a <= amax, b <= bmax: a b / 2^270 + m p / 2^270 with m < 2^270"""
    return p + (amax * bmax >> 270) + 1


def sub_table_top(p, K):
    """limb 8 of fe30.hip.h:KP30<M, K>"""
    return (K * p >> 240) - 1


def borrow_free(p, K, b):
    lb = limbs(b)
    return all(x <= MASK30 for x in lb[:8]) and lb[8] <= sub_table_top(p, K)


def mu(p):
    """icc30.hip.h:IccMu"""
    return (1 << 88) // ((p >> 192) + 1)


def reduce_top(v, p):
    qh = ((v >> 240) * mu(p)) >> 40
    return v - qh * p, qh


def unit(p):
    return R % p


def c526(p):
    return pow(2, 526, p)


def c284(p):
    return pow(2, 284, p)


def load_symbol(sym, p):
    """icc30_load_symbol on one plane: hi * (2^256 in the 2^270 form) / 2^270 + lo, left unreduced"""
    lo, hi = sym & CHUNK_MAX, sym >> 256
    return mont(hi, c526(p), p) + lo


def crt(rp, rq, q):
    """the value below LCM with the two residues (icc30_finish_q: A = P + p_icc t, t = (A mod q - P) p_icc^-1 mod q)"""
    return rp + P_ICC * ((rq - rp) * pow(P_ICC, -1, q) % q)


def finish(vp, vq, q):
    """the finish step on a residue pair -> (A mod LCM, A mod p_icc, alignment scalar (A mod p_icc - A) mod q, A mod q)"""
    rp, rq = vp % P_ICC, vq % q
    return crt(rp, rq, q), rp, (rp - rq) % q, rq


def twiddle_slot(vi, q):
    """the table entry of the twiddle vi (an integer below p_icc, reduced mod q on the q plane) in the 2^270 form"""
    return vi * R % P_ICC, (vi % q) * R % q


def mix(a0, a1, vi, q):
    """Server::mix on one symbol pair: (A0 + vi A1) mod LCM, (A0 - vi A1) mod LCM"""
    lcm = P_ICC * q
    return (a0 + vi * a1) % lcm, (a0 - vi * a1) % lcm


def chain(p, a, w3, w, times, scaled, feed):
    """tools/icc30_check.hip:icc30_chain on integers.  Every operand is asserted inside its helper's contract: a vector outside it
    is a bug of the test, not a finding about the kernel."""
    a = list(a)

    def plain(K, i, j):
        t = a[j]
        assert borrow_free(p, K, t) and t <= sub_b_tops(p, K)[-1], "bfly_plain<%d> operand outside its contract" % K
        a[i], a[j] = a[i] + t, a[i] - t + K * p

    def bfly(i, j, tw):
        assert a[j] <= A_MAX and a[i] <= A_MAX and tw <= W_MAX, "butterfly operand outside its contract"
        t = mont(tw, a[j], p)
        assert borrow_free(p, 2, t)
        a[i], a[j] = a[i] + t, a[i] - t + 2 * p

    if scaled:
        plain(2, 0, 1), plain(2, 2, 3), plain(4, 0, 2)
    else:
        plain(7, 0, 1), plain(7, 2, 3)
        assert a[2] <= SUM2_MAX
        a[2], _ = reduce_top(a[2], p)
        assert 0 <= a[2] < 2 * p
        plain(3, 0, 2)
    bfly(1, 3, w3)
    for _ in range(2, min(times, MAX_TIMES)):
        if feed:
            a[1], a[3] = a[3], a[1]
        bfly(1, 3, w)
    assert all(0 <= x <= A_MAX for x in a), "the chain left the 2^263 range"
    return a


# ---------------------------------------------------------------- operand families
def value_families(name, hi=A_MAX):
    """[(family, value)]: every stated maximum itself, the multiples of p with their neighbours, small and special values --
    those that lie in [0, hi]"""
    p = MODULI[name]
    out = [("max_limbs", limbs_value([MASK30] * 8 + [(1 << 23) - 1])), ("2^263-1", A_MAX), ("2^256-1", CHUNK_MAX),
           ("2^257-1", SUM2_MAX), ("2(p+2^248)-1", 2 * (p + (1 << 248)) - 1), ("product_max", product_top(p)),
           ("twiddle_max", limbs_value([MASK30] * 8 + [(1 << 17) - 1])), ("load_max", load_top(p)), ("table_twiddle_max", tw_top(p))]
    assert K_COUNT[name] == A_MAX // p
    for k in range(K_COUNT[name] + 1):
        for d in (-2, -1, 0, 1, 2):
            if 0 <= k * p + d <= A_MAX:
                out.append(("kp%+d" % d, k * p + d))
    out += [("small", v) for v in (0, 1, p - 1, p, p + 1)] + [("unit", unit(p))]
    out += [("single_limb", 1 << (30 * i)) for i in range(9)] + [("single_limb", 1 << 262)]
    out += [("low_ones", (1 << 240) - 1), ("top_only", ((1 << 23) - 1) << 240), ("top_only", ((1 << 16) - 1) << 240)]
    return [(f, v) for f, v in out if 0 <= v <= hi]


VALUE_FAMILIES = ["max_limbs", "2^263-1", "2^256-1", "2^257-1", "2(p+2^248)-1", "product_max", "twiddle_max", "kp-2", "kp-1", "kp+0",
                  "kp+1", "kp+2", "small", "unit", "single_limb", "low_ones", "top_only"]


def twiddle_families(name):
    p = MODULI[name]
    return [("tw_unit", unit(p)), ("tw_zero", 0), ("tw_one", 1), ("tw_p-1", p - 1), ("tw_p", p), ("tw_p+1", p + 1),
            ("twiddle_max", W_MAX), ("table_twiddle_max", tw_top(p)), ("tw_low_ones", (1 << 240) - 1), ("tw_top_only", ((1 << 17) - 1) << 240)]


TWIDDLE_FAMILIES = ["tw_unit", "tw_zero", "tw_one", "tw_p-1", "tw_p", "tw_p+1", "twiddle_max", "table_twiddle_max"]


def rand_value(rng, p, hi):
    """uniform below hi, or a multiple of p plus a small or a uniform residue"""
    mode = rng.randrange(4)
    if mode == 0:
        return rng.randint(0, hi)
    k = rng.randint(0, hi // p)
    v = k * p + (rng.randint(-3, 3) if mode == 1 else rng.randrange(p))
    return min(max(v, 0), hi)


def rand_twiddle(rng, p):
    return rng.randint(0, tw_top(p)) if rng.random() < 0.8 else rng.randint(0, W_MAX)


SYMBOL_FAMILIES = ["sym_0", "sym_1", "sym_lcm-1", "sym_lcm", "sym_2^512-1", "sym_hi_ones", "sym_lo_ones"]


def symbol_families(q):
    lcm = P_ICC * q
    return [("sym_0", 0), ("sym_1", 1), ("sym_lcm-1", lcm - 1), ("sym_lcm", lcm), ("sym_2^512-1", (1 << 512) - 1),
            ("sym_hi_ones", CHUNK_MAX << 256), ("sym_lo_ones", CHUNK_MAX), ("sym_p_icc", P_ICC), ("sym_q", q), ("sym_2^256", 1 << 256)]


MIX_N = 1 << 10
TWIDDLE_ROWS = [("row_0", 0), ("row_n/2", MIX_N // 2), ("row_random", 357)]
ROW_FAMILIES = [f for f, _ in TWIDDLE_ROWS]


def twiddle_of_row(e):
    return pow(icc_py.root_w(MIX_N), e, P_ICC)


# ---------------------------------------------------------------- generation: op -> records, metas
FIELD_OPS = ["icc30_mul", "icc30_mul_alias_x", "icc30_mul_alias_y", "icc30_mul_sqr", "icc30_add", "icc30_sub2", "icc30_bfly",
             "icc30_bfly_plain2", "icc30_bfly_plain3", "icc30_bfly_plain4", "icc30_bfly_plain7", "icc30_reduce_top", "icc30_canonical",
             "icc30_pslot", "icc30_work", "icc30_chain"]
P_OPS = ["icc30_finish_p"]
PAIR_OPS = ["icc30_finish_elem", "icc30_finish_q", "icc30_load_symbol", "icc30_from_elem", "icc30_mix_elem", "icc30_slot"]
FINISH_OUTS = [("x", 1, 0), ("al", 2, 0), ("sc_be", 4, 0), ("sc_le", 4, 1), ("qres", 8, 0), ("all_be", 15, 0), ("all_le", 15, 1)]


def ops_of(name):
    return FIELD_OPS + (P_OPS if name == "p_icc" else PAIR_OPS)


def put30(rec, at, v):
    rec[A0 + at:A0 + at + 9] = limbs(v)


def get30(row, at):
    return [int(x) for x in row[O0 + at:O0 + at + 9]]


def gen(name, op, rng, sweep):
    """-> (records, metas); a meta holds the family name, the operands and the expected integers"""
    p = MODULI[name]
    q = p
    metas = []

    def add(family, **kw):
        metas.append(dict(family=family, **kw))

    wide = value_families(name)
    tws = twiddle_families(name)
    tops = [(f, v) for f, v in wide if f in ("max_limbs", "2^263-1", "2^256-1", "2^257-1", "2(p+2^248)-1", "product_max")]
    if op in ("icc30_mul", "icc30_mul_alias_x", "icc30_mul_alias_y", "icc30_bfly"):
        pairs = [(f, v, tf, tv, A_MAX) for i, (f, v) in enumerate(wide) for tf, tv in [tws[i % len(tws)]]]
        pairs += [(f, v, tf, tv, A_MAX) for f, v in tops for tf, tv in tws for _ in range(2)]      # (twice: icc30_mul takes both orders)
        pairs += [(tf, tv, tf, tv, W_MAX) for tf, tv in tws]               # a twiddle in the wide operand's place as well
        pairs += [("sweep", rand_value(rng, p, A_MAX), "sweep", rand_twiddle(rng, p), A_MAX) for _ in range(sweep)]
        for i, (f, v, tf, tv, amax) in enumerate(pairs):
            if op == "icc30_bfly":
                a = [A_MAX, 0, rand_value(rng, p, A_MAX)][i % 3]
                add(f, also=tf, a=a, b=v, w=tv)
            else:
                # the kernels put the wide operand in either place: icc30_bfly multiplies (w, b), the load step and the mix (x, w).
                # y = icc30_mul(x, y) is icc30_bfly's shape: the wide operand is the one overwritten
                first_wide = (i & 1) == 0 if op == "icc30_mul" else op == "icc30_mul_alias_x"
                add(f, also=tf, a=v if first_wide else tv, b=tv if first_wide else v, amax=amax)
    elif op == "icc30_mul_sqr":
        # the kernels never square; the shape only asks whether the tied accumulators survive x = x * x, inside the column budget
        # tools/check_fe30_bounds.py proves (limb 8 < 2^17 on both sides is well inside 2^23 x 2^17)
        vals = value_families(name, W_MAX) + tws + [("sweep", rand_twiddle(rng, p)) for _ in range(sweep)]
        for f, v in vals:
            add(f, also=f, a=v, b=v, amax=W_MAX)
    elif op == "icc30_add":
        for i, (f, v) in enumerate(wide + [("sweep", rand_value(rng, p, A_MAX)) for _ in range(sweep)]):
            b = [0, 1, A_MAX - v, rng.randint(0, A_MAX - v), min(product_top(p), A_MAX - v)][i % 5]
            add(f, a=v, b=b)
    elif op == "icc30_sub2" or op.startswith("icc30_bfly_plain"):
        K = 2 if op == "icc30_sub2" else int(op[-1])
        btops = sub_b_tops(p, K)
        bs = [("b_top", t) for t in btops] + [(f, v) for f, v in value_families(name, btops[-1])]
        bs += [("sweep", rand_value(rng, p, btops[-1])) for _ in range(sweep)]
        for i, (f, b) in enumerate(bs):
            avals = [0, A_MAX] if f == "b_top" else [[rand_value(rng, p, A_MAX), 0, A_MAX, limbs_value([MASK30] * 8 + [0])][i % 4]]
            for a in avals:
                assert borrow_free(p, K, b), "a vector outside the contract of the K = %d difference" % K
                add(f, a=a, b=b, K=K, a_end="a_zero" if a == 0 else ("a_max" if a == A_MAX else None))
    elif op in ("icc30_reduce_top", "icc30_finish_p"):
        for f, v in wide + [("sweep", rand_value(rng, p, A_MAX)) for _ in range(sweep)]:
            add(f, a=v)
    elif op == "icc30_canonical":
        for f, v in value_families(name, 2 * p - 1) + [("2p-1", 2 * p - 1)] + [("sweep", rand_value(rng, p, 2 * p - 1)) for _ in range(sweep)]:
            add(f, a=v)
    elif op in ("icc30_pslot", "icc30_work", "icc30_slot"):
        nw = 18 if op == "icc30_slot" else 9
        pats = [[0] * nw, [0xffffffff] * nw, list(range(1, nw + 1)), limbs(A_MAX) * (nw // 9)]
        for i in range(sweep // 4 + len(pats)):
            add("pattern" if i < len(pats) else "sweep", w=pats[i] if i < len(pats) else [rng.getrandbits(32) for _ in range(nw)])
    elif op == "icc30_chain":
        t_list = [2, 3, 4, 5, 8, 16, 29, STAGES, STAGES, STAGES, MAX_TIMES + 8]        # the last is capped by the driver
        for i in range(max(sweep // 4, 60)):
            scaled = i & 1
            top = load_top(p) if scaled else CHUNK_MAX
            times = t_list[(i // 2) % len(t_list)] if i < 4 * len(t_list) else rng.randint(2, STAGES)
            if times > STAGES:
                fam = "capped"
            elif i < 4 * len(t_list):
                fam = "ends"
            else:
                fam = "sweep"
            if fam == "sweep":
                a = [rand_value(rng, p, top) for _ in range(4)]
                w3, w = rand_twiddle(rng, p) % (tw_top(p) + 1), rand_twiddle(rng, p) % (tw_top(p) + 1)
            else:
                a = [top, top, top, top] if (i // 2) % 2 == 0 else [top, 0, top, 0]
                w3 = w = [unit(p), tw_top(p), p - 1, unit(p) + p if unit(p) + p <= tw_top(p) else unit(p)][(i // 4) % 4]
            # a capped record runs MAX_TIMES stages: two more than the design's 30, still inside 2^263 (asserted by chain())
            feed = (i >> 2) & 1
            add(fam, a=a, w3=w3, w=w, times=times, scaled=scaled, feed=feed, want=chain(p, a, w3, w, times, scaled, feed))
    elif op in ("icc30_finish_elem", "icc30_finish_q"):
        wp = value_families("p_icc")
        wq = wide
        n = max(len(wp), len(wq))
        cases = [(wp[i % len(wp)], wq[i % len(wq)]) for i in range(n)]
        cases += [(("sweep", rand_value(rng, P_ICC, A_MAX)), ("sweep", rand_value(rng, q, A_MAX))) for _ in range(sweep)]
        outs = FINISH_OUTS if op == "icc30_finish_elem" else [o for o in FINISH_OUTS if o[0] != "al"]
        for i, ((fp, vp), (fq, vq)) in enumerate(cases):
            oname, mask, le = outs[i % len(outs)]
            if op == "icc30_finish_q":
                mask &= ~2
            add(fq, also=fp, vp=vp, vq=vq, outs=oname, mask=mask, le=le)
        for oname, mask, le in outs:                                       # every subset at the operand maxima and on p, 2p - 1
            for vp, vq in ((A_MAX, A_MAX), (P_ICC, q), (2 * P_ICC - 1, 2 * q - 1), (0, 0)):
                add("outs_" + oname, also="outs", vp=vp, vq=vq, outs=oname, mask=mask & (~2 if op == "icc30_finish_q" else 15), le=le)
    elif op in ("icc30_load_symbol", "icc30_from_elem"):
        syms = symbol_families(q) + [("sweep", rng.getrandbits(512) if i & 1 else rng.randrange(P_ICC * q)) for i in range(sweep)]
        for f, s in syms:
            add(f, sym=s)
    elif op == "icc30_mix_elem":
        syms = symbol_families(q)
        cases = [(fa, a, fb, b, fr, e) for fa, a in syms for fb, b in syms for fr, e in TWIDDLE_ROWS]
        lcm = P_ICC * q
        cases += [("sweep", rng.randrange(lcm), "sweep", rng.randrange(lcm), "sweep", rng.randrange(MIX_N)) for _ in range(sweep)]
        for fa, a, fb, b, fr, e in cases:
            add(fa, also=fb, row=fr, a0=a, a1=b, vi=twiddle_of_row(e))
    else:
        raise AssertionError("unknown operation " + op)

    recs = new_records(len(metas))
    for i, m in enumerate(metas):
        r = recs[i]
        if op in ("icc30_pslot", "icc30_work", "icc30_slot"):
            r[A0:A0 + len(m["w"])] = m["w"]
        elif op == "icc30_chain":
            for k in range(4):
                put30(r, 9 * k, m["a"][k])
            put30(r, 36, m["w3"]), put30(r, 45, m["w"])
            r[F_TIMES], r[F_SCALED], r[F_FEED] = m["times"], m["scaled"], m["feed"]
        elif op in ("icc30_finish_elem", "icc30_finish_q"):
            put30(r, 0, m["vp"]), put30(r, 9, m["vq"])
            if op == "icc30_finish_q":
                r[A0 + 18:A0 + 26] = words(m["vp"] % P_ICC)
            r[F_OUTS], r[F_SCALAR_LE] = m["mask"], m["le"]
        elif op in ("icc30_load_symbol", "icc30_from_elem"):
            r[A0:A0 + 16] = words(m["sym"], 16)
        elif op == "icc30_mix_elem":
            r[A0:A0 + 16], r[A0 + 16:A0 + 32] = words(m["a0"], 16), words(m["a1"], 16)
            tp, tq = twiddle_slot(m["vi"], q)
            lp, lq = limbs(tp), limbs(tq)
            r[A0 + 32:A0 + 52] = lp[:8] + lq[:8] + [lp[8], lq[8], SENTINEL, SENTINEL]
        else:
            put30(r, 0, m["a"])
            if "b" in m:
                put30(r, 9, m["b"])
            if "w" in m:
                put30(r, 18, m["w"])
    return recs, metas


# ---------------------------------------------------------------- checking
class Counter:
    """every generated record is checked: the tests assert checked == generated"""
    def __init__(self):
        self.checked = 0


def normal(l, where):
    assert all(x < 1 << 30 for x in l[:8]), "%s: a limb >= 2^30: %s" % (where, l)
    return limbs_value(l)


def check(name, op, recs, out, metas, counter):
    p = MODULI[name]
    q = p
    for i, m in enumerate(metas):
        where = "%s %s record %d (%s)" % (name, op, i, m["family"])
        row, rec = out[i], recs[i]
        assert np.array_equal(row[:O0], rec[:O0]), where + ": flags or operands changed"
        used = 0                                                    # words of the result area the operation owns
        if op.startswith("icc30_mul"):
            a, b = m["a"], m["b"]
            want = mont(a, b, p)
            assert min(a, b) <= W_MAX and max(a, b) <= m["amax"], where + ": operands outside the product's domain"
            bound = product_bound(p, m["amax"], W_MAX)              # from the operand maxima of the record's family
            assert bound <= product_top(p) + 1 and want < bound, where + ": the expectation itself exceeds the bound"
            got = get30(row, 0)
            port = get30(row, 18)
            if op == "icc30_mul_alias_y":
                got, other, other_want = get30(row, 9), get30(row, 0), a
            else:
                other, other_want = get30(row, 9), b
            assert limbs_value(got) < bound, where + ": value bound"
            assert normal(got, where) == want, "%s: %#x != %#x" % (where, limbs_value(got), want)
            assert got == port, where + ": the assembly and f30_mul_portable differ limb for limb"
            if op != "icc30_mul":
                assert limbs_value(other) == other_want, where + ": the operand that is not overwritten changed"
            used = 27
            if op == "icc30_mul":
                assert (row[O0 + 9:O0 + 18] == SENTINEL).all(), where
        elif op == "icc30_add":
            assert normal(get30(row, 0), where) == m["a"] + m["b"], where
            used = 9
        elif op == "icc30_sub2":
            assert normal(get30(row, 0), where) == m["a"] - m["b"] + 2 * p, where
            used = 9
        elif op == "icc30_bfly":
            t = mont(m["w"], m["b"], p)
            assert t < product_bound(p, A_MAX, W_MAX) and borrow_free(p, 2, t)
            assert normal(get30(row, 0), where) == m["a"] + t, where + ": a + w b"
            assert normal(get30(row, 9), where) == m["a"] - t + 2 * p, where + ": a - w b + 2 p"
            used = 18
        elif op.startswith("icc30_bfly_plain"):
            assert normal(get30(row, 0), where) == m["a"] + m["b"], where + ": a + b"
            assert normal(get30(row, 9), where) == m["a"] - m["b"] + m["K"] * p, where + ": a - b + K p"
            used = 18
        elif op == "icc30_reduce_top":
            want, qh = reduce_top(m["a"], p)
            assert 0 <= want < 2 * p and m["a"] // p - 1 <= qh <= m["a"] // p, where + ": the expectation leaves [0, 2 p)"
            assert normal(get30(row, 0), where) == want, where
            used = 9
        elif op in ("icc30_canonical", "icc30_finish_p"):
            assert words_value(row[O0:O0 + 8]) == m["a"] % p, where
            used = 8
        elif op in ("icc30_pslot", "icc30_work"):
            at = 0 if op == "icc30_pslot" else 1
            assert [int(x) for x in row[O0 + at:O0 + at + 9]] == m["w"], where + ": stored words"
            if op == "icc30_pslot":
                assert int(row[O0 + 9]) == 0, where + ": the pad word of a plane slot"
                assert (row[O0 + 10:O0 + 16] == SENTINEL).all(), where
            else:
                assert int(row[O0]) == SENTINEL and (row[O0 + 10:O0 + 16] == SENTINEL).all(), where + ": a neighbouring word changed"
            assert [int(x) for x in row[O0 + 16:O0 + 25]] == m["w"], where + ": loaded words"
            used = 25
        elif op == "icc30_slot":
            w = m["w"]
            assert [int(x) for x in row[O0:O0 + 20]] == w[:8] + w[9:17] + [w[8], w[17], SENTINEL, SENTINEL], where + ": slot layout"
            assert (row[O0 + 20:O0 + 32] == SENTINEL).all(), where
            assert [int(x) for x in row[O0 + 32:O0 + 50]] == w, where + ": loaded words"
            used = 50
        elif op == "icc30_chain":
            for k in range(4):
                assert normal(get30(row, 9 * k), where) == m["want"][k], where + ": symbol %d" % k
            used = 36
        elif op in ("icc30_finish_elem", "icc30_finish_q"):
            x, al, sc, qres = finish(m["vp"], m["vq"], q)
            b = row[O0:O0 + 40].tobytes()
            untouched = np.full(8, SENTINEL, dtype=np.uint32).tobytes()
            mask = m["mask"]
            assert b[0:64] == (x.to_bytes(64, "little") if mask & 1 else untouched * 2), where + ": value mod LCM"
            assert b[64:96] == (al.to_bytes(32, "little") if mask & 2 else untouched), where + ": value mod p_icc"
            assert b[96:128] == (sc.to_bytes(32, "little" if m["le"] else "big") if mask & 4 else untouched), where + ": alignment scalar"
            assert b[128:160] == (qres.to_bytes(32, "big") if mask & 8 else untouched), where + ": value mod q"
            used = 40
        elif op == "icc30_load_symbol":
            for at, mod in ((0, P_ICC), (9, q)):
                want = load_symbol(m["sym"], mod)
                assert want < 1 << 258 and want % mod == m["sym"] % mod
                assert normal(get30(row, at), where) == want, where
            used = 18
        elif op == "icc30_from_elem":
            for at, mod, e in ((0, P_ICC, m["sym"] & CHUNK_MAX), (9, q, m["sym"] >> 256)):
                want = mont(e, c284(mod), mod)
                assert want <= tw_top(mod) and want % mod == (e << 14) % mod
                assert normal(get30(row, at), where) == want, where
            used = 18
        elif op == "icc30_mix_elem":
            lo, hi = mix(m["a0"], m["a1"], m["vi"], q)
            b = row[O0:O0 + 32].tobytes()
            assert b[:64] == lo.to_bytes(64, "little"), where + ": A0 + v^i A1"
            assert b[64:] == hi.to_bytes(64, "little"), where + ": A0 - v^i A1"
            used = 32
        else:
            raise AssertionError(op)
        assert (row[O0 + used:] == SENTINEL).all() and (row[FO:O0] == SENTINEL).all(), where + ": wrote outside its result"
        counter.checked += 1


# ---------------------------------------------------------------- running the driver
def run(name, jobs):
    """jobs: [(op, records)] -> [records after the operation], one process for all of them"""
    with tempfile.TemporaryDirectory() as d:
        cmd = [EXE, name]
        for i, (op, recs) in enumerate(jobs):
            assert recs.dtype == np.uint32 and recs.shape[1] == REC
            recs.tofile(os.path.join(d, "in%d" % i))
            cmd += [op, os.path.join(d, "in%d" % i), os.path.join(d, "out%d" % i)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=RUN_TIMEOUT)
        assert r.returncode == 0, "icc30_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
        outs = []
        for i, (op, recs) in enumerate(jobs):
            o = np.fromfile(os.path.join(d, "out%d" % i), dtype=np.uint32).reshape(-1, REC)
            assert o.shape == recs.shape, "%s: %d records out for %d in" % (op, o.shape[0], recs.shape[0])
            outs.append(o)
        return outs


def seed_of(name, op):
    return 3000 + 100 * sorted(MODULI).index(name) + (FIELD_OPS + P_OPS + PAIR_OPS).index(op)


def generate(name, op, sweep):
    return gen(name, op, random.Random(seed_of(name, op)), sweep)


# ---------------------------------------------------------------- the named families are present whatever the seed
def assert_families_present(name, op, metas):
    fam = {m["family"] for m in metas}
    also = {m.get("also") for m in metas}

    def need(wanted, have, what="family"):
        missing = [f for f in wanted if f not in have]
        assert not missing, "%s %s: no record of %s %s" % (name, op, what, missing)

    if op in ("icc30_mul", "icc30_mul_alias_x", "icc30_mul_alias_y", "icc30_bfly"):
        need(VALUE_FAMILIES, fam), need(TWIDDLE_FAMILIES, also, "twiddle family")
        if op == "icc30_mul":                                      # the wide operand in either place
            assert any(m["a"] == A_MAX and m["b"] == W_MAX for m in metas) and any(m["a"] == W_MAX and m["b"] == A_MAX for m in metas)
    elif op == "icc30_mul_sqr":
        need(["2^256-1", "twiddle_max", "kp+0", "kp-1", "kp+1", "small", "unit", "single_limb", "low_ones"] + TWIDDLE_FAMILIES, fam)
    elif op in ("icc30_add", "icc30_reduce_top", "icc30_finish_p"):
        need(VALUE_FAMILIES, fam)
    elif op == "icc30_sub2" or op.startswith("icc30_bfly_plain"):
        K = metas[0]["K"]
        for top in sub_b_tops(MODULI[name], K):
            for end in ("a_zero", "a_max"):
                assert any(m["family"] == "b_top" and m["b"] == top and m["a_end"] == end for m in metas), \
                    "%s %s: b = %#x does not meet %s" % (name, op, top, end)
        need(["small", "kp+0", "kp-1", "kp+1", "single_limb"], fam)
    elif op == "icc30_canonical":
        p = MODULI[name]
        need(["2p-1", "small", "kp+0", "kp-1", "kp+1", "unit"], fam)
        assert {p, p - 1, 2 * p - 1, 0} <= {m["a"] for m in metas}
    elif op == "icc30_chain":
        need(["ends", "capped", "sweep"], fam)
        for scaled in (0, 1):
            for feed in (0, 1):
                assert any(m["scaled"] == scaled and m["feed"] == feed and m["times"] == STAGES and m["family"] == "ends" for m in metas)
    elif op in ("icc30_finish_elem", "icc30_finish_q"):
        need(VALUE_FAMILIES, fam), need(VALUE_FAMILIES, also, "p_icc residue family")
        need(["outs_" + o for o, _, _ in FINISH_OUTS if not (op == "icc30_finish_q" and o == "al")], fam, "output subset")
    elif op in ("icc30_load_symbol", "icc30_from_elem"):
        need(SYMBOL_FAMILIES, fam)
    elif op == "icc30_mix_elem":
        need(SYMBOL_FAMILIES, fam), need(SYMBOL_FAMILIES, also, "second symbol"), need(ROW_FAMILIES, {m["row"] for m in metas}, "twiddle row")
    else:
        need(["pattern", "sweep"], fam)

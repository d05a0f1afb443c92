"""GPU: the reduced-radix group law of porla_amd/csrc/ec30.hip.h (and the 8 x 32-bit forms of ec.hip.h) per operation, at the
operand bounds its comments state, through the driver tools/ec30_check.hip.  Expected values: Python integers
(tests/ec_vectors.py, where the residue convention is stated).  For every record: form (limbs 0..7 < 2^30, limb 8 < 2^18 /
2^19; memory words as the header says), value bound (ec_vectors.BOUNDS, within the operand bound of every consumer) and group
element (X / ZZ, Y / ZZZ, ZZ^3 = ZZZ^2; inf, the returned bool and flip exactly; a false return leaves p and flip bit-identical).
Comparison is exact; no record is skipped (checked == generated is asserted)."""
import functools
import os
import random

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests.ec_vectors import A0, FO, O0, BN254, SECP

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "secp256k1"]
SWEEP = 2000                                   # random records per operation, on top of the listed edge cases

FIELD_OPS = ["f30_sub2", "f30_sub3", "f30_sub4", "f30_sub5", "f30_sub6", "f30_sub_twice3", "f30_add2", "f30_small_mul2",
             "f30_small_mul3", "f30_ripple", "f30_product_is_zero", "f30_to_fe_canonical", "f30_pm_reduce", "f30_unpack",
             "f30_pack", "f30_const"]
POINT_OPS = ["xyzz30_double_affine", "xyzz30_madd_flip", "xyzz30_madd_flip_fast", "xyzz30_mmadd_flip_fast", "xyzz30_flip_finish",
             "xyzz30_double", "xyzz30_add", "xyzz30_to_xyzz", "xyzz30_store_load_lazy", "xyzz30_add_mem", "xyzz30_double_mem",
             "xyzz30_add_one_lane", "xyzz30_add_quad", "xyzz30_dbl_quad", "xyzz30_dbl_quadreg", "xyzz30_add_quadreg",
             "xyzz30_quadreg_ladder"]


def test_driver_is_built():
    assert os.path.exists(ev.EXE), "build it with make -C porla_amd/csrc"


def test_bounds_table_is_closed():
    """every output bound lies inside the operand bound of every operation that may consume the value"""
    for C in ev.CURVES.values():
        for key, (bx, by, bz) in ev.BOUNDS.items():
            y_in = C.in_y if key in ev.NOT_NEGATED else C.in_y_neg
            assert ev.bound(C, bx) - 1 <= C.in_x and ev.bound(C, by) - 1 <= y_in <= C.in_y and ev.bound(C, bz) - 1 <= C.in_z, key
        assert C.in_x < 1 << (240 + C.top_bits) and 2 * C.in_y < 1 << (240 + C.top_bits)          # U = 2Y of a doubling
        assert ev.on_curve(C, C.g) and pow(C.beta, 3, C.p) == 1 and C.beta != 1
    assert BN254.in_x < 1 << 256 and BN254.in_y < 1 << 256                                       # the lazy memory form


# ================================================================ field helpers
def normal_values(C, rng, hi, n):
    """values in [0, hi] as canonical limb lists: the ends, residues 0, 1, p - 1, all-ones low limbs, random"""
    v = [0, 1, C.p - 1, C.p, hi, hi - 1, ((hi >> 240) - 1 << 240) + (1 << 240) - 1, (1 << 240) - 1]
    v = [x for x in v if 0 <= x <= hi]
    return v + [rng.randint(0, hi) for _ in range(n)]


def gen_field(C, op, rng):
    p = C.p
    wide = [(1 << 30) + (1 << 29) - 1] * 9                       # "any limbs < 2^30 + 2^29" (f30_sub)
    wide_n8 = wide[:8] + [ev.limbs(C.in_x)[8]]
    recs = []                                                    # (limbs a, limbs b or None, expected)
    if op.startswith("f30_sub"):
        K = int(op[-1])
        twice = "twice" in op
        # b up to (K-1) p + 2^240 (fe30.hip.h KP30) and the 2^247 tools/check_fe30_bounds.py checks; 2 b for the doubled form
        tops = [(K - 1) * p + (1 << 240), (K - 1) * p + (1 << 247)]
        bs = []
        for t in tops:
            t = t // 2 if twice else t
            bs += normal_values(C, rng, t, 0)
        bs += [rng.randint(0, tops[1] // (2 if twice else 1)) for _ in range(SWEEP)]
        for i, b in enumerate(bs):
            a = [ev.limbs(rng.randint(0, C.in_x)), ev.limbs(0), ev.limbs(C.in_x), [ev.MASK30] * 8 + [(1 << C.top_bits) - 1]][i % 4 if i < 64 else 0]
            if not twice and i % 7 == 3:
                a = wide if i % 2 else wide_n8
            recs.append((a, ev.limbs(b), ev.limbs_value(a) - (2 if twice else 1) * b + K * p))
    elif op == "f30_add2":
        for i in range(SWEEP + 40):
            a, b = [rng.choice(normal_values(C, rng, C.in_z, 1)) for _ in range(2)]
            recs.append((ev.limbs(a), ev.limbs(b), a + 2 * b))
    elif op.startswith("f30_small_mul"):
        K = int(op[-1])
        hi = C.in_y if K == 2 else C.in_z                          # U = 2 Y, M = 3 XX
        for a in normal_values(C, rng, hi, SWEEP):
            recs.append((ev.limbs(a), None, K * a))
    elif op == "f30_ripple":
        for i in range(SWEEP):
            a = [rng.choice([0, ev.MASK30, (1 << 32) - 4, rng.getrandbits(32) & ~3 | 0]) for _ in range(8)] + [rng.getrandbits(16)]
            a = [min(x, (1 << 32) - 4) for x in a]
            recs.append((a, None, ev.limbs_value(a)))
    elif op == "f30_product_is_zero":
        vals = [0, p, p + 1, p - 1, 2 * p, 1, C.in_z]
        for k in range(9):
            for d in (1, -1):
                l = ev.limbs(p)
                l[k] += d
                if 0 <= l[k] < (1 << 30):
                    vals.append(ev.limbs_value(l))
        vals += [rng.randint(0, C.in_z) for _ in range(SWEEP)] + [rng.choice([0, p]) for _ in range(50)]
        recs = [(ev.limbs(v), None, 1 if v in (0, p) else 0) for v in vals]
    elif op == "f30_to_fe_canonical":
        # the comment above f30_to_fe_canonical: < p + 2^246, or < 2^256 + 2^49 in the special form, where bit 256 may be set
        hi = (1 << 256) + (1 << 49) - 1 if C is SECP else C.in_z
        vals = normal_values(C, rng, hi, SWEEP) + [p + 1, (1 << 256) - 1 if C is SECP else 1, 1 << 256 if C is SECP else 1]
        recs = [(ev.limbs(v), None, v % p) for v in vals]
    elif op == "f30_pm_reduce":
        vals = normal_values(C, rng, C.in_x, SWEEP) + [(1 << 256) - 1, 1 << 256, (1 << 256) + (1 << 49), p, p + 1, 2 * p - 1, 4 * p, (1 << 259) - 1]
        recs = [(ev.limbs(v), None, v) for v in vals]
    elif op in ("f30_unpack", "f30_const"):
        vals = [0, 1, (1 << 256) - 1, p, BN254.in_x] + [rng.getrandbits(256) for _ in range(SWEEP)]
        recs = [(ev.words(v), None, v) for v in vals]
    elif op == "f30_pack":
        vals = [0, 1, (1 << 256) - 1, p, BN254.in_x] + [rng.getrandbits(256) for _ in range(SWEEP)]
        recs = [(ev.limbs(v), None, v) for v in vals]
    R = ev.new_records(len(recs))
    for i, (a, b, _) in enumerate(recs):
        R[i, A0:A0 + len(a)] = a
        if b is not None:
            R[i, A0 + 9:A0 + 18] = b
    return R, [e for _, _, e in recs]


def check_field(C, op, out, want, counter):
    for i, e in enumerate(want):
        where = "%s %s record %d" % (C.name, op, i)
        row = out[i]
        if op == "f30_product_is_zero":
            assert int(row[FO]) == e, where
        elif op in ("f30_to_fe_canonical", "f30_pack"):
            assert ev.words_value(row[O0:O0 + 8]) == e, where
        else:
            l = [int(x) for x in row[O0:O0 + 9]]
            assert all(x < 1 << 30 for x in l[:8]), where + ": limb >= 2^30"
            got = ev.limbs_value(l)
            if op == "f30_pm_reduce":
                assert got % C.p == e % C.p and got < (1 << 256) + (1 << 49) and l[8] < 1 << C.top_bits, where
            else:
                assert got == e, "%s: %#x != %#x" % (where, got, e)
                if op in ("f30_unpack", "f30_const"):
                    assert l[8] < 1 << 16, where
        counter.checked += 1


# ================================================================ group operations
def elem(C, k):
    """k G; ("phi", k): the endomorphism's image of k G; ("pt", point): that point"""
    if isinstance(k, tuple):
        return ev.ec_phi(C, elem(C, k[1])) if k[0] == "phi" else k[1]
    G = ev.multiples(C)
    return None if k == 0 else (G[k] if k > 0 else ev.ec_neg(C, G[-k]))


def shaped(C, P, rng, kind, y_max=None, mem=False):
    """one representation of P: kind = min | top | xmax | zmax | high | yneg_top | rand (see ec_vectors)"""
    f = ev.rep_mem if mem else ev.rep30
    if P is None:
        return [0, 0, 0, 0]
    if kind == "min":
        return f(C, P, 1, [0, 0, 0, 0], y_max, rng)
    if kind == "xmax":                                           # X = 5p + eps - 1 with limbs to match (or the next square below)
        return f(C, P, ev.find_l(C, P, 0, C.eps - 1, rng)[0], "top", y_max, rng)
    if kind == "zmax":                                           # ZZ = p + eps - 1
        return f(C, P, ev.find_l(C, P, 2, C.eps - 1, rng)[0], "top", y_max, rng)
    if kind == "yneg_top":                                       # Y = 3p + t, t <= eps: the top of what 4p - Y accepts
        v = f(C, P, find_l_y_small(C, P, rng), "top", C.in_y_neg, rng)
        assert (C is SECP and mem) or 3 * C.p <= v[1] <= C.in_y_neg
        return v
    if kind == "high":                                           # Y just below its bound
        return f(C, P, ev.find_l_high(C, P, 1, rng), "top", y_max, rng)
    return f(C, P, rng.randrange(1, C.p), "top" if kind == "top" else None, y_max, rng)


def find_l_y_small(C, P, rng):
    """an l whose Y residue y l^3 (in the form) is at most eps: by search where eps / p is 2^-8 (BN254), else through a cube
    root of t / y for t walked down from eps (secp256k1)"""
    if C.eps << 12 >= C.p:
        for _ in range(1 << 14):
            l = rng.randrange(1, C.p)
            if ev.residues(C, P, l, C.r30)[1] <= C.eps:
                return l
        raise AssertionError("no l found")
    t = C.eps - rng.randrange(1 << 32)
    while True:
        l = ev.cbrt_mod(C, t * pow(P[1] * C.r30, -1, C.p) % C.p)
        if l:
            return l
        t -= 1


def is_yneg_top(C, y):
    return 3 * C.p <= y <= C.in_y_neg


KINDS = ["min", "top", "xmax", "zmax", "high"]


def pair_cases(C, rng, n, with_inf=True):
    """(a, b, kind_a, kind_b): multiples of the generator.  Equal x with the same and different l, P + (-P), infinity on either
    side and both, every operand shape, then a random sweep"""
    cases = []
    for ka in KINDS:
        for kb in KINDS:
            cases += [(3, 5, ka, kb), (4, 4, ka, kb), (6, -6, ka, kb)]
    cases += [(2, 2, "min", "min"), (2, -2, "min", "min"), (7, 7, "rand", "rand"), (7, -7, "rand", "top")]
    if with_inf:
        cases += [(0, 5, "min", k) for k in KINDS] + [(5, 0, k, "min") for k in KINDS] + [(0, 0, "min", "min")]
    while len(cases) < n:
        a = rng.randint(1, 40)
        b = a * rng.choice([1, -1]) if rng.random() < 0.1 else rng.choice([1, -1]) * rng.randint(1, 40)
        cases.append((a, b, rng.choice(["rand", "top"]), rng.choice(["rand", "top"])))
    return cases


def x_multiple_cases(C, P, rng):
    """representations of P whose X is (a small residue) + i p for i = 0..5: P = U2 - X1 + 6p then takes each of its zero
    representatives when the other operand is P or -P"""
    l, _ = ev.find_l(C, P, 0, 64, rng)
    return [ev.rep30(C, P, l, [i, rng.randint(0, 2), 0, 0]) for i in range(6)]


def x_top_small_u2_cases(C, rng, count=8):
    """named regression family "x_top_small_u2": an accumulator with X1 = 5p + t (t < eps, the top of its range) that meets a
    point whose U2 = X2 ZZ1 is a residue BELOW t, so P = U2 - X1 + 6p lies under p: one multiple of p less in that subtraction
    borrows out of limb 8 (and nothing else in the suite notices).  U2 is kept above 2^240 so that the product returns the
    residue itself, not residue + p.  Found by search over t (one try in ~2^8 for BN254); for secp256k1 the slack above 5p is
    2^73 of 2^256 and no such pair can be constructed, so the family is empty there."""
    out = []
    if C.eps << 12 < C.p:
        return out
    k1 = 2
    while len(out) < count:
        k1 += 1
        P, Q = elem(C, k1), elem(C, k1 + 7)
        ratio = Q[0] * pow(P[0], -1, C.p) % C.p
        t = C.eps - 1 - rng.randrange(1 << 200)
        for _ in range(1 << 14):
            t -= 1
            u = ratio * t % C.p
            if (1 << 240) < u < t:
                l = ev.sqrt_mod(C, t * pow(P[0] * C.r30, -1, C.p) % C.p)
                if l:
                    v = ev.rep30(C, P, l, "top")
                    assert v[0] == 5 * C.p + t and Q[0] * v[2] % C.p == u
                    out.append((k1, k1 + 7, v, None))
                    break
    return out


_SMALL_X = {}


def mmadd_x_top_cases(C, count=6):
    """the same hole for xyzz30_mmadd_flip_fast, whose accumulator IS an affine point (X1 = x R + i p, no free l): points k G
    whose x in the form is a residue t below eps, taken as accumulator at X1 = 5p + t, meeting another such point whose ax is
    below t, so Pp = ax - X1 + 6p lies under p.  BN254 only (one multiple of G in ~2^8 qualifies); none exists for secp256k1."""
    if C.eps << 12 < C.p:
        return []
    if C.name not in _SMALL_X:
        hits, pt = [], None
        for k in range(1, 6000):
            pt = ev.ec_add(C, pt, C.g)
            if pt[0] * C.r30 % C.p < C.eps:
                hits.append(pt)
        _SMALL_X[C.name] = sorted(hits, key=lambda q: q[0] * C.r30 % C.p)
    hits = _SMALL_X[C.name]
    assert len(hits) >= 4
    out = []
    for i in range(min(count, len(hits) - 1)):
        P, Q = hits[-1 - i], hits[i]                              # the accumulator's residue above the point's
        res = ev.residues(C, P, 1, C.r30)
        v = [res[0] + 5 * C.p, res[1] + (C.in_y - res[1]) // C.p * C.p, C.r30, C.r30]
        assert Q[0] * C.r30 % C.p < res[0] and v[0] <= C.in_x
        out.append((("pt", P), ("pt", Q), v, None))
    return out


def same_bits(row, rec, n=36):
    return np.array_equal(row[O0:O0 + n], rec[A0:A0 + n])


def gen_point_op(C, op, rng):
    """-> records, metas (dicts the checker reads)"""
    p = C.p
    rows, metas = [], []

    def add(meta, setup):
        r = ev.new_records(1)[0]
        setup(r)
        rows.append(r)
        metas.append(meta)

    if op in ("xyzz30_double_affine", "xyzz30_double", "xyzz30_dbl_quadreg"):
        for i in range(SWEEP // 2 + 200):
            k = rng.randint(1, 40) * rng.choice([1, -1])
            P = elem(C, k)
            if op == "xyzz30_double_affine":
                v = ev.aff30(C, P)
                add(dict(want=ev.ec_add(C, P, P), key="double"), lambda r: ev.put30(r, 36, v))
            else:
                v = shaped(C, P, rng, KINDS[i] if i < len(KINDS) else rng.choice(["rand", "top"]))
                add(dict(want=ev.ec_add(C, P, P), key="double"), lambda r: ev.put30(r, 0, v))
    elif op in ("xyzz30_madd_flip", "xyzz30_madd_flip_fast", "xyzz30_mmadd_flip_fast"):
        fast = op != "xyzz30_madd_flip"
        mm = op == "xyzz30_mmadd_flip_fast"
        cases = [(a, b, ka, None) for a, b, ka, _ in pair_cases(C, rng, SWEEP)]
        cases = [c for c in cases if fast or c[1] != 0]           # the general form has no a_is_inf: its callers never pass one
        extra = []
        for k in (3, 9):
            for sign in (1, -1):
                extra += [(k, sign * k, v, None) for v in x_multiple_cases(C, elem(C, k), rng)]
        extra += mmadd_x_top_cases(C) if mm else x_top_small_u2_cases(C, rng)
        for a, b, ka, _ in cases + extra:
            P, Q = elem(C, a), elem(C, b)
            if isinstance(ka, list):
                v = ka
            elif mm and P is not None:                            # an accumulator that IS an affine point: ZZ = ZZZ = the unit
                res = ev.residues(C, P, 1, C.r30)
                v = [res[0] + rng.randint(0, (C.in_x - res[0]) // p) * p, res[1] + rng.randint(0, (C.in_y - res[1]) // p) * p, C.r30, C.r30]
            else:
                v = shaped(C, P, rng, ka)
            if mm and isinstance(ka, list) and not isinstance(a, tuple):
                continue                                          # those representations have a free l: not an affine accumulator
            flip = rng.randint(0, 1)
            aq = ev.aff30(C, Q) if Q else [rng.randrange(p), rng.randrange(p)]
            if Q and not isinstance(a, tuple) and rng.random() < 0.3:   # X2, Y2 "< 1": a product's result, up to p + eps - 1
                aq = [x + p if x + p <= C.in_aff else x for x in aq]
            u2 = (aq[0] if mm else Q[0] * v[2] % p) if (P and Q) else None      # what stands against X1 in Pp = U2 - X1 + 6p
            m = dict(flip=flip, inf=P is None, x_top=bool(P and Q and v[0] >= 5 * p and u2 < v[0] - 5 * p))
            if P is None or Q is None:
                m.update(want=Q if not fast else None, key=None, ret=0 if fast else 1, same=fast, copy=not fast)
            elif P[0] == Q[0]:
                m.update(want=ev.ec_add(C, P, Q), key="double", ret=0 if fast else 1, same=fast, newflip=flip)
            else:
                m.update(want=ev.ec_neg(C, ev.ec_add(C, P, Q)), key="madd_flip", ret=1, same=False, newflip=1 - flip)

            def setup(r, v=v, aq=aq, flip=flip, P=P, Q=Q):
                ev.put30(r, 0, v)
                ev.put30(r, 36, aq)
                r[ev.F_INF], r[ev.F_FLIP], r[ev.F_AINF] = int(P is None), flip, int(Q is None)
            add(m, setup)
    elif op == "xyzz30_flip_finish":
        for i in range(SWEEP // 2):
            P = elem(C, rng.randint(1, 40))
            v = shaped(C, P, rng, "yneg_top" if i >= 40 and i % 16 == 2 else (KINDS[i % 5] if i < 40 else "rand"), y_max=C.in_y_neg)
            flip, inf = (i >> 1) & 1, int(i % 11 == 0)
            add(dict(want=None if inf else (ev.ec_neg(C, P) if flip else P), same=inf or not flip, vin=v,
                     yneg_top=bool(flip and not inf and is_yneg_top(C, v[1]))),
                lambda r: (ev.put30(r, 0, v), r.__setitem__(ev.F_FLIP, flip), r.__setitem__(ev.F_INF, inf)))
    elif op in ("xyzz30_add", "xyzz30_add_mem", "xyzz30_add_one_lane", "xyzz30_add_quad", "xyzz30_add_quadreg"):
        mem = op != "xyzz30_add"
        quadreg = op == "xyzz30_add_quadreg"
        cases = pair_cases(C, rng, SWEEP, with_inf=not quadreg)
        pinned = {}
        if op == "xyzz30_add_quad":
            cases, pinned = quad_waves(cases, rng)
        if op in ("xyzz30_add_mem", "xyzz30_add_quadreg"):
            # the negated operand's Y at the top of what 4p - Y accepts (neg forced below); and equal x together with the
            # endomorphism: the first operand is phi(k G) itself, so P + phi(Q) doubles and, through neg, P - phi(Q) vanishes
            cases += [(a, b, ka, "yneg_top") for a, b in ((3, 5), (4, 4), (6, -6), (9, 2)) for ka in ("top", "rand")]
            cases += [(("phi", k), sg * k, ka, kb) for k in (4, 7, 11) for sg in (1, -1) for ka in ("min", "top", "rand") for kb in ("top", "rand")]
        for idx, (a, b, ka, kb) in enumerate(cases):
            P, Q = elem(C, a), elem(C, b)
            neg = rng.randint(0, 1) if op in ("xyzz30_add_mem", "xyzz30_add_quadreg") else 0
            phi = rng.randint(0, 1) if op in ("xyzz30_add_mem", "xyzz30_add_quadreg") else 0
            if kb == "yneg_top":
                neg = 1
            if isinstance(a, tuple):
                phi = 1
            final = rng.randint(0, 1) if op in ("xyzz30_add_one_lane", "xyzz30_add_quad") else 0
            live = int(rng.random() < 0.85) if op == "xyzz30_add_quad" else 1
            alias = int(rng.random() < 0.3) if op == "xyzz30_add_quad" else 0
            if idx in pinned:                                     # the named wave layouts do not depend on the seed
                live, alias = pinned[idx]
            vp = shaped(C, P, rng, ka, mem=mem and not quadreg)
            vq = shaped(C, Q, rng, kb, y_max=C.in_y_neg if neg else None, mem=mem)
            Qe = Q
            vqx = None
            if phi and Q is not None:
                Qe = ev.ec_phi(C, Q)
                if quadreg:                                       # the table of X scaled by beta: the same l, its own multiple
                    vqx = vq[0] * C.beta % p
                    vqx += rng.randint(0, (min(C.in_x, (1 << 256) - 1) - vqx) // p) * p if C is BN254 else 0
            if neg:
                Qe = ev.ec_neg(C, Qe)
            want = ev.ec_add(C, P, Qe)
            eqx = P is not None and Qe is not None and P[0] == Qe[0]
            m = dict(want=want, eqx=eqx, pinf=P is None, qinf=Q is None, final=final, live=live, alias=alias, vp=vp,
                     key="double" if (eqx and want) else "add", phi=phi,
                     yneg_top=bool(neg and Q is not None and is_yneg_top(C, vq[1])))

            def setup(r, vp=vp, vq=vq, vqx=vqx, P=P, Q=Q, neg=neg, phi=phi, final=final, live=live, alias=alias):
                if op == "xyzz30_add":
                    ev.put30(r, 0, vp), ev.put30(r, 36, vq)
                elif quadreg:
                    ev.put30(r, 0, vp), ev.put_words(r, 40, vq)
                    if vqx is not None:
                        ev.put_words(r, 72, [vqx])
                    r[ev.F_SEPX] = int(vqx is not None)
                else:
                    ev.put_words(r, 0, vp), ev.put_words(r, 32, vq)
                r[ev.F_INF], r[ev.F_INF2], r[ev.F_NEG], r[ev.F_PHI] = int(P is None), int(Q is None), neg, phi
                r[ev.F_FINAL], r[ev.F_LIVE], r[ev.F_ALIAS] = final, live, alias
            add(m, setup)
    elif op == "xyzz30_to_xyzz":
        for i in range(SWEEP // 2):
            P = elem(C, rng.randint(0, 40) if i % 13 else 0)
            v = shaped(C, P, rng, KINDS[i % 5] if i < 40 else "rand")
            add(dict(want=P), lambda r: (ev.put30(r, 0, v), r.__setitem__(ev.F_INF, int(P is None))))
    elif op == "xyzz30_store_load_lazy":
        for i in range(SWEEP // 2):
            P = elem(C, rng.randint(0, 40) if i % 13 else 0)
            v = shaped(C, P, rng, KINDS[i % 5] if i < 40 else "rand")
            add(dict(want=P, vin=v, raw=False), lambda r: (ev.put30(r, 0, v), r.__setitem__(ev.F_INF, int(P is None))))
        if C is SECP:                                             # residues around 2^256 and p before the store
            xy = [(1 << 256) - 1, 1 << 256, (1 << 256) + (1 << 49), p, p + 1, 2 * p - 1, C.in_x, 4 * p]
            # ZZ / ZZZ go to f30_to_fe_canonical unfolded: a product's result, below 2^256 + 2^49
            zz = [(1 << 256) - 1, 1 << 256, (1 << 256) + (1 << 49) - 1, p + 1, p + 2, p - 1, 1]
            for i in range(len(xy) * len(zz)):
                v = [xy[i % len(xy)], xy[(i // 2) % len(xy)], zz[i % len(zz)], zz[(i // 3) % len(zz)]]
                add(dict(want="raw", vin=v, raw=True), lambda r: ev.put30(r, 0, v))
    elif op in ("xyzz30_double_mem", "xyzz30_dbl_quad"):
        quad = op == "xyzz30_dbl_quad"
        for i in range(SWEEP // 2 + 64):
            P = elem(C, rng.randint(1, 40) if i % 9 else 0)
            v = shaped(C, P, rng, KINDS[i % 5] if i < 60 else "rand", mem=True)
            times = 1 if quad else [0, 1, 2, 30][i % 4]
            live, alias = (int(rng.random() < 0.85), i % 3 == 0) if quad else (1, 1)
            add(dict(want=ev.ec_mul(C, 1 << times, P) if P else None, times=times, live=live, alias=alias, pinf=P is None, vp=v),
                lambda r: (ev.put_words(r, 0, v), r.__setitem__(ev.F_TIMES, times), r.__setitem__(ev.F_LIVE, live),
                           r.__setitem__(ev.F_ALIAS, int(alias))))
    elif op == "xyzz30_quadreg_ladder":
        for i in range(96):
            P = elem(C, rng.randint(1, 40))
            steps = 40 if i < 48 else rng.randint(1, 48)
            bits = rng.getrandbits(steps)
            neg = i & 1
            vc = shaped(C, P, rng, "rand")
            vq = shaped(C, ev.ec_neg(C, P) if neg else P, rng, "yneg_top" if neg and i % 4 == 1 else "rand", y_max=C.in_y_neg, mem=True)
            add(dict(want=ev.ec_mul(C, (1 << steps) | bits, P), key="add", yneg_top=bool(neg and bits and is_yneg_top(C, vq[1]))),
                lambda r: (ev.put30(r, 0, vc), ev.put_words(r, 40, vq), r.__setitem__(ev.F_TIMES, steps), r.__setitem__(ev.F_NEG, neg),
                           r.__setitem__(ev.F_BITS0, bits & 0xffffffff), r.__setitem__(ev.F_BITS1, bits >> 32)))
    return np.stack(rows), metas


def quad_waves(cases, rng):
    """the order of the file decides which 16 quads share a wave: mixed waves in several orders, the exceptional quad first,
    last, and sixteen exceptional quads together; then the sweep as it comes"""
    ordinary = [c for c in cases if c[0] and c[1] and abs(c[0]) != abs(c[1])]
    special = [c for c in cases if not (c[0] and c[1] and abs(c[0]) != abs(c[1]))]
    waves = []
    waves.append([special[0]] + ordinary[:15])
    waves.append(ordinary[15:30] + [special[1]])
    waves.append(special[2:18])
    for w in range(6):
        mix = special[18 + 3 * w: 21 + 3 * w] + ordinary[30 + 13 * w: 43 + 13 * w]
        rng.shuffle(mix)
        waves.append(mix)
    assert all(len(w) == 16 for w in waves)
    named = [c for w in waves for c in w]
    # every exceptional quad of these layouts is live (its result is stored and compared); a fixed few ordinary quads are not
    pinned = {i: (0 if (c in ordinary and i % 8 == 5) else 1, int(i % 3 == 0)) for i, c in enumerate(named)}
    return named + cases, pinned


def check_point_op(C, op, recs, out, metas, counter, one_lane=None):
    p = C.p
    for i, m in enumerate(metas):
        where = "%s %s record %d" % (C.name, op, i)
        row, rec = out[i], recs[i]
        assert np.array_equal(row[:A0], rec[:A0]), where + ": flags changed"
        if op in ("xyzz30_double_affine", "xyzz30_double", "xyzz30_dbl_quadreg"):
            ev.check_point30(C, row, m["want"], m["key"], where, inf=0 if op == "xyzz30_dbl_quadreg" else None)
        elif op in ("xyzz30_madd_flip", "xyzz30_madd_flip_fast", "xyzz30_mmadd_flip_fast"):
            assert int(row[FO]) == m["ret"], where + ": returned %d" % int(row[FO])
            if m["same"]:                                         # a false return leaves p and flip bit-identical
                assert same_bits(row, rec) and int(row[FO + 1]) == int(m["inf"]) and int(row[FO + 2]) == m["flip"], where + ": touched"
            elif m.get("copy"):                                   # the first point: (ax, ay, unit, unit), no flip
                assert int(row[FO + 1]) == 0 and int(row[FO + 2]) == m["flip"], where
                assert np.array_equal(row[O0:O0 + 18], rec[A0 + 36:A0 + 54]) and ev.get30(row, O0 + 18, 2) == [C.r30, C.r30], where
            else:
                assert int(row[FO + 2]) == m["newflip"], where + ": flip"
                ev.check_point30(C, row, m["want"], m["key"], where)
        elif op == "xyzz30_flip_finish":
            if m["same"]:
                assert same_bits(row, rec), where
            else:
                assert np.array_equal(row[O0:O0 + 9], rec[A0:A0 + 9]) and np.array_equal(row[O0 + 18:O0 + 36], rec[A0 + 18:A0 + 36]), where
                ev.check_point30(C, row, m["want"], "flip_finish", where, inf=0)
        elif op == "xyzz30_add":
            if m["qinf"]:
                assert same_bits(row, rec) and int(row[FO + 1]) == int(m["pinf"]), where
            elif m["pinf"]:
                assert np.array_equal(row[O0:O0 + 36], rec[A0 + 36:A0 + 72]) and int(row[FO + 1]) == 0, where
            else:
                ev.check_point30(C, row, m["want"], m["key"], where)
        elif op == "xyzz30_to_xyzz":
            ev.check_point_mem(C, row[O0:O0 + 32], m["want"], None, where, final=True)
        elif op == "xyzz30_store_load_lazy":
            stored, loaded = ev.get_words(row, O0), ev.get30(row, O0 + 32)
            if m["raw"] or m["want"] is not None:
                want = [v % p for v in m["vin"]] if C is SECP else m["vin"]
                assert stored == want and loaded == want, where
                ev.check_form(C, row, O0 + 32, 4, where)
                assert int(row[FO + 1]) == int(stored[2] == 0), where
                if not m["raw"]:
                    assert stored[2] != 0, where + ": finite point stored with an all-zero ZZ"
                    ev.check_element(C, loaded, m["want"], where)
            else:
                assert not row[O0:O0 + 32].any() and int(row[FO + 1]) == 1, where
        elif op in ("xyzz30_add_mem", "xyzz30_double_mem"):
            assert np.array_equal(row[A0 + 32:FO], rec[A0 + 32:FO]), where + ": second operand changed"
            key = m.get("key", "double")
            if m["pinf"] or m.get("qinf") or m.get("times") == 0:
                key = "operand"                                   # the other operand (negated / scaled), stored again
            if op == "xyzz30_double_mem" and (m["pinf"] or m["times"] == 0):
                assert np.array_equal(row[A0:A0 + 32], rec[A0:A0 + 32]), where + ": not the same bytes"
            ev.check_point_mem(C, row[A0:A0 + 32], m["want"], key, where)
        elif op in ("xyzz30_add_one_lane", "xyzz30_add_quad", "xyzz30_dbl_quad"):
            res = row[A0:A0 + 32] if m["alias"] else row[O0:O0 + 32]
            if not m["live"]:                                     # computed but not stored
                assert np.array_equal(row, rec), where + ": a quad that is not live stored something"
            else:
                if not m["alias"]:
                    assert np.array_equal(row[A0:A0 + 32], rec[A0:A0 + 32]), where + ": first operand changed"
                assert np.array_equal(row[A0 + 32:FO], rec[A0 + 32:FO]), where + ": second operand changed"
                key = m.get("key", "double")
                if m["pinf"] or m.get("qinf"):
                    key = "operand"
                ev.check_point_mem(C, res, m["want"], key, where, final=bool(m.get("final")))
                if one_lane is not None:
                    ref = one_lane[i][A0:A0 + 32] if op == "xyzz30_dbl_quad" else one_lane[i][O0:O0 + 32]
                    # the comment above xyzz30_add_quad's lane table: exceptional operands go to one lane's ordinary addition; inside
                    # xyzz30_add_quad: an infinite operand is copied in the memory form, which is what a load and a store of it give
                    if op == "xyzz30_add_quad" and (m["eqx"] or m["pinf"] or m["qinf"]):
                        assert np.array_equal(res, ref), where + ": bytes differ from the one-lane form"
                    elif m["want"] is None:
                        assert not res.any() and not ref.any(), where
                    else:
                        f = m.get("final")
                        a, b = ev.get_words(res, 0), ev.get_words(ref, 0)
                        assert a[0] * b[2] % p == b[0] * a[2] % p and a[1] * b[3] % p == b[1] * a[3] % p, where + ": one-lane form disagrees"
        elif op == "xyzz30_add_quadreg":
            assert int(row[FO]) == int(not m["eqx"]), where + ": returned %d" % int(row[FO])
            if m["eqx"]:
                assert same_bits(row, rec), where + ": c touched on a false return"
            else:
                ev.check_point30(C, row, m["want"], m["key"], where, inf=0)
        elif op == "xyzz30_quadreg_ladder":
            assert int(row[FO]) == 1, where + ": a step met equal x"
            ev.check_point30(C, row, m["want"], m["key"], where, inf=0)
        counter.checked += 1


# 4p - Y of a Y in [3p, 3p + eps]: the register forms on both curves; the memory-form operands of secp256k1 are canonical by the
# header (below p), so there the case does not exist for xyzz30_add_mem, xyzz30_add_quadreg and the ladder's table point
YNEG_TOP_REQUIRED = {("xyzz30_flip_finish", "bn254"), ("xyzz30_flip_finish", "secp256k1"), ("xyzz30_add_mem", "bn254"),
                     ("xyzz30_add_quadreg", "bn254"), ("xyzz30_quadreg_ladder", "bn254")}


# ================================================================ one process per curve for every one-shot operation
@functools.lru_cache(maxsize=None)
def batch(curve):
    C = ev.CURVES[curve]
    jobs, metas = [], {}
    for n, op in enumerate(FIELD_OPS + POINT_OPS):
        if op == "f30_pm_reduce" and C is not SECP:
            continue
        rng = random.Random(1000 + n)
        recs, m = gen_field(C, op, rng) if op in FIELD_OPS else gen_point_op(C, op, rng)
        jobs.append((op, recs))
        metas[op] = m
    # the quad forms' records once more through the one-lane forms
    jobs.append(("xyzz30_add_one_lane", dict(jobs)["xyzz30_add_quad"]))
    jobs.append(("xyzz30_double_mem", dict(jobs)["xyzz30_dbl_quad"]))
    outs = ev.run(C, jobs)
    res = {op: (recs, out, metas[op]) for (op, recs), out in zip(jobs[:-2], outs[:-2])}
    res["one_lane:xyzz30_add_quad"], res["one_lane:xyzz30_dbl_quad"] = outs[-2], outs[-1]
    return res


# f30_pm_reduce belongs to the special-form modulus only: there is no BN254 instance to test
FIELD_CASES = [(c, op) for c in CURVE_NAMES for op in FIELD_OPS if not (op == "f30_pm_reduce" and c != "secp256k1")]


@pytest.mark.parametrize("curve,op", FIELD_CASES, ids=["%s-%s" % co for co in FIELD_CASES])
def test_field_helper(curve, op):
    C = ev.CURVES[curve]
    recs, out, want = batch(curve)[op]
    counter = ev.Counter()
    check_field(C, op, out, want, counter)
    assert counter.checked == len(want) == recs.shape[0] > 0


@pytest.mark.parametrize("op", POINT_OPS)
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_group_operation(curve, op):
    C = ev.CURVES[curve]
    b = batch(curve)
    recs, out, metas = b[op]
    counter = ev.Counter()
    check_point_op(C, op, recs, out, metas, counter, one_lane=b.get("one_lane:" + op))
    assert counter.checked == len(metas) == recs.shape[0] > 0
    # the vectors the random sweep would only meet by luck are present, whatever the seed
    if (op, curve) in YNEG_TOP_REQUIRED:
        assert sum(1 for m in metas if m.get("yneg_top")) >= 1, "no negated Y in [3p, 3p + eps]"
    if op in ("xyzz30_add_mem", "xyzz30_add_quadreg"):
        assert sum(1 for m in metas if m["phi"] and m["eqx"] and m["want"] is None) >= 1, "no P - phi(Q) with equal x"
        assert sum(1 for m in metas if m["phi"] and m["eqx"] and m["want"] is not None) >= 1, "no P + phi(Q) with equal x"
    if curve == "bn254" and op in ("xyzz30_madd_flip", "xyzz30_madd_flip_fast", "xyzz30_mmadd_flip_fast"):
        assert sum(1 for m in metas if m["x_top"] and m["ret"] == 1 and not m["same"]) >= 4, "no X1 = 5p + t meeting U2 < t"
    if op == "xyzz30_add_quad":
        named = metas[:144]
        assert all(m["live"] for m in named if m["eqx"] or m["pinf"] or m["qinf"])
        assert (named[0]["eqx"] or named[0]["pinf"] or named[0]["qinf"]) and (named[31]["eqx"] or named[31]["pinf"] or named[31]["qinf"])
        assert all(m["eqx"] or m["pinf"] or m["qinf"] for m in named[32:48])


# ================================================================ sign-alternating chains
@pytest.mark.parametrize("form", ["xyzz30_madd_flip", "xyzz30_madd_flip_fast", "xyzz30_mmadd_flip_fast"])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_sign_alternating_chain(curve, form):
    """chains of 1..9 additions into one accumulator as the accumulation loops run them: the test negates the incoming point
    with xyzz30_flip_neg's rule (digit sign != flip), tries the fast form first where `form` is one and finishes the step with
    the general form on a false return, ends with xyzz30_flip_finish.  One element of a chain repeats the accumulated sum and
    one is its negative.  The chain's sum must equal the Python sum."""
    C = ev.CURVES[curve]
    rng = random.Random(77)
    G = ev.multiples(C)
    chains = []
    for length in range(1, 10):
        for variant in range(6):
            ks, total = [], 0
            for s in range(length):
                k = rng.randint(1, 6) * rng.choice([1, 1, -1])
                if variant >= 2 and s == 2 and total not in (0,) and abs(total) <= 40:
                    k = total                                     # repeats the accumulated sum: P + P inside the chain
                if variant >= 3 and s == 4 and total != 0 and abs(total) <= 40:
                    k = -total                                    # its negative: the accumulator becomes infinity
                if abs(total + k) > 40:
                    k = -k
                ks.append(k)
                total += k
            chains.append(ks)
    n = len(chains)
    acc = ev.new_records(n)                                       # the accumulators, in the layout of the operations' operands
    inf, flip = [1] * n, [0] * n
    steps_done = 0
    for s in range(9):
        live = [c for c in range(n) if len(chains[c]) > s]
        recs = ev.new_records(len(live))
        for j, c in enumerate(live):
            Q = elem(C, chains[c][s])
            if flip[c]:                                           # xyzz30_flip_neg(false, flip): the point goes in negated
                Q = ev.ec_neg(C, Q)
            recs[j, A0:A0 + 36] = acc[c, A0:A0 + 36]
            ev.put30(recs[j], 36, ev.aff30(C, Q))
            recs[j, ev.F_INF], recs[j, ev.F_FLIP] = inf[c], flip[c]
        outs = ev.run(C, [("xyzz30_madd_flip", recs), ("xyzz30_madd_flip_fast", recs), ("xyzz30_mmadd_flip_fast", recs)])
        general, fastf, mmf = outs
        for j, c in enumerate(live):
            use, tried_fast = general[j], form != "xyzz30_madd_flip"
            if form == "xyzz30_madd_flip_fast":
                use = fastf[j]
            elif form == "xyzz30_mmadd_flip_fast":                # only an accumulator that was just copied in is affine
                zz = ev.get30(recs[j], A0 + 18, 2)
                use = mmf[j] if (not inf[c] and zz == [C.r30, C.r30]) else fastf[j]
            if tried_fast and int(use[FO]) == 0:       # the fast form declined: p and flip untouched, the general form finishes
                assert same_bits(use, recs[j]) and int(use[FO + 2]) == flip[c] and int(use[FO + 1]) == inf[c]
                use = general[j]
            acc[c, A0:A0 + 36] = use[O0:O0 + 36]
            inf[c], flip[c] = int(use[FO + 1]), int(use[FO + 2])
            steps_done += 1
    for c in range(n):
        acc[c, ev.F_INF], acc[c, ev.F_FLIP] = inf[c], flip[c]
    fin = ev.run(C, [("xyzz30_flip_finish", acc)])[0]
    checked = 0
    for c in range(n):
        want = elem(C, sum(chains[c]))
        ev.check_point30(C, fin[c], want, "flip_finish", "%s chain %d %s" % (curve, c, chains[c]), inf=inf[c])
        checked += 1
    assert checked == n and steps_done == sum(len(c) for c in chains)
    assert any(sum(c[:3]) == 2 * sum(c[:2]) for c in chains if len(c) > 2) and any(sum(c[:5]) == 0 for c in chains if len(c) > 4)


# ================================================================ the two representations agree
@pytest.mark.parametrize("op", ev.OPS32)
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_ec_hip_h_on_the_device(curve, op):
    """the 8 x 32-bit forms on the device: the vectors of tests/test_ec_host_cpu.py; CALL = false and true give identical words"""
    C = ev.CURVES[curve]
    recs, want = ev.gen32(C, op, 1500, seed=32)
    plain, call = ev.run(C, [(op, recs), (op + "_call", recs)])
    counter = ev.Counter()
    ev.check32(C, op, plain, want, counter)
    assert counter.checked == len(want) == recs.shape[0]
    assert np.array_equal(plain, call), "CALL = false and CALL = true disagree"


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_cross_form_agreement(curve):
    """xyzz_add / xyzz_madd of ec.hip.h and xyzz30_add / xyzz30_madd_flip give the same affine point on the same group-level
    inputs (each in its own representation)"""
    C = ev.CURVES[curve]
    rng = random.Random(5)
    p = C.p
    cases = [(a, b) for a, b, _, _ in pair_cases(C, rng, 600)]
    r32a, r32m, r30a, r30m = [ev.new_records(len(cases)) for _ in range(4)]
    for i, (a, b) in enumerate(cases):
        P, Q = elem(C, a), elem(C, b)
        l, l2 = rng.randrange(1, p), rng.randrange(1, p)
        z32 = [1, 1, 0, 0]
        ev.put_words(r32a[i], 0, ev.rep32(C, P, l) if P else z32), ev.put_words(r32a[i], 32, ev.rep32(C, Q, l2) if Q else z32)
        ev.put_words(r32m[i], 0, ev.rep32(C, P, l) if P else z32)
        ev.put_words(r32m[i], 32, [Q[0] * C.r32 % p, Q[1] * C.r32 % p] if Q else [0, 0])
        ev.put30(r30a[i], 0, shaped(C, P, rng, "rand")), ev.put30(r30a[i], 36, shaped(C, Q, rng, "rand"))
        r30a[i, ev.F_INF], r30a[i, ev.F_INF2] = int(P is None), int(Q is None)
        ev.put30(r30m[i], 0, shaped(C, P, rng, "rand"))
        ev.put30(r30m[i], 36, ev.aff30(C, Q if Q else C.g))
        r30m[i, ev.F_INF] = int(P is None)
    o32a, o32m, o30a, o30m = ev.run(C, [("xyzz_add", r32a), ("xyzz_madd", r32m), ("xyzz30_add", r30a), ("xyzz30_madd_flip", r30m)])

    def affine(vals, inf):
        return None if inf else (vals[0] * pow(vals[2], -1, p) % p, vals[1] * pow(vals[3], -1, p) % p)
    checked = 0
    for i, (a, b) in enumerate(cases):
        want = ev.ec_add(C, elem(C, a), elem(C, b))
        got = [affine(ev.get_words(o32a[i], O0), int(o32a[i][FO + 1])), affine(ev.get30(o30a[i], O0), int(o30a[i][FO + 1]))]
        assert got[0] == got[1] == want, "%s add %d: %s" % (curve, i, got)
        if b != 0:                                               # the mixed forms take a finite point
            m30 = affine(ev.get30(o30m[i], O0), int(o30m[i][FO + 1]))
            if int(o30m[i][FO + 2]):
                m30 = ev.ec_neg(C, m30)
            assert affine(ev.get_words(o32m[i], O0), int(o32m[i][FO + 1])) == m30 == want, "%s madd %d" % (curve, i)
        checked += 1
    assert checked == len(cases)

"""Vectors and expected values for the per-operation checks of the group law (tools/ec30_check.hip): shared by
tests/test_ec30_gpu.py and tests/test_ec_host_cpu.py.

Every expected value is a Python integer computed here: affine chord-and-tangent arithmetic with pow(x, -1, p), the
endomorphism (x, y) -> (beta x, y), scalar multiples by double-and-add.  Nothing comes from the project's C++ or from the
oracle library's group law; oracle/bn254_py.py supplies the BN254 constants only.  Generation is deterministic (fixed seeds)
and reads nothing outside the repository.

RESIDUE CONVENTION (stated once): a residue x travels as  x * 2^270 mod p  in the 9 x 30-bit form of BN254 (Montgomery radix
2^270), as x itself for secp256k1 (special-form modulus: plain residues in both forms), and as  x * 2^256 mod p  in the 8 x 32-bit
Montgomery form of ec.hip.h (again x itself for secp256k1).  A product in a form with factor R is  a b / R.

An XYZZ operand of the group element (x, y) is (x l^2 + i p, y l^3 + j p, l^2 + k p, l^3 + m p) in that form: l a free non-zero
scalar, i, j, k, m free multiples within the bound the header states for that operand.
"""
import os
import random
import subprocess
import tempfile

import numpy as np

from oracle import bn254_py
from tests import common

EXE = os.path.join(common.ROOT, "porla_amd", "ec30_check")

# record layout of tools/ec30_check.hip
REC, A0, FO, O0 = 192, 16, 96, 112
F_INF, F_FLIP, F_NEG, F_PHI, F_AINF, F_FINAL, F_LIVE, F_TIMES, F_ALIAS, F_INF2, F_SEPX, F_BITS0, F_BITS1 = range(13)
SENTINEL = 0xA5A5A5A5          # what the result area holds before the operation: an untouched result is visible
MASK30 = (1 << 30) - 1


class Curve:
    def __init__(self, name, p, b, g, beta, r30, r32, top_bits, eps, eps2):
        self.name, self.p, self.b, self.g, self.beta = name, p, b, g, beta
        self.r30, self.r32 = r30 % p, r32 % p        # the factor of the 9 x 30 form and of the 8 x 32 form
        self.r30_inv = pow(self.r30, -1, p)
        self.top_bits = top_bits                     # a normal operand's limb 8 is below 2^top_bits
        self.eps, self.eps2 = eps, eps2              # a product's result is < p + eps, a two-product result < p + eps2
        self.one = 1                                 # slack of an inclusive bound: value <= k p
        # operand bounds of the group law (inclusive), the header comment of ec30.hip.h: "X1 <= 5, Y1 <= 4, ZZ1, ZZZ1 <= 1, X2, Y2 < 1"
        self.in_x = 5 * p + eps - 1
        self.in_y = 4 * p
        self.in_z = p + eps - 1
        self.in_aff = p + eps - 1
        # a Y that is negated by 4p - Y (f30_sub<4>: b <= 3p + slack) in xyzz30_flip_finish, xyzz30_add_mem, xyzz30_add_quadreg
        # and quad30.hip.h:macq_add
        self.in_y_neg = 3 * p + eps


BN254 = Curve("bn254", bn254_py.P, 3, (1, 2), 0x30644e72e131a0295e6dd9e7e0acccb0c28f069fbb966e3de4bd44e5607cfd48,
              1 << 270, 1 << 256, 18, 1 << 246, 1 << 247)
_SP = 2**256 - 2**32 - 977
# secp256k1: the issue's bound "< 2^256 + 2^73" for every product result
SECP = Curve("secp256k1", _SP, 7,
             (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
              0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8),
             0x7ae96a2b657c07106e64479eac3434e99cf0497512f58995c1396c28719501ee,
             1, 1, 19, 2**256 + 2**73 - _SP, 2**256 + 2**73 - _SP)
CURVES = {"bn254": BN254, "secp256k1": SECP}

# Output bounds, keyed by operation: (X, Y, ZZ / ZZZ) as (multiple of p, slack) -> value < multiple * p + slack, where slack is
# "eps" (one product) or "eps2" (the two-product reduction): a - b + K p of a product result a is below (K + 1) p + eps.  Each restates
# a line of porla_amd/csrc/ec30.hip.h.
BOUNDS = {
    # header comment: X3 = RR - E + 4p <= 5;  Y3 <= 1 as one two-product reduction;  products <= 1
    # (xyzz30_madd_flip, xyzz30_madd_flip_fast, xyzz30_mmadd_flip_fast)
    "madd_flip": ((5, "eps"), (1, "eps2"), (1, "eps")),
    # xyzz30_double_affine: "X3 <= 4", "Y3 <= 3";  the comment above xyzz30_double_body says the same
    # (xyzz30_double, xyzz30_double_mem, xyzz30_dbl_quad, xyzz30_dbl_quadreg)
    "double": ((4, "eps"), (3, "eps"), (1, "eps")),
    # the comment above xyzz30_add: X3 <= 5, Y3 = ... + 2p <= 3 (xyzz30_add, xyzz30_add_mem, xyzz30_add_one_lane and the
    # quad forms xyzz30_add_quad / xyzz30_add_quadreg with the same formulas)
    "add": ((5, "eps"), (3, "eps"), (1, "eps")),
    # the comment above xyzz30_flip_finish: "Y -> 4p - Y (<= 4p)"; X, ZZ, ZZZ are the operand's
    "flip_finish": ((5, "eps"), (4, "one"), (1, "eps")),
    # an operand that passes through (the other one is infinity, `times` = 0), possibly negated in xyzz30_add_mem
    # ("4p - Y <= 4p: fine as an operand")
    "operand": ((5, "eps"), (4, "one"), (1, "eps")),
}
NOT_NEGATED = ("flip_finish", "operand")      # a Y up to 4p: consumed by additions and doublings, never by another 4p - Y


def bound(C, entry):
    k, slack = entry
    return k * C.p + getattr(C, slack)


# ---------------------------------------------------------------- the group law on Python integers
def ec_neg(C, a):
    return None if a is None else (a[0], (-a[1]) % C.p)


def ec_add(C, a, b):
    p = C.p
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % p == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, p) % p
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, p) % p
    x = (lam * lam - a[0] - b[0]) % p
    return (x, (lam * (a[0] - x) - a[1]) % p)


def ec_mul(C, k, a):
    r = None
    for bit in bin(k)[2:]:
        r = ec_add(C, r, r)
        if bit == "1":
            r = ec_add(C, r, a)
    return r


def ec_phi(C, a):
    return None if a is None else (C.beta * a[0] % C.p, a[1])


def on_curve(C, a):
    return (a[1] * a[1] - a[0] ** 3 - C.b) % C.p == 0


_MULTIPLES = {}


def multiples(C, n=48):
    """[None, G, 2G, ..., nG]"""
    if C.name not in _MULTIPLES:
        t = [None]
        for _ in range(n):
            t.append(ec_add(C, t[-1], C.g))
        _MULTIPLES[C.name] = t
    return _MULTIPLES[C.name]


def sqrt_mod(C, a):
    s = pow(a, (C.p + 1) // 4, C.p)           # both moduli are 3 mod 4
    return s if s * s % C.p == a % C.p else None


def cbrt_mod(C, a):
    """a cube root for p = 7 mod 9 (secp256k1), None when a is not a cube"""
    assert C.p % 9 == 7
    s = pow(a, (C.p + 2) // 9, C.p)
    return s if pow(s, 3, C.p) == a % C.p else None


# ---------------------------------------------------------------- limbs and words
def limbs(v):
    """9 x 30-bit limbs; everything from bit 240 up sits in limb 8"""
    return [(v >> (30 * i)) & MASK30 for i in range(8)] + [v >> 240]


def limbs_value(l):
    return sum(int(x) << (30 * i) for i, x in enumerate(l))


def words(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def words_value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def new_records(n):
    r = np.zeros((n, REC), dtype=np.uint32)
    r[:, FO:] = SENTINEL
    return r


def put30(rec, at, vals):
    for k, v in enumerate(vals):
        rec[A0 + at + 9 * k: A0 + at + 9 * k + 9] = limbs(v)


def put_words(rec, at, vals):
    for k, v in enumerate(vals):
        rec[A0 + at + 8 * k: A0 + at + 8 * k + 8] = words(v)


def get30(row, base, count=4):
    return [limbs_value(row[base + 9 * k: base + 9 * k + 9]) for k in range(count)]


def get_words(row, base, count=4):
    return [words_value(row[base + 8 * k: base + 8 * k + 8]) for k in range(count)]


# ---------------------------------------------------------------- representations of a group element
def residues(C, pt, l, factor):
    p = C.p
    return [pt[0] * l * l * factor % p, pt[1] * l ** 3 * factor % p, l * l * factor % p, l ** 3 * factor % p]


def rep30(C, pt, l, mult=None, y_max=None, rng=None):
    """register form: values within (in_x, in_y, in_z, in_z); mult = the multiples of p, "top" = as many as fit, None = random"""
    res = residues(C, pt, l, C.r30)
    lim = [C.in_x, y_max if y_max is not None else C.in_y, C.in_z, C.in_z]
    room = [(b - r) // C.p for r, b in zip(res, lim)]
    if mult == "top":
        mult = room
    elif mult is None:
        mult = [rng.randint(0, m) for m in room]
    vals = [r + m * C.p for r, m in zip(res, mult)]
    assert all(0 <= v <= b for v, b in zip(vals, lim)), "operand outside the header's bound"
    return vals


def rep_mem(C, pt, l, mult=None, y_max=None, rng=None):
    """lazy memory form: BN254 as the register form (everything below 2^256), secp256k1 canonical; infinity = zeros"""
    if pt is None:
        return [0, 0, 0, 0]
    if C is SECP:
        return residues(C, pt, l, 1)
    v = rep30(C, pt, l, mult, y_max, rng)
    assert all(x < 1 << 256 for x in v)
    return v


def rep32(C, pt, l):
    """8 x 32-bit Montgomery form of ec.hip.h: canonical residues"""
    return residues(C, pt, l, C.r32)


def aff30(C, pt, lift=0):
    return [pt[0] * C.r30 % C.p + lift * C.p, pt[1] * C.r30 % C.p + lift * C.p]


def find_l(C, pt, coord, want, rng):
    """an l whose residue of coordinate `coord` (0 X, 2 ZZ) equals `want`, walking `want` down until a square root exists"""
    num = pt[0] if coord == 0 else 1
    while True:
        l = sqrt_mod(C, want * pow(num * C.r30, -1, C.p) % C.p)
        if l:
            return l, want
        want -= 1
        assert want > 0


def find_l_high(C, pt, coord, rng, tries=4096):
    """an l whose residue of coordinate `coord` is within 2^-6 of p (the value then sits just under a multiple of p)"""
    for _ in range(tries):
        l = rng.randrange(1, C.p)
        if residues(C, pt, l, C.r30)[coord] > C.p - (C.p >> 6):
            return l
    raise AssertionError("no l found")


# ---------------------------------------------------------------- checks shared by every operation
class Counter:
    """every generated record is checked: the tests assert checked == generated"""
    def __init__(self):
        self.checked = 0


def check_form(C, row, base, count, where):
    for k in range(count):
        l = [int(x) for x in row[base + 9 * k: base + 9 * k + 9]]
        assert all(x < 1 << 30 for x in l[:8]), "%s: residue %d has a limb >= 2^30: %s" % (where, k, l)
        assert l[8] < 1 << C.top_bits, "%s: residue %d limb 8 = %#x" % (where, k, l[8])


def check_element(C, vals, want, where):
    """X / ZZ, Y / ZZZ equal the Python point; ZZ^3 = ZZZ^2 in the stated form"""
    p = C.p
    X, Y, ZZ, ZZZ = [v % p for v in vals]
    assert ZZ != 0 and ZZZ != 0, "%s: a finite point with ZZ or ZZZ = 0 mod p" % where
    zz, zzz = ZZ * C.r30_inv % p, ZZZ * C.r30_inv % p
    assert pow(zz, 3, p) == zzz * zzz % p, "%s: ZZ^3 != ZZZ^2" % where
    got = (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)
    assert got == want, "%s: group element %s, expected %s" % (where, got, want)


def check_point30(C, row, want, key, where, base=O0, inf=None):
    """form, value bound (BOUNDS[key]) and group element of a register-form result; `inf`: the flag that came back"""
    if inf is None:
        inf = int(row[FO + 1])
    assert inf in (0, 1)
    assert bool(inf) == (want is None), "%s: inf = %d, expected %s" % (where, inf, want)
    if want is None:
        return
    check_form(C, row, base, 4, where)
    vals = get30(row, base)
    bx, by, bz = [bound(C, e) for e in BOUNDS[key]] if isinstance(key, str) else key
    assert vals[0] < bx and vals[1] < by and vals[2] < bz and vals[3] < bz, \
        "%s: value bound: %s" % (where, [v / C.p for v in vals])
    check_element(C, vals, want, where)


def check_point_mem(C, w32, want, key, where, final=False):
    """a memory-form result (32 words): BN254 unreduced below 2^256 within the operation's bound, secp256k1 canonical,
    infinity all-zero; final: the canonical 2^256 Montgomery form the host reads"""
    vals = get_words(w32, 0)
    if want is None:
        assert not any(int(x) for x in w32), "%s: infinity is not all-zero" % where
        return
    assert vals[2] != 0, "%s: a finite point stored with an all-zero ZZ" % where
    if final or C is SECP:
        assert all(v < C.p for v in vals), "%s: not canonical" % where
    else:
        bx, by, bz = [bound(C, e) for e in BOUNDS[key]] if isinstance(key, str) else key
        assert vals[0] < bx and vals[1] < by and vals[2] < bz and vals[3] < bz, "%s: value bound %s" % (where, [v / C.p for v in vals])
    if final:
        f = C.r30 * pow(C.r32, -1, C.p) % C.p          # bring the 2^256 form to the 2^270 form check_element decodes
        vals = [v * f % C.p for v in vals]
    check_element(C, vals, want, where)


# ---------------------------------------------------------------- running the driver
def run(C, jobs, host=False):
    """jobs: [(op, records)] -> [records after the operation], one process for all of them"""
    with tempfile.TemporaryDirectory() as d:
        cmd = [EXE] + (["--host"] if host else []) + [C.name]
        for i, (op, recs) in enumerate(jobs):
            assert recs.dtype == np.uint32 and recs.shape[1] == REC
            recs.tofile(os.path.join(d, "in%d" % i))
            cmd += [op, os.path.join(d, "in%d" % i), os.path.join(d, "out%d" % i)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, "ec30_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
        outs = []
        for i, (op, recs) in enumerate(jobs):
            o = np.fromfile(os.path.join(d, "out%d" % i), dtype=np.uint32).reshape(-1, REC)
            assert o.shape == recs.shape, "%s: %d records out for %d in" % (op, o.shape[0], recs.shape[0])
            outs.append(o)
        return outs


# ---------------------------------------------------------------- the 8 x 32-bit forms of ec.hip.h (device and --host)
OPS32 = ["xyzz_madd", "xyzz_add", "xyzz_double", "xyzz_double_affine"]


def gen32(C, op, n, seed):
    """records + expected points.  Operands: canonical Montgomery residues, XYZZ with a free l; infinity as ZZ = 0 (XYZZ)
    or (0, 0) (affine); equal-x pairs with the same and with different l"""
    rng = random.Random(seed)
    G = multiples(C)
    cases = []          # (P or None, l, Q or None, l2)
    for a, b in ((3, 3), (3, -3), (5, 5), (7, -7), (0, 4), (4, 0), (0, 0), (1, 1), (1, 2), (2, 1)):
        for l, l2 in ((1, 1), (rng.randrange(1, C.p), rng.randrange(1, C.p)), (C.p - 1, 2)):
            cases.append((a, l, b, l2))
    while len(cases) < n:
        cases.append((rng.randint(1, 40), rng.randrange(1, C.p), rng.choice([-1, 1]) * rng.randint(1, 40), rng.randrange(1, C.p)))
    pt = lambda k: None if k == 0 else (G[k] if k > 0 else ec_neg(C, G[-k]))
    recs, want = new_records(len(cases)), []
    for i, (a, l, b, l2) in enumerate(cases):
        P, Q = pt(a), pt(b)
        if op in ("xyzz_double", "xyzz_double_affine"):
            Q = P
        if op == "xyzz_double_affine" and P is None:
            P = Q = G[9]                                  # "a != infinity"
        put_words(recs[i], 0, rep32(C, P, l) if P else [rng.randrange(C.p), rng.randrange(C.p), 0, 0])
        if op == "xyzz_add":
            put_words(recs[i], 32, rep32(C, Q, l2) if Q else [rng.randrange(C.p), rng.randrange(C.p), 0, 0])
        else:
            put_words(recs[i], 32, [Q[0] * C.r32 % C.p, Q[1] * C.r32 % C.p] if Q else [0, 0])
        want.append(ec_add(C, P, Q))
    return recs, want


def check32(C, op, out, want, counter):
    f = C.r30 * pow(C.r32, -1, C.p) % C.p
    for i, w in enumerate(want):
        where = "%s %s record %d" % (C.name, op, i)
        vals = get_words(out[i], O0)
        assert all(v < C.p for v in vals), where + ": not canonical"
        inf = int(out[i][FO + 1])
        assert bool(inf) == (w is None) and bool(inf) == (vals[2] == 0), where + ": infinity"
        if w is not None:
            check_element(C, [v * f % C.p for v in vals], w, where)
        counter.checked += 1

"""Vectors and expected values for the per-form checks of the MAC-side ladders and their digit recoders (tools/ladder_check.hip):
shared by tests/test_ladder_gpu.py, tests/test_ladder_vectors_cpu.py and tests/test_msm_batch_gpu.py.

Everything here is computed on Python integers: the two recoder models, the scalar families built from their endomorphism
halves, the (n, s) shapes that make a stage kernel read the scalars the test wants, and the expected points um + k P, um - k P
(tests/ec_vectors.py's group law; a fixed-base Jacobian multiple of G where the affine double-and-add would make generation slow,
checked against it by the CPU test).  The endomorphism split is tools/gen_glv.py's bit-for-bit model of glv_split.  Generation is
deterministic (fixed seeds) and reads nothing outside the repository.
"""
import functools
import os
import random
import subprocess
import sys
import tempfile

import numpy as np

from tests import common
from tests import ec_vectors as ev

sys.path.insert(0, os.path.join(common.ROOT, "tools"))
import gen_glv  # noqa: E402

EXE = os.path.join(common.ROOT, "porla_amd", "ladder_check")

# recoder records of tools/ladder_check.hip
REC, A0, O0, F_FLIP = 192, 16, 32, 1
# launch files of tools/ladder_check.hip
HDR, H_MAGIC, H_N, H_S, H_TOTAL, H_ROWS, H_ENTRIES, H_WT = 32, 0, 1, 2, 3, 4, 5, 8
MAGIC = 0x4c414444
SENTINEL = ev.SENTINEL
WNAF_LEN = 129                 # mac_fft.hip.h: MACQ_WNAF_LEN
CODES_STRIDE = 132             # MACQ_CODES_STRIDE, 16-bit words per entry of the code table
CODES_EXP_SHIFT = 5            # MACQ_CODES_EXP_SHIFT: entry = exponent >> 5
MACQ_BF, MACO_BF = 64, 32      # butterflies per block of the four- and eight-lane kernels
PAD_TOTAL = 200                # a butterfly count that fills neither kernel's last block
M128 = (1 << 128) - 1
GLV_NAME = {"bn254": "Bn254", "secp256k1": "Secp256k1"}


@functools.lru_cache(maxsize=None)
def glv(name):
    return gen_glv.derive(GLV_NAME[name], gen_glv.CURVES[GLV_NAME[name]])


def order(C):
    return glv(C.name)["n"]


def lam(C):
    return glv(C.name)["lam"]


def split(C, k):
    """[(|k1|, neg1), (|k2|, neg2)] of k in [0, n): the model of glv_split"""
    return gen_glv.split_model(glv(C.name), k)


# ---------------------------------------------------------------- the recoders on Python integers
def signed_digits(m):
    """mac_signed_digit: the sequential rule of mac30_scalar_mul -- nibble plus carry, minus 16 above 8; 33 digits"""
    assert 0 <= m <= M128
    d, carry = [], 0
    for i in range(32):
        v = ((m >> (4 * i)) & 15) + carry
        if v > 8:
            d.append(v - 16)
            carry = 1
        else:
            d.append(v)
            carry = 0
    d.append(carry)
    return d


def wnaf5(m):
    """mac_wnaf5_step, 129 positions: the width-5 NAF digits of m, least significant first, and what is left of m"""
    assert 0 <= m <= M128
    d = []
    for _ in range(WNAF_LEN):
        dg = 0
        if m & 1:
            low = m & 31
            dg = low - 32 if low >= 16 else low
            m -= dg
        d.append(dg)
        m >>= 1
    return d, m


def wnaf_code(dg, flip):
    """code of a digit: 0, or 16 | sign << 3 | (|d| - 1) / 2 with sign = negative != flip"""
    if dg == 0:
        return 0
    return 16 | (8 if (dg < 0) != bool(flip) else 0) | ((abs(dg) - 1) // 2)


def decode_code(code):
    """(signed digit with the half's sign folded in) of a code"""
    if code == 0:
        return 0
    assert code & 16 and code < 32, "code %#x" % code
    mag = 2 * (code & 7) + 1
    return -mag if code & 8 else mag


def check_signed_digits(m, d):
    assert len(d) == 33 and all(-7 <= x <= 8 for x in d) and d[32] in (0, 1), (hex(m), d)
    assert sum(x << (4 * i) for i, x in enumerate(d)) == m, hex(m)


def check_wnaf5(m, d, left):
    assert len(d) == WNAF_LEN and left == 0, hex(m)
    assert all(x == 0 or (x & 1 and abs(x) <= 15) for x in d), hex(m)
    for i in range(WNAF_LEN - 4):
        assert sum(1 for x in d[i:i + 5] if x) <= 1, "%#x: two digits within five positions at %d" % (m, i)
    assert sum(x << i for i, x in enumerate(d)) == m, hex(m)


REP8 = int("8" * 32, 16)
POW_EDGES = (4, 5, 31, 32, 33, 63, 64, 65, 95, 96, 127)
# the 17 patterns the scalar families build their halves from (masked to HALF_BITS there)
PATTERNS17 = ([0, 1, M128, REP8, REP8 - 1, REP8 + 1, int("7" * 31 + "8", 16), int("7" * 32, 16), int("9" * 32, 16)]
              + [0x88888888 << (32 * q) for q in range(4)]
              + [int("a" * 32, 16), int("5" * 32, 16), int("1f" * 16, 16), int("10" * 16, 16)])
HALF_BITS = 125                # family (b): every sign pair of every pattern pair comes back from the split at 120 .. 125 bits


def pattern_magnitudes():
    """the chosen 128-bit magnitudes of both recoders: a window digit of exactly 8, carries that ripple across limbs, the 33rd
    window / position 128, long zero runs below and above"""
    v = list(PATTERNS17)
    v += [8 << (4 * i) for i in range(32)] + [9 << (4 * i) for i in range(32)]
    v += [1 << i for i in POW_EDGES] + [(1 << i) - 1 for i in POW_EDGES]
    assert all(0 <= x <= M128 for x in v)
    return v


@functools.lru_cache(maxsize=None)
def magnitudes():
    rng = random.Random(0x5eed1)
    return tuple(pattern_magnitudes() + [rng.getrandbits(128) >> rng.choice((0, 0, 0, 1, 7, 40, 90)) for _ in range(2000)])


# ---------------------------------------------------------------- scalar families
def from_halves(C, a, sa, b, sb):
    """k = +-a + lambda (+-b) mod n"""
    return ((-a if sa else a) + lam(C) * (-b if sb else b)) % order(C)


def halves_match(C, k, a, sa, b, sb):
    """the split of k is exactly (a, b) with these signs (a zero half has no sign)"""
    (m1, n1), (m2, n2) = split(C, k)
    return m1 == a and m2 == b and (a == 0 or n1 == sa) and (b == 0 or n2 == sb)


@functools.lru_cache(maxsize=None)
def family_a(C):
    n, l = order(C), lam(C)
    v = [0, 1, 2, n - 1, n - 2, (n + 1) // 2, (n - 1) // 2, l, l + 1, l - 1, n - l, l * l % n]
    v += [m * l % n for m in range(1, 17)]          # the first half is zero
    v += list(range(1, 17))                         # the second half is zero
    return tuple(v)


@functools.lru_cache(maxsize=None)
def family_b(C):
    """(k, a, sa, b, sb): halves from the patterns masked to HALF_BITS bits, all four sign pairs"""
    mask = (1 << HALF_BITS) - 1
    pats = [x & mask for x in PATTERNS17]
    assert len(set(pats)) == 17
    return tuple((from_halves(C, a, sa, b, sb), a, sa, b, sb) for a in pats for b in pats for sa in (0, 1) for sb in (0, 1))


FAMILY_C_WANTED, FAMILY_C_STREAM = 32, 4096


@functools.lru_cache(maxsize=None)
def family_c(C):
    """scalars with a half above 0x88..8 -- the 33rd window is set: the first FAMILY_C_WANTED of a seeded stream of
    FAMILY_C_STREAM scalars (about 2.6 % of secp256k1's halves qualify; BN254's stay below 2^126: none)"""
    rng = random.Random(0xc33)
    out = []
    for _ in range(FAMILY_C_STREAM):
        k = rng.randrange(order(C))
        if any(m > REP8 for m, _ in split(C, k)):
            out.append(k)
            if len(out) == FAMILY_C_WANTED:
                break
    return tuple(out)


@functools.lru_cache(maxsize=None)
def family_d(C):
    """(k, a, 0, b, 0): NAF shapes -- a long zero run below the first digit, a run of ones, on either side, the other half 0 or 1"""
    out = []
    for h in (1 << 120, 0x1f << 100, (1 << 124) - 1):
        for o in (0, 1):
            out.append((from_halves(C, h, 0, o, 0), h, 0, o, 0))
            out.append((from_halves(C, o, 0, h, 0), o, 0, h, 0))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def family_e(C):
    rng = random.Random(0xe256)
    return tuple(rng.randrange(order(C)) for _ in range(256))


def families(C, which="abcde"):
    """[(family, k)] in a fixed order"""
    out = []
    for f in which:
        members = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}[f](C)
        out += [(f, m[0] if isinstance(m, tuple) else m) for m in members]
    return out


# ---------------------------------------------------------------- multiples of G
@functools.lru_cache(maxsize=None)
def _g_table(C):
    """T[w][d] = d 2^(8 w) G, affine"""
    t, base = [], C.g
    for _ in range(32):
        row = [None]
        for _ in range(255):
            row.append(ev.ec_add(C, row[-1], base))
        t.append(row)
        base = ev.ec_add(C, row[255], base)
    return t


_MUL_G = {}


def mul_g(C, k):
    """k G by Jacobian mixed additions over the byte table of G: one inversion per call (equal to ev.ec_mul(C, k, C.g))"""
    k %= order(C)
    key = (C.name, k)
    if key in _MUL_G:
        return _MUL_G[key]
    p, T = C.p, _g_table(C)
    X = Y = Z = 0                                    # Z = 0: infinity
    for w in range(32):
        a = T[w][(k >> (8 * w)) & 255]
        if a is None:
            continue
        if Z == 0:
            X, Y, Z = a[0], a[1], 1
            continue
        zz = Z * Z % p
        u2, s2 = a[0] * zz % p, a[1] * zz * Z % p
        h, r = (u2 - X) % p, (s2 - Y) % p
        if h == 0:                                   # the same x: through the affine law
            zi = pow(Z, -1, p)
            q = ev.ec_add(C, (X * zi * zi % p, Y * zi ** 3 % p), a)
            X, Y, Z = (q[0], q[1], 1) if q else (0, 0, 0)
            continue
        hh = h * h % p
        hhh, v = h * hh % p, X * hh % p
        X3 = (r * r - hhh - 2 * v) % p
        Y, Z = (r * (v - X3) - Y * hhh) % p, Z * h % p
        X = X3
    if Z == 0:
        res = None
    else:
        zi = pow(Z, -1, p)
        res = (X * zi * zi % p, Y * zi ** 3 % p)
    _MUL_G[key] = res
    return res


# ---------------------------------------------------------------- which butterfly reads which table entry
def stage_index(t, n, s, share=1):
    """mac_fft.hip.h:mac_stage_index<share>: butterfly t of stage s over tables of n rows -> (k, m2, e): the pair of rows
    (k, k + m2) and the table entry e = j (n >> (s-1)) of its scalar"""
    m2 = 1 << (s - 1)
    if share > 1:
        rest = t // share
        j = rest & (m2 - 1)
        k = ((((rest >> (s - 1)) * share) | (t & (share - 1))) << s) + j
    else:
        j = t & (m2 - 1)
        k = ((t >> (s - 1)) << s) + j
    return k, m2, j * (n >> (s - 1))


class Shape:
    """one launch shape: n, s, the butterflies' (k, m2, e), and the table entries in the order the butterflies first read them"""
    def __init__(self, n, s, total, share):
        self.n, self.s, self.total, self.share = n, s, total, share
        self.bf = [stage_index(t, n, s, share) for t in range(total)]
        self.entries = []
        for _, _, e in self.bf:
            if e not in self.entries:
                self.entries.append(e)
        rows = sorted(r for k, m2, _ in self.bf for r in (k, k + m2))
        assert len(set(rows)) == 2 * total and rows[-1] < n, "butterflies share rows or leave the table"
        assert all(e < n for e in self.entries)
        self.readers = {e: [t for t, b in enumerate(self.bf) if b[2] == e] for e in self.entries}


@functools.lru_cache(maxsize=None)
def per_butterfly_shape(S):
    """S butterflies that read S different entries: the last stage of one table of 2 S rows"""
    assert S & (S - 1) == 0
    n = 2 * S
    found = [s for s in range(1, n.bit_length()) if len(Shape(n, s, n // 2, 1).entries) == S]
    assert found == [n.bit_length() - 1]
    sh = Shape(n, found[0], S, 1)
    assert all(len(r) == 1 for r in sh.readers.values())
    return sh


@functools.lru_cache(maxsize=None)
def uniform_shape(share, scalars, n=2048):
    """the stage of a table of n rows at which `share` butterflies (a wave's) read one entry and the launch reads `scalars`
    different entries, every one a multiple of 32 (the code table is keyed by exponent >> 5)"""
    found = []
    for s in range(2, n.bit_length()):
        if (n >> s) < share:                        # the launch rule of mac_stages for the wave-uniform forms
            continue
        sh = Shape(n, s, n // 2, share)
        if len(sh.entries) == scalars:
            found.append(sh)
    assert len(found) == 1, [f.s for f in found]
    sh = found[0]
    assert all(e % (1 << CODES_EXP_SHIFT) == 0 for e in sh.entries)
    assert all(len(r) == (n // 2) // scalars for r in sh.readers.values())
    # the `share` butterflies of a wave (consecutive t) read ONE entry
    assert all(len({sh.bf[t][2] for t in range(w, w + share)}) == 1 for w in range(0, n // 2, share))
    return sh


# ---------------------------------------------------------------- points
KINDS = ("min", "top", "xmax", "zmax")
UM_CASES = ("inf", "other", "same", "neg")


def shaped_mem(C, P, kind, rng, y_max=None):
    """one memory-form representation of P (ev.rep_mem): min = canonical with l = 1, top = as many multiples of p as the operand
    bound allows, xmax / zmax = X / ZZ at the very top of its bound"""
    if P is None:
        return [0, 0, 0, 0]
    if kind == "min":
        return ev.rep_mem(C, P, 1, [0, 0, 0, 0], y_max, rng)
    if kind == "xmax":
        return ev.rep_mem(C, P, ev.find_l(C, P, 0, C.eps - 1, rng)[0], "top", y_max, rng)
    if kind == "zmax":
        return ev.rep_mem(C, P, ev.find_l(C, P, 2, C.eps - 1, rng)[0], "top", y_max, rng)
    return ev.rep_mem(C, P, rng.randrange(1, C.p), "top", y_max, rng)


def point_words(vals):
    return [w for v in vals for w in ev.words(v)]


def affine_be_words(P):
    """64-byte big-endian affine point as the 16 little-endian words of a file; infinity = zeros"""
    raw = bytes(64) if P is None else P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big")
    return list(np.frombuffer(raw, dtype="<u4"))


MAX_M = 8                      # points are G .. MAX_M G


@functools.lru_cache(maxsize=None)
def scalar_multiples(C, k):
    """[None, T, 2 T, .. MAX_M T] with T = k G: k (m G) for every point multiplier m from ONE fixed-base multiple"""
    T = mul_g(C, k)
    out = [None]
    for _ in range(MAX_M):
        out.append(ev.ec_add(C, out[-1], T))
    return tuple(out)


class Butterfly:
    """one butterfly's inputs and expected outputs: hi = P = m G, lo = um, scalar k -> (um + k P, um - k P).  Built once per
    (curve, k, idx, slot) by butterfly() below and shared by every form that is fed scalar idx"""
    def __init__(self, C, k, idx, slot, trivial=False):
        G = ev.multiples(C)
        rng = random.Random(0xb77f + 4 * idx + slot)
        self.k = k
        if trivial:                                   # both inputs at infinity: the ladder is skipped, both outputs are zeros
            self.m, self.P, self.um, self.tm, self.case = 0, None, None, None, "trivial"
        else:
            self.m = 1 + (3 * idx + 5 * slot) % MAX_M
            self.P = G[self.m]
            self.tm = scalar_multiples(C, k)[self.m]
            self.case = UM_CASES[(idx + 2 * slot) % 4]
            self.um = {"inf": None, "other": G[41 + idx % 7], "same": self.tm, "neg": ev.ec_neg(C, self.tm)}[self.case]
        # (the um case walks with idx, the shapes with idx / 4 and idx / 16: 64 consecutive scalars meet every combination)
        self.p_kind, self.um_kind = KINDS[(idx // 4 + slot) % 4], KINDS[(idx // 16 + slot + 1) % 4]
        # P is negated by the ladders (4p - Y: Y <= 3p + eps); um is only ever added
        self.p_words = np.array(point_words(shaped_mem(C, self.P, self.p_kind, rng, C.in_y_neg)), dtype=np.uint32)
        self.um_words = np.array(point_words(shaped_mem(C, self.um, self.um_kind, rng)), dtype=np.uint32)
        self.lo = ev.ec_add(C, self.um, self.tm)
        self.hi = ev.ec_add(C, self.um, ev.ec_neg(C, self.tm))
        # a true sum carries the addition's bound; a value that passes through (possibly negated: Y <= 4p) the operand's
        self.key = "add" if self.um is not None and self.tm is not None else "operand"


@functools.lru_cache(maxsize=None)
def butterfly(C, k, idx, slot):
    return Butterfly(C, k, idx, slot)


def launch_words(n=0, s=0, total=0, rows=(), tws=(), wt=0):
    """one launch of a stage file: header, rows (lists of 32 or 16 words), table entries (integers)"""
    h = [0] * HDR
    h[H_MAGIC], h[H_N], h[H_S], h[H_TOTAL], h[H_ROWS], h[H_ENTRIES] = MAGIC, n, s, total, len(rows), len(tws)
    h[H_WT:H_WT + 8] = ev.words(wt)
    for r in rows:
        h.extend(r)
    for k in tws:
        h.extend(ev.words(k))
    return np.array(h, dtype=np.uint32)


SENTINEL_ROW = [SENTINEL] * 32


def stage_launch(C, shape, scalars, butterflies, total=None):
    """scalars: {entry: k}; butterflies: {t: Butterfly} for every live t < total.  Rows no live butterfly owns and entries none
    reads hold the sentinel."""
    total = shape.total if total is None else total
    rows = np.full((shape.n, 32), SENTINEL, dtype=np.uint32)
    tws = np.full((shape.n, 8), SENTINEL, dtype=np.uint32)
    for t in range(total):
        k, m2, e = shape.bf[t]
        b = butterflies[t]
        assert scalars[e] == b.k
        rows[k], rows[k + m2] = b.um_words, b.p_words
    for e, k in scalars.items():
        tws[e] = ev.words(k)
    h = np.zeros(HDR, dtype=np.uint32)
    h[[H_MAGIC, H_N, H_S, H_TOTAL, H_ROWS, H_ENTRIES]] = [MAGIC, shape.n, shape.s, total, shape.n, shape.n]
    return np.concatenate([h, rows.reshape(-1), tws.reshape(-1)])


@functools.lru_cache(maxsize=None)
def by_value_rows(C, affine):
    """per scalar idx of families (a)-(d): the point multipliers of a by-value launch (two points, their shapes walking with idx,
    and infinity) and the input rows; shared by the forms that read the same input form"""
    G = ev.multiples(C)
    out = []
    for idx in range(len(families(C, "abcd"))):
        rng = random.Random(0xb1a + idx)
        ms = [1 + idx % MAX_M, 1 + (idx + 3) % MAX_M, 0]
        pts = [G[m] if m else None for m in ms]
        if affine:
            words = [affine_be_words(P) for P in pts]
        else:
            words = [point_words(shaped_mem(C, P, KINDS[(idx + 2 * j + idx // 4) % 4], rng, C.in_y_neg)) for j, P in enumerate(pts)]
        out.append((ms, words))
    return out


def split_stage_output(raw, launches, with_codes):
    """raw output words -> [(work rows [rows][32], code table [n / 32][CODES_STRIDE] of 16-bit words or None)] per launch;
    launches: [(n, rows)]"""
    out, at = [], 0
    for n, rows in launches:
        work = raw[at:at + rows * 32].reshape(rows, 32)
        at += rows * 32
        codes = None
        if with_codes:
            words = (n >> CODES_EXP_SHIFT) * (CODES_STRIDE // 2)
            codes = raw[at:at + words].view("<u2").reshape(n >> CODES_EXP_SHIFT, CODES_STRIDE)
            at += words
        out.append((work, codes))
    assert at == len(raw), "the driver wrote %d words, %d expected" % (len(raw), at)
    return out


def trivial_butterfly(C, k):
    """both inputs at infinity (the ladder is skipped, both outputs are all-zero rows): needs no point, so one object per scalar"""
    return Butterfly(C, k, 0, 0, trivial=True)


def by_value_key(C, k):
    """value bound of k P out of a ladder: an addition's or a doubling's output, unless the only non-zero digit of both halves
    sits at position 0 -- then a table entry passed through, possibly negated (Y up to 4p)"""
    digits = [d for m, _ in split(C, k) for d in wnaf5(m)[0]]
    through = sum(1 for d in digits if d) == 1 and (digits[0] != 0 or digits[WNAF_LEN] != 0)
    return "operand" if through else "add"


def check_butterfly(C, work, shape, t, b, where):
    k, m2, _ = shape.bf[t]
    if b.lo is None and b.hi is None:
        assert not work[k].any() and not work[k + m2].any(), "%s: infinity is not all-zero (um %s)" % (where, b.case)
        return
    ev.check_point_mem(C, work[k], b.lo, b.key, "%s lo (um %s, P = %d G %s)" % (where, b.case, b.m, b.p_kind))
    ev.check_point_mem(C, work[k + m2], b.hi, b.key, "%s hi (um %s, P = %d G %s)" % (where, b.case, b.m, b.p_kind))


def check_codes_entry(C, entry, k, where):
    """an entry of k_mac_wnaf_codes' table decodes to the halves of k: low byte k1, high byte k2, signs folded in"""
    (m1, n1), (m2, n2) = split(C, k)
    assert not any(int(x) for x in entry[WNAF_LEN:]), where + ": padding of the entry"
    for h, (m, neg) in enumerate(((m1, n1), (m2, n2))):
        codes = [(int(x) >> (8 * h)) & 0xff for x in entry[:WNAF_LEN]]
        assert codes == [wnaf_code(d, neg) for d in wnaf5(m)[0]], "%s: codes of half %d" % (where, h)
        assert sum(decode_code(c) << i for i, c in enumerate(codes)) == (-m if neg else m), "%s: half %d" % (where, h)


# ---------------------------------------------------------------- running the driver
def run(C, jobs):
    """jobs: [(op, words)] -> [output words], one process for all of them"""
    with tempfile.TemporaryDirectory() as d:
        cmd = [EXE, C.name]
        for i, (op, data) in enumerate(jobs):
            assert data.dtype == np.uint32
            data.tofile(os.path.join(d, "in%d" % i))
            cmd += [op, os.path.join(d, "in%d" % i), os.path.join(d, "out%d" % i)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, "ladder_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
        return [np.fromfile(os.path.join(d, "out%d" % i), dtype=np.uint32) for i in range(len(jobs))]


def recoder_records(n):
    r = np.zeros((n, REC), dtype=np.uint32)
    r[:, O0:] = SENTINEL
    return r

"""Models, vectors and expected values for the stage-by-stage checks of the fixed-base commitment (tools/fb_check.hip, which runs the
kernels of porla_amd/csrc/fixed_base.hip.h): shared by tests/test_fb_gpu.py and tests/test_fb_vectors_cpu.py.

Everything here is Python integers: the group law is tests/ec_vectors.py's (affine chord and tangent), a scalar multiple of G a sum
of precomputed window multiples of G by that law.  Every base point of every test is a known multiple b G (or infinity), so a sum of
table entries is ONE scalar mod the group order -- which is how the models below know, without any curve arithmetic, where two equal
or two opposite points meet inside a kernel: G has prime order, so two multiples are equal exactly when their scalars are.

FORMS (restated from fe.hip.h / fe30.hip.h / fixed_base.hip.h):
  base point in        Affine<M>: x 2^256 mod p, y 2^256 mod p (secp256k1: the plain residues), 8 words each; all-zero = infinity
  table entry          k_fb_normalize multiplies the 2^256-form affine coordinate by M::R1_30 = 2^270 mod p in fe_mul (which divides by
                       2^256): the entry holds x 2^270 mod p, y 2^270 mod p -- the residues of the reduced-radix accumulation -- as
                       CANONICAL values in [0, p) (fe_mul's result range); secp256k1: R1_30 = 1, the plain residues.  All-zero = infinity.
  partial, S = 1       XYZZ in the canonical 2^256 form (store_xyzz of xyzz30_to_xyzz): what k_fb_finish and the host read
  partial, S > 1       XYZZ in the lazy memory form after xyzz30_flip_finish: BN254 X < 5p + eps, Y <= 4p, ZZ, ZZZ < p + eps below
                       2^256; secp256k1 canonical (ec_vectors.BOUNDS["flip_finish"])
  out                  64 bytes, big-endian affine x || y; 64 zero bytes = infinity
"""
import functools
import os
import random
import subprocess
import tempfile

import numpy as np

from tests import common
from tests import ec_vectors as ev

EXE = os.path.join(common.ROOT, "porla_amd", "fb_check")
GOLDEN_PLAN = os.path.join(common.ROOT, "tests", "golden", "fb_plan.txt")

MAGIC, HDR = 0x46424b31, 16
OP_TABLE, OP_COMMIT, OP_SMALL, OP_FOLD, OP_FINISH = 1, 2, 3, 4, 5
SENTINEL = ev.SENTINEL
SMALL_THREADS, SMALL_MAX_ROWS, SMALL_MAX_SLICES = 256, 64, 8     # msm_small.hip.h
MAX_ENTRIES = 1 << 23
SCRATCH_BUDGET = 1 << 30                                         # fixed_base.hip.h: FB_SCRATCH_BUDGET
XYZZ_BYTES = 128

ORDER = {"bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         "secp256k1": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141}
SCALAR_BITS = {"bn254": 254, "secp256k1": 256}                   # msm.hip.h


def order(C):
    return ORDER[C.name]


def windows(C, c):
    """W of FixedBase<C>::build: ceil((SCALAR_BITS + 1) / c)"""
    return (SCALAR_BITS[C.name] + 1 + c - 1) // c


# ---------------------------------------------------------------- the launch shapes, restated (fixed_base.hip.h: fb_table_plan)
def table_plan(c, pairs, budget=SCRATCH_BUDGET):
    H = 1 << (c - 1)
    lanes = 64 if H >= 1024 else (H // 16 if H >= 16 else 1)
    K = min(H // lanes, 64)
    return dict(H=H, lanes=lanes, K=K, runs=H // (lanes * K), groups_per_wave=64 // lanes,
                batch_pairs=min(max(budget // (H * XYZZ_BYTES), 1), pairs))


# ---------------------------------------------------------------- scalar multiples of G
@functools.lru_cache(maxsize=None)
def _g_windows(name):
    """[w][d] = d 2^(8w) G, d < 256"""
    C = ev.CURVES[name]
    out, base = [], C.g
    for _ in range(32):
        row = [None]
        for _ in range(255):
            row.append(ev.ec_add(C, row[-1], base))
        out.append(row)
        base = ev.ec_add(C, row[-1], base)
    return out


def mul_g(C, k):
    """(k mod order) G"""
    k %= order(C)
    t, r = _g_windows(C.name), None
    for w in range(32):
        d = (k >> (8 * w)) & 255
        if d:
            r = ev.ec_add(C, r, t[w][d])
    return r


def point(C, b):
    """base point b G; None = infinity"""
    return None if b is None else mul_g(C, b)


def ec_add_batch(C, pairs):
    """[a + b] for affine pairs with ONE inversion (Montgomery's trick); the exceptional pairs go through ev.ec_add"""
    p = C.p
    out, idx, dens = [None] * len(pairs), [], []
    for i, (a, b) in enumerate(pairs):
        if a is None or b is None or a[0] == b[0]:
            out[i] = ev.ec_add(C, a, b)
        else:
            idx.append(i)
            dens.append((b[0] - a[0]) % p)
    pre, run = [], 1
    for d in dens:
        pre.append(run)
        run = run * d % p
    inv = pow(run, -1, p) if dens else 0
    for j in range(len(idx) - 1, -1, -1):
        a, b = pairs[idx[j]]
        lam = (b[1] - a[1]) * (inv * pre[j] % p) % p
        inv = inv * dens[j] % p
        x = (lam * lam - a[0] - b[0]) % p
        out[idx[j]] = (x, (lam * (a[0] - x) - a[1]) % p)
    return out


# ---------------------------------------------------------------- signed digits
def signed_digits(C, k, c):
    """the textbook recoding of k mod order into W digits of c bits: a value above 2^(c-1) becomes negative and carries"""
    t, W, half = k % order(C), windows(C, c), 1 << (c - 1)
    digits, carry = [], 0
    for w in range(W):
        raw = ((t >> (c * w)) & ((1 << c) - 1)) + carry
        if raw > half:
            digits.append(raw - (1 << c))
            carry = 1
        else:
            digits.append(raw)
            carry = 0
    assert carry == 0, "carry out of the top window"
    return digits


def check_signed_digits(C, k, c, digits):
    half = 1 << (c - 1)
    assert len(digits) == windows(C, c)
    assert sum(d << (c * w) for w, d in enumerate(digits)) == k % order(C), hex(k)
    assert all(-(half - 1) <= d <= half for d in digits), hex(k)


RANDOM_MEMBERS = 1000


@functools.lru_cache(maxsize=None)
def families(name, c):
    """[(family, k)], k < 2^256:  edge the four edge values;  order q n - 1, q n, q n + 1;  half every window 2^(c-1), and +-1;
    win 2^(c-1) 2^(cw) and (2^(c-1) + 1) 2^(cw);  ripple 2^(cj) - 1;  top scalars whose only non-zero digit is the top window;
    random seeded 256-bit values"""
    C = ev.CURVES[name]
    n, W, half = order(C), windows(C, c), 1 << (c - 1)
    out = [("edge", v) for v in (0, 1, n - 1, (1 << 256) - 1)]
    q = 1
    while q * n < 1 << 256:
        out += [("order", q * n - 1), ("order", q * n), ("order", q * n + 1)]
        q += 1
    allhalf = sum(half << (c * w) for w in range(W))
    while allhalf >= n:                                       # truncated below the order: drop the top window's bits
        allhalf &= (1 << (allhalf.bit_length() - 1)) - 1
    out += [("half", allhalf - 1), ("half", allhalf), ("half", allhalf + 1)]
    for w in range(W):
        for v in (half << (c * w), (half + 1) << (c * w)):
            if v < 1 << 256:
                out.append(("win", v))
    for j in range(1, W + 1):
        out.append(("ripple", min((1 << (c * j)) - 1, (1 << 256) - 1)))
    top = c * (W - 1)
    for d in (1, 2, half - 1, half):
        if d >= 1 and (d << top) < n:
            out.append(("top", d << top))
    rng = random.Random(0xFB00 + c)
    out += [("random", rng.randrange(1 << 256)) for _ in range(RANDOM_MEMBERS)]
    return out


# ---------------------------------------------------------------- words
def le_words(v, count=8):
    return np.frombuffer(int(v).to_bytes(4 * count, "little"), dtype=np.uint32)


def base_words(C, pts):
    """the base as FixedBase<C>::build takes it"""
    w = np.zeros((len(pts), 16), dtype=np.uint32)
    for i, pt in enumerate(pts):
        if pt is not None:
            w[i, :8] = le_words(pt[0] * C.r32 % C.p)
            w[i, 8:] = le_words(pt[1] * C.r32 % C.p)
    return w


def entry_words(C, pt):
    """a table entry as k_fb_normalize stores it (FORMS above); the range is asserted"""
    w = np.zeros(16, dtype=np.uint32)
    if pt is not None:
        x, y = pt[0] * C.r30 % C.p, pt[1] * C.r30 % C.p
        assert 0 <= x < C.p and 0 <= y < C.p
        w[:8], w[8:] = le_words(x), le_words(y)
    return w


def row_bytes(coeffs, stride):
    """one row: 32 big-endian bytes per coefficient, the rest of the stride holds 0xA5"""
    b = bytearray(b"\xa5" * stride)
    for i, k in enumerate(coeffs):
        b[32 * i:32 * i + 32] = int(k).to_bytes(32, "big")
    return bytes(b)


def rows_words(rows, stride):
    assert stride % 4 == 0
    return np.frombuffer(b"".join(row_bytes(r, stride) for r in rows), dtype=np.uint32)


def header(op, c, n=0, n_rows=0, S=0, row_stride=0, flag=0, budget=0, sentinel=0):
    h = np.zeros(HDR, dtype=np.uint32)
    h[:11] = [MAGIC, op, c, n, n_rows, S, row_stride, flag, budget & 0xffffffff, budget >> 32, sentinel]
    return h


class Section:
    """one section of the driver's input and the length of what it answers with"""
    def __init__(self, words, out_words, **ctx):
        self.words, self.out_words, self.ctx = words, out_words, ctx


def table_section(C, c, pts, idx=None, budget=0):
    W, H = windows(C, c), 1 << (c - 1)
    entries = len(pts) * W * H
    assert entries <= MAX_ENTRIES
    idx = np.zeros(0, dtype=np.uint32) if idx is None else np.asarray(idx, dtype=np.uint32)
    words = np.concatenate([header(OP_TABLE, c, n=len(pts), flag=len(idx), budget=budget), base_words(C, pts).reshape(-1), idx])
    return Section(words, (len(idx) if len(idx) else entries) * 16, c=c)


def commit_section(c, rows, S, stride=None, guest=0, sentinel=0):
    n = len(rows[0])
    stride = 32 * n if stride is None else stride
    words = np.concatenate([header(OP_COMMIT, c, n=n, n_rows=len(rows), S=S, row_stride=stride, flag=guest, sentinel=sentinel),
                            rows_words(rows, stride)])
    return Section(words, (len(rows) + sentinel) * S * 32, S=S, n_rows=len(rows), sentinel=sentinel)


def small_section(c, rows, SL, stride=None):
    n = len(rows[0])
    stride = 32 * n if stride is None else stride
    assert 1 <= len(rows) <= SMALL_MAX_ROWS
    words = np.concatenate([header(OP_SMALL, c, n=n, n_rows=len(rows), S=SL, row_stride=stride), rows_words(rows, stride)])
    return Section(words, len(rows) * SL * 32 + len(rows) * 32 + SMALL_MAX_ROWS + 2, SL=SL, n_rows=len(rows))


def fold_section(c, partials, S, sentinel=0):
    """partials: [n_rows * S][32] words"""
    n_rows = len(partials) // S
    words = np.concatenate([header(OP_FOLD, c, n_rows=n_rows, S=S, sentinel=sentinel), np.asarray(partials, dtype=np.uint32).reshape(-1)])
    return Section(words, (n_rows + sentinel) * S * 32, S=S, n_rows=n_rows)


def finish_section(c, partials, S, per_lane, sentinel=0):
    n_rows = len(partials) // S
    words = np.concatenate([header(OP_FINISH, c, n_rows=n_rows, S=S, flag=per_lane, sentinel=sentinel),
                            np.asarray(partials, dtype=np.uint32).reshape(-1)])
    return Section(words, (n_rows + sentinel) * 16, S=S, n_rows=n_rows)


def run_file(curve, words, timeout=600):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in"), os.path.join(d, "out")
        np.asarray(words, dtype=np.uint32).tofile(src)
        r = subprocess.run([EXE, curve, src, dst], capture_output=True, text=True, timeout=timeout)
        out = np.fromfile(dst, dtype=np.uint32) if r.returncode == 0 and os.path.exists(dst) else None
        return r, out


def run(C, sections):
    """[Section] -> [output words of each], one process"""
    r, out = run_file(C.name, np.concatenate([s.words for s in sections]))
    assert r.returncode == 0, "fb_check failed (%d): %s%s" % (r.returncode, r.stdout, r.stderr)
    assert len(out) == sum(s.out_words for s in sections), "fb_check wrote %d words for %d" % (len(out), sum(s.out_words for s in sections))
    res, at = [], 0
    for s in sections:
        res.append(out[at:at + s.out_words])
        at += s.out_words
    return res


# ---------------------------------------------------------------- decoding what the kernels leave
OPERAND = ev.BOUNDS["operand"]          # X < 5p + eps, Y <= 4p, ZZ, ZZZ < p + eps: the widest bound a stored lazy-form point may have


def decode_mem(C, w32, where, final=False, key=OPERAND):
    """a memory-form XYZZ (32 words) -> the affine point it stands for (None = infinity, all-zero words), its form checked:
    final: canonical residues of the 2^256 form; else the lazy form within `key`'s bounds (secp256k1: canonical)"""
    if not w32.any():
        return None
    vals = ev.get_words(w32, 0)
    assert vals[2] != 0 and vals[3] != 0, "%s: a finite point stored with an all-zero ZZ or ZZZ" % where
    p = C.p
    if final or C is ev.SECP:
        assert all(v < p for v in vals), "%s: not canonical" % where
    else:
        bx, by, bz = [ev.bound(C, e) for e in key]
        assert vals[0] < bx and vals[1] < by and vals[2] < bz and vals[3] < bz, "%s: value bound %s" % (where, [v / p for v in vals])
    f = pow(C.r32 if final else C.r30, -1, p)
    X, Y, ZZ, ZZZ = [v * f % p for v in vals]
    assert ZZ and ZZZ, "%s: ZZ or ZZZ = 0 mod p" % where
    assert pow(ZZ, 3, p) == ZZZ * ZZZ % p, "%s: ZZ^3 != ZZZ^2" % where
    return (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)


def out_bytes(C, pt):
    """k_fb_finish's 64 bytes as 16 words"""
    b = bytes(64) if pt is None else pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")
    return np.frombuffer(b, dtype=np.uint32)


# ---------------------------------------------------------------- table: expected entries and structural boundaries
def entry_scalar(C, c, w, k):
    return ((k + 1) << (c * w)) % order(C)


class PairMultiples:
    """(k + 1) B for k < H by a two-level table of B's multiples: lo[j] = j B (j < 1024), hi[j] = 1024 j B"""
    def __init__(self, C, B, H):
        self.C = C
        self.lo = [None]
        for _ in range(min(H, 1023)):
            self.lo.append(ev.ec_add(C, self.lo[-1], B))
        self.hi = [None]
        if H > 1023:
            step = ev.ec_add(C, self.lo[1023], B)
            for _ in range(H >> 10):
                self.hi.append(ev.ec_add(C, self.hi[-1], step))

    def entries(self, ks):
        return ec_add_batch(self.C, [(self.hi[(k + 1) >> 10], self.lo[(k + 1) & 1023]) for k in ks])


def expected_entries(C, c, b, ks_by_w):
    """{w: [k]} -> {w: [point of entry (w, k) of base point b G]}"""
    if b is None:
        return {w: [None] * len(ks) for w, ks in ks_by_w.items()}
    H = 1 << (c - 1)
    return {w: PairMultiples(C, mul_g(C, (b << (c * w)) % order(C)), H).entries(ks) for w, ks in ks_by_w.items()}


def boundaries(c):
    """entries k (< H) of ONE pair at the structural boundaries of k_fb_multiples' lane groups: the first and the last entry of every
    run, both sides of every k * lanes stride inside a run, and the in-group doubling entry (lane `lanes - 1` of run 0 starts at
    lanes B = acc and adds step = lanes B: entry 2 lanes - 1)"""
    p = table_plan(c, 1)
    H, lanes, K, runs = p["H"], p["lanes"], p["K"], p["runs"]
    run = lanes * K
    ks = set()
    for j in range(runs):
        ks |= {j * run, j * run + run - 1}
        for kk in range(1, K):
            ks |= {j * run + kk * lanes - 1, j * run + kk * lanes}
    doubling = 2 * lanes - 1 if K > 1 else None
    if doubling is not None:
        ks.add(doubling)
    assert all(0 <= k < H for k in ks)
    return sorted(ks), doubling


# ---------------------------------------------------------------- rows for the recoder runs
def recoder_bases(C, c):
    """a few distinct multiples of G -- as many (up to 11) as the driver's 2^23-entry cap admits at this window"""
    per_point = windows(C, c) << (c - 1)
    return [1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29][:max(1, min(11, MAX_ENTRIES // per_point))]


def recoder_rows(C, c):
    """rows of len(recoder_bases) coefficients: chosen member m of the families sits at coefficient j of row (m - j) mod M for every j
    (every member at every position: the first, a middle and the last coefficient of every slicing); the random members fill rows of
    their own.  -> (rows, labels of the members fed)"""
    fam = families(C.name, c)
    nc = len(recoder_bases(C, c))
    chosen = [k for f, k in fam if f != "random"]
    rnd = [k for f, k in fam if f == "random"]
    rows = [[chosen[(r + j) % len(chosen)] for j in range(nc)] for r in range(len(chosen))]
    for at in range(0, len(rnd), nc):
        rows.append([rnd[(at + j) % len(rnd)] for j in range(nc)])
    return rows, [f for f, _ in fam]


def row_scalar(C, bs, coeffs):
    """the row's sum as a multiple of G: sum (k_i mod order) b_i"""
    n = order(C)
    return sum((k % n) * b for k, b in zip(coeffs, bs) if b is not None) % n


def slice_ranges(n_coeffs, S):
    """k_fb_commit's coefficient range of every slice"""
    per = (n_coeffs + S - 1) // S
    return [(min(s * per, n_coeffs), min(s * per + per, n_coeffs)) for s in range(S)]


# ---------------------------------------------------------------- degenerate rows for k_fb_commit
COMMIT_C = 5
COMMIT_BASES = [1, 1, 1, 1, -1, 3, None, 7]         # G, G, G, G, -G, H = 3 G, infinity, 7 G


def commit_degenerate_rows(C, n_rows=300):
    """-> (rows, {label: row index}); base COMMIT_BASES, window COMMIT_C"""
    c, W, n = COMMIT_C, windows(C, COMMIT_C), order(C)
    rng = random.Random(0xC0DE)
    k, m = rng.randrange(1, n), rng.randrange(1, n)
    last = 1 << (c * (W - 1))
    assert last < n
    named = [
        ("doubling", [1, 1, 1, 1, 0, 0, 0, 0]),                 # G + G with the gathers in flight, then 2G + G, 3G + G
        ("equal_rows", [k, k, 0, 0, 0, 0, 0, 0]),               # the second coefficient walks the first one's digits again
        ("cancel_then", [k, 0, 0, 0, k, m, 0, 0]),              # k G - k G: infinity mid-row, then m H
        ("cancel_first", [1, 0, 0, 0, 1, 0, 0, 0]),             # G - G and nothing else
        ("cancel_end", [0, 0, 0, k, k, 0, 0, 0]),               # (S = 2: the two halves are opposite partials)
        ("last_window", [0, 0, 0, 0, 0, 0, 0, last]),           # the only non-zero digit is the last window of the last coefficient
        ("zero", [0] * 8),
        ("order", [n, 2 * n if 2 * n < 1 << 256 else n, 0, 0, 0, 0, 0, 0]),      # reduces to zero: infinity
        ("inf_between", [0, 0, 0, 0, 0, k, m, rng.randrange(1, n)]),
        ("inf_only", [0, 0, 0, 0, 0, 0, m, 0]),
    ]
    for label, coeffs in named:
        assert len(coeffs) == len(COMMIT_BASES), label
    rows, where = [], {}
    for label, coeffs in named:                                  # once at the front ...
        where[label] = [len(rows)]
        rows.append(coeffs)
    while len(rows) < n_rows - len(named):
        rows.append([rng.randrange(1 << 256) for _ in range(8)])
    for label, coeffs in named:                                  # ... and once in the ragged last block of 256 lanes
        where[label].append(len(rows))
        rows.append(coeffs)
    return rows, where


# ---------------------------------------------------------------- k_fb_commit_small: the model of its lanes and folds
def small_model(C, c, bs, coeffs, SL):
    """-> (the row's scalar, [scalar of each slice], meetings).  A lane's sum and every node of the two folds is a scalar mod the
    order (0 = infinity); meetings: [("lds", h, kind) | ("slice", step, kind)] with kind "eq" (P + P) or "opp" (P - P) wherever two
    FINITE sums meet in the LDS fold's level h = 1 .. 128 or in step 0, 1, .. of the last block's slice fold"""
    n, W = order(C), windows(C, c)
    P = len(coeffs) * W
    meetings, slices = [], []
    digs = {i: signed_digits(C, k, c) for i, k in enumerate(coeffs) if k % n and bs[i] is not None}
    for sl in range(SL):
        p0, p1 = sl * P // SL, (sl + 1) * P // SL
        lane = [0] * SMALL_THREADS
        for i, ds in digs.items():
            for w, d in enumerate(ds):
                pp = i * W + w
                if d and p0 <= pp < p1:
                    t = (pp - p0) % SMALL_THREADS
                    lane[t] = (lane[t] + (d << (c * w)) * bs[i]) % n
        h = 1
        while h < SMALL_THREADS:
            for t in range(SMALL_THREADS // (2 * h)):
                a, b = lane[t * 2 * h], lane[t * 2 * h + h]
                if a and b and a == b:
                    meetings.append(("lds", h, "eq"))
                elif a and b and (a + b) % n == 0:
                    meetings.append(("lds", h, "opp"))
                lane[t * 2 * h] = (a + b) % n
            h *= 2
        slices.append(lane[0])
    pts, cnt, step = list(slices), SL, 0
    while cnt > 1:
        half = (cnt + 1) // 2
        for t in range(cnt - half):
            a, b = pts[t], pts[t + half]
            if a and b and a == b:
                meetings.append(("slice", step, "eq"))
            elif a and b and (a + b) % n == 0:
                meetings.append(("slice", step, "opp"))
            pts[t] = (a + b) % n
        cnt, step = half, step + 1
    return pts[0], slices, meetings


SMALL_C, SMALL_COEFFS = 7, 128              # W = 37 on both curves: 4736 (coefficient, window) pairs, lane = pair mod 256 at SL = 1


@functools.lru_cache(maxsize=None)
def small_degenerate(name):
    """-> (bases b_i, rows, labels).  Every LDS level h and the slice folds of SL = 2 and SL = 3 get a row each for "eq" and "opp": a
    row has two non-zero digits 1, in two coefficients kept for it, at pairs that land in lanes (or slices) that meet exactly there; the
    second coefficient's base point is +-2^(c (wL - wR)) times the first's, so the two lane sums are equal or opposite."""
    C = ev.CURVES[name]
    c, n, W, NC = SMALL_C, order(C), windows(C, SMALL_C), SMALL_COEFFS
    assert W == 37
    rng = random.Random(0x5A11)
    bs = [i + 2 for i in range(NC)]
    used = set()
    rows, labels = [], []
    inv2c = pow(1 << c, -1, n)

    def claim(ok):
        """an unused coefficient i and window w with ok(i W + w)"""
        for i in range(NC):
            if i not in used:
                for w in range(W):
                    if ok(i * W + w):
                        used.add(i)
                        return i, w
        raise AssertionError("no coefficient left")

    def pair_row(label, okL, okR):
        for kind, sign in (("eq", 1), ("opp", -1)):
            (iL, wL), (iR, wR) = claim(okL), claim(okR)
            m = rng.randrange(1, n)
            bs[iL] = m
            bs[iR] = sign * m * (pow(1 << c, wL - wR, n) if wL >= wR else pow(inv2c, wR - wL, n)) % n
            coeffs = [0] * NC
            coeffs[iL], coeffs[iR] = 1 << (c * wL), 1 << (c * wR)
            rows.append(coeffs)
            labels.append((label, kind))

    P = NC * W
    h = 1
    while h < SMALL_THREADS:
        L = 2 * h if 4 * h <= SMALL_THREADS else 0
        pair_row(("lds", h), lambda p, L=L: p % SMALL_THREADS == L, lambda p, L=L, h=h: p % SMALL_THREADS == L + h)
        h *= 2
    sl = lambda SL, s: (lambda p: s * P // SL <= p < (s + 1) * P // SL)
    pair_row(("slice2", 0), sl(2, 0), sl(2, 1))
    pair_row(("slice3", 0), sl(3, 0), sl(3, 2))
    pair_row(("slice3", 1), sl(3, 0), sl(3, 1))
    rows.append([0] * NC)
    labels.append(("zero", None))
    dense = [rng.randrange(1 << 256) for _ in range(NC)]
    rows.append(dense)
    labels.append(("dense", None))
    sparse = [0] * NC
    sparse[3], sparse[77] = rng.randrange(1, n), 5
    rows.append(sparse)
    labels.append(("sparse", None))
    while len(rows) < SMALL_MAX_ROWS:                        # FB_SMALL_MAX_ROWS rows: a few random coefficients each
        coeffs = [0] * NC
        for _ in range(3):
            coeffs[rng.randrange(NC)] = rng.randrange(1 << 256)
        rows.append(coeffs)
        labels.append(("fill", None))
    return bs, rows, labels


# ---------------------------------------------------------------- k_fb_fold_quad
@functools.lru_cache(maxsize=None)
def small_multiples(name, count=8192):
    C = ev.CURVES[name]
    t = [None]
    for _ in range(count):
        t.append(ev.ec_add(C, t[-1], C.g))
    return t


def small_point(C, m):
    """m G for a small signed m"""
    t = small_multiples(C.name)
    return t[m] if m >= 0 else ev.ec_neg(C, t[-m])


def fold_model(scalars, S):
    """k_fb_fold_quad on one row's slot scalars (small signed integers, 0 = infinity): level n = S/2 .. 1 adds slot q + n to slot q.
    -> (sum, meetings [(n, q, kind)])"""
    a, meetings, n = list(scalars), [], S // 2
    while n >= 1:
        for q in range(n):
            x, y = a[q], a[q + n]
            if x and y and x == y:
                meetings.append((n, q, "eq"))
            elif x and y and x == -y:
                meetings.append((n, q, "opp"))
            a[q] = x + y
        n //= 2
    return a[0], meetings


def fold_rows(S, seed):
    """-> [(label, [S slot scalars])]: all distinct, infinity scattered, all infinity, and for every level n a row whose slot q meets
    its equal in slot q + n at that level, and one where it meets its opposite (a dense row: one slot is set so that the two running
    sums coincide)"""
    rng = random.Random(seed)
    nz = lambda: rng.choice([-1, 1]) * rng.randint(1, 30)
    rows = [("distinct", [3 * s + 1 for s in range(S)]),
            ("scattered", [nz() if rng.random() < 0.5 else 0 for _ in range(S)]),
            ("all_inf", [0] * S)]
    n = S // 2
    while n >= 1:
        for kind, sign in (("eq", 1), ("opp", -1)):
            a = [nz() for _ in range(S)]
            q = rng.randrange(n)
            A = sum(a[s] for s in range(S) if s % (2 * n) == q)
            B = sum(a[s] for s in range(S) if s % (2 * n) == q + n) - a[q + n]
            while A == 0 or sign * A - B == 0:
                a[q] += 1
                A += 1
            a[q + n] = sign * A - B
            rows.append(((n, q, kind), a))
        n //= 2
    return rows


def fold_layout(S):
    """rows of one fold section: the labelled rows, then distinct rows up to a count that leaves padding quads in the last block
    (128 / S rows per block; at S = 128 every block is one row)"""
    rows = fold_rows(S, 0xF01D + S)
    per_block = 128 // S
    k = 0
    while len(rows) < 2 * per_block + 1 or (per_block > 1 and len(rows) % per_block == 0):
        rows.append(("fill", [7 * s + 2 + k for s in range(S)]))
        k += 1
    rows.append(rows.pop(3))                                      # a labelled degenerate row sits in the ragged last block
    return rows


def fold_partials(C, rows, S, seed):
    """the rows' slots in the lazy memory form, within the operand bounds of ec30.hip.h (ev.rep_mem): free l, random multiples of p,
    every fourth point at the top of its bound"""
    rng = random.Random(seed)
    out = np.zeros((len(rows) * S, 32), dtype=np.uint32)
    for r, (_, a) in enumerate(rows):
        for s, m in enumerate(a):
            if m:
                top = "top" if (r + s) % 4 == 0 else None
                vals = ev.rep_mem(C, small_point(C, m), rng.randrange(1, C.p), mult=top, rng=rng)
                out[r * S + s] = np.concatenate([le_words(v) for v in vals])
    return out


# ---------------------------------------------------------------- k_fb_finish
def finish_rows(per_lane, n_rows):
    """row scalars (0 = infinity): finite rows; lane t of block 0 (t < 16) has an infinity row in position t mod per_lane of its rows;
    lane 20's rows are all infinity; rows of the ragged last block: lane 3 infinity"""
    a = [r + 1 for r in range(n_rows)]
    if n_rows == 1:
        return a
    for t in range(16):
        r = t + 64 * (t % per_lane)
        if r < n_rows:
            a[r] = 0
    for k in range(per_lane):
        if 20 + 64 * k < n_rows:
            a[20 + 64 * k] = 0
    if 64 * per_lane + 3 < n_rows:
        a[64 * per_lane + 3] = 0
    return a


def finish_partials(C, scalars, S, seed):
    """partial[row * S] in the canonical 2^256 form (ev.rep32, free l); the slots between hold the sentinel: never read"""
    rng = random.Random(seed)
    out = np.full((len(scalars) * S, 32), SENTINEL, dtype=np.uint32)
    for r, m in enumerate(scalars):
        if m:
            out[r * S] = np.concatenate([le_words(v) for v in ev.rep32(C, small_point(C, m), rng.randrange(1, C.p))])
        else:
            out[r * S] = 0
    return out


# ---------------------------------------------------------------- --plan
PLAN_C = list(range(2, 21))
PLAN_COMMIT = [
    # the 393 216 target: n_rows * S crosses it at S = 128, 64, 2, 1
    (3071, 128, 15), (3072, 128, 15), (3073, 128, 15), (6143, 128, 15), (6144, 128, 15), (6145, 128, 15),
    (196607, 128, 15), (196608, 128, 15), (196609, 128, 15), (393215, 128, 15), (393216, 128, 15), (393217, 128, 15),
    # the 131 072-row rule: fewer than 16 additions per lane
    (131071, 2, 15), (131072, 2, 15), (131072, 2, 16), (131072, 4, 15), (131072, 4, 8), (131072, 4, 7), (131071, 128, 1),
    (131072, 128, 1), (131072, 128, 2), (65536, 2, 15), (131072, 64, 13), (131072, 3, 13),
    # S capped by n_coeffs, and by 128
    (1, 1, 15), (1, 2, 15), (1, 3, 15), (1, 37, 15), (1, 127, 15), (1, 128, 15), (1, 129, 15), (1, 255, 15), (1, 256, 15),
    (1, 257, 13), (1, 1000, 15), (1, 65535, 13), (2, 128, 15), (64, 128, 13), (300, 8, 51), (32768, 128, 15),
    # SL: 256 pairs per slice, at most FB_SMALL_MAX_SLICES
    (1, 17, 15), (1, 18, 15), (1, 136, 15), (1, 137, 15), (1, 256, 16), (1, 128, 37), (1, 1, 128), (1, 2, 129),
]
PLAN_ROWS = [1, 64, 32767, 32768, 32769, 65535, 65536, 65537, 1000000]


def plan_args():
    return ["c"] + [str(c) for c in PLAN_C] + ["commit"] + [str(v) for g in PLAN_COMMIT for v in g] + ["rows"] + [str(r) for r in PLAN_ROWS]


def dump_plan():
    """the text of fb_check --plan for both curves"""
    out = ""
    for curve in ("bn254", "secp256k1"):
        r = subprocess.run([EXE, "--plan", curve] + plan_args(), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out += r.stdout
    return out

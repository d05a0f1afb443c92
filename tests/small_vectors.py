"""Models, vectors and expected values for the block-by-block checks of the single-launch MSM (tools/small_check.hip, which launches
porla_amd/csrc/msm_small.hip.h's own k_small_msm): shared by tests/test_small_block_gpu.py, tests/test_small_vectors_cpu.py and
tests/test_msm_small_shape_cpu.py.

Everything here is Python integers.  Every point of every section is a known multiple m_i G (m_i signed, from a pool of at most 512
magnitudes; 0 = infinity), so every sum a block, a window or a launch leaves is ONE scalar mod the group order: a + lambda b, a the
weight that reached it through first sub-scalars and b through second ones (phi(P) = lambda P), both small integers.  G has prime
order, so two such sums are the same point exactly when their scalars agree -- which is how the models know where equal or opposite
points meet inside the kernel.

RESTATED from msm_small.hip.h:
  small_cfg                   the shape (split flag, L, c, W, S) from n, the scalars' bit length, c_flags and the blocks: restated_cfg,
                              float32 step by step as the C++ evaluates it
  small_block step 1          a scalar of 250 bits or more is reduced mod the order first; over 128 bits it is split (the model of
                              tools/gen_glv.py, which tests/test_glv_cpu.py pins to the compiled split); window w of a sub-scalar is the
                              signed digit of the recoding "digit > B = 2^(c-1): subtract 2^c and carry", walked here from window 0
                              (the kernel finds the carry with one masked compare); the digit's sign times the sub-scalar's sign goes
                              with the entry; the top window has cw = L + 1 - c (W - 1) bits and no negative digit
  blocks                      block bx = w S + s owns window w of the scalars [s n / S, (s + 1) n / S)
  the c sums of a block       S = the sum of its buckets, M_j = the sum of the buckets whose index (magnitude - 1) has bit j set
                              (tests/tree_vectors.py:fin_exponents), j < cw - 1; the sums beyond the window's own width are infinity
  fin[w c + k]                sum k of window w over all slices; the launch's value is sum_w 2^(c w) (S_w + sum_j 2^j M_w,j)
                              (host_fold64.hpp:h_fold_tree64)
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
from tests import fb_vectors as fv

EXE = os.path.join(common.ROOT, "porla_amd", "small_check")
MAGIC, HDR = 0x534d4b31, 16
SENTINEL = ev.SENTINEL
SMALL_MAX_N, SMALL_MAX_C, SMALL_MAX_SUB, SMALL_MAX_S, SMALL_DONE_SLOT = 32768, 8, 8192, 32, 255
SMALL_THREADS, SMALL_BLOCKS = 256, 256
SMALL_PAIR_STRIDE, XYZZ_BYTES, HDR_BYTES, HDR_WORDS = 64 * 1024, 128, 128, 32
SENTINEL_ENTRIES, COUNTER_WORDS = 8, 513                 # tools/small_check.hip
GLV_BITS = {0: 126, 1: 128}                              # glv.hip.h
SCALAR_BITS = {0: 254, 1: 256}                           # msm.hip.h
CURVE_ID = {"bn254": 0, "secp256k1": 1}
LONE, PAIR, HINT, ANY = 0, 1, 2, 3                       # include/porla_gpu.h: PORLA_SMALL_FORM_*
NO_SPLIT = 0x100
F = np.float32
POOL_SIZE = 512


# ---------------------------------------------------------------- the shape function, restated
def blocks_of(form, n):
    """small_lone_blocks / small_pair_blocks"""
    n = np.asarray(n)
    return np.where(n <= 4096, 192, 256) if form == LONE else np.where(n <= 8192, 96, 128)


def scalar_length(curve, used_bits, c_flags):
    """(split flag, L): the bits a sub-scalar can have"""
    glv = 1 if (used_bits > 128 and not (c_flags & NO_SPLIT)) else 0
    L = GLV_BITS[curve] if glv else (1 if used_bits < 1 else (SCALAR_BITS[curve] if used_bits >= 250 else used_bits))
    return glv, L


def restated_cfg(curve, n, used_bits, c_flags, blocks, recheck_fallback=True):
    """small_cfg for arrays n / blocks and one (curve, used_bits, c_flags): (glv, c, W, S, n_sub, fits).  recheck_fallback=False is the
    rule before the fit check: the fallback is taken on trust and every shape counts as fitting."""
    n = np.asarray(n, dtype=np.int64)
    blocks = np.asarray(blocks, dtype=np.int64)
    c_override = c_flags & 0xff
    glv, L = scalar_length(curve, used_bits, c_flags)
    n_sub = 2 * n if glv else n
    best_c = np.zeros(len(n), dtype=np.int64)
    best_cost = np.full(len(n), 1e30, dtype=F)
    gW, gS = np.zeros(len(n), dtype=np.int64), np.zeros(len(n), dtype=np.int64)
    for c in range(1, SMALL_MAX_C + 1):
        if 1 <= c_override <= SMALL_MAX_C and c != c_override:
            continue
        W = (L + c) // c
        ok = (W <= blocks) & (W < SMALL_DONE_SLOT)
        S = (blocks.astype(F) / F(W)).astype(np.int64)
        S = np.minimum(S, (n_sub + 7) // 8)
        S = np.minimum(S, SMALL_MAX_S)
        S = np.maximum(S, 1)
        ok &= (n_sub + S - 1) // S <= SMALL_MAX_SUB
        Bf = F(1 << (c - 1 if c > 1 else 0))
        per_bucket = n_sub.astype(F) / S.astype(F) * ((F(1.0) - F(1.0) / F(1 << c)) / Bf)
        lanes = F(256.0) / Bf
        per_lane = (per_bucket + F(3.0) * np.sqrt(per_bucket, dtype=F)) / lanes
        chain = per_lane.astype(np.int64)
        chain = chain + (chain.astype(F) < per_lane)
        lv = np.zeros(len(n), dtype=np.int64)
        for k in range(6):
            lv += (1 << k) < S
        recode = ((n.astype(F) / S.astype(F)).astype(np.int64) + 255) // 256
        cost = F(18.0) * np.maximum(chain - 1, 0).astype(F) + F(7.0) * (8 + lv).astype(F)
        cost = cost + F(4.0 if glv else 2.0) * recode.astype(F)
        cost = cost + F(0.01) * F(W)
        assert cost.dtype == F and per_lane.dtype == F
        take = ok & (cost < best_cost)
        best_cost = np.where(take, cost, best_cost)
        best_c = np.where(take, c, best_c)
        gW = np.where(take, W, gW)
        gS = np.where(take, S, gS)
    fb = best_c == 0
    Wf = (L + 1 + SMALL_MAX_C - 1) // SMALL_MAX_C
    Sf = np.clip(blocks // Wf, 1, SMALL_MAX_S)
    c_out = np.where(fb, SMALL_MAX_C, best_c)
    W_out = np.where(fb, Wf, gW)
    S_out = np.where(fb, Sf, gS)
    fits = (W_out <= blocks) & ((n_sub + S_out - 1) // S_out <= SMALL_MAX_SUB) if recheck_fallback else np.ones(len(n), dtype=bool)
    return np.full(len(n), glv), c_out, W_out, S_out, n_sub, fits


# ---------------------------------------------------------------- the curve's constants and the point pool
@functools.lru_cache(maxsize=None)
def glv(name):
    sys.path.insert(0, os.path.join(common.ROOT, "tools"))
    try:
        import gen_glv
    finally:
        sys.path.pop(0)
    key = {"bn254": "Bn254", "secp256k1": "Secp256k1"}[name]
    return gen_glv, gen_glv.derive(key, gen_glv.CURVES[key])


def order(C):
    return fv.order(C)


def lam(C):
    return glv(C.name)[1]["lam"]


def phi(C, pt):
    """(beta x, y) with the beta that goes with lam"""
    return None if pt is None else (glv(C.name)[1]["beta"] * pt[0] % C.p, pt[1])


@functools.lru_cache(maxsize=None)
def pool(name):
    """the magnitudes m of the pool's points m G: at most 512, distinct"""
    rng = random.Random("small pool " + name)
    ms = [1, 2, 3, 4, 5, 6, 7, 8]
    while len(ms) < POOL_SIZE:
        m = rng.randrange(9, 1 << 16)
        if m not in ms:
            ms.append(m)
    return ms


_POINT_BYTES = {}


def point_bytes(C, m, lift=(0, 0)):
    """the 64 wire bytes of m G (m signed; 0 = infinity); lift: multiples of p added to (x, y), where they still fit 32 bytes"""
    key = (C.name, m, lift)
    if key not in _POINT_BYTES:
        if m == 0:
            x, y = 0, 0
        else:
            pt = fv.mul_g(C, abs(m))
            x, y = pt if m > 0 else ev.ec_neg(C, pt)
        x, y = x + lift[0] * C.p, y + lift[1] * C.p
        assert x < 1 << 256 and y < 1 << 256, "a lifted coordinate no longer fits"
        _POINT_BYTES[key] = x.to_bytes(32, "big") + y.to_bytes(32, "big")
    return _POINT_BYTES[key]


_LIN = {}


def lin_point(C, a, b):
    """(a + lambda b) G = a G + phi(b G) for small signed a, b"""
    key = (C.name, a, b)
    if key not in _LIN:
        def small(v):
            pt = fv.mul_g(C, abs(v)) if v else None
            return ev.ec_neg(C, pt) if v < 0 else pt
        _LIN[key] = ev.ec_add(C, small(a), phi(C, small(b)))
    return _LIN[key]


def lin_value(C, a, b):
    return (int(a) + lam(C) * int(b)) % order(C)


# ---------------------------------------------------------------- sections
class Section:
    """one launch shape on chosen inputs.  scalars: n integers below 2^256; ms: per point set n signed multipliers of G (0 = infinity);
    lifts: {(set, i): (kx, ky)} multiples of p added to that point's coordinates"""
    def __init__(self, C, name, scalars, ms, blocks, c_flags=0, hint=0, stride=SMALL_PAIR_STRIDE, seq=1, launches=1, refusal=0, lifts=None):
        self.C, self.name, self.scalars, self.ms = C, name, list(scalars), [list(m) for m in ms]
        self.n, self.sets, self.blocks = len(self.scalars), len(self.ms), int(blocks)
        self.c_flags, self.hint, self.stride, self.seq, self.launches, self.refusal = c_flags, hint, stride, seq, launches, refusal
        self.lifts = dict(lifts or {})
        assert 1 <= self.n <= SMALL_MAX_N and self.sets in (1, 2) and all(len(m) == self.n for m in self.ms)
        assert all(0 <= k < 1 << 256 for k in self.scalars)
        mags = {abs(m) for s in self.ms for m in s if m}
        assert len(mags) <= POOL_SIZE, "more than %d distinct points" % POOL_SIZE
        self.part_words = (self.sets * self.blocks * SMALL_MAX_C + SENTINEL_ENTRIES) * 32
        self.pin_words = self.sets * self.stride // 4 + SENTINEL_ENTRIES * 32
        self.launch_words = self.part_words + COUNTER_WORDS + self.pin_words
        self.out_words = self.launch_words * self.launches

    @property
    def used_bits(self):
        return max(k.bit_length() for k in self.scalars)

    def words(self):
        h = np.zeros(HDR, dtype=np.uint32)
        h[:10] = [MAGIC, self.n, self.blocks, self.sets, self.c_flags, self.hint, self.stride, self.seq, self.launches, self.refusal]
        sc = b"".join(k.to_bytes(32, "big") for k in self.scalars)
        pt = b"".join(point_bytes(self.C, m, self.lifts.get((s, i), (0, 0))) for s in range(self.sets) for i, m in enumerate(self.ms[s]))
        return np.concatenate([h, np.frombuffer(sc, dtype=np.uint32), np.frombuffer(pt, dtype=np.uint32)])


class Launch:
    """what one launch left: part[set][block][k] (32 words each), the sentinel entries behind part, the counters, and per set the
    header words, the region behind them, and the words behind the last region"""
    def __init__(self, sec, w):
        at = 0
        own = sec.sets * sec.blocks * SMALL_MAX_C * 32
        self.part = w[:own].reshape(sec.sets, sec.blocks, SMALL_MAX_C, 32)
        self.part_tail = w[own:sec.part_words]
        at = sec.part_words
        self.counters = w[at:at + COUNTER_WORDS]
        at += COUNTER_WORDS
        regions = w[at:at + sec.sets * sec.stride // 4].reshape(sec.sets, sec.stride // 4)
        self.hdr = regions[:, :HDR_WORDS]
        self.fin = regions[:, HDR_WORDS:]
        self.pin_tail = w[at + sec.sets * sec.stride // 4:at + sec.pin_words]
        assert at + sec.pin_words == len(w)


def run(C, sections, timeout=300):
    """[Section] -> [[Launch] of each], one driver process"""
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in"), os.path.join(d, "out")
        np.concatenate([s.words() for s in sections]).tofile(src)
        r = subprocess.run(["timeout", "-k", "10", str(timeout), EXE, C.name, src, dst], capture_output=True, text=True, timeout=timeout + 30)
        assert r.returncode == 0, "small_check failed (%d): %s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        out = np.fromfile(dst, dtype=np.uint32)
    assert len(out) == sum(s.out_words for s in sections), "small_check wrote %d words for %d" % (len(out), sum(s.out_words for s in sections))
    res, at = [], 0
    for s in sections:
        res.append([Launch(s, out[at + l * s.launch_words:at + (l + 1) * s.launch_words]) for l in range(s.launches)])
        at += s.out_words
    return res


# ---------------------------------------------------------------- the model of one launch
def sub_scalars(C, k, split, reduce):
    """[(magnitude, sign)] of the sub-scalars of k: the scalar itself, or the two halves of the endomorphism split"""
    if reduce:
        k %= order(C)
    if not split:
        return [(k, 0)]
    gen_glv, d = glv(C.name)
    return gen_glv.split_model(d, k)


def signed_digits(mag, c, W, L):
    """digits in (-B, B], B = 2^(c-1), by the carry walk from window 0; -> (digits, raw values = bits + carry in)"""
    assert mag.bit_length() <= L
    B, out, raws, carry = 1 << (c - 1), [], [], 0
    for w in range(W):
        raw = ((mag >> (c * w)) & ((1 << c) - 1)) + carry
        raws.append(raw)
        if raw > B:
            out.append(raw - (1 << c))
            carry = 1
        else:
            out.append(raw)
            carry = 0
    top = L + 1 - c * (W - 1)
    assert carry == 0 and 1 <= top <= c and 0 <= out[-1] <= 1 << (top - 1), "the top window overflows"
    assert sum(d << (c * w) for w, d in enumerate(out)) == mag
    return out, raws


class Model:
    pass


def model(sec, keep_buckets=False):
    """the launch on Python integers: the shape, and per set and block the c sums as (a, b) weights (sum = (a + lambda b) G)"""
    C, n = sec.C, sec.n
    cid = CURVE_ID[C.name]
    eff = sec.hint if sec.hint else sec.used_bits          # the kernel's `used`
    assert not sec.hint or sec.used_bits <= sec.hint
    g, c, W, S, n_sub, fits = [int(v[0]) for v in restated_cfg(cid, [n], eff, sec.c_flags, [sec.blocks])]
    m = Model()
    m.glv, m.c, m.W, m.S, m.fits = g, c, W, S, bool(fits)
    m.L = scalar_length(cid, eff, sec.c_flags)[1]
    m.top = m.L + 1 - c * (W - 1)
    m.reduce = eff >= 250
    m.subs = 2 if g else 1
    m.bounds = [(s * n // S, (s + 1) * n // S) for s in range(S)]
    if not m.fits:
        return m
    uniq = sorted(set(sec.scalars))
    at = {k: j for j, k in enumerate(uniq)}
    sid = np.array([at[k] for k in sec.scalars], dtype=np.int64)
    D = np.zeros((len(uniq), m.subs, W), dtype=np.int64)
    R = np.zeros((len(uniq), m.subs, W), dtype=np.int64)
    for j, k in enumerate(uniq):
        for e, (mag, neg) in enumerate(sub_scalars(C, k, g, m.reduce)):
            ds, raws = signed_digits(mag, c, W, m.L)
            D[j, e] = [-d if neg else d for d in ds]
            R[j, e] = raws
    m.digits, m.raws, m.sid = D, R, sid
    ms = [np.array(x, dtype=np.int64) for x in sec.ms]
    m.sums = np.zeros((sec.sets, W * S, SMALL_MAX_C, 2), dtype=np.int64)
    m.buckets = {}
    Bfull = 1 << (c - 1)
    idx = np.arange(Bfull)
    for w in range(W):
        cw = m.top if w == W - 1 else c
        for s, (i0, i1) in enumerate(m.bounds):
            for e in range(m.subs):
                d = D[sid[i0:i1], e, w]
                nz = d != 0
                b, sg = np.abs(d[nz]) - 1, np.sign(d[nz])
                assert len(b) == 0 or b.max() < 1 << (cw - 1)
                for st in range(sec.sets):
                    bk = np.rint(np.bincount(b, weights=(sg * ms[st][i0:i1][nz]).astype(np.float64), minlength=Bfull)).astype(np.int64)
                    m.sums[st, w * S + s, 0, e] = bk.sum()
                    for j in range(cw - 1):
                        m.sums[st, w * S + s, 1 + j, e] = bk[((idx >> j) & 1) == 1].sum()
                    if keep_buckets:
                        m.buckets.setdefault((st, w * S + s), np.zeros((Bfull, 2), dtype=np.int64))[:, e] = bk
    m.fin = m.sums.reshape(sec.sets, W, S, SMALL_MAX_C, 2).sum(axis=2)
    return m


def launch_value(C, m, st):
    """sum_w 2^(c w) (S_w + sum_j 2^j M_w,j) mod the order, from the blocks' sums"""
    n, total = order(C), 0
    for w in range(m.W):
        for s in range(m.S):
            t = m.sums[st, w * m.S + s]
            v = lin_value(C, t[0, 0], t[0, 1]) + sum(lin_value(C, t[1 + j, 0], t[1 + j, 1]) << j for j in range(m.c - 1))
            total += v << (m.c * w)
    return total % n


def msm_value(sec, st):
    n = order(sec.C)
    return sum(k * mi for k, mi in zip(sec.scalars, sec.ms[st])) % n


# ---------------------------------------------------------------- where equal and opposite sums meet
def _meet(a, b, n):
    if a and b and a == b:
        return "eq"
    if a and b and (a + b) % n == 0:
        return "opp"
    return None


def slice_meetings(C, m, st, w):
    """[(step, kind)]: the last block's fold of the S slices' sums of window w (half = (cnt + 1) / 2), any of the c sums"""
    n, out = order(C), []
    pts = [[lin_value(C, *m.sums[st, w * m.S + s, k]) for k in range(m.c)] for s in range(m.S)]
    cnt, step = m.S, 0
    while cnt > 1:
        half = (cnt + 1) // 2
        for t in range(cnt - half):
            for k in range(m.c):
                kind = _meet(pts[t][k], pts[t + half][k], n)
                if kind:
                    out.append((step, kind))
                pts[t][k] = (pts[t][k] + pts[t + half][k]) % n
        cnt, step = half, step + 1
    return out


def tree_meetings(C, m, st, bx):
    """[("S" | "M", level, kind)]: step 3b on the block's bucket sums (model(..., keep_buckets=True))"""
    n, out = order(C), []
    w = bx // m.S
    cw = m.top if w == m.W - 1 else m.c
    B, nlev = 1 << (cw - 1), cw - 1
    Ss = [[lin_value(C, *v) for v in m.buckets[(st, bx)][:B]]]
    M = []
    for l in range(nlev):
        nw = B >> (l + 1)
        newM = []
        for s in range(l):
            if s == l - 1:
                src = Ss[l - 1]
                ops = [(src[4 * i + 1], src[4 * i + 3]) for i in range(nw)]
            else:
                ops = [(M[s][2 * i], M[s][2 * i + 1]) for i in range(nw)]
            out += [("M", l, k) for k in (_meet(a, b, n) for a, b in ops) if k]
            newM.append([(a + b) % n for a, b in ops])
        ops = [(Ss[-1][2 * i], Ss[-1][2 * i + 1]) for i in range(nw)]
        out += [("S", l, k) for k in (_meet(a, b, n) for a, b in ops) if k]
        Ss.append([(a + b) % n for a, b in ops])
        M = newM
    return out


def lane_fold_meetings(C, lanes):
    """[(h, kind)]: step 3a on one bucket's lane sums (multipliers of G, 0 = infinity; a power of two of them)"""
    n, v, out, h = order(C), [x % order(C) for x in lanes], [], 1
    while h < len(v):
        for t in range(len(v) // (2 * h)):
            a, b = v[t * 2 * h], v[t * 2 * h + h]
            kind = _meet(a, b, n)
            if kind:
                out.append((h, kind))
            v[t * 2 * h] = (a + b) % n
        h *= 2
    return out


def lane_fold_levels(cw):
    """levels h = 1, 2, .. of step 3a for a window of cw bits: T = 256 / 2^(cw-1) lanes per bucket"""
    T = SMALL_THREADS >> (cw - 1)
    return [h for h in (1, 2, 4, 8, 16, 32, 64, 128) if h < T]


# ---------------------------------------------------------------- the families of sections
def _rng(name, tag):
    return random.Random("small %s %s" % (name, tag))


def rand_scalars(rng, n, bits, distinct=256, extra=()):
    """n scalars of at most `bits` bits from a set of `distinct` random ones (+ extra); one has exactly `bits` bits"""
    base = [(1 << (bits - 1)) | 1] + [rng.getrandbits(bits) for _ in range(distinct - 1)] + list(extra)
    out = base[:n] + [rng.choice(base) for _ in range(max(0, n - len(base)))]
    rng.shuffle(out)
    return out


def rand_ms(rng, name, n, zeros=0):
    ms = [rng.choice((-1, 1)) * rng.choice(pool(name)) for _ in range(n)]
    for i in rng.sample(range(n), zeros):
        ms[i] = 0
    return ms


def lone_blocks(n):
    return int(blocks_of(LONE, [n])[0])


def pair_blocks(n):
    return int(blocks_of(PAIR, [n])[0])


@functools.lru_cache(maxsize=None)
def capacity(name):
    """the largest launches that fit: a slice of exactly 8 192 sub-scalars, the local index 8 191 beside the sign bit"""
    C, rng = ev.CURVES[name], _rng(name, "capacity")
    full = lambda n: rand_scalars(rng, n, 256)
    if name == "bn254":
        return [Section(C, "pair 32768", full(32768), [rand_ms(rng, name, 32768), rand_ms(rng, name, 32768)], 128)]
    return [Section(C, "pair 28672 split on", full(28672), [rand_ms(rng, name, 28672), rand_ms(rng, name, 28672)], 128),
            Section(C, "pair 24576 split off", full(24576), [rand_ms(rng, name, 24576), rand_ms(rng, name, 24576)], 128, c_flags=NO_SPLIT),
            Section(C, "lone 32768", full(32768), [rand_ms(rng, name, 32768)], 256)]


@functools.lru_cache(maxsize=None)
def refusal(name):
    """an unfit shape: secp256k1, 32 768 pairs of full scalars on 128 blocks per set -- k_small_msm must leave without a write"""
    C, rng = ev.CURVES[name], _rng(name, "refusal")
    assert name == "secp256k1"
    return [Section(C, "refused", rand_scalars(rng, 32768, 256), [rand_ms(rng, name, 32768), rand_ms(rng, name, 32768)], 128, refusal=1)]


DIGIT_N, DIGIT_L = 300, 64


def threshold_scalars(c, L):
    """(raw value B in every full window and no carry, raw value B + 1 in every full window: every one carries).  A one-bit window never
    carries -- its raw value is at most 1 = B -- so c = 1 has the first scalar only, twice."""
    B = 1 << (c - 1)
    x0 = sum(B << (c * w) for w in range(L // c))
    return x0, x0 + 1 if c >= 2 else x0


@functools.lru_cache(maxsize=None)
def digits(name):
    """n = 300, every forced width: {label: Section}"""
    C, n = ev.CURVES[name], order(ev.CURVES[name])
    out = {}
    for c in range(1, SMALL_MAX_C + 1):
        rng = _rng(name, "digits %d" % c)
        x0, x1 = threshold_scalars(c, DIGIT_L)
        sc = rand_scalars(rng, DIGIT_N, DIGIT_L, distinct=200, extra=[x0, x1, 0, 1, (1 << DIGIT_L) - 1] * 4)
        out[("threshold", c)] = Section(C, "threshold c=%d" % c, sc, [rand_ms(rng, name, DIGIT_N)], lone_blocks(DIGIT_N), c_flags=c)
        sc = rand_scalars(rng, DIGIT_N, 256, distinct=200, extra=[0, n - 1, n, (1 << 256) - 1, n + 1, 1] * 4)
        out[("full", c)] = Section(C, "full c=%d" % c, sc, [rand_ms(rng, name, DIGIT_N)], lone_blocks(DIGIT_N), c_flags=c)
        for top in range(1, c + 1):
            L = 3 * c + top - 1
            sc = rand_scalars(rng, DIGIT_N, L, distinct=100, extra=[(1 << L) - 1] * 4)
            out[("top", c, top)] = Section(C, "top c=%d cw=%d" % (c, top), sc, [rand_ms(rng, name, DIGIT_N)], lone_blocks(DIGIT_N), c_flags=c)
    rng = _rng(name, "digits lengths")
    for bits in (128, 129, 249, 250):
        for flags in (0, 5, NO_SPLIT, NO_SPLIT | 5):
            sc = rand_scalars(rng, DIGIT_N, bits, distinct=200)
            out[("length", bits, flags)] = Section(C, "length %d flags %#x" % (bits, flags), sc, [rand_ms(rng, name, DIGIT_N)],
                                                   lone_blocks(DIGIT_N), c_flags=flags)
    # W == blocks: one-bit windows over 191-bit unsplit scalars on the lone call's 192 blocks; W S < blocks: most of the others
    sc = rand_scalars(rng, DIGIT_N, 191, distinct=200)
    out[("w_is_blocks",)] = Section(C, "W == blocks", sc, [rand_ms(rng, name, DIGIT_N)], lone_blocks(DIGIT_N), c_flags=NO_SPLIT | 1)
    return out


# (target S, forced c, scalar length L, scalars per slice): lone, 192 blocks -> S = min(192 // W, (n + 7) // 8, 32)
SLICE_SHAPES = {3: (2, 96, 40), 5: (4, 128, 40), 7: (4, 96, 40), 32: (8, 32, 8)}


def fold_steps(S):
    steps, cnt = 0, S
    while cnt > 1:
        cnt, steps = (cnt + 1) // 2, steps + 1
    return steps


def find_factors(rng, S, step, kind):
    """factors f_s (slice s = the base slice with every point multiplied by f_s) whose fold has a meeting of `kind` at `step`"""
    for _ in range(200000):
        f = [rng.choice((-2, -1, 1, 2, 0)) for _ in range(S)]
        v, cnt, st, hit = list(f), S, 0, False
        while cnt > 1:
            half = (cnt + 1) // 2
            for t in range(cnt - half):
                a, b = v[t], v[t + half]
                if st == step and a and b and ((a == b) if kind == "eq" else (a + b == 0)):
                    hit = True
                v[t] = a + b
            cnt, st = half, st + 1
        if hit and max(abs(x) for x in f) <= 2:
            return f
    raise AssertionError("no factors found")


@functools.lru_cache(maxsize=None)
def accumulate(name):
    """{label: Section}: one bucket takes everything, infinity points and lifted coordinates, equal and opposite sums meeting in the lane
    fold (3a), the tree (3b) and the slice fold (4)"""
    C = ev.CURVES[name]
    out = {}
    rng = _rng(name, "accumulate")
    P = pool(name)
    for c in (4, 8):
        out[("one_bucket", c)] = Section(C, "one bucket c=%d" % c, [rng.getrandbits(64) | (1 << 63)] * 300, [rand_ms(rng, name, 300)],
                                         lone_blocks(300), c_flags=c)
    ms = rand_ms(rng, name, 300, zeros=60)
    for i in (0, 1, 149, 150, 299):
        ms[i] = 0
    lifts = {}
    if name == "bn254":                                   # p has 254 bits: x + 4 p still fits 32 bytes; (p, p) reads as infinity
        for i, l in zip((2, 3, 4, 5, 6, 298), ((1, 0), (0, 1), (3, 3), (4, 2), (2, 4), (4, 4))):
            lifts[(0, i)] = l
        lifts[(0, 1)] = (1, 1)
        lifts[(0, 150)] = (4, 4)
    out[("infinity",)] = Section(C, "infinity and lifted", rand_scalars(rng, 300, 64, distinct=200), [ms], lone_blocks(300), lifts=lifts)
    # 3a, one-bit windows: T = 256 lanes share the one bucket of a window; 127-bit all-ones scalars put every entry into every window
    ones = (1 << 127) - 1
    out[("lane", "eq")] = Section(C, "lane fold eq", [ones] * 512, [[P[9]] * 512], lone_blocks(512), c_flags=1)
    # P and -P at level k of 8: 2^k entries, one per lane 0 .. 2^k - 1 in whatever order the sort leaves them -- the multiples 1 ..
    # 2^k - 1 of G and minus their sum.  After k - 1 levels lane 0 holds the sum of the entries in lanes 0 .. 2^(k-1) - 1 and lane
    # 2^(k-1) the sum of the rest; the half without the negative entry is positive, the other its opposite, and no smaller group of
    # lanes sums to zero: X and -X meet at h = 2^(k-1) for EVERY order, and nowhere before
    for k in range(1, 9):
        pos = list(range(1, 1 << k))
        out[("lane", "opp", k)] = Section(C, "lane fold opp level %d" % k, [ones] * (1 << k), [pos + [-sum(pos)]], lone_blocks(1 << k), c_flags=1)
    out[("lane", "cancel")] = Section(C, "lane fold cancel", [ones] * 512, [[P[11]] * 256 + [-P[11]] * 256], lone_blocks(512), c_flags=1)
    # 3b, c = 8: bucket = scalar - 1; a third entry, the point at infinity with an 8-bit scalar, keeps the window 8 bits wide
    for l in range(7):
        for kind, sign in (("eq", 1), ("opp", -1)):
            out[("tree", "S", l, kind)] = Section(C, "tree S level %d %s" % (l, kind), [1, 1 + (1 << l), 128],
                                                  [[P[20 + l], sign * P[20 + l], 0]], lone_blocks(3), c_flags=8)
            if l >= 1:
                out[("tree", "M", l, kind)] = Section(C, "tree M level %d %s" % (l, kind), [(1 << (l - 1)) + 1, 3 * (1 << (l - 1)) + 1, 128],
                                                      [[P[20 + l], sign * P[20 + l], 0]], lone_blocks(3), c_flags=8)
    # 4: the slices' sums equal or opposite at every step of the ragged fold
    for S, (c, L, q) in SLICE_SHAPES.items():
        base_sc = rand_scalars(rng, q, L, distinct=q)
        base_ms = [abs(m) for m in rand_ms(rng, name, q)]
        for step in range(fold_steps(S)):
            for kind in ("eq", "opp"):
                f = find_factors(rng, S, step, kind)
                out[("slice", S, step, kind)] = Section(C, "slice fold S=%d step %d %s" % (S, step, kind), base_sc * S,
                                                        [[fs * m for fs in f for m in base_ms]], lone_blocks(q * S), c_flags=c)
    return out


@functools.lru_cache(maxsize=None)
def pairs(name):
    """{label: Section}: the pair form at the audit's shape -- set b's own part, counters and region; a set that sums to infinity;
    three launches in a row on one workspace"""
    C, rng = ev.CURVES[name], _rng(name, "pairs")
    n = 300
    out = {}
    sc = rand_scalars(rng, n, 64, distinct=200)
    out[("generic",)] = Section(C, "pair", sc, [rand_ms(rng, name, n), rand_ms(rng, name, n)], pair_blocks(n))
    sc31 = rand_scalars(rng, n, 31, distinct=200)
    out[("audit",)] = Section(C, "pair hint 32", sc31, [rand_ms(rng, name, n), rand_ms(rng, name, n)], pair_blocks(n), hint=32, seq=0x7ffffff0)
    half = rand_scalars(rng, n // 2, 256, distinct=150)
    mb = [rng.choice(pool(name)) for _ in range(n // 2)]
    # (entries 2 j + 1 and 2 j + 2 share a scalar and cancel in set b, and so do the last and the first: pairs that straddle a slice
    # boundary leave block sums that only cancel in the slice fold)
    rot = lambda v: v[-1:] + v[:-1]
    out[("infinity",)] = Section(C, "pair, set b sums to infinity", rot([k for k in half for _ in (0, 1)]),
                                 [rand_ms(rng, name, n), rot([s * m for m in mb for s in (1, -1)])], pair_blocks(n))
    out[("three",)] = Section(C, "pair, three launches", rand_scalars(rng, n, 256, distinct=200), [rand_ms(rng, name, n), rand_ms(rng, name, n)],
                              pair_blocks(n), seq=5, launches=3)
    return out

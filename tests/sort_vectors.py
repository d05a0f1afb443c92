"""Scalars, the digit model and the driver files for the sort front of the general MSM path driven stage by stage
(tools/sort_check.hip): shared by tests/test_sort_gpu.py and tests/test_sort_vectors_cpu.py.

THE MODEL, on Python integers: a 32-byte scalar is reduced mod the group order by at most MAX_Q subtractions, split with the
endomorphism (tools/gen_glv.py:split_model, pinned against the engine's porla_glv_split by tests/test_glv_cpu.py) where the section
says so, and every sub-scalar is recoded into W signed c-bit digits: raw + carry is a positive digit up to and including 2^(c-1),
above that the digit raw + carry - 2^c with a carry into the next window; magnitude 0 gives no entry, a carry out of the last
window is dropped.  Sub-scalar e of scalar i is sub-point i SUBS + e; its entry in window w lies in bucket |digit| - 1 with the sign
(digit < 0) XOR (sub-scalar < 0) in bit 31.  recode() is that rule one sub-scalar at a time; digits() is the same rule on numpy
arrays for the large sections (the CPU module compares the two).

A SECTION is one header of the driver's input -- (n, glv, c, W, lowbits, sort_half, wg) with its scalars and points; a FILE is one
driver run: a list of sections.  Generation is deterministic (fixed seeds) and reads nothing outside the repository.
"""
import functools
import os
import random
import subprocess
import tempfile

import numpy as np

from tests import common
from tests import ec_vectors as ev
from tests import ladder_vectors as lv

EXE = os.path.join(common.ROOT, "porla_amd", "sort_check")
MAGIC, HDR, DEFAULT, FILL = 0x534f5254, 12, 0xffffffff, 0xA5A5A5A5
# msm.hip.h
TILE, MAX_PARTS, SORT_LOWBITS, SORT_MAX_LOW, STAGE_CAP, CTRL_WORDS = 4096, 128, 10, 4096, 34816, 4 + 128
SIGN = 1 << 31
M256 = (1 << 256) - 1
MAX_Q = {"bn254": 5, "secp256k1": 1}                      # floor((2^256 - 1) / order)
SCALAR_BITS = {"bn254": 254, "secp256k1": 256}
GLV_BITS = {"bn254": 126, "secp256k1": 128}               # glv.hip.h: |k1|, |k2| < 2^BITS
SHAPE_C = [2, 3, 8, 11, 12, 13, 16, 17, 20]
SHORT_W = {17: 3, 20: 2}                                  # windows of the sections at c >= 17 (their bucket arrays stay at a few MB)
RUN_L = [0, 1, 63, 64, 65, 127, 128, 129, 200, 4096]
TILE_N = [1, 1023, 1024, 1025, 4095, 4096, 4097]
BIG_N = 35 * TILE - 5
CURVE_NAMES = ["bn254", "secp256k1"]


def full_W(curve, glv, c):
    bits = GLV_BITS[curve] if glv else SCALAR_BITS[curve]
    return (bits + 1 + c - 1) // c


# ---------------------------------------------------------------- the launch shape: msm.hip.h:sort_front_plan restated
def sort_lowbits(c, m, W):
    lb = min(c - 1, SORT_LOWBITS)
    while lb < c - 1 and lb < 12 and (m >> (c - 1 - lb - 1)) <= 32768 and (W << (c - 1 - lb - 1)) >= 256:
        lb += 1
    if c - 1 - lb > 7:
        lb = c - 1 - 7
    return lb


def plan_model(n, glv, c, W):
    n_sub = 2 * n if glv else n
    tile_cap = 2 * TILE if glv else TILE
    T = (n + TILE - 1) // TILE
    lowbits, half = sort_lowbits(c, n_sub, W), 0
    lb2 = lowbits - 1
    parts_log = c - 1 - lb2
    if 0 <= lb2 <= 11 and parts_log <= 7 and (n_sub >> parts_log) <= 16384 and (tile_cap >> parts_log) >= 64:
        lowbits, half = lb2, 1
    wg = 256 // T if T < 256 else 1
    wg = min(wg, 16, W)
    return dict(n=n, glv=int(glv), c=c, W=W, tile_cap=tile_cap, T_tiles=T, lowbits=lowbits, sort_half=half, P=1 << (c - 1 - lowbits), wg=wg)


def dump_plans(groups):
    """sort_check --plan for (n, glv, c, W) groups: one dict per group; needs no device"""
    out = []
    for at in range(0, len(groups), 500):
        args = [str(int(x)) for g in groups[at:at + 500] for x in g]
        r = subprocess.run([EXE, "--plan"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        for line in r.stdout.splitlines():
            out.append({k: int(v) for k, v in (f.split("=") for f in line.split())})
    assert len(out) == len(groups)
    return out


# ---------------------------------------------------------------- the model
def reduce_order(curve, k):
    """SetBytes: at most MAX_Q subtractions of the order"""
    r = lv.order(ev.CURVES[curve])
    for _ in range(MAX_Q[curve]):
        if k < r:
            break
        k -= r
    assert 0 <= k < r
    return k


def sub_scalars(curve, glv, k):
    """[(magnitude, negative)] of the sub-scalars of the 256-bit scalar k"""
    k = reduce_order(curve, k)
    if not glv:
        return [(k, 0)]
    return [(m, int(neg)) for m, neg in lv.split(ev.CURVES[curve], k)]


def compose(curve, k1, k2):
    """the scalar whose split is exactly (k1, k2), signed"""
    C = ev.CURVES[curve]
    k = (k1 + lv.lam(C) * k2) % lv.order(C)
    assert lv.split(C, k) == [(abs(k1), int(k1 < 0)), (abs(k2), int(k2 < 0))], (k1, k2)
    return k


def recode(v, c, W, limbs=8):
    """signed digits of the magnitude v in W windows: [(digit, raw, carry_in)]; the kernel reads 32 `limbs`-limb words, a window at
    or beyond the last limb reads zeros"""
    v &= (1 << (32 * limbs)) - 1
    out, carry = [], 0
    for w in range(W):
        raw = (v >> (w * c)) & ((1 << c) - 1)
        t = raw + carry
        if t > 1 << (c - 1):
            out.append((t - (1 << c), raw, carry))
            carry = 1
        else:
            out.append((t, raw, carry))
            carry = 0
    return out, carry


def digits(mags, c, W, limbs):
    """recode() for an array of magnitudes: (W, len) signed digits as int64"""
    raw = np.frombuffer(b"".join((m & ((1 << (32 * limbs)) - 1)).to_bytes(32, "little") for m in mags), dtype=np.uint8).reshape(-1, 32)
    bits = np.unpackbits(raw, axis=1, bitorder="little")
    if W * c > 256:
        bits = np.concatenate([bits, np.zeros((bits.shape[0], W * c - 256), dtype=np.uint8)], axis=1)
    weights = (1 << np.arange(c, dtype=np.int64))
    out = np.zeros((W, len(mags)), dtype=np.int64)
    carry = np.zeros(len(mags), dtype=np.int64)
    for w in range(W):
        t = bits[:, w * c:(w + 1) * c].astype(np.int64) @ weights + carry
        neg = t > (1 << (c - 1))
        out[w] = np.where(neg, t - (1 << c), t)
        carry = neg.astype(np.int64)
    return out


class Model:
    """what the section's scalars put where: per window the signed digit of every sub-point"""

    def __init__(self, sec):
        self.subs = [s for k in sec.scalars for s in sub_scalars(sec.curve, sec.glv, k)]
        self.SUBS = 2 if sec.glv else 1
        self.n_sub = len(self.subs)
        self.digit = digits([m for m, _ in self.subs], sec.c, sec.W, 4 if sec.glv else 8)
        self.sneg = np.array([neg for _, neg in self.subs], dtype=bool)
        self.bucket = np.abs(self.digit) - 1                                   # -1: no entry
        self.sign = (self.digit < 0) ^ self.sneg[None, :]
        self.B = 1 << (sec.c - 1)

    def entries(self, w):
        """(buckets, entry words) of window w, in sub-point order"""
        live = np.nonzero(self.bucket[w] >= 0)[0]
        return self.bucket[w][live], (live.astype(np.uint32) | (self.sign[w][live].astype(np.uint32) << 31))

    def counts(self, w):
        return np.bincount(self.bucket[w][self.bucket[w] >= 0], minlength=self.B)

    def total(self):
        return int(np.count_nonzero(self.bucket >= 0))


class Section:
    def __init__(self, curve, label, family, scalars, glv, c, W=None, lowbits=None, sort_half=None, wg=None, points=(), edges=()):
        self.curve, self.label, self.family, self.scalars, self.glv, self.c = curve, label, family, list(scalars), int(glv), c
        self.W = W if W is not None else full_W(curve, glv, c)
        self.forced = (lowbits, sort_half, wg)
        self.points, self.edges = list(points), list(edges)       # edges: (kind, scalar index, sub-scalar, window) the section was built for
        self.n = len(self.scalars)
        assert 1 <= self.n <= 1 << 18 and all(0 <= k <= M256 for k in self.scalars)
        pl = plan_model(self.n, self.glv, c, self.W)
        if sort_half is not None:
            pl["sort_half"] = sort_half
        if lowbits is not None:
            pl["lowbits"], pl["P"] = lowbits, 1 << (c - 1 - lowbits)
        if wg is not None:
            pl["wg"] = wg
        self.plan = pl
        # the driver's own limits
        assert 2 <= c <= 20 and self.W >= 1 and (self.W << (c - 1)) <= 1 << 21
        assert pl["lowbits"] <= (11 if pl["sort_half"] else 12) and 0 <= c - 1 - pl["lowbits"] <= 7 and 1 <= pl["wg"] <= min(16, self.W)

    def __repr__(self):
        return "%s %s/%s n=%d glv=%d c=%d W=%d %s" % (self.curve, self.family, self.label, self.n, self.glv, self.c, self.W,
                                                      {k: self.plan[k] for k in ("lowbits", "sort_half", "wg")})

    @functools.cached_property
    def model(self):
        return Model(self)

    @property
    def stage_cap(self):
        return STAGE_CAP // 2 if self.plan["sort_half"] else STAGE_CAP

    def words(self):
        h = [MAGIC, self.n, self.glv, self.c, self.W] + [DEFAULT if v is None else v for v in self.forced] + [len(self.points), 0, 0, 0]
        body = b"".join(k.to_bytes(32, "big") for k in self.scalars) + b"".join(self.points)
        return np.concatenate([np.array(h, dtype=np.uint32), np.frombuffer(body, dtype=np.uint32)])

    def sizes(self):
        """the words of each output array, in file order"""
        S, T = (2 if self.glv else 1), self.plan["T_tiles"]
        nb = self.W << (self.c - 1)
        return [("or", 8), ("pts", 16 * S * len(self.points)), ("tile_off", (self.W * T * (MAX_PARTS + 1) + 1) // 2),
                ("tile_items", self.W * T * TILE * S), ("counts", nb), ("starts", nb), ("entries", self.W * S * self.n), ("ctrl", CTRL_WORDS)]


class File:
    def __init__(self, curve, name, sections):
        self.curve, self.name, self.sections = curve, name, sections

    def words(self):
        return np.concatenate([s.words() for s in self.sections])


def run(F, timeout=120):
    """one driver run: a dict of arrays per section"""
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        F.words().tofile(fin)
        r = subprocess.run([EXE, F.curve, fin, fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stderr
        raw = np.fromfile(fout, dtype=np.uint32)
    out, at = [], 0
    for s in F.sections:
        o = {}
        for name, words in s.sizes():
            o[name] = raw[at:at + words]
            at += words
        T = s.plan["T_tiles"]
        o["tile_off"] = o["tile_off"].view(np.uint16)[:s.W * T * (MAX_PARTS + 1)].reshape(s.W, T, MAX_PARTS + 1).astype(np.int64)
        o["tile_items"] = o["tile_items"].reshape(s.W, T, -1)
        out.append(o)
    assert at == raw.size
    return out


# ---------------------------------------------------------------- scalar families
def from_raw(raws, c):
    return sum(r << (w * c) for w, r in enumerate(raws))


def order_edges(curve, c, W):
    r, q = lv.order(ev.CURVES[curve]), MAX_Q[curve]
    vals = [("0", 0), ("1", 1), ("r-1", r - 1), ("r", r), ("r+1", r + 1), ("2r", 2 * r), ("MAX_Q*r", q * r), ("MAX_Q*r+1", q * r + 1),
            ("2^256-1", M256)]
    for w in range(1, W + 1):
        if w * c < 256:
            vals += [("2^%d" % (w * c), 1 << (w * c)), ("2^%d-1" % (w * c), (1 << (w * c)) - 1)]
    return [(name, v) for name, v in vals if v <= M256]           # 2r does not fit 256 bits on secp256k1


def digit_edge_values(c, W, top):
    """(kind, window, magnitude) for a sub-scalar below 2^top: the recode's edges, window by window"""
    B, ones = 1 << (c - 1), (1 << c) - 1
    out = []
    for w in range(W):
        out.append(("last_positive", w, B << (w * c)))                                         # raw = 2^(c-1): bucket B - 1
        out.append(("first_negative", w, (B + 1) << (w * c)))                                  # raw = 2^(c-1) + 1: -(B - 1), carry
        if w >= 1:
            out.append(("ones_with_carry", w, ((B + 1) << ((w - 1) * c)) | (ones << (w * c))))     # digit 0, carry out
    if W >= 2:
        # a carry from window 0 through all-ones windows into the top window, which holds nothing else
        out.append(("carry_run", W - 1, from_raw([B + 1] + [ones] * (W - 2), c)))
        out.append(("carry_only_top", W - 1, (B + 1) << ((W - 2) * c)))
    return [(kind, w, v) for kind, w, v in out if v < 1 << top]


def check_edge(sec, kind, i, e, w):
    """the edge (kind, scalar i, sub-scalar e, window w) is what the model sees: asserted by the CPU module for every edge"""
    m = sec.model
    mag = m.subs[i * m.SUBS + e][0]
    dg, carry_out = recode(mag, sec.c, sec.W, 4 if sec.glv else 8)
    B = 1 << (sec.c - 1)
    d, raw, cin = dg[w]
    nxt = dg[w + 1][2] if w + 1 < sec.W else carry_out
    if kind == "last_positive":
        assert (d, raw, nxt) == (B, B, 0) and m.bucket[w][i * m.SUBS + e] == B - 1
    elif kind == "first_negative":
        assert (d, raw, cin, nxt) == (-(B - 1), B + 1, 0, 1) and m.bucket[w][i * m.SUBS + e] == B - 2
    elif kind == "ones_with_carry":
        assert (d, raw, cin, nxt) == (0, 2 * B - 1, 1, 1) and m.bucket[w][i * m.SUBS + e] == -1
    elif kind == "carry_run":
        assert w == sec.W - 1 and all(x[2] == 1 for x in dg[1:]) and (d, raw) == (1, 0) and all(x[0] == 0 for x in dg[1:-1])
    elif kind == "carry_only_top":
        assert w == sec.W - 1 and (d, raw, cin) == (1, 0, 1)
    elif kind == "straddle":                                       # the window reaches over the end of limb 3 and holds something there
        assert sec.glv and w * sec.c < 128 < (w + 1) * sec.c and raw != 0
    elif kind == "beyond":                                         # the window starts at or behind the end of limb 3: only a carry can be there
        assert sec.glv and w * sec.c >= 128 and raw == 0
    elif kind == "top_bit":
        assert sec.glv and mag >> (GLV_BITS[sec.curve] - 1) == 1
    else:
        raise AssertionError(kind)
    return True


@functools.lru_cache(maxsize=None)
def top_bit_scalars(curve, count=6):
    """scalars whose split has a sub-scalar with bit BITS - 1 set (found by search: the split is not invertible by hand up there)"""
    rng, C = random.Random(77), ev.CURVES[curve]
    out = []
    for _ in range(200000):
        k = rng.randrange(lv.order(C))
        for e, (mag, _) in enumerate(lv.split(C, k)):
            if mag >> (GLV_BITS[curve] - 1) == 1:
                out.append((k, e))
        if len(out) >= count:
            return out[:count]
    raise AssertionError("no sub-scalar with the top bit found")


def edge_section(curve, glv, c, W=None, label=None):
    """order edges, then the digit edges of every window; with the split the digit edges stand in k1 or in k2 (the other one small)"""
    rng = random.Random(1000 * c + glv)
    W = W if W is not None else SHORT_W.get(c, full_W(curve, glv, c))
    scalars, edges = [], []
    for _, v in order_edges(curve, c, W):
        scalars.append(v)
    r = lv.order(ev.CURVES[curve])
    if not glv:
        for kind, w, v in digit_edge_values(c, W, 256):
            if v < r:
                edges.append((kind, len(scalars), 0, w))
                scalars.append(v)
    else:
        # magnitudes up to 2^(BITS - 3) come back from the split as they went in (compose asserts it); the top of the range is
        # reached by search
        for kind, w, v in digit_edge_values(c, W, GLV_BITS[curve] - 3):
            for e in (0, 1):
                other = rng.randrange(1, 1 << 20) * rng.choice([1, -1])
                sgn = rng.choice([1, -1])
                edges.append((kind, len(scalars), e, w))
                scalars.append(compose(curve, sgn * v, other) if e == 0 else compose(curve, other, sgn * v))
        for k, e in top_bit_scalars(curve):
            edges.append(("top_bit", len(scalars), e, 0))
            mag = lv.split(ev.CURVES[curve], k)[e][0]
            for w in range(W):
                raw = ((mag & ((1 << 128) - 1)) >> (w * c)) & ((1 << c) - 1)
                if w * c < 128 < (w + 1) * c and raw:
                    edges.append(("straddle", len(scalars), e, w))
                if w * c >= 128:
                    edges.append(("beyond", len(scalars), e, w))
            scalars.append(k)
    scalars += [rng.getrandbits(256) for _ in range(40)]
    return Section(curve, label or "c%d_glv%d" % (c, glv), "edges", scalars, glv, c, W, edges=edges)


def edges_file(curve):
    secs = [edge_section(curve, glv, c) for c in SHAPE_C for glv in (0, 1)]
    secs.append(edge_section(curve, 1, 17, W=full_W(curve, 1, 17), label="c17_glv1_fullW"))
    # one window more than the sub-scalars need: it starts behind limb 3 on both curves
    secs.append(edge_section(curve, 1, 16, W=9, label="c16_glv1_W9"))
    return File(curve, "edges", secs)


def in_partition(rng, sec_c, lowbits, part, avoid=False):
    """a raw window-0 digit (positive, no carry) whose bucket lies in partition `part` -- or, with avoid, in any other"""
    P, nlow = 1 << (sec_c - 1 - lowbits), 1 << lowbits
    p = part if not avoid else rng.choice([q for q in range(P) if q != part])
    return ((rng.randrange(nlow) * P) | p) + 1


def high_windows(rng, c, W, top):
    return sum(rng.getrandbits(c) << (w * c) for w in range(1, W)) & ((1 << top) - 1) & ~((1 << c) - 1)


def skew_scalars(curve, glv, c, W, lowbits, per_tile, seed, front=True):
    """tiles of 4096 scalars: tile t sends exactly per_tile[t] window-0 items into partition 0 and every other sub-scalar into the other
    partitions (the windows above are random); with the split both sub-scalars count, k2 of an odd last scalar goes elsewhere"""
    rng = random.Random(seed)
    S = 2 if glv else 1
    top = 100 if glv else 250
    scalars = []
    for L in per_tile:
        assert 0 <= L <= TILE * S
        tile = []
        for j in range(TILE):
            raws = []
            for e in range(S):
                inside = j * S + e < L
                raws.append(in_partition(rng, c, lowbits, 0, avoid=not inside) | high_windows(rng, c, W, top))
            tile.append(raws[0] if not glv else compose(curve, raws[0] * rng.choice([1, -1]), raws[1] * rng.choice([1, -1])))
        scalars += tile if front else tile[::-1]
    return scalars


def runs_file(curve):
    """run lengths: partition 0 of tile t holds exactly RUN_L[t] items of window 0"""
    secs = []
    for glv, c, lowbits, half in ((0, 13, 10, 0), (1, 12, 9, 1)):
        Ls = RUN_L + ([2 * TILE] if glv else [])
        sc = skew_scalars(curve, glv, c, 2, lowbits, Ls, seed=31 + glv)
        secs.append(Section(curve, "runs_glv%d" % glv, "runs", sc, glv, c, 2, lowbits=lowbits, sort_half=half, edges=[("run", t, 0, L) for t, L in enumerate(Ls)]))
    # staging: exactly STAGE_CAP - 1, STAGE_CAP, STAGE_CAP + 1 entries in (window 0, partition 0), full and half size
    for half, tiles in ((0, 9), (1, 5)):
        cap = STAGE_CAP // 2 if half else STAGE_CAP
        for d in (-1, 0, 1):
            total = cap + d
            per = [min(TILE, total - t * TILE) if total > t * TILE else 0 for t in range(tiles)]
            assert sum(per) == total and per[-1] < TILE
            sc = skew_scalars(curve, 0, 13, 2, 10, per, seed=50 + d + 10 * half)
            secs.append(Section(curve, "stage_half%d_%+d" % (half, d), "staging", sc, 0, 13, 2, lowbits=10, sort_half=half, edges=[("stage", 0, 0, total)]))
    secs.append(lane_section(curve))
    return File(curve, "runs", secs)


LANE_COMPS = [(k, two) for k in (7, 8, 9) for two in (0, 1)] + [(64, 0)]


def lane_section(curve):
    """lane sharing: partition 0 of every tile holds one 64-item chunk of window 0 -- k items of one bucket X, with `two` as many of a
    second bucket Y (whichever of the two lane 0 holds, the other one is shared by lanes that are not the first), strays in distinct
    buckets for the rest; the 64 scalars stand first in their tile with the shared buckets in front, then last with the strays in front"""
    c, lowbits, W = 11, 8, 2
    P = 1 << (c - 1 - lowbits)
    rng = random.Random(97)
    scalars, edges = [], []
    for front in (True, False):
        for k, two in LANE_COMPS:
            lows = rng.sample(range(1 << lowbits), 64)
            comp = [lows[0]] * k + ([lows[1]] * k if two else [])
            comp += lows[2:2 + 64 - len(comp)]
            assert len(comp) == 64
            chunk = [((low * P) | 0) + 1 for low in comp]
            rest = [in_partition(rng, c, lowbits, 0, avoid=True) for _ in range(TILE - 64)]
            tile = chunk + rest if front else rest + chunk[::-1]      # ... and there the strays come first
            edges.append(("lanes", len(scalars) // TILE, 0, (k, two, lows[0] * P, lows[1] * P)))
            scalars += [v | high_windows(rng, c, W, 250) for v in tile]
    return Section(curve, "lanes", "lanes", scalars, 0, c, W, lowbits=lowbits, sort_half=0, edges=edges)


def tiles_file(curve):
    rng = random.Random(5)
    secs = []
    for i, n in enumerate(TILE_N):
        glv = i % 2
        secs.append(Section(curve, "n%d" % n, "tiles", [rng.getrandbits(256) for _ in range(n)], glv, 8 if n < TILE else 12))
    # each of the 16 waves of a sort block walks three tiles (tiles wv, wv + 16, wv + 32), the last one partial
    secs.append(Section(curve, "n%d" % BIG_N, "tiles", [rng.getrandbits(256) for _ in range(BIG_N)], 0, 12, 3))
    # blocks per tile: the same scalars with 1, 2, 16 blocks and with a number that does not divide W
    sc = [rng.getrandbits(256) for _ in range(TILE + 1)]
    for wg in (1, 2, 16, 5):
        secs.append(Section(curve, "wg%d" % wg, "wg", sc, 0, 8, wg=wg))
    sc = [rng.getrandbits(256) for _ in range(TILE + 1)]
    for wg in (1, 5):
        secs.append(Section(curve, "glv_wg%d" % wg, "wg", sc, 1, 11, wg=wg))
    # partition widths: one partition and 128 of them, four and two counters per thread
    sc = [rng.getrandbits(256) for _ in range(6000)]
    for label, c, lowbits, half in (("P1", 11, 10, 0), ("P128", 13, 5, 0), ("P128_half", 13, 5, 1), ("per4", 13, 12, 0), ("per4_P16", 17, 12, 0),
                                    ("per2", 12, 11, 1), ("per2_P16", 16, 11, 1), ("P1_c2", 2, 1, 0)):
        secs.append(Section(curve, label, "shapes", sc, int(label in ("P128_half", "per2")), c, SHORT_W.get(c, 3), lowbits=lowbits, sort_half=half))
    return File(curve, "tiles", secs)


FILL_C_GLV = 13


def fill_file(curve):
    """uniform scalars in the launch shape the product itself takes"""
    rng = random.Random(8)
    secs = [Section(curve, "glv_2p15+1", "fill", [rng.getrandbits(256) for _ in range((1 << 15) + 1)], 1, FILL_C_GLV)]
    if curve == "secp256k1":      # 256-bit scalars at c = 16: the 17th window holds only carries
        secs.append(Section(curve, "plain_2p17", "fill", [rng.getrandbits(256) for _ in range(1 << 17)], 0, 16))
    return File(curve, "fill", secs)


# ---------------------------------------------------------------- scalar OR and points
OR_CASES = ["n1", "n255", "n256", "n257", "stride", "last_scalar", "lane63"]


def or_file(curve):
    """k_scalar_or: sections of one window of two bits -- the digit and sort stages run on them like on any other"""
    rng = random.Random(3)
    low = lambda n: [rng.getrandbits(64) for _ in range(n)]
    secs = []
    for n in (1, 255, 256, 257):
        secs.append(Section(curve, "n%d" % n, "or", [rng.getrandbits(256) for _ in range(n)], 0, 2, 1))
    secs.append(Section(curve, "stride", "or", low(131072 + 300 - 1) + [1 << 255], 0, 2, 1))       # the grid-stride loop goes round
    secs.append(Section(curve, "last_scalar", "or", low(999) + [(1 << 255) | (1 << 200)], 0, 2, 1))
    sc = low(1000)
    sc[64 * 5 + 63] |= 1 << 231                                                                    # lane 63 of wave 5 (block 1, wave 1)
    secs.append(Section(curve, "lane63", "or", sc, 0, 2, 1))
    assert [s.label for s in secs] == OR_CASES
    return File(curve, "or", secs)


def scalar_or(scalars):
    v = 0
    for k in scalars:
        v |= k
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def point_cases(curve):
    """(name, x, y) as 256-bit integers on the wire: k G lifted by multiples of p, and the coordinates SetBytes treats specially"""
    C = ev.CURVES[curve]
    p = C.p
    out = []
    for i, pt in enumerate(ev.multiples(C)[1:9]):
        kmax = (M256 - pt[0]) // p
        for k in range(kmax + 1):
            out.append(("%dG+%dp" % (i + 1, k), pt[0] + k * p, pt[1] + min(k, (M256 - pt[1]) // p) * p))
    out += [("inf", 0, 0), ("inf+p", p, p), ("x0", 0, 5), ("x=p-1", p - 1, 7), ("small+p", 5 + p, 7 + p), ("max", M256, M256)]
    return out


def points_file(curve):
    pts = [x.to_bytes(32, "big") + y.to_bytes(32, "big") for _, x, y in point_cases(curve)]
    pts = (pts * (300 // len(pts) + 1))[:300]                                                      # more than one block of 256
    sc = [1] * 4
    return File(curve, "points", [Section(curve, "glv%d" % glv, "points", sc, glv, 2, 1, points=pts) for glv in (0, 1)])


def expected_point_words(curve, glv, pt64):
    """the table form of ec_vectors.aff30: canonical residues times the factor of the reduced-radix form; with the split the pair
    (x, y), (beta x, y); (0, 0) -- also as (p, p) -- stays all zero"""
    C = ev.CURVES[curve]
    x, y = int.from_bytes(pt64[:32], "big") % C.p, int.from_bytes(pt64[32:], "big") % C.p
    rows = [ev.words(x * C.r30 % C.p) + ev.words(y * C.r30 % C.p)]
    if glv:
        rows.append(ev.words(C.beta * x * C.r30 % C.p) + ev.words(y * C.r30 % C.p))
    return rows


FILES = {"edges": edges_file, "runs": runs_file, "tiles": tiles_file, "fill": fill_file, "or": or_file, "points": points_file}
FILE_NAMES = list(FILES)


@functools.lru_cache(maxsize=None)
def file(curve, name):
    return FILES[name](curve)

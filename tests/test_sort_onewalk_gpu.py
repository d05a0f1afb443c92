"""GPU: k_partition_sort of porla_amd/csrc/msm.hip.h in the form that walks global memory once -- a wave holds the first 128 items of
the run of each of its up to 16 tiles (tiles wv, wv + 16, ...) in registers from the count to the place, and reads only what a run
holds beyond 128 items again -- and the boundary to the form that walks twice (more than 256 tiles).  The stage contract is that of
tests/test_sort_gpu.py, whose check_digits / check_sort do the checking here: the same counts, starts, ctrl[0], per bucket the same
multiset of entries, the fill word wherever no kernel wrote.  Sections are written by this file and run by tools/sort_check.hip, which
launches the product's own kernel through msm.hip.h:sort_launch:
  runs    partition 0 of window 0 receives exactly L items from tile 0, L = 0, 1, 63, 64, 65, 127, 128, 129, 4096 (129 and 4096 reach
          beyond the held head), at n = 4096 and n = 8192, full- and half-size instantiation forced; with the split at n = 4096
  tiles   T = 1, 15, 16, 17, 33, 64 tiles, the last one of one scalar: a wave's held slots 0 .. 3, partly filled last rounds; runs
          of 64 items (c = 17: the shape of 2^20 pairs, with the split the half-size form) and of 2048 (c = 12)
  skew    all scalars equal (every chunk takes the shared atomic of >= 8 equal buckets, in both phases) and all zero (every run
          empty), at n = 3 * 4096 + 5
Then the depth of 16 held tiles and the first size beyond it through the public porla_bn254_msm_device, whose answer is computed in
the exponent: T = 256 (every held slot of every wave is live) and T = 257 (the kernel that walks twice)."""
import functools
import random

import numpy as np
import pytest

from tests import bucket_vectors as bv
from tests import ec_vectors as ev
from tests import ladder_vectors as lv
from tests import sort_vectors as sv
from tests.test_sort_gpu import check_digits, check_sort

pytestmark = pytest.mark.gpu

TILE = sv.TILE
FILL = np.uint32(sv.FILL)
RUN_L = [0, 1, 63, 64, 65, 127, 128, 129, 4096]
RUN_L_SPLIT = [65, 129, 4096]
TILE_T = [1, 15, 16, 17, 33, 64]
SKEW_N = 3 * TILE + 5
HOLD_TILES = 16 * 16                       # msm.hip.h: sort_holds_runs


def runs_file(curve):
    secs = []
    for half in (0, 1):
        for tiles in (1, 2):
            for L in RUN_L:
                per = [L] + [5] * (tiles - 1)
                sc = sv.skew_scalars(curve, 0, 13, 2, 10, per, seed=700 + L + 10000 * half + 100000 * tiles)
                secs.append(sv.Section(curve, "L%d_n%d_half%d" % (L, tiles * TILE, half), "runs", sc, 0, 13, 2, lowbits=10, sort_half=half,
                                       edges=[("run", 0, 0, L)]))
    for L in RUN_L_SPLIT:
        sc = sv.skew_scalars(curve, 1, 12, 2, 9, [L], seed=900 + L)
        secs.append(sv.Section(curve, "L%d_split" % L, "runs", sc, 1, 12, 2, lowbits=9, sort_half=1, edges=[("run", 0, 0, L)]))
    return sv.File(curve, "onewalk_runs", secs)


def tiles_file(curve):
    rng = random.Random(41)
    secs = []
    shapes = [(T, 0, 17) for T in TILE_T] + [(16, 1, 17), (17, 1, 17), (1, 0, 12), (17, 0, 12)]
    for T, glv, c in shapes:
        n = (T - 1) * TILE + 1
        secs.append(sv.Section(curve, "T%d_glv%d_c%d" % (T, glv, c), "tiles", [rng.getrandbits(256) for _ in range(n)], glv, c, 3))
    return sv.File(curve, "onewalk_tiles", secs)


def skew_file(curve):
    k = random.Random(43).getrandbits(256)
    secs = []
    for glv in (0, 1):
        secs.append(sv.Section(curve, "equal_glv%d" % glv, "skew", [k] * SKEW_N, glv, 13))
        secs.append(sv.Section(curve, "zero_glv%d" % glv, "skew", [0] * SKEW_N, glv, 13))
    return sv.File(curve, "onewalk_skew", secs)


FILES = {"runs": runs_file, "tiles": tiles_file, "skew": skew_file}


@functools.lru_cache(maxsize=None)
def file(curve, name):
    return FILES[name](curve)


@functools.lru_cache(maxsize=None)
def outputs(curve, name):
    """one driver run per curve and file"""
    return sv.run(file(curve, name), timeout=120)


def run_of(s, o, w, t, p):
    off = o["tile_off"][w, t]
    return int(off[p + 1] - off[p]) if p + 1 < s.plan["P"] else int(off[sv.MAX_PARTS] - off[p])


@pytest.mark.parametrize("curve", sv.CURVE_NAMES)
def test_sections_are_what_they_say(curve):
    """the shapes the families were chosen for, on the plan and on the device's own tile_off"""
    F, outs = file(curve, "runs"), outputs(curve, "runs")
    seen = set()
    for s, o in zip(F.sections, outs):
        L = s.edges[0][3]
        assert run_of(s, o, 0, 0, 0) == L, "%r: the run of partition 0 in tile 0" % s
        assert s.plan["T_tiles"] <= HOLD_TILES
        seen.add((L, s.n, s.plan["sort_half"], s.glv))
    assert seen >= {(L, n, half, 0) for L in RUN_L for n in (TILE, 2 * TILE) for half in (0, 1)}
    assert seen >= {(L, TILE, 1, 1) for L in RUN_L_SPLIT}
    F = file(curve, "tiles")
    assert sorted({s.plan["T_tiles"] for s in F.sections}) == TILE_T and all(s.n % TILE == 1 for s in F.sections)
    by = {s.label: s for s in F.sections}
    # 64-item runs as at 2^20 pairs: 64 partitions per tile of 4096, with the split 128 half-size ones per 8192
    assert (by["T64_glv0_c17"].plan["P"], by["T64_glv0_c17"].plan["sort_half"]) == (64, 0)
    assert (by["T16_glv1_c17"].plan["P"], by["T16_glv1_c17"].plan["sort_half"]) == (128, 1)
    assert by["T17_glv0_c12"].plan["P"] <= 4                                  # runs of 1024 items and more: mostly beyond the head
    for s, o in zip(file(curve, "skew").sections, outputs(curve, "skew")):
        assert s.n == SKEW_N and s.plan["T_tiles"] == 4
        total = int(o["ctrl"][0])
        if s.label.startswith("zero"):
            assert total == 0 and not o["tile_off"].any()
        else:
            # one bucket per window and sub-scalar: a tile's run is all of its items
            assert total == s.model.total() > 0
            for w in range(s.W):
                assert np.count_nonzero(s.model.counts(w)) <= (2 if s.glv else 1)


@pytest.mark.parametrize("name", list(FILES))
@pytest.mark.parametrize("curve", sv.CURVE_NAMES)
def test_digits(curve, name):
    F, outs = file(curve, name), outputs(curve, name)
    checked = sum(check_digits(s, o) for s, o in zip(F.sections, outs))
    assert checked == sum(s.W * s.plan["T_tiles"] for s in F.sections) > 0


@pytest.mark.parametrize("name", list(FILES))
@pytest.mark.parametrize("curve", sv.CURVE_NAMES)
def test_sort(curve, name):
    F, outs = file(curve, name), outputs(curve, name)
    checked = sum(check_sort(s, o) for s, o in zip(F.sections, outs))
    assert checked == sum(s.W << (s.c - 1) for s in F.sections) > 0


@pytest.mark.parametrize("name", list(FILES))
@pytest.mark.parametrize("curve", sv.CURVE_NAMES)
def test_fill_words(curve, name):
    """no held register is stored for an inactive lane: entries behind ctrl[0] and tile_items behind each tile's total are untouched,
    and what lies in front of ctrl[0] was all written (an entry is a sub-point index and a sign: never the fill word)"""
    for s, o in zip(file(curve, name).sections, outputs(curve, name)):
        total = int(o["ctrl"][0])
        assert total == s.model.total()
        entries = o["entries"]
        assert (entries[total:] == FILL).all(), "%r: entries written behind ctrl[0] = %d" % (s, total)
        assert ((entries[:total] & 0x7fffffff) < s.model.n_sub).all(), "%r: an entry in front of ctrl[0] is no sub-point" % s
        for w in range(s.W):
            for t in range(s.plan["T_tiles"]):
                tot = int(o["tile_off"][w, t][sv.MAX_PARTS])
                assert (o["tile_items"][w, t][tot:] == FILL).all(), "%r window %d tile %d: tile_items written behind %d" % (s, w, t, tot)


# ================================================================ depth and fallback boundary through the public API
N_POINTS = 16


@functools.lru_cache(maxsize=None)
def api_inputs(n):
    """(scalar bytes, point bytes, expected 64 bytes): 16 distinct multiples of G tiled over the input, seeded random 254-bit scalars;
    the expected sum is (sum_j (sum of the scalars on point j mod r) k_j) G"""
    C = ev.CURVES["bn254"]
    r = lv.order(C)
    G = ev.multiples(C)
    ks = list(range(3, 3 + N_POINTS))
    raw = np.random.RandomState(n & 0xffff).randint(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3f                                                       # big endian: below 2^254
    limbs = raw.reshape(n, 8, 4).astype(np.uint64)
    limbs = (limbs[:, :, 0] << 24) | (limbs[:, :, 1] << 16) | (limbs[:, :, 2] << 8) | limbs[:, :, 3]      # [n][8], most significant first
    e = 0
    for j, k in enumerate(ks):
        col = limbs[j::N_POINTS].sum(axis=0)                                 # < 2^32 * 2^20: exact in 64 bits
        e += k * sum(int(col[i]) << (32 * (7 - i)) for i in range(8))
    want = bv.mul(C, e % r)
    assert want is not None
    rows = np.frombuffer(b"".join(G[k][0].to_bytes(32, "big") + G[k][1].to_bytes(32, "big") for k in ks), dtype=np.uint8).reshape(N_POINTS, 64)
    pts = np.tile(rows, (n // N_POINTS + 1, 1))[:n]
    return raw.tobytes(), pts.tobytes(), want[0].to_bytes(32, "big") + want[1].to_bytes(32, "big")


@pytest.mark.parametrize("tiles", [HOLD_TILES, HOLD_TILES + 1])
def test_depth_and_fallback_boundary(tiles):
    """T = 256: the deepest held form, every slot of every wave live (the last tile holds one scalar); T = 257: the walk-twice kernel"""
    import torch
    from porla_amd import multiexp as mx
    n = (tiles - 1) * TILE + 1
    sc, pt, want = api_inputs(n)
    d_sc = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
    d_pt = torch.frombuffer(bytearray(pt), dtype=torch.uint8).cuda()
    got = mx.msm_device("bn254", d_sc.data_ptr(), d_pt.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    c, W, glv = mx.last_msm_shape()
    assert sv.plan_model(n, glv, c, W)["T_tiles"] == tiles
    assert got == want, "n=%d (T=%d): c=%d W=%d glv=%d" % (n, tiles, c, W, glv)

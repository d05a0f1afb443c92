"""GPU: the sort front of the general MSM path -- k_scalar_or, k_points_to_mont, k_digits_partition and k_partition_sort of
porla_amd/csrc/msm.hip.h as they are, launched by tools/sort_check.hip in the launch shape of sort_front_plan on scalars the test
wrote (tests/sort_vectors.py: the families edges, runs, staging, lanes, tiles, wg, shapes, fill, or, points;
tests/test_sort_vectors_cpu.py asserts that all of them are there and reach their edges).  Per curve and section:
  digits   per (window, tile): tile_off non-decreasing, off[MAX_PARTS] the tile's entry count, flat from partition P on; every item of
           run p decodes (high bucket bits, sign, local index) to a model entry whose bucket has the low bits p; the decoded multiset
           equals the model's; tile_items behind the tile's total still hold the fill word
  sort     counts against the model for every bucket of every window; per (window, partition) starts is the exclusive prefix of
           counts in bucket order from a base, the partitions' ranges are disjoint and tile [0, ctrl[0]); ctrl[0] is the model's total,
           ctrl[1 ..] zero; every bucket's slice of entries equals the model's multiset (the order inside a bucket comes from LDS
           atomics and is no part of the contract); entries behind ctrl[0] still hold the fill word
  or       the 8 words equal the OR of the scalars
  points   the table words in the field form tests/ec_vectors.py models for table points
Comparison is exact; a failure names the section, the window, the tile or bucket and the first entry that differs.
Then the window trimming of msm_launch through the public API, on scalars of a chosen length over points k G."""
import functools
import os
import random

import numpy as np
import pytest

from tests import bucket_vectors as bv
from tests import ec_vectors as ev
from tests import ladder_vectors as lv
from tests import sort_vectors as sv

pytestmark = pytest.mark.gpu

CURVE_NAMES = sv.CURVE_NAMES
SORT_FILES = ["edges", "runs", "tiles", "fill"]
FILL = np.uint32(sv.FILL)


def test_driver_is_built():
    assert os.path.exists(sv.EXE), "build it with make -C porla_amd/csrc"


@functools.lru_cache(maxsize=None)
def outputs(curve, name):
    """one driver run per curve and file; seconds, the kernels themselves take milliseconds"""
    return sv.run(sv.file(curve, name), timeout=120)


def first_diff(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if len(d) else n


def check_digits(s, o):
    """the stage contract of k_digits_partition; returns the number of (window, tile) pairs checked"""
    m, pl = s.model, s.plan
    P, lowbits, cap, T = pl["P"], pl["lowbits"], pl["tile_cap"], pl["T_tiles"]
    logP = s.c - 1 - lowbits
    checked = 0
    for w in range(s.W):
        bucket, sign = m.bucket[w], m.sign[w]
        for t in range(T):
            where = "%r window %d tile %d" % (s, w, t)
            off = o["tile_off"][w, t]
            assert (np.diff(off) >= 0).all(), where + ": tile_off decreases"
            lo, hi = t * cap, min((t + 1) * cap, m.n_sub)
            live = np.nonzero(bucket[lo:hi] >= 0)[0]
            total = int(off[sv.MAX_PARTS])
            assert total == len(live), where + ": off[MAX_PARTS] = %d, the model has %d entries" % (total, len(live))
            assert (off[P:] == total).all(), where + ": offsets of the partitions >= P are not flat"
            items = o["tile_items"][w, t]
            assert (items[total:] == FILL).all(), where + ": tile_items written behind the tile's total %d" % total
            items = items[:total].astype(np.int64)
            part = np.searchsorted(off[1:P + 1], np.arange(total), side="right")     # the run an item lies in
            b_dev = ((items & ((1 << lowbits) - 1)) << logP) | part
            s_dev = (items >> lowbits) & 1
            l_dev = items >> (lowbits + 1)
            # (local index, bucket, sign) as one key: each local index occurs once
            got = np.sort((l_dev << 32) | (b_dev << 1) | s_dev)
            want = (live.astype(np.int64) << 32) | (bucket[lo:hi][live] << 1) | sign[lo:hi][live].astype(np.int64)
            if not np.array_equal(got, want):
                at = first_diff(got, want)
                g = int(got[at]) if at < len(got) else None
                x = int(want[at]) if at < len(want) else None
                fmt = lambda v: "none" if v is None else "sub-point %d bucket %d sign %d" % (lo + (v >> 32), (v >> 1) & 0x7fffffff, v & 1)
                raise AssertionError("%s: item %d of the sorted multiset: device %s, model %s" % (where, at, fmt(g), fmt(x)))
            checked += 1
    return checked


def check_sort(s, o):
    """the stage contract of k_partition_sort; returns the number of buckets checked"""
    m, pl = s.model, s.plan
    P, B = pl["P"], m.B
    ctrl = o["ctrl"].astype(np.int64)
    counts = o["counts"].astype(np.int64).reshape(s.W, B)
    starts = o["starts"].astype(np.int64).reshape(s.W, B)
    entries = o["entries"]
    total = m.total()
    ranges, checked = [], 0
    for w in range(s.W):
        want_counts = m.counts(w)
        if not np.array_equal(counts[w], want_counts):
            b = first_diff(counts[w], want_counts)
            raise AssertionError("%r window %d bucket %d (partition %d): counts %d, the model has %d" % (s, w, b, b & (P - 1), counts[w][b], want_counts[b]))
        # bucket order inside a partition: the buckets p, p + P, p + 2P, ...
        cw = counts[w].reshape(-1, P)                                     # [low index][partition]
        sw = starts[w].reshape(-1, P)
        base = sw[0]
        prefix = np.cumsum(cw, axis=0) - cw + base[None, :]
        if not np.array_equal(sw, prefix):
            low, p = map(int, np.argwhere(sw != prefix)[0])
            raise AssertionError("%r window %d bucket %d (partition %d): starts %d is not base %d + the counts before it = %d" % (
                s, w, low * P + p, p, sw[low, p], base[p], prefix[low, p]))
        ranges += [(int(base[p]), int(base[p] + cw[:, p].sum()), w, p) for p in range(P)]
        # every bucket's slice against the model's multiset
        bk, vals = m.entries(w)
        order = np.lexsort((vals, bk))
        want = vals[order]
        nz = np.nonzero(counts[w])[0]
        cnt = counts[w][nz]
        seg0 = np.cumsum(cnt) - cnt
        idx = np.repeat(starts[w][nz] - seg0, cnt) + np.arange(int(cnt.sum()))
        assert idx.size == 0 or (0 <= idx.min() and idx.max() < total), "%r window %d: a bucket's slice leaves [0, ctrl[0])" % (s, w)
        dev = entries[idx]
        owner = np.repeat(nz, cnt)
        got = dev[np.lexsort((dev, owner))]
        if not np.array_equal(got, want):
            at = first_diff(got, want)
            b = int(owner[at])
            raise AssertionError("%r window %d bucket %d (partition %d): entry %d of the sorted slice is %s, the model has %s (slice at %d, %d entries)" % (
                s, w, b, b & (P - 1), at - int(seg0[np.searchsorted(nz, b)]), "sub-point %d sign %d" % (got[at] & 0x7fffffff, got[at] >> 31),
                "sub-point %d sign %d" % (want[at] & 0x7fffffff, want[at] >> 31), starts[w][b], counts[w][b]))
        checked += B
    # the totals behind the per-bucket checks, so that a wrong count is reported with its window and bucket first
    assert ctrl[0] == total, "%r: ctrl[0] = %d, the model has %d entries" % (s, ctrl[0], total)
    assert (ctrl[1:] == 0).all(), "%r: ctrl[1 ..] not cleared: %s" % (s, np.nonzero(ctrl[1:])[0][:4] + 1)
    assert (entries[total:] == FILL).all(), "%r: entries written behind ctrl[0] = %d (first at %s)" % (s, total, total + np.nonzero(entries[total:] != FILL)[0][:1])
    at = 0
    for lo, hi, w, p in sorted(ranges):                                   # disjoint, and they fill [0, ctrl[0])
        assert lo == at, "%r window %d partition %d: its range starts at %d, the ranges before it end at %d" % (s, w, p, lo, at)
        at = hi
    assert at == total
    return checked


@pytest.mark.parametrize("name", SORT_FILES + ["or", "points"])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_digits(curve, name):
    F, outs = sv.file(curve, name), outputs(curve, name)
    checked = sum(check_digits(s, o) for s, o in zip(F.sections, outs))
    assert checked == sum(s.W * s.plan["T_tiles"] for s in F.sections) > 0


@pytest.mark.parametrize("name", SORT_FILES + ["or", "points"])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_sort(curve, name):
    F, outs = sv.file(curve, name), outputs(curve, name)
    checked = sum(check_sort(s, o) for s, o in zip(F.sections, outs))
    assert checked == sum(s.W << (s.c - 1) for s in F.sections) > 0


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_staged_and_unstaged_partitions(curve):
    """the staging family's edge on the device's own counts: partition 0 of window 0 holds STAGE_CAP - 1, STAGE_CAP, STAGE_CAP + 1
    entries (half size: of its half)"""
    F, outs = sv.file(curve, "runs"), outputs(curve, "runs")
    seen = []
    for s, o in zip(F.sections, outs):
        if s.family == "staging":
            got = int(o["counts"].astype(np.int64).reshape(s.W, -1)[0].reshape(-1, s.plan["P"])[:, 0].sum())
            seen.append(got - s.stage_cap)
            assert got == s.edges[0][3]
    assert seen == [-1, 0, 1, -1, 0, 1]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_blocks_per_tile_variants_agree(curve):
    """the same scalars with 1, 2, 16 and 5 blocks per tile: identical tile_off, identical counts (the multisets are compared with
    the model by test_digits and test_sort)"""
    F, outs = sv.file(curve, "tiles"), outputs(curve, "tiles")
    groups = {}
    for s, o in zip(F.sections, outs):
        if s.family == "wg":
            groups.setdefault(s.glv, []).append((s, o))
    assert sorted(len(g) for g in groups.values()) == [2, 4]
    for g in groups.values():
        s0, o0 = g[0]
        for s, o in g[1:]:
            assert np.array_equal(o["tile_off"], o0["tile_off"]), "%r against %r: tile_off" % (s, s0)
            assert np.array_equal(o["counts"], o0["counts"]), "%r against %r: counts" % (s, s0)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_lane_sharing_chunks(curve):
    """the 64-item runs of the lanes family as they lie in tile_items: the bucket of lane 0 and how many lanes share it.  Which item
    lands in lane 0 is decided by LDS atomics; what holds whatever they decide: with two buckets of k >= 8 items each, one of them is
    shared by k lanes that do not include the first.  The tiles whose shared items stand first put them in lane 0."""
    F, outs = sv.file(curve, "runs"), outputs(curve, "runs")
    s, o = [(s, o) for s, o in zip(F.sections, outs) if s.family == "lanes"][0]
    lowbits, P = s.plan["lowbits"], s.plan["P"]
    lane0, elsewhere = set(), set()
    for _, t, _, (k, two, X, Y) in s.edges:
        off = o["tile_off"][0, t]
        assert off[1] - off[0] == 64
        low = o["tile_items"][0, t][off[0]:off[1]].astype(np.int64) & ((1 << lowbits) - 1)
        mult = np.bincount(low, minlength=1 << lowbits)
        assert mult[X // P] == k and (not two or mult[Y // P] == k)
        lane0.add(int(mult[low[0]]))                                              # lanes that share lane 0's bucket
        others = [int(c) for b, c in enumerate(mult) if c > 1 and b != low[0]]
        elsewhere.update(others)                                                  # lanes that share a bucket which is not lane 0's
        if two and k >= 8:
            assert k in others
        if k == 64:
            assert mult[low[0]] == 64
    # both situations were seen: the shared bucket in lane 0 just below, at and above the threshold of 8 lanes, and the same
    # numbers of lanes sharing a bucket that the first lane does not hold
    assert {7, 8, 9, 64} <= lane0, "%s: lanes sharing lane 0's bucket: %s" % (curve, sorted(lane0))
    assert {8, 9} <= elsewhere, "%s: lanes sharing another bucket: %s" % (curve, sorted(elsewhere))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_scalar_or(curve):
    F = sv.file(curve, "or")
    checked = 0
    for name in ["or"] + SORT_FILES:
        for s, o in zip(sv.file(curve, name).sections, outputs(curve, name)):
            assert [int(x) for x in o["or"]] == sv.scalar_or(s.scalars), "%r: the OR words" % s
            checked += 1
    assert [s.label for s in F.sections] == sv.OR_CASES and checked > len(sv.OR_CASES)


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_points(curve, glv):
    F = sv.file(curve, "points")
    s, o = F.sections[glv], outputs(curve, "points")[glv]
    assert s.glv == glv
    rows = o["pts"].reshape(len(s.points), -1)
    names = [nm for nm, _, _ in sv.point_cases(curve)]
    checked = 0
    for i, pt in enumerate(s.points):
        want = [x for row in sv.expected_point_words(curve, glv, pt) for x in row]
        assert [int(x) for x in rows[i]] == want, "%s glv %d point %d (%s)" % (curve, glv, i, names[i % len(names)])
        if names[i % len(names)] in ("inf", "inf+p"):
            assert not rows[i].any()
        checked += 1
    assert checked == len(s.points) > 256


# ================================================================ window trimming through the public API
@pytest.fixture(scope="module")
def mx():
    from porla_amd import multiexp
    return multiexp


TRIM_BITS = [1, 32, 33, 126, 127, 249, 250, 254]


@functools.lru_cache(maxsize=None)
def trim_inputs(curve, b):
    """n pairs (scalar bytes, point bytes, n, expected point): all scalars below 2^b, bit b - 1 set only in the last one"""
    C = ev.CURVES[curve]
    rng = random.Random(1000 + b)
    n = 32769 + 7 * b
    assert 32769 <= n <= 40000
    ks = [rng.randrange(1, 49) for _ in range(n)]
    sc = [rng.getrandbits(b - 1) if b > 1 else 0 for _ in range(n - 1)] + [(1 << (b - 1)) | (rng.getrandbits(b - 1) if b > 1 else 0)]
    assert all(x < 1 << (b - 1) for x in sc[:-1]) and sc[-1] >> (b - 1) == 1
    G = ev.multiples(C)
    pt = {k: G[k][0].to_bytes(32, "big") + G[k][1].to_bytes(32, "big") for k in range(1, 49)}
    want = bv.mul(C, sum(x * k for x, k in zip(sc, ks)) % lv.order(C))
    assert want is not None
    return b"".join(x.to_bytes(32, "big") for x in sc), b"".join(pt[k] for k in ks), n, want[0].to_bytes(32, "big") + want[1].to_bytes(32, "big")


@pytest.mark.parametrize("b", TRIM_BITS)
@pytest.mark.parametrize("split", ["default", "off"])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_window_trimming(mx, curve, split, b):
    """k_scalar_or finds the scalars' length b, msm_launch drops the windows above it.  Points are k G, so the expected sum is computed
    in the exponent.
      off      the split forced off (porla_gpu_set_msm_glv(0)): W = ceil((b + 1) / c) while b < 250, from there on the windows of the
               full scalar length
      default  the split is on at this size on both curves and is dropped where there is nothing to split (b <= BITS of the
               sub-scalars: 126 on BN254, 128 on secp256k1) -- then W = ceil((b + 1) / c) as well; where it stays on the windows are the
               sub-scalars', ceil((BITS + 1) / c)"""
    from porla_amd import lib
    sc, pt, n, want = trim_inputs(curve, b)
    full, sub = sv.SCALAR_BITS[curve], sv.GLV_BITS[curve]
    lib.porla_gpu_set_msm_glv(0 if split == "off" else -1)
    try:
        got = mx.msm_host(curve, sc, pt, n)
        c, W, glv = mx.last_msm_shape()
    finally:
        lib.porla_gpu_set_msm_glv(-1)
    where = "%s split %s b=%d n=%d: c=%d W=%d glv=%d" % (curve, split, b, n, c, W, glv)
    assert glv == (split == "default" and b > sub), where
    bits = sub if glv else (b if b < 250 else full)
    assert 2 <= c <= 20 and W == -(-(bits + 1) // c), where
    assert got == want, where

"""GPU: the bucket accumulation of porla_amd/csrc/msm.hip.h -- k_size_hist / k_size_scan / k_size_order, k_bucket_sum30 and
k_bucket_combine as they are, launched by tools/bucket_sum_check.hip on bucket lists the test wrote, so every exceptional operand
stands at a chosen position of a chosen item (tests/bucket_vectors.py: the families position, items, heavy_stride, accumulate, glv,
fill; tests/test_bucket_vectors_cpu.py asserts that all of them are there).  Per curve and pass:
  sums        every bucket through ec_vectors.check_point_mem: the memory form's value bound for the curve (flip_finish where
              k_bucket_sum30 stored the bucket, add where k_bucket_combine did, operand where a sum passed through), then the group
              element against the sum computed in the exponent; infinity is all-zero words; a bucket a later pass does not touch, or
              brings only points at infinity to, is bit-identical to what the previous pass left
  scheduling  ctrl[1..3], the size rows ctrl[4..], order, chunk_base and heavy_list against the counts
Comparison is exact; every bucket of every pass is checked (checked == generated is asserted).
Then the accumulating ranges of msm_host_multi through the public API, against the oracle's naive sum."""
import functools
import os
import random

import numpy as np
import pytest

from tests import bucket_vectors as bv
from tests import common
from tests import ec_vectors as ev

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "secp256k1"]
FILE_NAMES = ["single", "accumulate", "glv"]


def test_driver_is_built():
    assert os.path.exists(bv.EXE), "build it with make -C porla_amd/csrc"


@functools.lru_cache(maxsize=None)
def outputs(curve, name):
    """one driver run per curve and file; tens of seconds at the most, the kernels themselves take milliseconds"""
    return bv.run(bv.FILES[name](curve), timeout=60)


@pytest.mark.parametrize("name", FILE_NAMES)
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_bucket_sums(curve, name):
    C = ev.CURVES[curve]
    F = bv.FILES[name](curve)
    outs, exp = outputs(curve, name), bv.expected(F)
    checked = 0
    for p in range(F.n_passes):
        rows = outs[p]["buckets"]
        assert rows.shape == (len(F.cases), 32)
        for b, (c, e) in enumerate(zip(F.cases, exp[p])):
            where = "%s %s pass %d bucket %d: %s %s L=%s j=%s %s, %d entries" % (
                curve, name, p, b, c["family"], c["kind"], c["L"], c["j"], c["form"], len(c["passes"][p]))
            if e["same"]:
                assert np.array_equal(rows[b], outs[p - 1]["buckets"][b]), where + ": not the bits the previous pass left"
            ev.check_point_mem(C, rows[b], bv.mul(C, e["exp"]), e["key"], where)
            checked += 1
    assert checked == len(F.cases) * F.n_passes > 0
    if name == "single":                                          # the combine's grid-stride loop went round again
        assert int(outs[0]["ctrl"][2]) > bv.COMBINE_BLOCKS


@pytest.mark.parametrize("name", FILE_NAMES)
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_scheduling(curve, name):
    F = bv.FILES[name](curve)
    outs = outputs(curve, name)
    for p in range(F.n_passes):
        where = "%s %s pass %d" % (curve, name, p)
        o = outs[p]
        counts = np.array(F.counts(p), dtype=np.int64)
        items = (counts + bv.CHUNK - 1) // bv.CHUNK
        ctrl = [int(x) for x in o["ctrl"]]
        assert ctrl[3] == int(items.sum()), where
        order = o["order"].astype(np.int64)
        assert order.shape == (ctrl[3], 2)
        # each (bucket, item) pair exactly once: the order itself comes from LDS atomics, so compare sorted
        want_pairs = sorted((b, i) for b, it in enumerate(items.tolist()) for i in range(it))
        assert sorted(map(tuple, order.tolist())) == want_pairs, where + ": order is not every (bucket, item) once"
        sizes = np.minimum(bv.CHUNK, counts[order[:, 0]] - bv.CHUNK * order[:, 1]) if ctrl[3] else np.zeros(0, dtype=np.int64)
        assert np.all(sizes[:-1] >= sizes[1:]), where + ": item sizes increase along order"
        for r in range(bv.CHUNK):
            assert ctrl[4 + r] == int(np.count_nonzero(sizes == bv.CHUNK - r)), where + ": size row %d" % r
        multi = [b for b, it in enumerate(items.tolist()) if it > 1]
        cb = [int(x) for x in o["chunk_base"]]
        assert [b for b in range(len(cb)) if cb[b] != bv.NO_CHUNK] == multi, where + ": chunk_base"
        at = 0
        for lo, hi in sorted((cb[b], cb[b] + int(items[b])) for b in multi):       # disjoint, and they fill [0, ctrl[1])
            assert lo == at, where + ": item-sum ranges overlap or leave a gap at %d" % at
            at = hi
        assert at == ctrl[1], where
        assert ctrl[2] == len(multi) and sorted(int(x) for x in o["heavy"]) == multi, where + ": heavy_list"


def test_malformed_files_are_refused(tmp_path):
    """an index beyond the table, counts that do not sum to the entry count, a truncated file: a message and a non-zero status,
    before anything reaches the device"""
    import subprocess
    F = bv.glv_file("bn254")
    good = F.words()
    n_points, nb = int(good[1]), int(good[3])
    first_pass = bv.HDR + 16 * n_points
    entries_at = first_pass + 1 + nb

    def refused(words, what):
        fin = str(tmp_path / "in")
        words.tofile(fin)
        r = subprocess.run([bv.EXE, "bn254", fin, str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr, (r.returncode, r.stderr)
    bad = good.copy()
    bad[entries_at + 5] = 2 * n_points                            # the doubled table ends at 2 n_points - 1
    refused(bad, "addresses point")
    bad = good.copy()
    bad[entries_at + 5] = (2 * n_points) | bv.SIGN
    refused(bad, "addresses point")
    bad = good.copy()
    bad[first_pass + 1] += 1
    refused(bad, "counts sum")
    bad = good.copy()
    bad[first_pass] += 1
    refused(bad, "file ends inside the entries")
    refused(good[:-3], "file ends inside the entries")
    bad = good.copy()
    bad[2] = 0                                                    # the same entries over the plain table: half as many points
    refused(bad, "addresses point")
    bad = good.copy()
    bad[0] ^= 1
    refused(bad, "not a bucket_sum_check file")


# ================================================================ the accumulating ranges of msm_host_multi
@pytest.fixture(scope="module")
def mx():
    from porla_amd import multiexp
    return multiexp


def multi_inputs(C, S, variant):
    """n = S m pairs whose range boundaries (s n / S = s m) cut through the compositions of the accumulate family: the scalar v
    chooses the bucket, so all pairs of one v meet in the same buckets, range after range.  Points are k G for known k (0: the
    point at infinity); every range is filled up to m pairs with random scalars over random points.
    variant "inf_range": one whole range (the first of two, the middle one of three) holds only points at infinity"""
    rng = random.Random(1000 * S + len(variant))
    ks = rng.sample(range(1, bv.SMALL + 1), 40)
    fresh = lambda: [ks.pop() * rng.choice([1, -1]) for _ in range(3)]

    def multi(count):
        return [k * rng.choice([1, -1]) for k in rng.sample(range(1, bv.SMALL + 1), count)]
    comps = []
    P, Q, R = fresh()
    comps.append(([P], [P], [P]))                                 # the stored sum equals the incoming point
    P, Q, R = fresh()
    comps.append(([P], [-P], [Q]))                                # ... its negative: P -> infinity -> Q
    P, Q, R = fresh()
    comps.append(([P], [-P, Q], [-Q]))
    P, Q, R = fresh()
    comps.append(([P], [], [P]))                                  # a range that leaves the bucket alone
    P, Q, R = fresh()
    comps.append(([P, -P], [Q], [R]))                             # a stored infinity
    P, Q, R = fresh()
    comps.append(([P], [0, 0], [-P]))                             # only points at infinity in this range
    P, Q, R = fresh()
    comps.append(([P, Q], [-Q, -P], [R, P]))
    P, Q, R = fresh()
    comps.append(([P, Q, R], [P], [Q, R]))
    m0 = multi(130)                                               # a multi-item bucket, then one entry equal to its sum / its negative
    comps.append((m0, [sum(m0)], [sum(m0)]))
    m1 = multi(130)
    comps.append((m1, [-sum(m1)], [Q]))
    P, Q, R = fresh()
    m2 = multi(129)
    comps.append(([P], m2 + [P - sum(m2)], [-2 * P]))             # a multi-item range whose total equals the stored sum
    ranges = [[] for _ in range(S)]
    for v, comp in enumerate(comps, start=1):
        for s in range(S):
            ranges[s] += [(v, k) for k in comp[s]]
    P, Q, R = fresh()
    ranges[S - 1].append((len(comps) + 1, Q))                     # a bucket only the last range touches
    m = max(len(r) for r in ranges) + 7
    sc, pt = [], []
    for s, r in enumerate(ranges):
        rng.shuffle(r)
        pairs = [(v.to_bytes(32, "big"), k) for v, k in r]
        pairs += [(rng.getrandbits(256).to_bytes(32, "big"), rng.randrange(1, bv.SMALL + 1)) for _ in range(m - len(r))]
        if variant == "inf_range" and s == (0 if S == 2 else 1):
            pairs = [(b, 0) for b, _ in pairs]
        for b, k in pairs:
            P = bv.mul(C, k)
            sc.append(b)
            pt.append(bytes(64) if P is None else P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big"))
    assert len(sc) == S * m and all(len(r) <= m for r in ranges)
    return b"".join(sc), b"".join(pt), S * m


@pytest.mark.parametrize("variant", ["compositions", "inf_range"])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_msm_host_multi_accumulating_ranges(mx, curve, S, variant):
    """the ranges of one device share one bucket array (PORLA_MSM_SHARED_BUCKETS at its default): the second and third range
    run with accumulate = 1"""
    assert os.environ.get("PORLA_MSM_SHARED_BUCKETS", "1") != "0"
    C = ev.CURVES[curve]
    sc, pt, n = multi_inputs(C, S, variant)
    assert n % S == 0 and 300 <= n <= 1000
    want = common.oracle_msm(sc, pt, n, naive=True) if curve == "bn254" else common.oracle_secp_msm(sc, pt, n, naive=True)
    got = mx.msm_host_multi(curve, sc, pt, n, shards=S, devices=1)
    assert mx.last_msm_multi() == (S, 1)
    assert got == want
    assert want != bytes(64)

"""The pipelined MSM path (msm_begin / msm_end: k_bucket_sum30, the tree's first two levels in one launch, k_tree_front2) against
the oracle (GPU box only).  Bar: bit-exact 64-byte output.

The order of a bucket's entries is whatever the counting sort leaves (LDS atomics: it differs from run to run), so a test
cannot pin an entry to a position.  The exceptional-operand case below therefore builds thousands of small buckets out of a few
compositions (P and -P, P twice, points at infinity, among ordinary points) and mixes uniformly random pairs into the same
buckets: over that many buckets every composition meets every position -- first (the copy), second (the affine + affine form),
third (the first iteration of the straight-line loop) and last -- and every such meeting is a lane that leaves the fast loop with
that entry still to do.  The same buckets feed k_tree_front2 infinite, equal and opposite operands in neighbouring buckets.
Pinned positions are tests/test_bucket_sum_gpu.py's: it launches the accumulation kernels on bucket lists it wrote itself.
"""
import random

import pytest

from tests import common

pytestmark = pytest.mark.gpu

N20 = 1 << 20


@pytest.fixture(scope="module")
def mx():
    from porla_amd import multiexp
    return multiexp


def in_flight(mx, jobs, curve="bn254"):
    """jobs: [(scalars, points, n)], at most three; all begun on their own streams before the first is collected"""
    import torch
    assert len(jobs) <= 3
    bufs, streams = [], [torch.cuda.Stream() for _ in jobs]
    for sc, pt, n in jobs:
        bufs.append((torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(pt), dtype=torch.uint8).cuda()))
    torch.cuda.synchronize()
    for k, (_, _, n) in enumerate(jobs):
        mx.msm_begin(1 + k, bufs[k][0].data_ptr(), bufs[k][1].data_ptr(), n, streams[k].cuda_stream, curve=curve)
    return [mx.msm_end(1 + k, curve=curve) for k in range(len(jobs))]


def test_2_20_uniform_audit_and_all_equal_scalars_in_flight(mx):
    """three 2^20-pair MSMs in flight: uniform 256-bit scalars; the audit's abs(int32) coefficients over 64-way repeated points
    (two windows, ~2^20 / 2^16 entries per bucket with repeats of one point inside a bucket); ONE scalar for every pair (each
    window is a single bucket of 2^20 entries: 8 192 work items of CHUNK entries, folded by k_bucket_combine)"""
    sc, pt = common.cached_inputs(N20)
    rnd = random.Random(11)
    sc_audit = b"".join((rnd.getrandbits(31)).to_bytes(32, "big") for _ in range(N20))
    pt_audit = pt[:64 * (N20 // 64)] * 64
    sc_equal = sc[:32] * N20
    jobs = [(sc, pt, N20), (sc_audit, pt_audit, N20), (sc_equal, pt_audit, N20)]
    got = in_flight(mx, jobs)
    for g, (s, p, n) in zip(got, jobs):
        assert g == common.oracle_msm(s, p, n)


def exceptional_inputs(n_special_buckets, n_fill, seed):
    """buckets v = 1 .. n_special_buckets of window 0 receive one of eight compositions (scalar v for each of its points);
    n_fill pairs with uniformly random 256-bit scalars land in the same buckets"""
    import bn254_py as o
    rnd = random.Random(seed)
    base = common.synth_points(64, start=5000)
    P = [base[64 * i:64 * i + 64] for i in range(64)]
    INF = bytes(64)
    neg = o.neg_point
    pairs = []
    for v in range(1, n_special_buckets + 1):
        a, b, c, d = rnd.sample(P, 4)
        comp = [[a, neg(a)],
                [INF, a],
                [a, neg(a), b],
                [a, a, b],
                [INF, a, b, neg(a)],
                [a, b, c, d, neg(d)],
                [INF, INF, INF],
                [a, b, INF, c, neg(b), a, INF, d]][v % 8]
        for q in comp:
            pairs.append((v, q))
    fill_sc = common.synth_scalars(n_fill, start=77000)
    fill_pt = common.synth_points(n_fill, start=77000)
    for i in range(n_fill):
        pairs.append((int.from_bytes(fill_sc[32 * i:32 * i + 32], "big"), fill_pt[64 * i:64 * i + 64]))
    rnd.shuffle(pairs)
    sc = b"".join(k.to_bytes(32, "big") for k, _ in pairs)
    pt = b"".join(q for _, q in pairs)
    return sc, pt, len(pairs)


@pytest.mark.parametrize("fill", [0, 30000])
def test_infinity_and_opposite_points_at_every_entry_position(mx, fill):
    """fill = 0: the special buckets alone (short scalars: one window, buckets of 2 .. 8 entries, so the first, second, third and last
    positions are most of them); fill = 30 000: the same buckets with ~4 random entries mixed in, all windows populated.  More than
    32 768 pairs, so the general path runs (k_bucket_sum30, the tree), begun and collected through msm_begin / msm_end"""
    sc, pt, n = exceptional_inputs(8192 if fill else 12288, fill, seed=fill + 1)
    assert n > 32768
    got, = in_flight(mx, [(sc, pt, n)])
    assert got == common.oracle_msm(sc, pt, n, naive=True)
    # the blocking call (the unfused tree levels) agrees
    assert mx.msm_host("bn254", sc, pt, n) == got


def test_secp256k1_2_18_in_flight(mx):
    """the same kernel template on the special-form field (three waves per SIMD, canonical memory form): 2^18 pairs of the
    reference bench's inputs, two MSMs in flight"""
    n = 1 << 18
    sc = common.secp_bench_scalars(n)
    pt = common.secp_bench_points(n)
    got = in_flight(mx, [(sc, pt, n), (sc[:32 * (n - 5)], pt[:64 * (n - 5)], n - 5)], curve="secp256k1")
    assert got[0] == common.secp_bench_expected(sc, n)
    assert got[1] == common.secp_bench_expected(sc, n - 5)

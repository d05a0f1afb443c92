"""The guest-room form of the pipelined MSM (msm_begin / msm_end from GUEST_MIN pairs: k_bucket_sum30 launched so that a compute
unit keeps room, k_bucket_combine and the reduction tree held to 128 registers at wave priority 3) against the oracle (GPU box only).
Bar: bit-exact 64-byte output.

Every case runs at the threshold size, the smallest at which the form is taken; the MSMs of a case are all begun before the first is
collected, so accumulations, combines and trees of different MSMs do run side by side.
"""
import random

import pytest

from tests import common
from tests.test_msm_pipelined_gpu import exceptional_inputs, in_flight

pytestmark = pytest.mark.gpu

GUEST_MIN = 1 << 17          # engine.hpp: MSM_GUEST_MIN_PAIRS


@pytest.fixture(scope="module")
def mx():
    from porla_amd import multiexp
    return multiexp


@pytest.fixture(scope="module")
def uniform():
    """three inputs of GUEST_MIN pairs with uniform 256-bit scalars (one point set, three scalar ranges) and their oracle results"""
    sc, pt = common.cached_inputs(GUEST_MIN)
    jobs = [(sc, pt, GUEST_MIN)]
    for k in (1, 2):
        jobs.append((common.synth_scalars(GUEST_MIN, start=k * GUEST_MIN + 12345), pt, GUEST_MIN))
    return jobs, [common.oracle_msm(s, p, n) for s, p, n in jobs]


@pytest.mark.parametrize("depth", [2, 3])
def test_uniform_scalars_in_flight(mx, uniform, depth):
    jobs, want = uniform
    assert in_flight(mx, jobs[:depth]) == want[:depth]


def test_degenerate_scalars_in_flight_together(mx, uniform):
    """ONE scalar for all pairs (every window is one bucket of GUEST_MIN / CHUNK items: k_bucket_combine folds them as a guest of
    the neighbours' accumulations); 31-bit scalars (two windows: another tree plan); and a uniform input between them"""
    jobs, want = uniform
    sc, pt, n = jobs[0]
    rnd = random.Random(23)
    sc_equal = sc[:32] * n
    sc_31 = b"".join(rnd.getrandbits(31).to_bytes(32, "big") for _ in range(n))
    got = in_flight(mx, [(sc_equal, pt, n), (sc, pt, n), (sc_31, pt, n)])
    assert got[0] == common.oracle_msm(sc_equal, pt, n)
    assert got[1] == want[0]
    assert got[2] == common.oracle_msm(sc_31, pt, n)


def test_exceptional_operands_in_flight(mx, uniform):
    """P and -P, P twice and points at infinity in thousands of small buckets of window 0 (tests/test_msm_pipelined_gpu.py), under
    GUEST_MIN uniform pairs that land in the same buckets: two such MSMs in flight"""
    import bn254_py as o
    jobs, want = uniform
    sc, pt, n = jobs[0]
    cases = []
    for seed in (5, 6):
        s_sc, s_pt, s_n = exceptional_inputs(4096, 0, seed=seed)
        special = common.oracle_msm(s_sc, s_pt, s_n, naive=True)
        cases.append(((s_sc + sc, s_pt + pt, s_n + n), o.add_point(special, want[0])))
    got = in_flight(mx, [c[0] for c in cases])
    assert got == [c[1] for c in cases]


def test_lone_call_beside_a_guest_and_slot_reuse(mx, uniform):
    """a blocking msm_device call on a third stream while a begun MSM is in flight (the lone form beside the guest form); then the
    slot is collected and used again"""
    import torch
    jobs, want = uniform
    dev = [(torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda())
           for s, p, _ in jobs[:2]]
    s1, s3 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    mx.msm_begin(1, dev[0][0].data_ptr(), dev[0][1].data_ptr(), GUEST_MIN, s1.cuda_stream)
    lone = mx.msm_device("bn254", dev[1][0].data_ptr(), dev[1][1].data_ptr(), GUEST_MIN, s3.cuda_stream)
    assert lone == want[1]
    assert mx.msm_end(1) == want[0]
    mx.msm_begin(1, dev[1][0].data_ptr(), dev[1][1].data_ptr(), GUEST_MIN, s1.cuda_stream)
    assert mx.msm_end(1) == want[1]


@pytest.mark.parametrize("n", [GUEST_MIN - 1, GUEST_MIN])
def test_below_and_at_the_threshold(mx, uniform, n):
    """in flight (two of the same input), just below the threshold and at it: the bytes of the blocking call"""
    import torch
    jobs, want = uniform
    sc, pt, _ = jobs[0]
    d_sc = torch.frombuffer(bytearray(sc[:32 * n]), dtype=torch.uint8).cuda()
    d_pt = torch.frombuffer(bytearray(pt[:64 * n]), dtype=torch.uint8).cuda()
    blocking = mx.msm_device("bn254", d_sc.data_ptr(), d_pt.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    if n == GUEST_MIN:
        assert blocking == want[0]
    else:
        assert blocking == common.oracle_msm(sc[:32 * n], pt[:64 * n], n)
    assert in_flight(mx, [(sc[:32 * n], pt[:64 * n], n)] * 2) == [blocking, blocking]

"""GPU box: the batched ICC MAC decode (porla_icc_mac_decode_batch_device / porla_icc_mac_decode_host) -- the coded MAC rows of a
level back to its per-block MACs -- byte for byte against the Python model tests/mac_decode_model.py, against the device encode's own
input at the sizes where the launch form changes, on the top level the cached server rebuild batch leaves in HBM (with the
complements as d_sub), and in the flow the feature exists for: decode a level's data and MACs, recompute each block's MAC from the
decoded chunks, compare.  Every comparison is byte equality; a guard region behind every output keeps its sentinel.

(The issue names n_rows = 32 as the first size with a wave-uniform stage; stage 1 has no ladder, so the first laddered stage whose
waves share a twiddle, n_rows >> s >= 16 with s >= 2, is stage 2 of n_rows = 64.  Both sizes are cases here.)"""
import functools
import random

import pytest

from tests import common  # noqa: F401  (puts oracle/ on the path)
import icc_py
from tests import mac_decode_model as model

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
SENTINEL = 0xA5
GUARD = 256                       # bytes behind every output that must keep the sentinel


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy())


def decode(inputs, n_rows, n_total, curve, steps=None, subs=None, stream=None):
    """one call on len(inputs) requests.  inputs / subs: bytes or device tensors (subs: None = NULL; "same" = the request's own
    input); steps: per request a list of write steps or None.  Returns [output bytes]; the guard behind every output is checked."""
    import torch
    from porla_amd import icc
    k = len(inputs)
    steps = steps or [None] * k
    subs = subs or [None] * k
    out_b = n_rows * 64
    ins = [x if hasattr(x, "is_cuda") else _dev(x) for x in inputs]
    d_subs = [None if s is None else (ins[a] if isinstance(s, str) else (s if hasattr(s, "is_cuda") else _dev(s))) for a, s in enumerate(subs)]
    outs = [torch.full((out_b + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(k)]
    d_steps = [None if s is None else torch.tensor(s, dtype=torch.int64).cuda() for s in steps]
    reqs = [(ins[a].data_ptr(), outs[a].data_ptr(), 0 if d_steps[a] is None else d_steps[a].data_ptr(),
             0 if d_subs[a] is None else d_subs[a].data_ptr()) for a in range(k)]
    torch.cuda.synchronize()
    icc.mac_decode_batch_device(reqs, n_rows, n_total, curve, stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    for a in range(k):
        assert bool(torch.all(outs[a][out_b:] == SENTINEL)), "request %d: the guard behind the output changed" % a
    return [_host(o[:out_b]) for o in outs]


def first_diff(got, want):
    return next((i // 64 for i in range(min(len(got), len(want))) if got[i] != want[i]), None)


def same(got, want, what=""):
    assert got == want, "%s: first differing row %s" % (what, first_diff(got, want))


def small_multiples(n, curve, seed):
    rng = random.Random(seed)
    g = model.GEN[curve]
    return [icc_py.ec_mul(curve, g, rng.randrange(1, 1 << 16)) for _ in range(n)]


def encode(macs_bytes, n_rows, curve, write_step=0, part=0):
    from porla_amd import icc
    return icc.mac_crebuild_host(macs_bytes, n_rows, curve, write_step, part)


@functools.lru_cache(maxsize=None)
def encoded_case(curve, n_rows):
    """(the encode of n_rows small multiples of the generator, what the model decodes it to): computed once, shared, left unchanged"""
    macs = small_multiples(n_rows, curve, 40 + n_rows)
    x = encode(model.points_to_bytes(macs), n_rows, curve)
    want = model.decode_bytes(x, n_rows, n_rows, curve)
    assert want == model.points_to_bytes(macs)                      # (the model inverts the device's encode)
    return x, want


# ---- 1. the device against the model
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_rows,n_total", [(2, 2), (4, 4), (32, 32), (64, 64), (64, 1 << 10)])
def test_decode_equals_the_model(curve, n_rows, n_total):
    """stage 1 only; the first laddered stage; 32 and 64 rows (wave-uniform stages from 64 on); the result does not depend on n_total
    without write steps"""
    x, want = encoded_case(curve, n_rows)
    same(decode([x], n_rows, n_total, curve)[0], want, "n_rows %d, n_total %d" % (n_rows, n_total))


@pytest.mark.parametrize("curve", CURVES)
def test_arbitrary_rows_and_reduced_bytes(curve):
    """rows that are no encode of anything small, one of them with x >= p in its bytes (reduced as SetBytes does), one at infinity"""
    from tests import ec_vectors as ev
    from tests import mac_decode_vectors as mv
    n = 4
    raw, _ = mv.noncanonical_bytes(ev.CURVES[curve])
    rows = model.points_to_bytes(small_multiples(2, curve, 8)) + raw + bytes(64)
    same(decode([rows], n, n, curve)[0], model.decode_bytes(rows, n, n, curve))


@pytest.mark.parametrize("curve", CURVES)
def test_unit_vectors(curve):
    """the encode of P at position i and infinity elsewhere is a constant column up to the twiddles: the first stage meets equal and
    opposite operands in every butterfly, every later stage infinity.  All 16 positions of 16 rows in one call, four of 32 rows"""
    p = small_multiples(1, curve, 3)[0]
    for n, positions in ((16, range(16)), (32, (0, 1, 17, 31))):
        units = [model.points_to_bytes([p if j == i else None for j in range(n)]) for i in positions]
        xs = [encode(u, n, curve) for u in units]
        got = decode(xs, n, n, curve)
        for i, g, x, u in zip(positions, got, xs, units):
            same(g, model.decode_bytes(x, n, n, curve), "n %d, position %d against the model" % (n, i))
            same(g, u, "n %d, position %d against the encode's input" % (n, i))


@pytest.mark.parametrize("curve", CURVES)
def test_infinity_levels(curve):
    """an all-infinity level; a level with a single non-infinity row (it passes through every stage beside infinity)"""
    n = 32
    p = small_multiples(1, curve, 4)[0]
    rows = [bytes(64 * n)] + [model.points_to_bytes([p if j == i else None for j in range(n)]) for i in (0, 1, 21, 31)]
    got = decode(rows, n, n, curve)
    assert got[0] == bytes(64 * n)
    for g, r in zip(got[1:], rows[1:]):
        same(g, model.decode_bytes(r, n, n, curve))


# ---- 2. write steps and d_sub
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_rows,n_total", [(16, 16), (16, 64), (64, 1 << 10)])
def test_write_steps_and_sub_equal_the_model(curve, n_rows, n_total):
    x, _ = encoded_case(curve, n_rows)
    sub = model.points_to_bytes([None if i % 5 == 2 else q for i, q in enumerate(small_multiples(n_rows, curve, 77))])
    steps = [n_total + 3 + 5 * i for i in range(n_rows)]
    got = decode([x, x, x, x], n_rows, n_total, curve, steps=[steps, None, steps, None], subs=[None, sub, sub, "same"])
    same(got[0], model.decode_bytes(x, n_rows, n_total, curve, steps), "write steps")
    same(got[1], model.decode_bytes(x, n_rows, n_total, curve, None, sub), "sub")
    same(got[2], model.decode_bytes(x, n_rows, n_total, curve, steps, sub), "write steps and sub")
    assert got[3] == bytes(64 * n_rows)                             # d_sub = d_macs: all infinity


# ---- 3. round trips with the device encode at the sizes where the launch form changes
@functools.lru_cache(maxsize=None)
def generator_base(curve):
    from porla_amd import multiexp as mx
    return mx.FixedBase(curve, model.point_bytes(model.GEN[curve]), 1, window_bits=8)


def device_points(curve, n, seed):
    """s_i G for n random 256-bit s_i, made on the device by a one-point fixed-base commit; a device tensor of n * 64 bytes"""
    import torch
    g = torch.Generator().manual_seed(seed)
    sc = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, generator=g).cuda()
    out = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    generator_base(curve).commit_device(sc.data_ptr(), n, 1, out.data_ptr())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n,k", [(10, 3), (13, 1), (14, 1), (15, 1), (16, 1)])
def test_decode_of_the_device_encode_is_the_input(curve, log_n, k):
    import torch
    from porla_amd import icc
    n = 1 << log_n
    macs = [device_points(curve, n, 100 * log_n + a) for a in range(k)]
    xs = [torch.empty(64 * n, dtype=torch.uint8, device="cuda") for _ in range(k)]
    for m, x in zip(macs, xs):
        icc.mac_crebuild_device(m.data_ptr(), n, curve, 0, 0, x.data_ptr())
    torch.cuda.synchronize()
    got = decode(xs, n, n, curve)
    for a in range(k):
        same(got[a], _host(macs[a]), "2^%d rows, request %d" % (log_n, a))


@pytest.mark.parametrize("curve", CURVES)
def test_y_part_round_trip(curve):
    """the Y output of the xy encode (Y_k = wt X_k) with the write step repeated per row decodes to the input; n_total = n_rows, as the
    encode takes wt from the table of its own row count"""
    import torch
    from porla_amd import icc
    n, step = 1 << 10, (1 << 10) + 37
    macs = device_points(curve, n, 5)
    x, y = (torch.empty(64 * n, dtype=torch.uint8, device="cuda") for _ in range(2))
    icc.mac_crebuild_xy_device(macs.data_ptr(), n, curve, step, x.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    assert not torch.equal(x, y)
    gx, gy = decode([x, y], n, n, curve, steps=[None, [step] * n])
    same(gx, _host(macs), "X")
    same(gy, _host(macs), "Y")


# ---- 4. K = 3 requests in one call on a non-default stream, one with a tampered row
@pytest.mark.parametrize("curve", CURVES)
def test_three_requests_one_tampered(curve):
    import torch
    n = 16
    cases = [encode(model.points_to_bytes(small_multiples(n, curve, 300 + a)), n, curve) for a in range(3)]
    tampered = bytearray(cases[1])
    tampered[64 * 11:64 * 12] = model.point_bytes(small_multiples(1, curve, 999)[0])
    xs = [cases[0], bytes(tampered), cases[2]]
    got = decode(xs, n, n, curve, stream=torch.cuda.Stream())
    for a in (0, 2):
        same(got[a], decode([xs[a]], n, n, curve)[0], "request %d against its single call" % a)
        same(got[a], model.points_to_bytes(small_multiples(n, curve, 300 + a)), "request %d against the encode's input" % a)
    same(got[1], model.decode_bytes(xs[1], n, n, curve), "the tampered request against the model")
    clean = model.points_to_bytes(small_multiples(n, curve, 301))
    assert all(got[1][64 * i:64 * i + 64] != clean[64 * i:64 * i + 64] for i in range(n))     # linearity: every row differs


# ---- 5. the top of the cached server rebuild at n_total = 2^6: mac_x / mac_y minus the complements decode to MAC_U
@pytest.mark.parametrize("curve", CURVES)
def test_top_of_the_cached_server_rebuild(curve):
    from tests import test_server_rebuild_batch_gpu as sr
    from tests.update_model import pt_bytes
    n = 64
    files = sr.make_requests(curve, n, False)
    devs = sr.run_on_device(curve, n, files)
    seen_sub = 0
    for d, (_, _, _, comps, step, _) in zip(devs, files):
        u_macs = d.bytes()["u_macs"]
        assert len(u_macs) == 64 * n
        cx = None if comps is None else b"".join(pt_bytes(p) for p in comps[:n])
        cy = None if comps is None else b"".join(pt_bytes(p) for p in comps[n:])
        seen_sub += comps is not None
        mx_, my_ = d.t["mac_x"][:64 * n].clone(), d.t["mac_y"][:64 * n].clone()
        gx, gy = decode([mx_, my_], n, n, curve, steps=[None, [step] * n], subs=[cx, cy])
        same(gx, u_macs, "mac_x, write step %d" % step)
        same(gy, u_macs, "mac_y, write step %d" % step)
    assert seen_sub == 2


# ---- 6. the flow the feature exists for (KZG): decode data and MACs, recompute the MACs from the decoded chunks, compare
def test_decoded_blocks_check_against_decoded_macs():
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    from tests.test_fixed_base_gpu import ALPHA, TAU
    n, ncols, curve = 16, 128, "bn254"
    mx.init_key(TAU, ALPHA)
    mx.init_SRS(ncols)
    g = torch.Generator().manual_seed(2024)
    u = torch.randint(0, 256, (n * ncols * 32,), dtype=torch.uint8, generator=g).cuda()          # the blocks: little-endian chunks
    prf = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    prf[:, :16] = 0                                                                                # 16-byte PRF values, big-endian
    prf = prf.reshape(-1).cuda()

    def block_macs(chunks_le):
        rows_be = chunks_le.reshape(-1, 32).flip(1).contiguous().reshape(-1)
        out = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        mx.kzg_mac_batch_device(rows_be.data_ptr(), prf.data_ptr(), n, out.data_ptr())
        torch.cuda.synchronize()
        return out

    macs = block_macs(u)
    x = torch.empty(n * ncols * 64, dtype=torch.uint8, device="cuda")
    mac_x = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    icc.crebuild_device(u.data_ptr(), n, ncols, curve, 0, 0, d_x=x.data_ptr())
    icc.mac_crebuild_device(macs.data_ptr(), n, curve, 0, 0, mac_x.data_ptr())
    torch.cuda.synchronize()

    def retrieve(rows):
        """(blocks whose recomputed MAC equals the decoded MAC, decoded chunks, decoded MACs)"""
        out = torch.empty(n * ncols * 32, dtype=torch.uint8, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        icc.decode_batch_device([(rows.data_ptr(), out.data_ptr(), 0, bad.data_ptr())], n, ncols, n, curve, "exact")
        got_macs = decode([mac_x], n, n, curve)[0]
        re = _host(block_macs(out))
        return [re[64 * i:64 * i + 64] == got_macs[64 * i:64 * i + 64] for i in range(n)], out, got_macs

    ok, chunks, got_macs = retrieve(x)
    assert got_macs == _host(macs) and torch.equal(chunks, u)
    assert ok == [True] * n
    altered = x.clone()
    altered[64 * (5 * ncols + 9)] ^= 1                                                             # row 5, column 9
    ok, _, _ = retrieve(altered)
    assert ok == [False] * n


# ---- 7. the host form; two streams
@pytest.mark.parametrize("curve", CURVES)
def test_host_form_equals_device_form(curve):
    from porla_amd import icc
    n, n_total = 16, 32
    x, _ = encoded_case(curve, n)
    sub = model.points_to_bytes(small_multiples(n, curve, 12))
    steps = [7 + 3 * i for i in range(n)]
    assert icc.mac_decode_host(x, n, n_total, curve) == decode([x], n, n_total, curve)[0]
    dev = decode([x], n, n_total, curve, steps=[steps], subs=[sub])[0]
    assert icc.mac_decode_host(x, n, n_total, curve, write_steps=steps, sub=sub) == dev
    assert dev == model.decode_bytes(x, n, n_total, curve, steps, sub)


@pytest.mark.parametrize("curve", CURVES)
def test_two_streams_one_after_the_other(curve):
    """the workspace (work array, derived tables) is reused by the next call on another stream behind the fence: the second call
    changes the table (another n_total) while the first may still run, the third changes it back"""
    import torch
    n = 1 << 10
    macs = device_points(curve, n, 9)
    x = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    from porla_amd import icc
    icc.mac_crebuild_device(macs.data_ptr(), n, curve, 0, 0, x.data_ptr())
    torch.cuda.synchronize()
    want = _host(macs)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [torch.full((64 * n,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(3)]
    for out, stream, n_total in zip(outs, (s1, s2, s1), (n, 2 * n, n)):
        icc.mac_decode_batch_device([(x.data_ptr(), out.data_ptr(), 0, 0)], n, n_total, curve, stream.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    for a, out in enumerate(outs):
        same(_host(out), want, "call %d" % a)

"""GPU box: the batched ICC decode (porla_icc_decode_batch_device / porla_icc_decode_host) -- the coded rows of a level back to its
blocks -- bit-exact against the Python model tests/icc_decode_model.py, against the oracle's input (icc_py.crebuild), against the
device encode's input, and on the levels the update batch and both server rebuild batches leave in HBM.  No tolerance anywhere."""
import functools
import random

import pytest

import icc_py
from tests import icc_decode_model as model

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
P = icc_py.P_ICC
SENTINEL = 0xA5
GUARD = 256                       # bytes behind every output that must keep the sentinel
BAD_PRESET = 0xDEADBEEF


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy())


def decode(form, inputs, n_rows, n_cols, n_total, curve, steps=None, want_bad=None, stream=None):
    """one call on len(inputs) requests.  inputs: bytes or device tensors; steps: per request a list of write steps or None; want_bad:
    per request whether it has a counter (preset to BAD_PRESET).  Returns ([output bytes], [counter or None]); the guard behind every
    output is checked here."""
    import torch
    from porla_amd import icc
    k = len(inputs)
    steps = steps or [None] * k
    want_bad = want_bad or [False] * k
    out_b = n_rows * n_cols * 32
    ins = [x if hasattr(x, "is_cuda") else _dev(x) for x in inputs]
    outs = [torch.full((out_b + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(k)]
    d_steps = [None if s is None else torch.tensor(s, dtype=torch.int64).cuda() for s in steps]
    d_bad = [torch.tensor([BAD_PRESET - (1 << 32)], dtype=torch.int32).cuda() if w else None for w in want_bad]
    reqs = [(ins[a].data_ptr(), outs[a].data_ptr(), 0 if d_steps[a] is None else d_steps[a].data_ptr(),
             0 if d_bad[a] is None else d_bad[a].data_ptr()) for a in range(k)]
    torch.cuda.synchronize()
    icc.decode_batch_device(reqs, n_rows, n_cols, n_total, curve, form, stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    for a in range(k):
        assert bool(torch.all(outs[a][out_b:] == SENTINEL)), "request %d: the guard behind the output changed" % a
    return [_host(o[:out_b]) for o in outs], [None if b is None else int(b.cpu()[0]) & 0xffffffff for b in d_bad]


def first_diff(got, want):
    return next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)


def chunks_with_edges(n, ncols, curve, seed):
    """n rows of ncols random chunks, the edge chunks pinned to row 0, row n / 2 and the last row"""
    rng = random.Random(seed)
    rows = [[rng.getrandbits(256) for _ in range(ncols)] for _ in range(n)]
    edges = model.edge_chunks(curve)
    for r, shift in ((0, 0), (n // 2, 3), (n - 1, 5)):
        for c in range(ncols):
            rows[r][c] = edges[(c + shift) % len(edges)]
    return rows


@functools.lru_cache(maxsize=None)
def oracle_case(curve, n_rows, n_cols):
    """(the chunks as bytes, their X part by the oracle as bytes): computed once per shape"""
    rows = chunks_with_edges(n_rows, n_cols, curve, 31 * n_rows + n_cols)
    X, _ = icc_py.crebuild(rows, curve)
    return model.rows_to_bytes(rows, 32), model.rows_to_bytes(X, 64)


# ---- 1. EXACT against the oracle: the radix-2 only, radix-4 only, odd count and two-round cases; the largest single pass; the first
# two-pass plan (n_cols = 3: a ragged column tile)
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_rows,n_cols", [(n, c) for n in (2, 4, 8, 16) for c in (1, 3, 128)] + [(512, 3), (1024, 3)])
def test_exact_equals_the_oracles_input(curve, n_rows, n_cols):
    want, x = oracle_case(curve, n_rows, n_cols)
    (got,), (bad,) = decode("exact", [x], n_rows, n_cols, n_rows, curve, want_bad=[True])
    assert got == want, "first differing byte %s" % first_diff(got, want)
    assert bad == 0
    if n_rows <= 16 and n_cols <= 3:
        assert model.decode_bytes("exact", x, n_rows, n_cols, n_rows, curve) == (want, 0)


@pytest.mark.parametrize("curve", CURVES)
def test_the_network_does_not_depend_on_n_total(curve):
    want, x = oracle_case(curve, 8, 3)
    for n_total in (8, 64, 1 << 16):
        (got,), _ = decode("exact", [x], 8, 3, n_total, curve)
        assert got == want, n_total
    (got,), _ = decode("residue64", [x], 8, 3, 64, curve)
    assert model.bytes_to_rows(got, 8, 3, 32) == [[v % P for v in r] for r in model.bytes_to_rows(want, 8, 3, 32)]


# ---- 2. worst-case operands: every symbol the largest its form allows, two passes
@pytest.mark.parametrize("curve", CURVES)
def test_worst_case_operands(curve):
    n_rows, n_cols = 1024, 3
    x = (icc_py.LCM[curve] - 1).to_bytes(64, "little") * (n_rows * n_cols)
    want, want_bad = model.decode_bytes("exact", x, n_rows, n_cols, n_rows, curve)
    (got,), (bad,) = decode("exact", [x], n_rows, n_cols, n_rows, curve, want_bad=[True])
    assert got == want, "exact: first differing byte %s" % first_diff(got, want)
    assert bad == want_bad
    r = (P - 1).to_bytes(32, "little") * (n_rows * n_cols)
    want, _ = model.decode_bytes("residue32", r, n_rows, n_cols, n_rows, curve)
    (got,), _ = decode("residue32", [r], n_rows, n_cols, n_rows, curve)
    assert got == want, "residue32: first differing byte %s" % first_diff(got, want)


# ---- 3. end to end on the device: decode(encode(U).x) == U
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_rows,n_cols", [(1024, 128), (1 << 16, 2)])
def test_decode_of_the_device_encode_is_the_input(curve, n_rows, n_cols):
    import torch
    from porla_amd import icc
    g = torch.Generator().manual_seed(n_rows + n_cols)
    u = torch.randint(0, 256, (n_rows * n_cols * 32,), dtype=torch.uint8, generator=g).cuda()
    x = torch.empty(n_rows * n_cols * 64, dtype=torch.uint8, device="cuda")
    icc.crebuild_device(u.data_ptr(), n_rows, n_cols, curve, 0, 0, d_x=x.data_ptr())
    torch.cuda.synchronize()
    (got,), (bad,) = decode("exact", [x], n_rows, n_cols, n_rows, curve, want_bad=[True])
    want = _host(u)
    assert got == want, "first differing byte %s" % first_diff(got, want)
    assert bad == 0


# ---- 4. the levels the update batch leaves: 7 writes at n_total = 8 (KZG build) put blocks 1-4 on level 2, 5-6 on level 1
@functools.lru_cache(maxsize=None)
def updated_file():
    """(the DevFile after the 7 writes, the blocks in write order as lists of chunks)"""
    import torch
    from tests import test_update_batch_gpu as ub
    from tests.update_model import FileModel
    from tests.test_server_rebuild_aligned_batch_gpu import server_of
    S = server_of("bn254")
    rnd = random.Random(77)
    n_total = 8
    d = ub.DevFile(FileModel(n_total, ub.NCOLS, "bn254", S.base, fill=ub.SENTINEL))
    blocks = []
    for step in range(1, n_total):
        level = (step & -step).bit_length() - 1
        chunks, mac, comps = ub.random_write(rnd, S, level, False)
        if step == 1:
            chunks[:7] = model.edge_chunks("bn254")
        blocks.append(chunks)
        S.call([d.req(chunks, mac, comps, step, level)], n_total)
    torch.cuda.synchronize()
    return d, blocks


@pytest.mark.parametrize("level,first", [(2, 1), (1, 5)])
def test_levels_of_the_update_batch(level, first):
    from tests import test_update_batch_gpu as ub
    d, blocks = updated_file()
    n, n_total, ncols = 1 << level, 8, ub.NCOLS
    mine = blocks[first - 1:first - 1 + n]
    steps = list(range(first, first + n))
    raw = model.rows_to_bytes(mine, 32)
    mod_p = model.rows_to_bytes([[v % P for v in r] for r in mine], 32)
    x = d.t["data_x"][level][:n * ncols * 64]
    y = d.t["data_y"][level][:n * ncols * 64]
    (gx, gy), _ = decode("residue64", [x, y], n, ncols, n_total, "bn254", steps=[None, steps])
    assert gx == mod_p, "X: first differing byte %s" % first_diff(gx, mod_p)
    assert gy == mod_p, "Y: first differing byte %s" % first_diff(gy, mod_p)
    (ex,), (bad,) = decode("exact", [x], n, ncols, n_total, "bn254", want_bad=[True])
    assert ex == raw and bad == 0


# ---- 5. the tops of both server rebuild batches at n_total = 16: X decodes to U, Y (= wt X, one write step for the whole level) too
@pytest.mark.parametrize("curve", CURVES)
def test_top_of_the_cached_server_rebuild(curve):
    from tests import test_server_rebuild_batch_gpu as sr
    n = 16
    files = sr.make_requests(curve, n, False)
    devs = sr.run_on_device(curve, n, files)
    for d, (_, _, _, _, step, _) in zip(devs, files):
        u = d.bytes()["u_blocks"]
        mod_p = model.rows_to_bytes([[v % P for v in r] for r in model.bytes_to_rows(u, n, sr.NCOLS, 32)], 32)
        x, y = d.t["data_x"][:n * sr.NCOLS * 64], d.t["data_y"][:n * sr.NCOLS * 64]
        (gx, gy), _ = decode("residue64", [x, y], n, sr.NCOLS, n, curve, steps=[None, [step] * n])
        assert gx == mod_p and gy == mod_p, "write step %d" % step
        (ex,), (bad,) = decode("exact", [x], n, sr.NCOLS, n, curve, want_bad=[True])
        assert ex == u and bad == 0


@pytest.mark.parametrize("curve", CURVES)
def test_top_of_the_aligned_server_rebuild(curve):
    from tests import test_server_rebuild_aligned_batch_gpu as ar
    n = 16
    ar.server_of(curve)
    files = ar.make_requests(curve, n, False)
    devs = ar.run_on_device(curve, n, files)
    for d, (_, _, _, _, step, _) in zip(devs, files):
        u = d.bytes()["u_blocks"]
        mod_p = model.rows_to_bytes([[v % P for v in r] for r in model.bytes_to_rows(u, n, ar.NCOLS, 32)], 32)
        x, y = d.t["data_x"][:n * ar.NCOLS * 32], d.t["data_y"][:n * ar.NCOLS * 32]
        (gx, gy), _ = decode("residue32", [x, y], n, ar.NCOLS, n, curve, steps=[None, [step] * n])
        assert gx == mod_p and gy == mod_p, "write step %d" % step


# ---- 6. K = 3 requests with different contents in one call on a non-default stream: a tampered one with a counter, an untampered one
# with a counter, one without
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_rows,n_cols", [(16, 5), (1024, 3)])
def test_three_requests_one_tampered(curve, n_rows, n_cols):
    import torch
    lcm = icc_py.LCM[curve]
    cases = []
    for a in range(3):
        rows = chunks_with_edges(n_rows, n_cols, curve, 900 + 10 * a + n_rows)
        X, _ = icc_py.crebuild(rows, curve)
        cases.append((rows, X))
    tr, tc = n_rows // 2 + 1, n_cols - 1
    cases[0][1][tr][tc] = (cases[0][1][tr][tc] + 1) % lcm
    xs = [model.rows_to_bytes(X, 64) for _, X in cases]
    (got, bad) = decode("exact", xs, n_rows, n_cols, n_rows, curve, want_bad=[True, True, False], stream=torch.cuda.Stream())
    assert bad == [n_rows, 0, None]
    want0, wbad0 = model.decode_bytes("exact", xs[0], n_rows, n_cols, n_rows, curve)
    assert wbad0 == n_rows
    assert got[0] == want0, "first differing byte %s" % first_diff(got[0], want0)
    g0 = model.bytes_to_rows(got[0], n_rows, n_cols, 32)
    for i in range(n_rows):                                      # every other column intact, the tampered one below p_icc
        assert g0[i][:tc] == cases[0][0][i][:tc] and g0[i][tc] < P
    for a in (1, 2):
        assert got[a] == model.rows_to_bytes(cases[a][0], 32), "request %d" % a


# ---- 7. the host form equals the device form
@pytest.mark.parametrize("curve", CURVES)
def test_host_form_equals_device_form(curve):
    from porla_amd import icc
    n_rows, n_cols, n_total = 16, 3, 32
    want, x = oracle_case(curve, n_rows, n_cols)
    assert icc.decode_host(x, n_rows, n_cols, n_total, curve, "exact") == (want, 0)
    tampered = bytearray(x)
    tampered[64 * (5 * n_cols + 1)] ^= 1
    (dev,), (bad,) = decode("exact", [bytes(tampered)], n_rows, n_cols, n_total, curve, want_bad=[True])
    assert icc.decode_host(bytes(tampered), n_rows, n_cols, n_total, curve, "exact") == (dev, bad) and bad == n_rows
    steps = [3 + 5 * i for i in range(n_rows)]
    (dev,), _ = decode("residue64", [x], n_rows, n_cols, n_total, curve, steps=[steps])
    assert icc.decode_host(x, n_rows, n_cols, n_total, curve, "residue64", write_steps=steps) == (dev, None)
    assert dev == model.decode_bytes("residue64", x, n_rows, n_cols, n_total, curve, steps)[0]
    x32 = model.rows_to_bytes([[v % P for v in r] for r in model.bytes_to_rows(x, n_rows, n_cols, 64)], 32)
    (dev,), _ = decode("residue32", [x32], n_rows, n_cols, n_total, curve)
    assert icc.decode_host(x32, n_rows, n_cols, n_total, curve, "residue32") == (dev, None)
    assert dev == model.decode_bytes("residue32", x32, n_rows, n_cols, n_total, curve)[0]

"""GPU box: the verified retrieval (porla_{kzg,ipa}_retrieve_batch_device / porla_{kzg,ipa}_retrieve_host) -- every coded row of an
exact half checked against its stored MAC row in the coded domain, then the EXACT data decode -- against the Python model
tests/retrieve_model.py (status bytes; the expected MACs are the model's), against the stand-alone decode (d_out, d_counts[1]), and in
the flow the call exists for: a level built by the device encodes from per-block MACs checks clean, X half and Y half, and so does the
top level the server rebuild batch leaves behind the client rebuild batch, all three calls on one stream.  Every comparison is byte
equality; a 256-byte guard behind every output keeps its sentinel.

The KZG build draws its MAC hiding base anew at every init_SRS, so every test initialises the state itself and reads h back
(compute_digest_complement(1)); the alpha-commitment halves of the expected MACs are computed once per case and shared."""
import functools
import random

import pytest

from tests import common  # noqa: F401  (puts oracle/ on the path)
import icc_py
from tests import mac_decode_model as mdm
from tests import retrieve_model as model
from tests.update_model import pt_tuple

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
SENTINEL = 0xA5
GUARD = 256
IPA_COLS = 128
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy())


# ---- the two builds
@functools.lru_cache(maxsize=None)
def ipa_bases():
    """128 alpha generators and a hiding point with known discrete logarithms (the model then needs one multiplication per row), and
    their fixed bases"""
    from porla_amd import multiexp as mx
    rng = random.Random(4242)
    g = mdm.GEN["secp256k1"]
    dlogs = [rng.randrange(1, 1 << 40) for _ in range(IPA_COLS)]
    h_dlog = rng.randrange(1, 1 << 40)
    gens = [icc_py.ec_mul("secp256k1", g, d) for d in dlogs]
    h = icc_py.ec_mul("secp256k1", g, h_dlog)
    afb = mx.FixedBase("secp256k1", model.points_to_bytes(gens), IPA_COLS, window_bits=8)
    hfb = mx.FixedBase("secp256k1", model.point_bytes(h), 1, window_bits=8)
    key = {"curve": "secp256k1", "alpha_generators": gens, "h": h, "dlogs": dlogs, "h_dlog": h_dlog}
    return key, afb, hfb


class Setup:
    """one build ready to be called: the model's key, the device call, the host form"""

    def __init__(self, curve, ncols=128):
        from porla_amd import multiexp as mx
        self.curve, self.ncols = curve, ncols
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS(ncols)
            q = icc_py.Q[curve]
            self.key = {"curve": curve, "alpha": int.from_bytes(ALPHA, "big") % q, "tau": int.from_bytes(TAU, "big") % q,
                        "h": pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))}
            self.call = lambda reqs, n_rows, n_total, stream=0: mx.kzg_retrieve_batch_device(reqs, n_rows, n_total, stream)
            self.host = lambda rows, macs, prf, n_rows, n_total, blocks=True: mx.kzg_retrieve_host(rows, macs, prf, n_rows, n_total, blocks)
        else:
            assert ncols == IPA_COLS
            self.key, afb, hfb = ipa_bases()
            self.call = lambda reqs, n_rows, n_total, stream=0: afb.ipa_retrieve_batch_device(hfb, reqs, n_rows, n_total, stream)
            self.host = lambda rows, macs, prf, n_rows, n_total, blocks=True: afb.ipa_retrieve_host(hfb, rows, macs, prf, n_rows, n_total, blocks)

    def expected(self, commits, prf):
        """the expected MACs from the rows' alpha-commitments (shared, they do not depend on h) and this state's hiding base"""
        return [icc_py.ec_add(self.curve, c, model.hiding(s, self.key)) for c, s in zip(commits, prf)]


def commit_key(curve):
    """what alpha_commit needs: no hiding base"""
    if curve == "bn254":
        q = icc_py.Q[curve]
        return {"curve": curve, "alpha": int.from_bytes(ALPHA, "big") % q, "tau": int.from_bytes(TAU, "big") % q}
    return ipa_bases()[0]


class Level:
    """one request's inputs as integers and bytes"""

    def __init__(self, curve, rows, prf, commits=None):
        self.curve, self.rows, self.prf = curve, rows, prf
        self.commits = commits if commits is not None else [model.alpha_commit(r, commit_key(curve)) for r in rows]
        self.rows_b, self.prf_b = model.rows_bytes(rows), model.prf_bytes(curve, prf)

    def with_row(self, j, row):
        rows = list(self.rows)
        rows[j] = row
        commits = list(self.commits)
        commits[j] = model.alpha_commit(row, commit_key(self.curve))
        return Level(self.curve, rows, self.prf, commits)


@functools.lru_cache(maxsize=None)
def coded_level(curve, n_rows, ncols, seed=0):
    """the X half of icc_py.crebuild on random blocks with random 128-bit PRF values: computed once, shared, left unchanged"""
    rng = random.Random(7000 + 131 * n_rows + ncols + seed)
    blocks = [[rng.getrandbits(256) for _ in range(ncols)] for _ in range(n_rows)]
    rows = icc_py.crebuild(blocks, curve, 0)[0]
    return Level(curve, rows, [rng.getrandbits(128) for _ in range(n_rows)])


def run(S, items, n_rows, n_total, stream=None, want_out=True, want_counts=True):
    """one call.  items: (rows bytes, macs bytes, prf bytes) per request.  Returns per request (status bytes, [counts] or None, blocks
    or None); the guards behind every output are checked."""
    import torch
    k, ncols = len(items), S.ncols
    out_b = n_rows * ncols * 32
    ins = [tuple(_dev(b) for b in it) for it in items]
    outs = [torch.full((out_b + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") if want_out else None for _ in range(k)]
    sts = [torch.full((n_rows + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(k)]
    cns = [torch.full((8 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") if want_counts else None for _ in range(k)]
    reqs = [(ins[a][0].data_ptr(), ins[a][1].data_ptr(), ins[a][2].data_ptr(), outs[a].data_ptr() if want_out else 0, sts[a].data_ptr(),
             cns[a].data_ptr() if want_counts else 0) for a in range(k)]
    torch.cuda.synchronize()
    S.call(reqs, n_rows, n_total, stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res = []
    for a in range(k):
        assert bool(torch.all(sts[a][n_rows:] == SENTINEL)), "request %d: the guard behind the status bytes changed" % a
        assert not want_out or bool(torch.all(outs[a][out_b:] == SENTINEL)), "request %d: the guard behind the blocks changed" % a
        assert not want_counts or bool(torch.all(cns[a][8:] == SENTINEL)), "request %d: the guard behind the counters changed" % a
        counts = list(cns[a][:8].cpu().view(torch.int32).tolist()) if want_counts else None
        res.append((_host(sts[a][:n_rows]), counts, _host(outs[a][:out_b]) if want_out else None))
    return res


def stand_alone_decode(rows_b, n_rows, ncols, n_total, curve):
    from porla_amd import icc
    return icc.decode_host(rows_b, n_rows, ncols, n_total, curve, "exact")


# ---- 1. the device against the model
SHAPES = [("bn254", 2, 2, 8), ("bn254", 4, 4, 9), ("bn254", 2, 2, 128), ("bn254", 4, 4, 128), ("bn254", 32, 32, 128), ("bn254", 64, 64, 128),
          ("bn254", 64, 1 << 10, 128), ("bn254", 2, 2, 1024), ("bn254", 2, 2, 1032), ("bn254", 32, 32, 9),
          ("secp256k1", 2, 2, 128), ("secp256k1", 4, 4, 128), ("secp256k1", 32, 32, 128), ("secp256k1", 64, 64, 128),
          ("secp256k1", 64, 1 << 10, 128)]


@pytest.mark.parametrize("curve,n_rows,n_total,ncols", SHAPES)
def test_statuses_equal_the_model(curve, n_rows, n_total, ncols):
    """SRS sizes 8 and 9 (a ragged eight-lane step), 128 (the protocol's), 1024 (the dot-product form's last size: 96 KiB of dynamic LDS,
    above the 64 KiB a kernel has without being told), 1032 (the Horner path); the MAC rows are the model's expected
    MACs, one of them replaced by its neighbour: the device's status bytes are the model's, and nothing depends on n_total"""
    S = Setup(curve, ncols)
    L = coded_level(curve, n_rows, ncols)
    want_macs = model.points_to_bytes(S.expected(L.commits, L.prf))
    macs = bytearray(want_macs)
    macs[64:128] = want_macs[:64]
    want = model.statuses(L.rows, bytes(macs), L.prf, S.key)
    assert want == bytes([1, 0] + [1] * (n_rows - 2))
    (st, counts, out), = run(S, [(L.rows_b, bytes(macs), L.prf_b)], n_rows, n_total)
    assert st == want
    assert counts == [1, 0]
    blocks, bad = stand_alone_decode(L.rows_b, n_rows, ncols, n_total, curve)
    assert out == blocks and bad == 0


def test_the_kzg_key_is_the_model_s():
    """the model's reading of the key bytes, G1[0] and h: its MAC of a small block is porla_kzg_mac_batch_device's"""
    import torch
    from porla_amd import multiexp as mx
    S = Setup("bn254", 8)
    coeffs, hide = [3, 1 << 200, 5, 0, 0, 7, 0, 1], (1 << 127) + 12345
    rows = _dev(b"".join(c.to_bytes(32, "big") for c in coeffs))
    sc = _dev(hide.to_bytes(32, "big"))
    out = torch.empty(64, dtype=torch.uint8, device="cuda")
    mx.kzg_mac_batch_device(rows.data_ptr(), sc.data_ptr(), 1, out.data_ptr())
    torch.cuda.synchronize()
    assert _host(out) == model.point_bytes(model.block_mac(coeffs, hide, S.key))


# ---- 2. the bounds of the symbol arithmetic
@pytest.mark.parametrize("curve", CURVES)
def test_chosen_symbols_in_every_column_position(curve):
    """0, 1, q - 1, q, q + 1, 2^256 - 1, 2^256, p_icc, LCM - 1 in every column position mod 8 (row t holds special[(c + t) % 9] in column
    c; 9 is coprime to 8), and one row of LCM - 1 throughout: the worst case for the columns between two ripples"""
    n_rows, ncols = 16, 128
    q, lcm = icc_py.Q[curve], icc_py.LCM[curve]
    special = [0, 1, q - 1, q, q + 1, (1 << 256) - 1, 1 << 256, icc_py.P_ICC, lcm - 1]
    rng = random.Random(99)
    rows = [[special[(c + t) % 9] for c in range(ncols)] for t in range(9)] + [[lcm - 1] * ncols]
    rows += [[(1 << 512) - 1] * ncols]                                        # (beyond the contract's < LCM: still sym mod q)
    rows += [[rng.randrange(lcm) for _ in range(ncols)] for _ in range(n_rows - len(rows))]
    S = Setup(curve, ncols)
    L = Level(curve, rows, [rng.getrandbits(128) for _ in range(n_rows - 1)] + [(1 << 128) - 1])
    macs = model.points_to_bytes(S.expected(L.commits, L.prf))
    (st, counts, _), = run(S, [(L.rows_b, macs, L.prf_b)], n_rows, n_rows, want_out=False)
    assert st == bytes([1] * n_rows) and counts == [0, 0]
    assert model.statuses(rows, macs, L.prf, S.key) == st


# ---- 3. the tamper sweep
@pytest.mark.parametrize("curve", CURVES)
def test_tamper_sweep(curve):
    from tests import ec_vectors as ev
    from tests import mac_decode_vectors as mv
    n, ncols = 16, 128
    S = Setup(curve, ncols)
    L = coded_level(curve, n, ncols)
    clean = model.points_to_bytes(S.expected(L.commits, L.prf))
    only = lambda j: bytes(0 if i == j else 1 for i in range(n))
    # one data symbol (row 5, column 9, low bit): only row 5; the blocks and the bad count are the stand-alone decode's of the altered rows
    altered = bytearray(L.rows_b)
    altered[64 * (5 * ncols + 9)] ^= 1
    # one MAC row replaced by another valid point; one PRF value altered
    swapped = bytearray(clean)
    swapped[64 * 3:64 * 4] = clean[64 * 12:64 * 13]
    prf2 = bytearray(L.prf_b)
    prf2[16 * 7 + 15] ^= 1
    # a MAC row rewritten with x + p: the same point, not its canonical form.  BN254: row 2 becomes (alpha^-1, 0, ...) with PRF 0, whose
    # expected MAC is the generator itself -- the canonical bytes pass (checked below), the bytes with x + p, y + p do not.  secp256k1:
    # only a tiny x leaves room for x + p below 2^256 and no row with that MAC can be made; the bytes stand in row 2 as they are
    raw, pt = mv.noncanonical_bytes(ev.CURVES[curve])
    N = L
    if curve == "bn254":
        q = icc_py.Q[curve]
        N = L.with_row(2, [pow(S.key["alpha"], -1, q)] + [0] * (ncols - 1))
        N = Level(curve, N.rows, N.prf[:2] + [0] + N.prf[3:], N.commits)
        assert S.expected(N.commits, N.prf)[2] == pt
    canon = bytearray(model.points_to_bytes(S.expected(N.commits, N.prf)))
    nonc = bytearray(canon)
    nonc[64 * 2:64 * 3] = raw
    assert mdm.bytes_to_points(raw, curve) == [pt]
    zero_row = [0] * ncols
    inf = bytearray(clean)
    inf[64 * 9:64 * 10] = bytes(64)
    # an all-zero data row with PRF 0 and 64 zero MAC bytes: the expected MAC is infinity, the row is OK
    Z = L.with_row(4, zero_row)
    Z = Level(curve, Z.rows, Z.prf[:4] + [0] + Z.prf[5:], Z.commits)
    z_macs = bytearray(model.points_to_bytes(S.expected(Z.commits, Z.prf)))
    assert bytes(z_macs[64 * 4:64 * 5]) == bytes(64)
    items = [(L.rows_b, clean, L.prf_b), (bytes(altered), clean, L.prf_b), (L.rows_b, bytes(swapped), L.prf_b), (L.rows_b, clean, bytes(prf2)),
             (N.rows_b, bytes(nonc), N.prf_b), (L.rows_b, bytes(inf), L.prf_b), (Z.rows_b, bytes(z_macs), Z.prf_b), (N.rows_b, bytes(canon), N.prf_b)]
    wants = [bytes([1] * n), only(5), only(3), only(7), only(2), only(9), bytes([1] * n), bytes([1] * n)]
    got = run(S, items, n, n)
    for a, ((st, counts, out), want) in enumerate(zip(got, wants)):
        assert st == want, "case %d" % a
        blocks, bad = stand_alone_decode(items[a][0], n, ncols, n, curve)
        assert counts == [want.count(0), bad], "case %d" % a
        assert out == blocks, "case %d" % a
    assert got[1][1][1] > 0                                                   # (the altered symbol decodes to values that are no chunks)
    # each case alone gives what it gave in the batch
    (st, counts, _), = run(S, [items[1]], n, n)
    assert st == only(5) and counts == got[1][1]


# ---- 4. d_out and the counters
@pytest.mark.parametrize("curve", CURVES)
def test_optional_outputs(curve):
    n, ncols = 16, 128
    S = Setup(curve, ncols)
    L = coded_level(curve, n, ncols)
    macs = model.points_to_bytes(S.expected(L.commits, L.prf))
    item = (L.rows_b, macs, L.prf_b)
    blocks, bad = stand_alone_decode(L.rows_b, n, ncols, n, curve)
    (st, counts, out), = run(S, [item], n, n)
    assert st == bytes([1] * n) and counts == [0, bad] and out == blocks
    (st, counts, out), = run(S, [item], n, n, want_out=False)
    assert st == bytes([1] * n) and counts == [0, 0] and out is None
    (st, counts, out), = run(S, [item], n, n, want_counts=False)
    assert st == bytes([1] * n) and counts is None and out == blocks
    (st, counts, out), = run(S, [item], n, n, want_out=False, want_counts=False)
    assert st == bytes([1] * n)


# ---- 5. K = 3 in one call on a non-default stream, the middle request tampered
@pytest.mark.parametrize("curve", CURVES)
def test_three_requests_one_tampered(curve):
    import torch
    n, ncols = 16, 128
    S = Setup(curve, ncols)
    levels = [coded_level(curve, n, ncols, seed) for seed in (0, 1, 2)]
    items = [[lv.rows_b, model.points_to_bytes(S.expected(lv.commits, lv.prf)), lv.prf_b] for lv in levels]
    mid = bytearray(items[1][0])
    mid[64 * (11 * ncols + 127) + 63 - 8] ^= 0x40
    items[1][0] = bytes(mid)
    items = [tuple(i) for i in items]
    got = run(S, items, n, n, stream=torch.cuda.Stream())
    for a in range(3):
        assert got[a] == run(S, [items[a]], n, n)[0], "request %d against its single call" % a
    assert got[0][0] == got[2][0] == bytes([1] * n)
    assert got[1][0] == bytes(0 if i == 11 else 1 for i in range(n)) and got[1][1][0] == 1


# ---- 6. two calls on two streams, one after the other with another n_total in between
@pytest.mark.parametrize("curve", CURVES)
def test_two_streams_one_after_the_other(curve):
    """the workspace (expected MACs, the packed rows; the decode's planes and the resident tables behind it) is reused by the next
    call on another stream behind its fence"""
    import torch
    n, ncols, k = 64, 128, 4
    S = Setup(curve, ncols)
    L = coded_level(curve, n, ncols)
    macs = bytearray(model.points_to_bytes(S.expected(L.commits, L.prf)))
    macs[64 * 40] ^= 1
    d = [_dev(L.rows_b), _dev(bytes(macs)), _dev(L.prf_b)]
    out_b = n * ncols * 32
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # every buffer is filled before the first call: torch fills on its own stream, which the calls' streams do not wait for
    calls = [([torch.full((out_b,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(k)],
              [torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(k)],
              [torch.full((2,), -1, dtype=torch.int32, device="cuda") for _ in range(k)]) for _ in range(3)]
    torch.cuda.synchronize()
    for (outs, sts, cns), stream, n_total in zip(calls, (s1, s2, s1), (n, 2 * n, n)):
        S.call([(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), outs[a].data_ptr(), sts[a].data_ptr(), cns[a].data_ptr()) for a in range(k)],
               n, n_total, stream.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    blocks, bad = stand_alone_decode(L.rows_b, n, ncols, n, curve)
    want = bytes(0 if i == 40 else 1 for i in range(n))
    for c, (outs, sts, cns) in enumerate(calls):
        for a in range(k):
            assert _host(sts[a]) == want and cns[a].tolist() == [1, bad] and _host(outs[a]) == blocks, "call %d, request %d" % (c, a)


# ---- 7. the host form equals the device form
@pytest.mark.parametrize("curve", CURVES)
def test_host_form_equals_device_form(curve):
    n, ncols = 16, 128
    S = Setup(curve, ncols)
    L = coded_level(curve, n, ncols)
    macs = bytearray(model.points_to_bytes(S.expected(L.commits, L.prf)))
    macs[64 * 6 + 40] ^= 0x80
    rows = bytearray(L.rows_b)
    rows[64 * (13 * ncols)] ^= 2
    item = (bytes(rows), bytes(macs), L.prf_b)
    (st, counts, out), = run(S, [item], n, 32)
    assert st == bytes(0 if i in (6, 13) else 1 for i in range(n))
    assert S.host(*item, n, 32) == (st, counts, out)
    assert S.host(*item, n, 32, False) == (st, [counts[0], 0], None)


# ---- 8. the flow: a level built by the device encodes from per-block MACs checks clean, X half and Y half with a write step
@pytest.mark.parametrize("curve", CURVES)
def test_a_level_built_by_the_device_encodes_checks_clean(curve):
    import torch
    from porla_amd import icc
    from porla_amd import multiexp as mx
    n, ncols, step = 16, 128, 16 + 3
    S = Setup(curve, ncols)
    q = icc_py.Q[curve]
    g = torch.Generator().manual_seed(2025)
    u = torch.randint(0, 256, (n * ncols * 32,), dtype=torch.uint8, generator=g).cuda()            # the blocks: little-endian chunks
    rows_be = u.reshape(-1, 32).flip(1).contiguous().reshape(-1)                                     # the commitment's coefficient rows
    rng = random.Random(31)

    def block_macs(hide):
        """alpha Commit(block_i) + hide_i h on the device: porla_kzg_mac_batch_device, or one commit against (alpha generators, h)"""
        out = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        sc = _dev(b"".join(x.to_bytes(32, "big") for x in hide))
        if curve == "bn254":
            mx.kzg_mac_batch_device(rows_be.data_ptr(), sc.data_ptr(), n, out.data_ptr())
        else:
            key = S.key
            both = mx.FixedBase(curve, model.points_to_bytes(key["alpha_generators"] + [key["h"]]), ncols + 1, window_bits=8)
            rows = torch.cat([rows_be.reshape(n, ncols * 32), sc.reshape(n, 32)], dim=1).contiguous().reshape(-1)
            both.commit_device(rows.data_ptr(), n, ncols + 1, out.data_ptr())
        torch.cuda.synchronize()
        return out

    for part, ws in ((0, 0), (1, step)):
        s = [rng.getrandbits(128) for _ in range(n)]
        macs = block_macs(model.hiding_scalars_for(s, curve, part, ws))
        x = torch.empty(n * ncols * 64, dtype=torch.uint8, device="cuda")
        mac_x = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
        icc.crebuild_device(u.data_ptr(), n, ncols, curve, ws, part, d_x=x.data_ptr())
        icc.mac_crebuild_device(macs.data_ptr(), n, curve, ws, part, mac_x.data_ptr())
        torch.cuda.synchronize()
        item = (_host(x), _host(mac_x), model.prf_bytes(curve, s))
        (st, counts, out), = run(S, [item], n, n, want_out=part == 0)
        assert st == bytes([1] * n), "part %d" % part
        if part == 0:
            assert counts == [0, 0] and out == _host(u)                       # the X half decodes to the blocks
        else:
            assert counts == [0, 0]
        # and a damaged stored row is named
        bad = bytearray(item[0])
        bad[64 * (9 * ncols + 77) + 31] ^= 0x10
        (st, counts, _), = run(S, [(bytes(bad), item[1], item[2])], n, n, want_out=False)
        assert st == bytes(0 if i == 9 else 1 for i in range(n)) and counts == [1, 0]
    assert q  # (both halves ran)


# ---- 9. the full chain at n_total = 16: client rebuild batch -> server rebuild batch -> this call, one stream, no host wait.  The U
# blocks' MACs are made with the PRF values the client rebuild request carries (complements_U[i] = prf[1 + i], the written block's own
# among them), so mac_x / mac_y hide exactly the rebuild's 2 n_total new PRF values
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("step_of", ["3 n", "n + 1"])
def test_the_full_chain_behind_the_two_rebuild_batches(curve, step_of):
    import torch
    from porla_amd import multiexp as mx
    from tests import test_client_rebuild_batch_gpu as cr, test_server_rebuild_batch_gpu as sr, test_update_batch_gpu as ub
    from tests.client_rebuild_model import n_prf
    from tests.update_model import pt_bytes
    n, ncols, index = 16, 128, 7
    step = 3 * n if step_of == "3 n" else n + 1                               # wt = 1 (CRebuild's own step), and a wt that is not 1
    S, client_call = cr.setup_of(curve)
    h = S.h
    if curve == "bn254":
        # the library's key, SRS and hiding point are process state: the setup's key goes in again, h is read as it stands now
        mx.init_key(ub.TAU, ub.ALPHA)
        mx.init_SRS_from_data(ncols, mx.init_SRS(ncols))
        h = pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))
        retrieve = lambda reqs, s: mx.kzg_retrieve_batch_device(reqs, n, n, s)
    else:
        retrieve = lambda reqs, s: S.afb.ipa_retrieve_batch_device(S.hfb, reqs, n, n, s)
    rnd = random.Random(500 + step)
    u = [[rnd.getrandbits(256) for _ in range(ncols)] for _ in range(n)]
    block = [rnd.getrandbits(256) for _ in range(ncols)]
    prf = [rnd.getrandbits(128) for _ in range(n_prf(n))]
    prf[index] = prf[0]                                                       # complements_U of the written slot is the block's own
    old, new_x, new_y = prf[1:1 + n], prf[1 + n:1 + 2 * n], prf[1 + 2 * n:]
    u_macs = [None if i == index - 1 else icc_py.ec_add(curve, S.block_commit(u[i]), icc_py.ec_mul(curve, h, old[i])) for i in range(n)]
    d = sr.DevFile(n, b"".join(sr.block_bytes(c) for c in u), b"".join(pt_bytes(p) for p in u_macs))
    d_block = _dev(sr.block_bytes(block))
    d_prf = _dev(b"".join(cr.raw_of(curve, v) for v in prf))
    d_new = [_dev(b"".join(cr.raw_of(curve, v) for v in part)) for part in (new_x, new_y)]
    d_mac = torch.full((64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_comp = torch.full((128 * n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out_b = n * ncols * 32
    outs = [torch.full((out_b + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    sts = [torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    cns = [torch.full((2,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    both_decode = step % n == 0                                               # Y = wt X: with wt = 1 the Y half decodes to U too
    reqs = [(d.t["data_" + p].data_ptr(), d.t["mac_" + p].data_ptr(), d_new[a].data_ptr(),
             outs[a].data_ptr() if a == 0 or both_decode else 0, sts[a].data_ptr(), cns[a].data_ptr()) for a, p in enumerate("xy")]
    server_req = d.req(d_block, d_mac, d_comp, step, index)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    client_call([(d_block.data_ptr(), d_prf.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), step)], n, stream.cuda_stream)
    sr.call([server_req], n, curve, stream.cuda_stream)
    retrieve(reqs, stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    u[index - 1] = block
    want_u = b"".join(sr.block_bytes(c) for c in u)
    assert _host(d.t["u_blocks"][:out_b]) == want_u
    for a, part in enumerate("xy"):
        assert _host(sts[a]) == bytes([1] * n) + bytes([SENTINEL]) * GUARD, "mac_%s" % part
        assert cns[a].tolist() == [0, 0], "mac_%s" % part
        if a == 0 or both_decode:
            assert _host(outs[a]) == want_u + bytes([SENTINEL]) * GUARD, "data_%s does not decode to U" % part


# ---- 10. the IPA bases are checked (behind the device check: a handle exists only where a device does)
def test_ipa_bad_bases_are_refused():
    """a base of 100 points, a BN254 base in either position, a hiding base of more than one point: PORLA_ERR_ARG with the entry point's
    name, from the batch and from the host form, and status, blocks and counters keep their sentinels"""
    import torch
    from porla_amd import multiexp as mx
    n, ncols = 4, IPA_COLS
    key, afb, hfb = ipa_bases()
    L = coded_level("secp256k1", n, ncols)
    macs = model.points_to_bytes(model.expected_macs(L.rows, L.prf, key))
    short = mx.FixedBase("secp256k1", model.points_to_bytes(key["alpha_generators"][:100]), 100, window_bits=8)
    bn = mx.FixedBase("bn254", common.synth_points(ncols), ncols, window_bits=8)
    d = [_dev(L.rows_b), _dev(macs), _dev(L.prf_b)]
    out = torch.full((n * ncols * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    cn = torch.full((8,), SENTINEL, dtype=torch.uint8, device="cuda")
    req = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), out.data_ptr(), st.data_ptr(), cn.data_ptr())
    torch.cuda.synchronize()
    for a, h, word in ((short, hfb, "128"), (afb, short, "exactly one"), (afb, afb, "exactly one"), (bn, hfb, "secp256k1"), (afb, bn, "secp256k1")):
        with pytest.raises(RuntimeError, match="porla_ipa_retrieve_batch_device.*" + word):
            a.ipa_retrieve_batch_device(h, [req], n, n)
        with pytest.raises(RuntimeError, match="porla_ipa_retrieve_host.*" + word):
            a.ipa_retrieve_host(h, L.rows_b, macs, L.prf_b, n, n)
    torch.cuda.synchronize()
    for t in (out, st, cn):
        assert bool(torch.all(t == SENTINEL)), "a refused call wrote"
    afb.ipa_retrieve_batch_device(hfb, [req], n, n)                            # (the same request with the right bases is served)
    torch.cuda.synchronize()
    assert _host(st) == bytes([1] * n)


# ---- 11. more rows than one group of the IPA build's coefficient workspace holds (2^16): K = 3 levels of 2^15 rows share their inputs,
# so the second group starts inside request 2.  The expected MACs come from the device's own fixed-base commit over the 128 alpha
# generators and h (symbols below 2^255, so sym mod n = sym and the coefficient row is the symbol's lower half, byte-flipped)
def test_ipa_rows_beyond_one_workspace_group():
    import torch
    from porla_amd import multiexp as mx
    n, ncols, k = 1 << 15, IPA_COLS, 3
    key, afb, hfb = ipa_bases()
    both = mx.FixedBase("secp256k1", model.points_to_bytes(key["alpha_generators"] + [key["h"]]), ncols + 1, window_bits=8)
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    lo = torch.randint(0, 256, (n * ncols, 32), dtype=torch.uint8, device="cuda", generator=g)
    lo[:, 31] &= 0x7f
    rows = torch.cat([lo, torch.zeros_like(lo)], dim=1).contiguous()                              # 64-byte little-endian symbols
    prf = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=g)            # r.d[0], r.d[1]: little-endian
    coeffs = torch.cat([lo.flip(1).reshape(n, ncols * 32), torch.zeros((n, 16), dtype=torch.uint8, device="cuda"), prf.flip(1)], dim=1).contiguous()
    macs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    both.commit_device(coeffs.data_ptr(), n, ncols + 1, macs.data_ptr())
    torch.cuda.synchronize()
    tampered = {0: 5, 1: n - 1, 2: 4464}                                       # rows 5, 65535 (the last of group 0) and 70000 (group 1) of the call
    macs_of = []
    for a in range(k):
        m = macs.clone()
        m[64 * tampered[a] + 63] ^= 1
        macs_of.append(m)
    sts = [torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(k)]
    cns = [torch.full((2,), -1, dtype=torch.int32, device="cuda") for _ in range(k)]
    torch.cuda.synchronize()
    afb.ipa_retrieve_batch_device(hfb, [(rows.data_ptr(), macs_of[a].data_ptr(), prf.data_ptr(), 0, sts[a].data_ptr(), cns[a].data_ptr())
                                        for a in range(k)], n, n)
    torch.cuda.synchronize()
    for a in range(k):
        want = torch.ones(n, dtype=torch.uint8, device="cuda")
        want[tampered[a]] = 0
        assert torch.equal(sts[a][:n], want), "request %d" % a
        assert bool(torch.all(sts[a][n:] == SENTINEL)) and cns[a].tolist() == [1, 0], "request %d" % a

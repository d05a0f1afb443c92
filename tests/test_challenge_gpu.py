"""GPU: AES on the device (include/porla_gpu.h: porla_mac_prf_batch_device, porla_audit_challenge_batch_device,
porla_audit_complement_scalar_batch_device, porla_diag_audit_walk(on_device = 1)).

The device forms equal the model / the host forms byte for byte, with a guard fill behind every output; and what they produce is what
the existing entry points consume: the complement scalar times h is the MSM over the challenged complements
(porla_bn254_msm_device), porla_kzg_audit_batch_device gives the same records from device-drawn lists as from uploaded ones, and
porla_kzg_verify_batch_device accepts honest replies -- and refuses a reply with an altered combined MAC -- both with a full
complement store plus drawn lists and with the ONE point of verify_reqs_from_scalars.

The IPA leg does the same through FixedBase.ipa_audit_batch_device / ipa_verify_batch_device on the fixtures of
tests/test_ipa_verify_batch_gpu.py (64 rows: a file of 32 blocks, whose levels are all-rows levels)."""
import random

import pytest

from tests import challenge_model as model
from tests.test_challenge_cpu import CHALLENGE_SHAPES, WALK_SHAPES, levels_for, seed_of, written_stream
from tests.test_kzg_verify_batch_gpu import ALPHA, ALPHA32, FULL, PASS, TAU, _dev, _records, server_records

pytestmark = pytest.mark.gpu

KEY = model.SECRET_KEY
assert KEY == ALPHA
GUARD = 0xA5
NCOLS, STORE_ROWS = 128, 512
LISTS = ("idx64", "coef64", "idx32", "coef32", "mac_idx", "mac_coef")


def _guarded(nbytes, slack=64):
    import torch
    return torch.full((nbytes + slack,), GUARD, dtype=torch.uint8, device="cuda")


def _bytes(t):
    import torch
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


# ---------------------------------------------------------------- the MAC PRF
PRF_CASES = {
    "one": [(3, 7, 1, 99, 0)],
    "sixty-five": [(2, -3, 65, (1 << 32) - 30, 1)],
    "group-boundaries": [(0, 0, 1, 5, 0), (1, 10, 255, 6, 1), (2, 20, 256, 7, 0), (3, 30, 257, 1 << 40, 1)],
    "rebuild-8": None,
    "three-runs-4097": [(4, 0, 2000, 1, 1), (5, 2000, 97, 77, 0), (6, -1000, 2000, -5, 1)],
    "empty-runs-between": [(0, 0, 0, 0, 0), (1, 1, 300, 1, 0), (2, 2, 0, 0, 0), (3, 3, 0, 0, 0), (4, 4, 300, 1, 1), (5, 5, 0, 0, 0)],
}


@pytest.mark.parametrize("name", list(PRF_CASES))
def test_mac_prf_batch_device_equals_the_model(name):
    from porla_amd import challenge as ch
    runs = PRF_CASES[name] or ch.client_prf_runs("rebuild", 3, 8, 8)[0]
    n = sum(r[2] for r in runs)
    if name == "three-runs-4097":
        assert n == 4097
    d = _guarded(16 * n)
    ch.mac_prf_batch_device(KEY, runs, d.data_ptr())
    got = _bytes(d)
    assert got[:16 * n] == b"".join(model.mac_prf(KEY, *t) for t in model.expand_runs(runs))
    assert got[16 * n:] == bytes([GUARD]) * 64


def test_mac_prf_on_a_side_stream_and_with_another_key():
    import torch
    from porla_amd import challenge as ch
    key = bytes(range(16, 32))
    runs = [(1, 0, 700, 3, 1)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = _guarded(16 * 700)
        ch.mac_prf_batch_device(key, runs, d.data_ptr(), stream=s.cuda_stream)
        ch.mac_prf_batch_device(key, [(1, 0, 10, 3, 1)], d.data_ptr() + 16 * 100, stream=s.cuda_stream)   # rewrites slots 100 .. 109
    s.synchronize()
    want = [model.mac_prf(key, *t) for t in model.expand_runs(runs)]
    want[100:110] = want[0:10]
    assert _bytes(d)[:16 * 700] == b"".join(want)


# ---------------------------------------------------------------- the challenge
def _list_tensors(info):
    import torch
    n = dict(idx64=info["n64"], coef64=info["n64"], idx32=info["n32"], coef32=info["n32"], mac_idx=info["n_macs"], mac_coef=info["n_macs"])
    return n, {name: _guarded((8 if "idx" in name else 4) * n[name], slack=32) for name in LISTS}


def _read_lists(n, tensors):
    import numpy as np
    out = {}
    for name in LISTS:
        raw = _bytes(tensors[name])
        w = 8 if "idx" in name else 4
        body, guard = raw[:w * n[name]], raw[w * n[name]:]
        assert guard == bytes([GUARD]) * 32, name
        out[name] = [int(v) for v in np.frombuffer(body, dtype=np.uint64 if w == 8 else np.uint32)]
    return out


def _draw_on_device(reqs):
    """reqs: (seed, write_step, num_blocks, levels); returns [(info, lists)] from ONE device call"""
    from porla_amd import challenge as ch
    plans = ch.audit_challenge_plan(reqs)
    bufs = [_list_tensors(p) for p in plans]
    full = [r + ([t[name].data_ptr() if n[name] else 0 for name in LISTS],) for r, (n, t) in zip(reqs, bufs)]
    infos = ch.audit_challenge_batch_device(full)
    assert infos == plans
    return [(info, _read_lists(n, t)) for info, (n, t) in zip(infos, bufs)]


@pytest.mark.parametrize("case", range(len(CHALLENGE_SHAPES)))
def test_audit_challenge_batch_device_equals_the_host_form(case):
    from porla_amd import challenge as ch
    num_blocks, write_step, kw = CHALLENGE_SHAPES[case]
    lv, seed = levels_for(num_blocks, **kw), seed_of(case)
    (info, lists), = _draw_on_device([(seed, write_step, num_blocks, lv)])
    assert (info, lists) == ch.audit_challenge_host(seed, write_step, num_blocks, lv)


def test_five_challenges_of_different_sizes_in_one_call():
    from porla_amd import challenge as ch
    reqs = [(seed_of(70 + i), ws, nb, levels_for(nb, mixed=True)) for i, (nb, ws) in
            enumerate([(2, 1), (1 << 15, (1 << 15) - 1), (64, 0), (256, 256 + 37), (1 << 12, 0xabc)])]
    got = _draw_on_device(reqs)
    assert got == [ch.audit_challenge_host(*r) for r in reqs]
    assert got[1][0]["n32"] > 0 and got[1][0]["n64"] > 0


@pytest.mark.parametrize("num_blocks,write_step", WALK_SHAPES)
def test_diag_walk_on_the_device_with_pinned_magnitudes(num_blocks, write_step):
    from porla_amd import challenge as ch
    lv = levels_for(num_blocks, mixed=True)
    ints = written_stream(num_blocks, write_step)
    got = ch.diag_audit_walk(ints, write_step, num_blocks, lv, on_device=True)
    assert got == model.challenge(ints, write_step, num_blocks, lv)
    assert got == ch.diag_audit_walk(ints, write_step, num_blocks, lv, on_device=False)


@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
def test_complement_scalars_on_the_device_equal_the_host_form(curve):
    from porla_amd import challenge as ch
    reqs = [(seed_of(40), 1, 2), (seed_of(41), (7 << 33) + 85, 256), (seed_of(43), (1 << 15) - 1, 1 << 15)]
    d = _guarded(32 * 3)
    ch.audit_complement_scalar_batch_device(KEY, reqs, curve, d.data_ptr())
    raw = _bytes(d)
    assert [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(3)] == ch.audit_complement_scalar_host(KEY, reqs, curve)
    assert raw[96:] == bytes([GUARD]) * 64


# ---------------------------------------------------------------- through the existing entry points (KZG)
class World:
    """SRS of NCOLS; one data store of STORE_ROWS encoded blocks with their MACs M_r, which every level's halves address directly
    (data_x = 0, data_y = 2^i: point `index` is row `index`); per file (num_blocks, write_step) an honest MAC store with one entry
    per (level, index), M'[off_i + index] = alpha M_index + PRF(i, index, write_step & ~(2^i - 1)) h, off_i = 2^(i+1) - 2, the
    client's complements in the same order, and a zero alignment store (fresh levels).  The PRF values are made on the device."""

    def __init__(self):
        import hashlib
        import torch
        from porla_amd import icc, multiexp as mx
        mx.init_key(TAU, ALPHA)
        mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
        rows = b"".join(hashlib.sha256(b"chal" + i.to_bytes(4, "little") + j.to_bytes(4, "little")).digest()
                        for i in range(STORE_ROWS) for j in range(NCOLS))
        rows_be = b"".join(rows[32 * k:32 * k + 32][::-1] for k in range(STORE_ROWS * NCOLS))
        macs_u = mx.kzg_commit_batch_host(rows_be, STORE_ROWS)
        self.x_rows = icc.crebuild_host(rows, STORE_ROWS, NCOLS, "bn254", 5, 0, want_aligned=False, want_scalars=False)[0]
        self.macs = icc.mac_crebuild_host(macs_u, STORE_ROWS, "bn254", 5, 0)
        self.d_rows64 = _dev(self.x_rows)
        rnd = random.Random(4321)
        pattern = b"".join(rnd.getrandbits(248).to_bytes(32, "little") for _ in range(31))       # 32-byte rows mod p_icc (> 2^248)
        self.d_rows32 = _dev(pattern * (STORE_ROWS * NCOLS // 31 + 1))
        self.files = {}
        torch.cuda.synchronize()

    def levels(self, num_blocks, mixed=False):
        return [(0, 1 << i, (2 << i) - 2, (2 << i) - 2 + (1 << i), 1 if mixed and i > 4 else 0) for i in range(num_blocks.bit_length())]

    def file(self, num_blocks, write_step):
        """(d_comp, d_mac_store, d_zero, complements as bytes) of one file"""
        import torch
        from porla_amd import challenge as ch, multiexp as mx
        if (num_blocks, write_step) not in self.files:
            height = num_blocks.bit_length()
            runs = [(i, 0, 2 << i, write_step & ~((1 << i) - 1), 0) for i in range(height)]
            n = sum(r[2] for r in runs)
            d_prf = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
            d_sc = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
            d_comp = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            ch.mac_prf_batch_device(KEY, runs, d_prf.data_ptr(), stream=st)
            d_sc[:, 16:] = d_prf.view(n, 16)            # compute_digest_complement's input: the 16 bytes, left-padded
            mx.kzg_complement_batch_device(d_sc.data_ptr(), n, d_comp.data_ptr(), stream=st)
            comp = _bytes(d_comp)
            rows = [index for i in range(height) for index in range(2 << i)]
            sc = (ALPHA32 + (1).to_bytes(32, "big")) * n
            pt = b"".join(self.macs[64 * r:64 * r + 64] + comp[64 * e:64 * e + 64] for e, r in enumerate(rows))
            store = b"".join(mx.msm_batch_host("bn254", sc, pt, mx.batch_offsets([2] * n)))
            self.files[(num_blocks, write_step)] = (d_comp, _dev(store), torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), comp)
            torch.cuda.synchronize()
        return self.files[(num_blocks, write_step)]


_WORLD = None


def world():
    global _WORLD
    if _WORLD is None:
        _WORLD = World()
    return _WORLD


def _upload_lists(lists):
    import numpy as np
    import torch
    out = {}
    for name in LISTS:
        a = np.array(lists[name], dtype=np.uint64 if "idx" in name else np.uint32)
        out[name] = torch.from_numpy(a.view(np.int64 if "idx" in name else np.int32).copy()).cuda() if len(a) else None
    return out


def _audit_tuple(W, num_blocks, write_step, info, ptr):
    """porla_kzg_audit_req of one file from a challenge's info and a function name -> device address of its list"""
    _, d_store, d_zero, _ = W.file(num_blocks, write_step)
    return (W.d_rows64.data_ptr() if info["n64"] else 0, ptr("idx64"), ptr("coef64"), info["n64"],
            W.d_rows32.data_ptr() if info["n32"] else 0, ptr("idx32"), ptr("coef32"), info["n32"],
            d_store.data_ptr(), d_zero.data_ptr(), ptr("mac_idx"), ptr("mac_coef"), info["n_macs"], info["random_point"])


def test_the_scalar_times_h_is_the_msm_over_the_challenged_complements():
    import torch
    from porla_amd import challenge as ch, multiexp as mx
    W = world()
    num_blocks, write_step, seed = 256, 85, seed_of(90)
    d_comp, _, _, comp = W.file(num_blocks, write_step)
    _, lists = ch.audit_challenge_host(seed, write_step, num_blocks, W.levels(num_blocks))
    n = len(lists["mac_idx"])
    d_pts = _dev(b"".join(comp[64 * e:64 * e + 64] for e in lists["mac_idx"]))
    d_coef = _dev(b"".join(c.to_bytes(32, "big") for c in lists["mac_coef"]))
    torch.cuda.synchronize()
    want = mx.msm_device("bn254", d_coef.data_ptr(), d_pts.data_ptr(), n)
    d_s = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ch.audit_complement_scalar_batch_device(KEY, [(seed, write_step, num_blocks)], "bn254", d_s.data_ptr(), stream=st)
    mx.kzg_complement_batch_device(d_s.data_ptr(), 1, d_p.data_ptr(), stream=st)
    assert _bytes(d_p) == want and want != bytes(64)


def test_audit_batch_records_from_device_drawn_lists_equal_uploaded_ones():
    W = world()
    files = [(64, 64 + 21, seed_of(91)), (256, 85, seed_of(92))]
    reqs = [(seed, ws, nb, W.levels(nb, mixed=True)) for nb, ws, seed in files]
    drawn = _draw_on_device(reqs)
    # the same call again, its lists kept on the device this time, the audit batch right behind it on the same stream
    import torch
    from porla_amd import challenge as ch
    bufs = [_list_tensors(info) for info, _ in drawn]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    infos = ch.audit_challenge_batch_device([r + ([t[name].data_ptr() for name in LISTS],) for r, (n, t) in zip(reqs, bufs)],
                                            stream=s.cuda_stream)
    audits = [_audit_tuple(W, nb, ws, info, lambda name, t=t: t[name].data_ptr()) for (nb, ws, _), info, (n, t) in zip(files, infos, bufs)]
    got = _records(server_records(audits, stream=s), 2)
    keep, audits = [], []
    for (nb, ws, seed), r in zip(files, reqs):
        info, lists = model.challenge(model.PrgInts(seed), ws, nb, r[3])
        up = _upload_lists(lists)
        keep.append(up)
        audits.append(_audit_tuple(W, nb, ws, info, lambda name, up=up: up[name].data_ptr() if up[name] is not None else 0))
    torch.cuda.synchronize()
    want = _records(server_records(audits), 2)
    assert got == want
    assert all(info["n64"] and info["n32"] for info in infos)
    assert got[0] != got[1] and got[0][:64] != bytes(64)


def test_the_seeded_client_check_through_the_unchanged_verifier():
    import torch
    from porla_amd import challenge as ch, multiexp as mx
    W = world()
    files = [(256, 85, seed_of(93)), (64, 64 + 21, seed_of(94)), (256, 85, seed_of(95))]
    k = len(files)
    reqs = [(seed, ws, nb, W.levels(nb)) for nb, ws, seed in files]
    infos = ch.audit_challenge_plan(reqs)
    bufs = [_list_tensors(info) for info in infos]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        d_s = torch.zeros(32 * k, dtype=torch.uint8, device="cuda")
        d_p = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
    st = s.cuda_stream
    # server: seed -> lists -> records; client: seed -> scalar -> ONE point; all on one stream, no host wait in between
    ch.audit_challenge_batch_device([r + ([t[name].data_ptr() if n[name] else 0 for name in LISTS],) for r, (n, t) in zip(reqs, bufs)], stream=st)
    audits = [_audit_tuple(W, nb, ws, info, lambda name, t=t, n=n: t[name].data_ptr() if n[name] else 0)
              for (nb, ws, _), info, (n, t) in zip(files, infos, bufs)]
    d_rec = server_records(audits, stream=s)
    ch.audit_complement_scalar_batch_device(KEY, [(seed, ws, nb) for nb, ws, seed in files], "bn254", d_s.data_ptr(), stream=st)
    mx.kzg_complement_batch_device(d_s.data_ptr(), k, d_p.data_ptr(), stream=st)
    with_store = [(W.file(nb, ws)[0].data_ptr(), t["mac_idx"].data_ptr(), t["mac_coef"].data_ptr(), info["n_macs"], ALPHA)
                  for (nb, ws, _), info, (n, t) in zip(files, infos, bufs)]
    with torch.cuda.stream(s):
        from_scalars, keep = ch.verify_reqs_from_scalars(d_p.data_ptr(), k, [ALPHA] * k)
    assert mx.kzg_verify_batch_device(with_store, d_rec.data_ptr(), stream=st) == [PASS] * k
    assert mx.kzg_verify_batch_device(from_scalars, d_rec.data_ptr(), stream=st) == [PASS] * k
    # one byte of combined_mac of reply 1 altered: FULL is lost both ways, the neighbours keep it
    recs = _records(d_rec, k)
    bad = bytearray(recs[1])
    bad[192 + 63] ^= 1
    d_bad = _dev(recs[0] + bytes(bad) + recs[2])
    torch.cuda.synchronize()
    for verifs in (with_store, from_scalars):
        got = mx.kzg_verify_batch_device(verifs, d_bad.data_ptr())
        assert got[0] == PASS and got[2] == PASS and not got[1] & FULL
    # and a reply checked against another audit's point fails
    swapped = [from_scalars[2], from_scalars[1], from_scalars[0]]
    got = mx.kzg_verify_batch_device(swapped, d_rec.data_ptr())
    assert got[1] == PASS and not got[0] & FULL and not got[2] & FULL


def test_the_seeded_client_check_ipa():
    """the honest store is made from the fixture's: M'[e] = macs_a[r] - comp_r + PRF_e h (macs_a[r] = alpha M_r + comp_r), the PRF
    values read as r.d[0], r.d[1]; a_value comes from the challenge's info"""
    import torch
    from porla_amd import challenge as ch, multiexp as mx
    from tests import common
    from tests import test_ipa_verify_batch_gpu as iv
    P = iv.pipe()
    hfb = mx.FixedBase("secp256k1", common.secp_bench_points(iv.NCOLS + 2)[64 * (iv.NCOLS + 1):], 1, iv.WINDOW)
    nb, height = 32, 6
    files = [(3 * nb + 21, seed_of(96)), (5 * nb + 31, seed_of(97))]
    k = len(files)
    levels = [(0, 1 << i, (2 << i) - 2, (2 << i) - 2 + (1 << i), 0) for i in range(height)]
    rows = [index for i in range(height) for index in range(2 << i)]
    n = len(rows)
    st = torch.cuda.current_stream().cuda_stream
    comps, stores, zeros = [], [], torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    for ws, _ in files:
        runs = [(i, 0, 2 << i, ws & ~((1 << i) - 1), 0) for i in range(height)]
        d_prf = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
        d_sc = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        d_comp = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
        ch.mac_prf_batch_device(KEY, runs, d_prf.data_ptr(), stream=st)
        d_sc[:, 16:] = torch.flip(d_prf.view(n, 16), dims=[1])          # r.d[0], r.d[1]: the 16 bytes as a little-endian integer
        hfb.commit_device(d_sc.data_ptr(), n, 1, d_comp.data_ptr(), stream=st)
        comp = _bytes(d_comp)
        sc = ((1).to_bytes(32, "big") + (iv.N - 1).to_bytes(32, "big") + (1).to_bytes(32, "big")) * n
        pt = b"".join(P.macs_a[64 * r:64 * r + 64] + P.comp_list[r] + comp[64 * e:64 * e + 64] for e, r in enumerate(rows))
        stores.append(_dev(b"".join(mx.msm_batch_host("secp256k1", sc, pt, mx.batch_offsets([3] * n)))))
        comps.append(d_comp)
    reqs = [(seed, ws, nb, levels) for ws, seed in files]
    infos = ch.audit_challenge_plan(reqs)
    assert [i["n_macs"] for i in infos] == [2 + 8 + 32 + 64, 2 + 4 + 8 + 16 + 32 + 64]
    bufs = [_list_tensors(info) for info in infos]
    d_s = torch.zeros(32 * k, dtype=torch.uint8, device="cuda")
    d_p = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ch.audit_challenge_batch_device([r + ([t[name].data_ptr() if m[name] else 0 for name in LISTS],)
                                            for r, (m, t) in zip(reqs, bufs)], stream=st) == infos
    audits = [(P.d_rows64.data_ptr(), t["idx64"].data_ptr(), t["coef64"].data_ptr(), info["n64"], 0, 0, 0, 0, store.data_ptr(),
               zeros.data_ptr(), t["mac_idx"].data_ptr(), t["mac_coef"].data_ptr(), info["n_macs"], info["a_value"])
              for info, (m, t), store in zip(infos, bufs, stores)]
    d_rec = iv.server_records(audits)
    ch.audit_complement_scalar_batch_device(KEY, [(seed, ws, nb) for ws, seed in files], "secp256k1", d_s.data_ptr(), stream=st)
    hfb.commit_device(d_s.data_ptr(), k, 1, d_p.data_ptr(), stream=st)
    with_store = [(d_comp.data_ptr(), t["mac_idx"].data_ptr(), t["mac_coef"].data_ptr(), info["n_macs"], ALPHA, info["a_value"])
                  for d_comp, info, (m, t) in zip(comps, infos, bufs)]
    from_scalars, keep = ch.verify_reqs_from_scalars(d_p.data_ptr(), k, [ALPHA] * k, a_values=[i["a_value"] for i in infos])
    torch.cuda.synchronize()
    assert P.fb.ipa_verify_batch_device(with_store, d_rec.data_ptr()) == [iv.BOUND] * k
    assert P.fb.ipa_verify_batch_device(from_scalars, d_rec.data_ptr()) == [iv.BOUND] * k
    recs = iv._records(d_rec, k)
    bad = bytearray(recs[1])
    bad[33 + 32] ^= 1                                                     # one byte of combined_MAC's x
    d_bad = _dev(recs[0] + bytes(bad))
    torch.cuda.synchronize()
    for verifs in (with_store, from_scalars):
        got = P.fb.ipa_verify_batch_device(verifs, d_bad.data_ptr())
        assert got[0] == iv.BOUND and not got[1] & iv.FULL
    hfb.close()

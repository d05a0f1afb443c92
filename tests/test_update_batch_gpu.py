"""GPU box: the batched server update (porla_kzg_update_batch_device / porla_ipa_update_batch_device) -- Server::update's H path for K
files in one asynchronous call on level stores resident in HBM -- bit-exact against the Python restatement tests/update_model.py (both
curves), against the composition of the host entry points it replaces, and as the input of the batched audit."""
import ctypes
import random

import pytest

from tests import common
from tests.update_model import FAMILIES, FileModel, pt_bytes, pt_tuple

pytestmark = pytest.mark.gpu
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")
NCOLS = 128
WINDOW = 11            # an explicit small table for the generators, as tests/test_ipa_audit_batch_gpu.py takes
SENTINEL = 0xA5
CURVES = ["bn254", "secp256k1"]


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


class Setup:
    """per curve: the commitment base as bytes (for the model), the call, some points to take MACs and complements from"""

    def __init__(self, curve):
        from porla_amd import icc, multiexp as mx
        self.curve = curve
        if curve == "bn254":
            mx.init_key(TAU, ALPHA)
            mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
            o = common.oracle()
            o.oracle_kzg_init_key(TAU, ctypes.c_size_t(len(TAU)), ALPHA, ctypes.c_size_t(len(ALPHA)))
            o.oracle_kzg_init_srs(ctypes.c_size_t(NCOLS), (1).to_bytes(32, "big"))
            raw = ctypes.create_string_buffer(64 * NCOLS)
            o.oracle_kzg_srs_g1_raw(raw)
            self.base = raw.raw
            self.fb = None
            pts = common.synth_points(40)
            self.call = lambda reqs, n_total, stream=0: icc.kzg_update_batch_device(reqs, n_total, stream)
        else:
            pts = common.secp_bench_points(NCOLS + 40)
            self.base = pts[:64 * NCOLS]
            self.fb = mx.FixedBase("secp256k1", self.base, NCOLS, WINDOW)
            pts = pts[64 * NCOLS:]
            self.call = lambda reqs, n_total, stream=0: self.fb.ipa_update_batch_device(reqs, n_total, stream)
        self.points = [pt_tuple(pts[64 * i:64 * i + 64]) for i in range(40)]


_SETUPS = {}


def setup_of(curve):
    if curve not in _SETUPS:
        _SETUPS[curve] = Setup(curve)
    return _SETUPS[curve]


class DevFile:
    """the six level families of a model on the device, one allocation per level"""

    def __init__(self, model):
        self.n_cols = model.n_cols
        self.t = {f: [_dev(b) for b in model.fam[f]] for f in FAMILIES}
        self.keep = []

    def req(self, chunks, mac, comps, write_step, level):
        block = _dev(b"".join(c.to_bytes(32, "little") for c in chunks))
        d_mac = _dev(pt_bytes(mac))
        d_comp = _dev(b"".join(pt_bytes(p) for p in comps)) if comps is not None else None
        self.keep += [block, d_mac, d_comp]
        return (block.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr() if d_comp is not None else 0, write_step, level) + \
            tuple([t.data_ptr() for t in self.t[f][:level + 1]] for f in FAMILIES)

    def bytes(self):
        return {f: [bytes(t.cpu().numpy()) for t in self.t[f]] for f in FAMILIES}


def assert_families_equal(got, want, what=""):
    for f in FAMILIES:
        for lv, (g, w) in enumerate(zip(got[f], want[f])):
            assert g == w, "%s %s level %d differs (first byte %d)" % (what, f, lv, next(i for i in range(len(g)) if g[i] != w[i]))


def random_write(rnd, S, level, complements):
    chunks = [rnd.getrandbits(256) for _ in range(NCOLS)]
    mac = rnd.choice(S.points)
    comps = [rnd.choice(S.points) for _ in range(2 << level)] if complements else None
    return chunks, mac, comps


def prepared_file(rnd, S, n_total, level, write_step):
    """a model whose levels below `level` are occupied (random rows < LCM and points, resident halves) and whose next write is
    `write_step` and lands on `level`; everything else holds the sentinel"""
    import icc_py
    m = FileModel(n_total, NCOLS, S.curve, S.base, fill=SENTINEL)
    lcm = icc_py.LCM[S.curve]
    for i in range(level):
        m.empty[i] = False
        for f in FAMILIES:
            r = m._row(f)
            for j in range(1 << i):
                if f.startswith("data"):
                    m.fam[f][i][j * r:(j + 1) * r] = b"".join(rnd.randrange(lcm).to_bytes(64, "little") for _ in range(NCOLS))
                else:
                    m.fam[f][i][j * r:(j + 1) * r] = pt_bytes(rnd.choice(S.points + [None]))
    m.write_step = write_step - 1
    assert m.next_level() == level
    return m


# ---- 1. one file, the 15 writes of a full cycle, one request per call, all on one stream with no host synchronisation in between
def run_cycle(curve, n_total, complements_on_odd, seed):
    import torch
    S = setup_of(curve)
    rnd = random.Random(seed)
    m = FileModel(n_total, NCOLS, curve, S.base, fill=SENTINEL)
    d = DevFile(m)
    stream = torch.cuda.Stream()
    snaps, want = {}, {}
    writes = []
    for step in range(1, n_total):
        level = (step & -step).bit_length() - 1                 # the ruler sequence a fresh log follows; the model confirms it below
        writes.append((step, level) + random_write(rnd, S, level, complements_on_odd and step % 2 == 1))
    with torch.cuda.stream(stream):
        reqs = [d.req(chunks, mac, comps, step, level) for step, level, chunks, mac, comps in writes]
        stream.synchronize()                                    # (the inputs are uploaded; from here on nothing waits on the host)
        for (step, level, chunks, mac, comps), req in zip(writes, reqs):
            S.call([req], n_total, stream.cuda_stream)
            if step in (5, 10):                                 # checkpoints: device-side copies in stream order
                snaps[step] = {f: [t.clone() for t in d.t[f]] for f in FAMILIES}
    for step, level, chunks, mac, comps in writes:
        assert m.update(chunks, mac, comps) == (step, level)
        if step in (5, 10):
            want[step] = m.family_bytes()
    stream.synchronize()
    for step in (5, 10):
        assert_families_equal({f: [bytes(t.cpu().numpy()) for t in snaps[step][f]] for f in FAMILIES}, want[step], "after write %d:" % step)
    assert_families_equal(d.bytes(), m.family_bytes(), "after the last write:")
    return S, m, d


@pytest.mark.parametrize("curve", CURVES)
def test_one_file_a_full_cycle_of_sequential_writes(curve):
    run_cycle(curve, 16, True, 11)


# ---- 2. mixed levels in one call, against the model and against the composition of the host entry points
def host_composition(S, m0, chunks, mac, comps, write_step, level, n_total):
    """the same write through porla_kzg_hadd_host / porla_icc_hadd_host, porla_icc_hrebuild_host, porla_icc_mac_hrebuild_host on host
    copies of the model's initial levels, the complements by host point adds"""
    import icc_py
    from porla_amd import icc
    data = b"".join(c.to_bytes(32, "little") for c in chunks)
    if S.curve == "bn254":
        b2, m2, ma = icc.kzg_hadd_host(data, pt_bytes(mac), n_total, write_step)
    else:
        b2, sc, _ = icc.hadd_host(data, n_total, write_step, S.curve)
        m2 = icc.mac_scale_host(pt_bytes(mac), n_total, write_step, S.curve)
        ma = S.fb.commit_host(sc, 1, NCOLS)
    new = {"data_x": b"".join(c.to_bytes(64, "little") for c in chunks),
           "data_y": b"".join(b2[32 * i:32 * i + 32] + bytes(32) for i in range(NCOLS)),
           "mac_x": pt_bytes(mac), "mac_y": m2, "align_x": bytes(64), "align_y": ma}
    out = {}
    for f in FAMILIES:
        r = m0._row(f)
        bufs = [ctypes.create_string_buffer(bytes(b), len(b)) for b in m0.fam[f][:level + 1]]
        slot = 1 if level else 0
        ctypes.memmove(ctypes.addressof(bufs[0]) + slot * r, new[f], r)
        if level:
            if f.startswith("data"):
                icc.hrebuild_host(bufs, level, n_total, S.curve, n_cols=NCOLS)
            else:
                icc.mac_hrebuild_host(bufs, level, n_total, S.curve)
        out[f] = [bytearray(b.raw) for b in bufs]
    if comps is not None:
        top = 1 << level
        for j in range(2 * top):
            buf, o = out["mac_x" if j < top else "mac_y"][level], 64 * (j % top)
            buf[o:o + 64] = pt_bytes(icc_py.ec_add(S.curve, pt_tuple(buf[o:o + 64]), comps[j]))
    return {f: [bytes(b) for b in out[f]] for f in FAMILIES}


@pytest.mark.parametrize("curve", CURVES)
def test_mixed_levels_in_one_call(curve):
    import copy
    import torch
    S = setup_of(curve)
    rnd = random.Random(22)
    n_total = 1024
    shapes = [(0, 2), (1, 1025 + 2), (1, 7), (3, 8 + 1024), (5, 32 * 5), (7, 128 * 3)]      # (level, write_step)
    models, devs, writes, reqs = [], [], [], []
    for a, (level, ws) in enumerate(shapes):
        m = prepared_file(rnd, S, n_total, level, ws)
        chunks, mac, comps = random_write(rnd, S, level, a != 2)
        if a == 1:
            mac = None                                           # an infinity MAC
        if a == 3:
            comps[0] = comps[5] = None                           # infinity complements
            comps[2] = pt_tuple(m.fam["mac_x"][0][0:64])         # (a complement may be any point)
        models.append(m); writes.append((chunks, mac, comps, ws, level))
        devs.append(DevFile(m))
        reqs.append(devs[-1].req(chunks, mac, comps, ws, level))
    initial = [copy.deepcopy(m) for m in models]
    torch.cuda.synchronize()
    S.call(reqs, n_total)
    torch.cuda.synchronize()
    for a, (m, d, (chunks, mac, comps, ws, level)) in enumerate(zip(models, devs, writes)):
        assert m.update(chunks, mac, comps) == (ws, level)
        got = d.bytes()
        assert_families_equal(got, m.family_bytes(), "file %d (level %d), model:" % (a, level))
        host = host_composition(S, initial[a], chunks, mac, comps, ws, level, n_total)
        for f in FAMILIES:
            r = m._row(f)
            for lv in range(level + 1):
                # the rows the reference writes (level 0's slot, incoming halves above it, the resident half of `level`)
                lo = (0 if level == 0 else 1) if lv == 0 else (0 if lv == level else (1 << lv))
                hi = (1 if level == 0 else 2) if lv == 0 else (2 << lv)
                assert got[f][lv][lo * r:hi * r] == host[f][lv][lo * r:hi * r], (a, f, lv)


# ---- 3. untouched rows, stated without the model
@pytest.mark.parametrize("curve", CURVES)
def test_rows_the_reference_does_not_write_stay_untouched(curve):
    import torch
    S = setup_of(curve)
    rnd = random.Random(33)
    n_total = 64
    files = [(0, 1), (2, 4), (3, 8)]
    models = [prepared_file(rnd, S, n_total, level, ws) for level, ws in files]
    devs = [DevFile(m) for m in models]
    before = [d.bytes() for d in devs]
    reqs = [d.req(*random_write(rnd, S, level, True), ws, level) for d, (level, ws) in zip(devs, files)]
    torch.cuda.synchronize()
    S.call(reqs, n_total)
    torch.cuda.synchronize()
    for (level, ws), m, d, b in zip(files, models, devs, before):
        got = d.bytes()
        for f in FAMILIES:
            r = m._row(f)
            for lv in range(m.height):
                g, w = got[f][lv], b[f][lv]
                if lv > level:
                    assert g == w, (level, f, lv)                                 # levels above the write: nothing
                elif lv == 0 and level == 0:
                    assert g[r:] == w[r:] and g[:r] != w[:r]                      # row 0 written, row 1 kept
                elif lv == 0:
                    assert g[:r] == w[:r] and g[r:] != w[r:]                      # the resident row kept, the incoming row written
                elif lv < level:
                    assert g[:(1 << lv) * r] == w[:(1 << lv) * r]                 # resident halves below `level` kept
                    assert g[(1 << lv) * r:] != w[(1 << lv) * r:]
                else:
                    assert SENTINEL.to_bytes(1, "little") * 64 != g[:64]          # level `level`: both halves written


# ---- 4. the identity of tests/test_update_batch_cpu.py on device state, the right-hand side through compute_digest
def test_mac_identity_on_device_state():
    import icc_py
    import torch
    from porla_amd import multiexp as mx
    from tests.update_model import row_vals
    S = setup_of("bn254")
    rnd = random.Random(44)
    n_total = 8
    m = FileModel(n_total, NCOLS, "bn254", S.base, fill=SENTINEL)
    d = DevFile(m)
    q = icc_py.Q["bn254"]
    alpha = ALPHA.rjust(32, b"\0")
    for step in range(1, n_total):
        level = m.next_level()
        chunks = [rnd.getrandbits(256) for _ in range(NCOLS)]
        mac = pt_tuple(mx.compute_digest(b"".join(c.to_bytes(32, "big") for c in chunks)))     # the block's MAC as the client makes it
        S.call([d.req(chunks, mac, None, step, level)], n_total)
        m.update(chunks, mac, None)
        torch.cuda.synchronize()
        got = d.bytes()
        for lv in range(m.height):
            if m.empty[lv]:
                continue
            for part in ("x", "y"):
                for r in range(1 << lv):
                    row = row_vals(got["data_" + part][lv][r * 64 * NCOLS:(r + 1) * 64 * NCOLS])
                    mac_r = got["mac_" + part][lv][64 * r:64 * r + 64]
                    al_r = got["align_" + part][lv][64 * r:64 * r + 64]
                    lhs = mx.bn254_add(mac_r, mx.bn254_mult(al_r, alpha))
                    rhs = mx.compute_digest(b"".join((v % q).to_bytes(32, "big") for v in row))   # alpha * Commit_srs(row mod r)
                    assert lhs == rhs, (step, lv, part, r)


# ---- 5. the launch sequence depends on the highest level, not on K
@pytest.mark.parametrize("curve", CURVES)
def test_launch_count_does_not_depend_on_k(curve):
    import torch
    from porla_amd import multiexp as mx
    S = setup_of(curve)
    rnd = random.Random(55)
    n_total, level = 256, 4

    def launches(k):
        models = [prepared_file(rnd, S, n_total, level if a == 0 else rnd.randrange(level + 1), 16 * (a + 1)) for a in range(k)]
        devs = [DevFile(m) for m in models]
        reqs = [dv.req(*random_write(rnd, S, m.next_level(), True), 16 * (a + 1), m.next_level()) for a, (m, dv) in enumerate(zip(models, devs))]
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        S.call(reqs, n_total)
        torch.cuda.synchronize()
        return sum(c for _, _, c in mx.profile_get()) - before

    launches(1)                                                  # (tables and workspaces built outside the count)
    mx.profile_enable(1)
    try:
        one, eight = launches(1), launches(8)
    finally:
        mx.profile_enable(0)
    assert one == eight and one >= 4 + 2 * level


# ---- 6. write, then audit: the stores the call leaves are what the batched audit consumes
def test_write_then_audit():
    import numpy as np
    import torch
    from porla_amd import multiexp as mx
    S, m, d = run_cycle("bn254", 16, True, 66)
    rnd = random.Random(66)
    lv = 3                                                       # after 15 writes every level 0 .. 3 is occupied; take the widest
    n = 1 << lv
    idx = torch.tensor([rnd.randrange(n) for _ in range(6)], dtype=torch.int64).cuda()
    coef = torch.tensor(np.array([rnd.getrandbits(31) for _ in range(6)], dtype=np.uint32).view(np.int32)).cuda()
    a = (d.t["data_x"][lv].data_ptr(), idx.data_ptr(), coef.data_ptr(), 6, 0, 0, 0, 0, d.t["mac_x"][lv].data_ptr(),
         d.t["align_x"][lv].data_ptr(), idx.data_ptr(), coef.data_ptr(), 6, 12345)
    one = mx.kzg_audit_device(*a)
    rec = one["commitment"] + one["proof_h"] + one["point"] + one["claim"] + one["combined_mac"] + \
        mx.bn254_add(one["combined_align"], one["align_value"])
    d_out = torch.zeros(320, dtype=torch.uint8, device="cuda")
    mx.kzg_audit_batch_device([a], d_out.data_ptr())
    torch.cuda.synchronize()
    assert bytes(d_out.cpu().numpy()) == rec
    assert mx.verify_proof(rec[0:64], rec[64:128], rec[128:160], rec[160:192])


def test_ipa_bad_bases_are_refused():
    from porla_amd import multiexp as mx
    S = setup_of("secp256k1")
    m = FileModel(16, NCOLS, "secp256k1", S.base, fill=SENTINEL)
    d = DevFile(m)
    req = d.req([1] * NCOLS, S.points[0], None, 1, 0)
    short = mx.FixedBase("secp256k1", S.base[:64 * 100], 100, WINDOW)
    with pytest.raises(RuntimeError, match="128"):
        short.ipa_update_batch_device([req], 16)
    bn = mx.FixedBase("bn254", common.synth_points(NCOLS), NCOLS, 8)
    with pytest.raises(RuntimeError, match="secp256k1"):
        bn.ipa_update_batch_device([req], 16)
    assert d.bytes() == m.family_bytes()                         # nothing was written

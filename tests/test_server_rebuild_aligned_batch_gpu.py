"""GPU box: the server's rebuild write in the CRebuild_No_Cached form (porla_kzg_server_rebuild_aligned_batch_device /
porla_ipa_server_rebuild_aligned_batch_device) -- top-level data rows mod p_icc in the 256-bit row format, an alignment commitment per
row -- bit-exact against the Python restatement tests/server_rebuild_aligned_model.py at n_total = 2, 8, 64 (both curves, 128 columns,
K = 3) and on edge files at n_total = 2, against the single-file entry points at 1 024 rows (two passes of the data network) and at
2^15 / 2^16 rows, with the rows the reference does not write and a guard region behind every buffer checked for the sentinel, the seam
between two groups of requests (PORLA_REBUILD_ROWS_MAX in a child process), the launch count, a whole KZG cycle through audit and
verify and a whole IPA cycle through the MAC relation on one stream, a second call on another stream while the first is in flight,
and the refusals that need a device (the IPA build's bad bases, the KZG build without an SRS).
The model's point network and its commitments are computed once per curve and size and shared by the tests that need them."""
import functools
import hashlib
import os
import random
import subprocess
import sys

import pytest

from tests import common
from tests.server_rebuild_aligned_model import AlignedRebuildFileModel, row32_vals
from tests.update_model import FAMILIES, pt_bytes, pt_tuple

pytestmark = pytest.mark.gpu
NCOLS = 128
SENTINEL = 0xA5
GUARD = 256                       # bytes behind every buffer that must keep the sentinel
CURVES = ["bn254", "secp256k1"]
STORES = ("u_blocks", "u_macs")


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy())


def server_of(curve, fresh=True):
    """the update batch test's setup (commitment base as bytes, the fixed base of the IPA build).  The library's key and SRS are process
    state and another test module may have installed its own since the setup was made: with `fresh`, which every test below asks for
    once before its first call, the KZG side goes in again (every init_SRS also draws a new hiding point)."""
    from porla_amd import multiexp as mx
    from tests import test_update_batch_gpu as ub
    S = ub.setup_of(curve)
    if curve == "bn254" and fresh:
        mx.init_key(ub.TAU, ub.ALPHA)
        mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
    return S


def call(curve, reqs, n_total, stream=0):
    from porla_amd import icc
    S = server_of(curve, fresh=False)
    if curve == "bn254":
        icc.kzg_server_rebuild_aligned_batch_device(reqs, n_total, stream)
    else:
        S.fb.ipa_server_rebuild_aligned_batch_device(reqs, n_total, stream)


class DevFile:
    """the top level of the six families (data rows: 32 bytes a symbol) and the two stores of one file on the device, each with GUARD
    bytes of sentinel behind it"""

    def __init__(self, n_total, u_blocks, u_macs):
        import torch
        self.n = n_total
        self.size = {f: 2 * n_total * (32 * NCOLS if f.startswith("data") else 64) for f in FAMILIES}
        self.t = {f: torch.full((self.size[f] + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for f in FAMILIES}
        for f, b in zip(STORES, (u_blocks, u_macs)):
            src = b if hasattr(b, "is_cuda") else _dev(b)
            self.size[f] = src.numel()
            self.t[f] = torch.cat([src, torch.full((GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")])
        self.keep = []

    def req(self, block, mac, comps, write_step, index):
        """block / mac / comps: bytes (or device tensors); comps None = NULL"""
        d = [x if x is None or hasattr(x, "is_cuda") else _dev(x) for x in (block, mac, comps)]
        self.keep += d
        return (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if d[2] is not None else 0, self.t["u_blocks"].data_ptr(),
                self.t["u_macs"].data_ptr()) + tuple(self.t[f].data_ptr() for f in FAMILIES) + (write_step, index)

    def bytes(self):
        return {f: _host(self.t[f][:self.size[f]]) for f in FAMILIES + STORES}

    def assert_untouched(self, what=""):
        """the incoming halves of the six buffers and the guard behind every buffer hold the sentinel"""
        import torch
        for f in FAMILIES + STORES:
            lo = self.size[f] // 2 if f in FAMILIES else self.size[f]
            assert bool(torch.all(self.t[f][lo:] == SENTINEL)), "%s %s: an untouched byte changed" % (what, f)


def block_bytes(chunks):
    return b"".join(c.to_bytes(32, "little") for c in chunks)


def aligned_model(curve, n_total, u_blocks=None, u_macs=None):
    m = AlignedRebuildFileModel(n_total, NCOLS, curve, server_of(curve, fresh=False).base, fill=SENTINEL)
    if u_blocks is not None:
        m.u_blocks[:], m.u_macs[:] = u_blocks, u_macs
    return m


# ---- 1. three requests in one call against the model: the write steps, block ids, infinities and cancelling complement of the cached
# call's test (tests/test_server_rebuild_batch_gpu.py: make_requests), on this form's model
def make_requests(curve, n_total, with_negative):
    from tests import test_server_rebuild_batch_gpu as sr
    return [(aligned_model(curve, n_total, m.u_blocks, m.u_macs),) + tuple(rest)
            for m, *rest in sr.make_requests(curve, n_total, with_negative)]


def run_on_device(curve, n_total, files, stream=0):
    """the call on copies of the models' state BEFORE the write; returns the DevFiles"""
    import torch
    devs, reqs = [], []
    for m, chunks, mac, comps, step, index in files:
        d = DevFile(n_total, bytes(m.u_blocks), bytes(m.u_macs))
        devs.append(d)
        reqs.append(d.req(block_bytes(chunks), pt_bytes(mac), None if comps is None else b"".join(pt_bytes(p) for p in comps), step, index))
    torch.cuda.synchronize()
    call(curve, reqs, n_total, stream)
    torch.cuda.synchronize()
    return devs


def assert_equals_model(d, m, what):
    got, want = d.bytes(), m.top_bytes()
    for f in FAMILIES + STORES:
        assert len(got[f]) == len(want[f]), "%s %s: %d bytes, the model has %d" % (what, f, len(got[f]), len(want[f]))
        assert got[f] == want[f], "%s %s differs (first byte %d)" % (what, f, next(i for i in range(len(want[f])) if got[f][i] != want[f][i]))


@functools.lru_cache(maxsize=None)
def model_case(curve, n_total):
    """(DevFiles after the call, the models after the same writes): computed once, shared by the tests below, left unchanged"""
    server_of(curve)
    files = make_requests(curve, n_total, True)
    devs = run_on_device(curve, n_total, files)
    for m, chunks, mac, comps, step, index in files:
        assert m.update(chunks, mac, comps, index=index, write_step=step) == (step, m.height - 1)
    return devs, [f[0] for f in files]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_total", [2, 8, 64])
def test_three_requests_equal_the_model(curve, n_total):
    devs, models = model_case(curve, n_total)
    for a, (d, m) in enumerate(zip(devs, models)):
        assert_equals_model(d, m, "n_total %d, request %d:" % (n_total, a))
    top = models[0].height - 1
    assert pt_tuple(models[0].fam["mac_x"][top][64:128]) is None           # the complement that cancels its target
    assert any(pt_tuple(models[1].fam["align_y"][top][64 * j:64 * j + 64]) is not None for j in range(n_total))


# ---- 2. edge files at n_total = 2 (one pass that is first and last), three requests in one call
def edge_files(curve):
    import icc_py
    rnd = random.Random(2200)
    p_icc = icc_py.P_ICC
    pts = [pt_tuple(common.synth_points(4)[64 * i:64 * i + 64]) for i in range(4)] if curve == "bn254" else \
        [pt_tuple(common.secp_bench_points(4)[64 * i:64 * i + 64]) for i in range(4)]
    # a: block 1 >= block 2 in every column, both below 2^200, wt = 1: no sum or difference leaves [0, p_icc), every c is 0
    hi = [(1 << 199) | rnd.getrandbits(199) for _ in range(NCOLS)]
    lo = [rnd.getrandbits(199) for _ in range(NCOLS)]
    # b: the extreme chunk values mixed over the columns, in both blocks, wt != 1
    ext = [(1 << 256) - 1, p_icc, p_icc - 1, 0]
    b0 = [ext[c % 4] for c in range(NCOLS)]
    b1 = [ext[(c // 4) % 4] for c in range(NCOLS)]
    # c: two equal blocks: X row 1 = block 1 - block 2 = 0
    eq = [rnd.getrandbits(256) for _ in range(NCOLS)]
    files = []
    for rows, step, index in (((hi, lo), 2, 1), ((b0, b1), 3, 2), ((eq, eq), 4, 2)):
        m = aligned_model(curve, 2)
        for i in (1, 2):
            m.store(i, rows[i - 1] if i != index else [0] * NCOLS, pts[i])
        files.append((m, rows[index - 1], pts[0], None, step, index))
    return files


@pytest.mark.parametrize("curve", CURVES)
def test_edge_files_at_two_rows(curve):
    import icc_py
    server_of(curve)
    files = edge_files(curve)
    devs = run_on_device(curve, 2, files)
    for m, chunks, mac, comps, step, index in files:
        assert m.update(chunks, mac, comps, index=index, write_step=step) == (step, 1)
    for a, (d, f) in enumerate(zip(devs, files)):
        assert_equals_model(d, f[0], "edge file %d:" % a)
        d.assert_untouched("edge file %d:" % a)
    ma, mb, mc = (f[0] for f in files)
    assert all(c == 0 for part in ma.scalars.values() for row in part for c in row)
    assert bytes(ma.fam["align_x"][1][:128]) == bytes(128) and bytes(ma.fam["align_y"][1][:128]) == bytes(128)
    assert _host(devs[0].t["align_x"][:128]) == bytes(128) and _host(devs[0].t["align_y"][:128]) == bytes(128)
    assert any(c for row in mb.scalars["x"] for c in row) and any(c for row in mb.scalars["y"] for c in row)
    row1 = row32_vals(bytes(mc.fam["data_x"][1][32 * NCOLS:64 * NCOLS]))
    assert row1 == [0] * NCOLS and bytes(mc.fam["align_x"][1][64:128]) == bytes(64)
    assert all(v < icc_py.P_ICC for f in files for v in row32_vals(bytes(f[0].fam["data_y"][1][:64 * NCOLS])))


# ---- 3. the rows the reference does not write and the guards
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_total", [2, 8])
def test_untouched_rows_and_guards_keep_the_sentinel(curve, n_total):
    devs, models = model_case(curve, n_total)
    for a, d in enumerate(devs):
        d.assert_untouched("n_total %d, request %d:" % (n_total, a))
        assert d.size["data_x"] == d.size["data_y"] == 2 * n_total * NCOLS * 32      # the data rows end here: the guard starts behind
        got = d.bytes()
        for f in FAMILIES:                                                  # ... and the resident halves were all written
            half = d.size[f] // 2
            assert got[f][half:] == bytes([SENTINEL]) * half
            row = half // n_total
            assert all(got[f][j * row:(j + 1) * row] != bytes([SENTINEL]) * row for j in range(n_total)), f


# ---- 4. / 5. against the single-file entry points: 1 024 rows (a first pass that is not last, a last pass that is not first), 2^15 and
# 2^16.  All on the device: the stores after the write, the single-file calls on them, the complements by host point additions (every
# point at 1 024 rows, 16 sampled points per part at the large sizes)
def single_file_case(curve, n_total, seed, k, add_all):
    import torch
    import icc_py
    from porla_amd import icc
    from tests import test_server_rebuild_batch_gpu as sr
    S = server_of(curve)
    rnd = random.Random(seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    pts = sr.points_of(curve)
    table = _dev(b"".join(pt_bytes(p) for p in pts + [None])).view(41, 64)
    steps = (2 * n_total + 5, 7 * n_total)
    devs, reqs, writes = [], [], []
    for a in range(k):
        u = torch.randint(0, 256, (n_total * NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen)
        pick = torch.randint(0, 41, (n_total,), device="cuda", generator=gen)
        macs = table[pick].reshape(-1).contiguous()
        d = DevFile(n_total, u.clone(), macs.clone())
        block = torch.randint(0, 256, (NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen)
        mac = _dev(pt_bytes(rnd.choice(pts)))
        comps = None
        if a == 0:
            comps = table[torch.randint(0, 41, (2 * n_total,), device="cuda", generator=gen)].reshape(-1).contiguous()
        index = (n_total, 1)[a]
        devs.append(d)
        reqs.append(d.req(block, mac, comps, steps[a], index))
        writes.append((u, macs, block, mac, comps, index))
    torch.cuda.synchronize()
    call(curve, reqs, n_total)
    torch.cuda.synchronize()
    for a, (d, (u, macs, block, mac, comps, index)) in enumerate(zip(devs, writes)):
        what = "n_total %d, request %d:" % (n_total, a)
        u[(index - 1) * NCOLS * 32:index * NCOLS * 32] = block
        macs[(index - 1) * 64:index * 64] = mac
        assert torch.equal(d.t["u_blocks"][:u.numel()], u) and torch.equal(d.t["u_macs"][:macs.numel()], macs), what + " the stores"
        half = n_total * NCOLS * 32
        new = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
        ax, ay, sc, cm, mx_, my_ = new(half), new(half), new(2 * half), new(128 * n_total), new(64 * n_total), new(64 * n_total)
        if curve == "bn254":
            icc.kzg_crebuild_stage_device(u.data_ptr(), n_total, steps[a], ax.data_ptr(), ay.data_ptr(), sc.data_ptr(), cm.data_ptr(),
                                          macs.data_ptr(), mx_.data_ptr(), my_.data_ptr())
        else:
            icc.crebuild_xy_device(u.data_ptr(), n_total, NCOLS, curve, steps[a], d_aligned=ax.data_ptr(), d_scalars=sc.data_ptr(),
                                   d_y_aligned=ay.data_ptr(), d_y_scalars=sc.data_ptr() + half)
            S.fb.commit_device(sc.data_ptr(), 2 * n_total, NCOLS, cm.data_ptr())
            icc.mac_crebuild_xy_device(macs.data_ptr(), n_total, curve, steps[a], mx_.data_ptr(), my_.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(d.t["data_x"][:half], ax), what + " data X"
        assert torch.equal(d.t["data_y"][:half], ay), what + " data Y"
        assert torch.equal(d.t["align_x"][:64 * n_total], cm[:64 * n_total]), what + " align X"
        assert torch.equal(d.t["align_y"][:64 * n_total], cm[64 * n_total:]), what + " align Y"
        assert bool(cm.any())
        if comps is None:
            assert torch.equal(d.t["mac_x"][:64 * n_total], mx_) and torch.equal(d.t["mac_y"][:64 * n_total], my_), what + " MACs"
        else:
            sample = range(n_total) if add_all else sorted({0, 1, n_total - 1} | set(rnd.sample(range(2, n_total - 1), 13)))
            hc = _host(comps)
            for part, enc, f in ((0, _host(mx_), "mac_x"), (1, _host(my_), "mac_y")):
                got = _host(d.t[f][:64 * n_total])
                for j in sample:
                    want = icc_py.ec_add(curve, pt_tuple(enc[64 * j:64 * j + 64]), pt_tuple(hc[64 * (part * n_total + j):64 * (part * n_total + j) + 64]))
                    assert got[64 * j:64 * j + 64] == pt_bytes(want), what + " %s[%d]" % (f, j)
        d.assert_untouched(what)


@pytest.mark.parametrize("curve", CURVES)
def test_1024_rows_equal_the_single_file_entry_points(curve):
    single_file_case(curve, 1024, 6100, 2, True)


@pytest.mark.parametrize("curve,n_total", [("bn254", 1 << 15), ("secp256k1", 1 << 16)])
def test_the_protocol_size_and_the_cap_equal_the_single_file_entry_points(curve, n_total):
    single_file_case(curve, n_total, 6200, 1, False)


# ---- 6. the seam between groups: PORLA_REBUILD_ROWS_MAX=128 puts each of the three requests at n_total = 64 (128 rows of scalars
# each) into a group of its own; the bytes are those of the one group the parent process runs
def digest_of(curve, n_total):
    """(sha256 over every buffer of the three requests of make_requests (without the model's negative) after the call, the launches)"""
    from porla_amd import multiexp as mx
    server_of(curve)
    files = make_requests(curve, n_total, False)
    run_on_device(curve, n_total, files)                                   # (tables and workspaces built outside the count)
    mx.profile_enable(1)
    try:
        before = sum(c for _, _, c in mx.profile_get())
        devs = run_on_device(curve, n_total, files)
        launches = sum(c for _, _, c in mx.profile_get()) - before
    finally:
        mx.profile_enable(0)
    h = hashlib.sha256()
    for d in devs:
        got = d.bytes()
        for f in FAMILIES + STORES:
            h.update(got[f])
    return h.hexdigest(), launches


def test_the_seam_between_groups_gives_the_same_bytes():
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
           "from tests import test_server_rebuild_aligned_batch_gpu as t\n" \
           "a, b = t.digest_of('bn254', 64), t.digest_of('secp256k1', 64)\n" \
           "print('digests', a[0], a[1], b[0], b[1])\n" % (common.ROOT, os.path.join(common.ROOT, "oracle"))
    env = dict(os.environ, PORLA_REBUILD_ROWS_MAX="128")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=common.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("digests ")][-1].split()
    for curve, (digest, launches) in zip(CURVES, ((line[1], int(line[2])), (line[3], int(line[4])))):
        want, one_group = digest_of(curve, 64)
        assert digest == want, curve
        # two more groups: two more times the last data pass, the commitment pass with its fold, and the close
        assert launches == one_group + 2 * 4, (curve, launches, one_group)


# ---- 7. the launch sequence depends on n_total (and the number of groups), not on K
def test_launch_count_does_not_depend_on_k():
    import torch
    from porla_amd import multiexp as mx
    from tests import test_server_rebuild_batch_gpu as sr
    n_total = 256
    server_of("bn254")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(61)
    table = _dev(b"".join(pt_bytes(p) for p in sr.points_of("bn254"))).view(40, 64)

    def launches(k):
        devs, reqs = [], []
        for a in range(k):
            u = torch.randint(0, 256, (n_total * NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen)
            macs = table[torch.randint(0, 40, (n_total,), device="cuda", generator=gen)].reshape(-1).contiguous()
            comps = table[torch.randint(0, 40, (2 * n_total,), device="cuda", generator=gen)].reshape(-1).contiguous()
            d = DevFile(n_total, u, macs)
            devs.append(d)
            reqs.append(d.req(u[:NCOLS * 32].clone(), macs[:64].clone(), comps if a % 2 == 0 else None, n_total * (a + 1) + a % 3, 1 + a))
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        call("bn254", reqs, n_total)
        torch.cuda.synchronize()
        return sum(c for _, _, c in mx.profile_get()) - before

    launches(8)                                                  # (tables and workspaces built outside the count)
    mx.profile_enable(1)
    try:
        one, eight = launches(1), launches(8)
    finally:
        mx.profile_enable(0)
    # the store, one data pass, the MAC load, eight stages, the Y scaling, one commitment pass and the close
    assert one == eight and one >= 1 + 1 + 1 + 8 + 1 + 1 + 1


# ---- 8. / 9. a whole cycle of a file of 8 blocks on one non-default stream with nothing in between: writes 1 .. 7 through the update
# batch, write 8 through the client's rebuild call and then this call, which reads the client's output buffers.  Every MAC is the
# client's, alpha Commit(block) + s h with the PRF values write 8 names as complements_U, so the top level carries the MAC relation.
class Cycle:
    def __init__(self, curve, seed):
        import icc_py
        import torch
        from porla_amd import multiexp as mx
        from tests import test_client_rebuild_batch_gpu as cr, test_update_batch_gpu as ub
        from tests.client_rebuild_model import n_prf, rebuild_points
        n = self.n = 8
        self.curve = curve
        self.S, self.client_call = cr.setup_of(curve)             # (the caller has asked for a fresh server_of(curve))
        S = self.S
        if curve == "bn254":                                      # every init_SRS draws a new hiding point: h as the library holds it now
            self.h = pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))
        else:
            self.h = S.h
        rnd = random.Random(seed)
        self.m = m = aligned_model(curve, n)
        self.d = ub.DevFile(m)                                    # every level of the six families, as the update batch takes them
        row = 32 * NCOLS
        self.d_u = torch.full((n * row + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.d_um = torch.full((n * 64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        s = [rnd.getrandbits(128) for _ in range(n)]              # the PRF value behind block i's MAC
        self.writes = []
        for step in range(1, n):
            level = (step & -step).bit_length() - 1
            chunks = [rnd.getrandbits(256) for _ in range(NCOLS)]
            mac = icc_py.ec_add(curve, S.block_commit(chunks), icc_py.ec_mul(curve, self.h, s[step - 1]))
            comps = [rnd.choice(S.server.points) for _ in range(2 << level)] if step % 2 else None
            self.writes.append((step, level, chunks, mac, comps))
        self.last_chunks = [rnd.getrandbits(256) for _ in range(NCOLS)]
        self.new = [rnd.getrandbits(128) for _ in range(2 * n)]   # the complements of the top level after the write, X then Y
        self.prf = [s[n - 1]] + s + self.new
        assert len(self.prf) == n_prf(n)
        self.d_block = _dev(block_bytes(self.last_chunks))
        self.d_prf = _dev(b"".join(cr.raw_of(curve, v) for v in self.prf))
        self.d_mac = torch.full((64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.d_comp = torch.full((128 * n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.reqs = [self.d.req(chunks, mac, comps, step, level) for step, level, chunks, mac, comps in self.writes]
        self.up = {step: (_dev(block_bytes(chunks)), _dev(pt_bytes(mac))) for step, level, chunks, mac, comps in self.writes}
        self.mac8, self.out8 = rebuild_points(curve, n, n, self.prf, self.h, S.block_commit(self.last_chunks))

    def enqueue_writes(self, stream):
        """writes 1 .. 7 and the client's half of write 8 on `stream`; returns this file's request of the server's rebuild call"""
        n, row, top = self.n, 32 * NCOLS, self.m.height - 1
        for (step, level, chunks, mac, comps), req in zip(self.writes, self.reqs):
            self.d_u[(step - 1) * row:step * row].copy_(self.up[step][0], non_blocking=True)      # U and MAC_U as Server::update keeps them
            self.d_um[(step - 1) * 64:step * 64].copy_(self.up[step][1], non_blocking=True)
            self.S.server.call([req], n, stream.cuda_stream)
        self.client_call([(self.d_block.data_ptr(), self.d_prf.data_ptr(), self.d_mac.data_ptr(), self.d_comp.data_ptr(), n)], n, stream.cuda_stream)
        return (self.d_block.data_ptr(), self.d_mac.data_ptr(), self.d_comp.data_ptr(), self.d_u.data_ptr(), self.d_um.data_ptr()) + \
            tuple(self.d.t[f][top].data_ptr() for f in FAMILIES) + (n, n)

    def assert_equals_model(self):
        """after the stream has drained: every level and both stores against the model after the same eight writes"""
        m, n, top = self.m, self.n, self.m.height - 1
        for step, level, chunks, mac, comps in self.writes:
            assert m.update(chunks, mac, comps, index=step) == (step, level)
        assert m.update(self.last_chunks, self.mac8, self.out8, index=n) == (n, top)
        assert _host(self.d_mac[:64]) == pt_bytes(self.mac8)
        got = self.d.bytes()
        for f in FAMILIES:
            assert got[f][top] == bytes(m.fam[f][top]), "%s of the top level differs" % f
            for lv in range(top):
                assert got[f][lv] == bytes(m.fam[f][lv]), "%s level %d was touched" % (f, lv)
        assert _host(self.d_u) == bytes(m.u_blocks) + bytes([SENTINEL]) * GUARD and _host(self.d_um) == bytes(m.u_macs) + bytes([SENTINEL]) * GUARD


def test_a_whole_kzg_cycle_through_audit_and_verify():
    import numpy as np
    import torch
    from porla_amd import multiexp as mx
    from tests import test_update_batch_gpu as ub
    server_of("bn254")
    good, bad = Cycle("bn254", 81), Cycle("bn254", 81)            # the same file twice, in buffers of their own
    n, top = good.n, good.m.height - 1
    idx = torch.tensor(list(range(n)), dtype=torch.int64).cuda()
    coef = torch.tensor(np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32).view(np.int32)).cuda()
    comp_store = _dev(b"".join(mx.compute_digest_complement(v.to_bytes(16, "big")) for v in good.new[:n]))
    d_rec = torch.zeros(320 * 2, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()                                      # (the inputs are uploaded; from here on nothing waits on the host)
    with torch.cuda.stream(stream):
        reqs = [good.enqueue_writes(stream), bad.enqueue_writes(stream)]
        call("bn254", reqs, n, stream.cuda_stream)
        bad.d.t["align_x"][top][64 * 5:64 * 6].zero_()            # one top-level alignment point of the second file lost
        audits = [(0, 0, 0, 0, f.d.t["data_x"][top].data_ptr(), idx.data_ptr(), coef.data_ptr(), n, f.d.t["mac_x"][top].data_ptr(),
                   f.d.t["align_x"][top].data_ptr(), idx.data_ptr(), coef.data_ptr(), n, 777 + a) for a, f in enumerate((good, bad))]
        mx.kzg_audit_batch_device(audits, d_rec.data_ptr(), stream=stream.cuda_stream)
        status = mx.kzg_verify_batch_device([(comp_store.data_ptr(), idx.data_ptr(), coef.data_ptr(), n, ub.ALPHA)] * 2, d_rec.data_ptr(),
                                            stream=stream.cuda_stream)
    assert status[0] == mx.KZG_VERIFY_FULL | mx.KZG_VERIFY_PROOF
    assert status[1] == mx.KZG_VERIFY_PROOF                       # the alignments carry the MAC relation: FULL is lost, the opening holds
    stream.synchronize()
    good.assert_equals_model()
    assert any(bytes(good.m.fam["align_x"][top][64 * j:64 * j + 64]) != bytes(64) for j in range(n))


def test_a_whole_ipa_cycle_keeps_the_mac_relation():
    import icc_py
    import torch
    c = "secp256k1"
    server_of(c)
    f = Cycle(c, 82)
    n, top, S = f.n, f.m.height - 1, f.S
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        call(c, [f.enqueue_writes(stream)], n, stream.cuda_stream)
    stream.synchronize()
    f.assert_equals_model()
    # mac + alpha * align == alpha * Commit(row mod q) + s_new * h for every resident row of the top level, X and Y
    got = f.d.bytes()
    for part, new in (("x", f.new[:n]), ("y", f.new[n:])):
        for r in range(n):
            row = row32_vals(got["data_" + part][top][r * 32 * NCOLS:(r + 1) * 32 * NCOLS])
            mac_r = pt_tuple(got["mac_" + part][top][64 * r:64 * r + 64])
            al_r = pt_tuple(got["align_" + part][top][64 * r:64 * r + 64])
            lhs = icc_py.ec_add(c, mac_r, icc_py.ec_mul(c, al_r, S.alpha))
            rhs = icc_py.ec_add(c, icc_py.ec_mul(c, S.commit([v % S.q for v in row]), S.alpha), icc_py.ec_mul(c, f.h, new[r]))
            assert lhs == rhs, (part, r)


# ---- 10. the scaffold: a larger call on another stream while the first is in flight (tests/test_batch_scaffold_gpu.py drives the
# other batched calls the same way); both calls share one workspace, the second's buffers are larger
@pytest.mark.parametrize("curve", CURVES)
def test_a_larger_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    from tests import test_server_rebuild_batch_gpu as sr
    rnd = random.Random(1010)
    pts = sr.points_of(curve)
    server_of(curve)

    def make(k, n_total):
        files = []
        for a in range(k):
            m = aligned_model(curve, n_total)
            for i in range(1, n_total + 1):
                m.store(i, [rnd.getrandbits(256) for _ in range(NCOLS)], rnd.choice(pts))
            comps = [rnd.choice(pts) for _ in range(2 * n_total)] if a % 2 else None
            files.append((m, [rnd.getrandbits(256) for _ in range(NCOLS)], rnd.choice(pts), comps, n_total + a, 1 + a % n_total))
        devs, reqs = [], []
        for m, chunks, mac, comps, step, index in files:
            d = DevFile(n_total, bytes(m.u_blocks), bytes(m.u_macs))
            devs.append(d)
            reqs.append(d.req(block_bytes(chunks), pt_bytes(mac), None if comps is None else b"".join(pt_bytes(p) for p in comps), step, index))
        return files, devs, reqs

    a, b = make(2, 4), make(5, 8)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ballast = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            ballast.normal_()                       # a few milliseconds ahead of A on its stream: A is in flight when B comes
    call(curve, a[2], 4, s1.cuda_stream)
    call(curve, b[2], 8, s2.cuda_stream)
    torch.cuda.synchronize()
    for name, (files, devs, reqs) in (("first", a), ("second", b)):
        for i, (d, (m, chunks, mac, comps, step, index)) in enumerate(zip(devs, files)):
            assert m.update(chunks, mac, comps, index=index, write_step=step) == (step, m.height - 1)
            assert_equals_model(d, m, "%s call, request %d:" % (name, i))
            d.assert_untouched("%s call, request %d:" % (name, i))


# ---- 11. the refusals that need a device: the IPA build's bad bases (a handle exists only where a device does), and the KZG build
# before any SRS is loaded
def test_ipa_bad_bases_are_refused():
    import torch
    from porla_amd import multiexp as mx
    from tests import test_update_batch_gpu as ub
    S = server_of("secp256k1")
    m = aligned_model("secp256k1", 4)
    d = DevFile(4, bytes(m.u_blocks), bytes(m.u_macs))
    req = d.req(block_bytes([1] * NCOLS), pt_bytes(S.points[0]), None, 4, 1)
    torch.cuda.synchronize()
    short = mx.FixedBase("secp256k1", S.base[:64 * 100], 100, ub.WINDOW)
    with pytest.raises(RuntimeError, match="porla_ipa_server_rebuild_aligned_batch_device.*128"):
        short.ipa_server_rebuild_aligned_batch_device([req], 4)
    bn = mx.FixedBase("bn254", common.synth_points(NCOLS), NCOLS, 8)
    with pytest.raises(RuntimeError, match="porla_ipa_server_rebuild_aligned_batch_device.*secp256k1"):
        bn.ipa_server_rebuild_aligned_batch_device([req], 4)
    torch.cuda.synchronize()
    got = d.bytes()
    assert all(got[f] == bytes([SENTINEL]) * len(got[f]) for f in FAMILIES)        # nothing was written
    assert got["u_blocks"] == bytes(m.u_blocks) and got["u_macs"] == bytes(m.u_macs)


def test_kzg_without_an_srs_is_a_state_error():
    """in a child process that has loaded no SRS: PORLA_ERR_STATE, before any pointer of the request is read (they are fake)"""
    code = "import sys; sys.path.insert(0, %r)\n" \
           "from porla_amd import lib, icc\n" \
           "req = tuple(0x10000 + 0x100 * (i + 1) for i in range(11)) + (16, 1)\n" \
           "print('rc', lib.porla_kzg_server_rebuild_aligned_batch_device(icc.server_rebuild_requests([req]), 1, 16, None))\n" \
           "print('msg', lib.porla_gpu_last_error().decode())\n" % common.ROOT
    r = subprocess.run([sys.executable, "-c", code], cwd=common.ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = dict(ln.split(" ", 1) for ln in r.stdout.splitlines() if ln.startswith(("rc ", "msg ")))
    assert lines["rc"] == "-4" and "SRS" in lines["msg"], r.stdout

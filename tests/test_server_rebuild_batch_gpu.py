"""GPU box: the server's rebuild write (porla_server_rebuild_batch_device) -- the step of Server::update that calls CRebuild, for K files
in one asynchronous call on stores resident in HBM -- bit-exact against the Python restatement tests/server_rebuild_model.py at
n_total = 2, 8, 64 (both curves, 128 columns, K = 3), against the single-file entry points at 1 024 rows (two passes of the data
network) and at 2^15 / 2^16 rows (the protocol's size, the cap), with the rows the reference does not write and a guard region behind
every buffer checked for the sentinel, the launch count, a whole cycle behind the client's rebuild call on one stream, and
PORLA_MAC_QUAD_MAX=0 in a child process.
The point network of the model costs about 400 scalar multiplications in Python per request at n_total = 64: that case is computed
once per curve and takes a few seconds, the others well under one."""
import functools
import hashlib
import os
import random
import subprocess
import sys

import pytest

from tests import common
from tests.server_rebuild_model import RebuildFileModel
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


@functools.lru_cache(maxsize=None)
def points_of(curve):
    pts = common.synth_points(40) if curve == "bn254" else common.secp_bench_points(40)
    return [pt_tuple(pts[64 * i:64 * i + 64]) for i in range(40)]


def call(reqs, n_total, curve, stream=0, n_cols=NCOLS):
    from porla_amd import icc
    icc.server_rebuild_batch_device(reqs, n_total, n_cols, curve, stream)


class DevFile:
    """the top level of the six families and the two stores of one file on the device, each with GUARD bytes of sentinel behind it"""

    def __init__(self, n_total, u_blocks, u_macs, n_cols=NCOLS):
        import torch
        self.n, self.n_cols = n_total, n_cols
        self.size = {f: 2 * n_total * (64 * n_cols if f.startswith("data") else 64) for f in FAMILIES}
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


# ---- 1. three requests in one call against the model
def make_requests(curve, n_total, with_negative):
    """three files with random stores and their writes: write_steps 3 n (wt = 1), n + 1 and 5 n + (n / 2 | 1); block ids 1, n and one
    in between; request 1 without complements; infinity among the MAC_U entries, the MACs and the complements; with_negative (needs
    the model's network): request 0's complement 1 is the negative of its target, so that sum is infinity"""
    import icc_py
    rnd = random.Random(4000 + n_total)
    pts = points_of(curve)
    steps = (3 * n_total, n_total + 1, 5 * n_total + (n_total // 2 | 1))
    assert [s % n_total == 0 for s in steps] == [True, False, False]
    indexes = (1, n_total, max(1, n_total // 2))
    files = []
    for a in range(3):
        m = RebuildFileModel(n_total, NCOLS, curve, b"", fill=SENTINEL)
        for i in range(1, n_total + 1):
            m.store(i, [rnd.getrandbits(256) for _ in range(NCOLS)], None if (i + a) % 5 == 2 else rnd.choice(pts))
        chunks = [rnd.getrandbits(256) for _ in range(NCOLS)]
        mac = None if a == 2 else rnd.choice(pts)
        comps = None if a == 1 else [None if j % 7 == 3 else rnd.choice(pts) for j in range(2 * n_total)]
        if a == 0 and with_negative:
            m.store(indexes[a], chunks, mac)
            comps[1] = icc_py.ec_neg(curve, m.mac_network(steps[a])[0][1])
        files.append((m, chunks, mac, comps, steps[a], indexes[a]))
    return files


def run_on_device(curve, n_total, files):
    """the call on copies of the models' state BEFORE the write; returns the DevFiles"""
    import torch
    devs, reqs = [], []
    for m, chunks, mac, comps, step, index in files:
        d = DevFile(n_total, bytes(m.u_blocks), bytes(m.u_macs))
        devs.append(d)
        reqs.append(d.req(block_bytes(chunks), pt_bytes(mac), None if comps is None else b"".join(pt_bytes(p) for p in comps), step, index))
    torch.cuda.synchronize()
    call(reqs, n_total, curve)
    torch.cuda.synchronize()
    return devs


@functools.lru_cache(maxsize=None)
def model_case(curve, n_total):
    """(DevFiles after the call, the models after the same writes): computed once, shared by the tests below, left unchanged.
    (Request 0's model holds its own row already, for the negative: requests 1 and 2 show that the call stores the block.)"""
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
        got, want = d.bytes(), m.top_bytes()
        for f in FAMILIES + STORES:
            assert got[f] == want[f], "n_total %d, request %d: %s differs (first byte %d)" % (
                n_total, a, f, next(i for i in range(len(want[f])) if got[f][i] != want[f][i]))
    top = models[0].height - 1
    assert pt_tuple(models[0].fam["mac_x"][top][64:128]) is None           # the complement that cancels its target
    assert any(pt_tuple(models[1].u_macs[64 * i:64 * i + 64]) is None for i in range(n_total))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_total", [2, 8])
def test_untouched_rows_and_guards_keep_the_sentinel(curve, n_total):
    devs, models = model_case(curve, n_total)
    for a, (d, m) in enumerate(zip(devs, models)):
        d.assert_untouched("n_total %d, request %d:" % (n_total, a))
        got = d.bytes()
        for f in FAMILIES:                                                  # ... and the resident halves were all written
            half = d.size[f] // 2
            assert got[f][half:] == bytes([SENTINEL]) * half and got[f][:half] != bytes([SENTINEL]) * half


# ---- 2. against the single-file entry points: 1 024 rows (two passes of the data network, the MAC side's n >= 128 forms), 2^15 (the
# protocol's size, more than 2^13 butterflies per stage) and 2^16 (the cap).  All on the device: the stores after the write, the two
# encodes of each on them, the complements by host point additions on 16 sampled points per part at the large sizes.
def single_file_case(curve, n_total, seed, add_all):
    import torch
    import icc_py
    from porla_amd import icc
    rnd = random.Random(seed)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    pts = points_of(curve)
    table = _dev(b"".join(pt_bytes(p) for p in pts + [None])).view(41, 64)
    steps = (7 * n_total, 2 * n_total + 5)
    devs, reqs, writes = [], [], []
    for a in range(2):
        u = torch.randint(0, 256, (n_total * NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen)
        pick = torch.randint(0, 41, (n_total,), device="cuda", generator=gen)
        macs = table[pick].reshape(-1).contiguous()
        d = DevFile(n_total, u.clone(), macs.clone())
        block = torch.randint(0, 256, (NCOLS * 32,), dtype=torch.uint8, device="cuda", generator=gen)
        mac = _dev(pt_bytes(rnd.choice(pts)))
        comps = None
        if a == 1:
            comps = table[torch.randint(0, 41, (2 * n_total,), device="cuda", generator=gen)].reshape(-1).contiguous()
        index = (1, n_total)[a]
        devs.append(d)
        reqs.append(d.req(block, mac, comps, steps[a], index))
        writes.append((u, macs, block, mac, comps, index))
    torch.cuda.synchronize()
    call(reqs, n_total, curve)
    torch.cuda.synchronize()
    for a, (d, (u, macs, block, mac, comps, index)) in enumerate(zip(devs, writes)):
        what = "n_total %d, request %d:" % (n_total, a)
        u[(index - 1) * NCOLS * 32:index * NCOLS * 32] = block
        macs[(index - 1) * 64:index * 64] = mac
        assert torch.equal(d.t["u_blocks"][:u.numel()], u) and torch.equal(d.t["u_macs"][:macs.numel()], macs), what + " the stores"
        half = n_total * NCOLS * 64
        x, y = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        icc.crebuild_xy_device(u.data_ptr(), n_total, NCOLS, curve, steps[a], d_x=x.data_ptr(), d_y_x=y.data_ptr())
        mx_, my_ = torch.empty(64 * n_total, dtype=torch.uint8, device="cuda"), torch.empty(64 * n_total, dtype=torch.uint8, device="cuda")
        icc.mac_crebuild_xy_device(macs.data_ptr(), n_total, curve, steps[a], mx_.data_ptr(), my_.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(d.t["data_x"][:half], x), what + " data X"
        assert torch.equal(d.t["data_y"][:half], y), what + " data Y"
        for f in ("align_x", "align_y"):
            assert not bool(d.t[f][:64 * n_total].any()), what + " " + f
        if comps is None:
            assert torch.equal(d.t["mac_x"][:64 * n_total], mx_) and torch.equal(d.t["mac_y"][:64 * n_total], my_), what + " MACs"
        else:
            sample = range(n_total) if add_all else sorted({0, 1, n_total - 1} | set(rnd.sample(range(n_total), 13)))
            hc = _host(comps)
            for part, enc, f in ((0, _host(mx_), "mac_x"), (1, _host(my_), "mac_y")):
                got = _host(d.t[f][:64 * n_total])
                for j in sample:
                    want = icc_py.ec_add(curve, pt_tuple(enc[64 * j:64 * j + 64]), pt_tuple(hc[64 * (part * n_total + j):64 * (part * n_total + j) + 64]))
                    assert got[64 * j:64 * j + 64] == pt_bytes(want), what + " %s[%d]" % (f, j)
        d.assert_untouched(what)


@pytest.mark.parametrize("curve", CURVES)
def test_1024_rows_equal_the_single_file_entry_points(curve):
    single_file_case(curve, 1024, 5100, True)


@pytest.mark.parametrize("curve,n_total", [("bn254", 1 << 15), ("secp256k1", 1 << 16)])
def test_at_the_cap_equal_the_single_file_entry_points(curve, n_total):
    single_file_case(curve, n_total, 5200, False)


# ---- 3. the launch sequence depends on n_total, not on K
def test_launch_count_does_not_depend_on_k():
    import torch
    from porla_amd import multiexp as mx
    n_total = 256
    gen = torch.Generator(device="cuda")
    gen.manual_seed(61)
    table = _dev(b"".join(pt_bytes(p) for p in points_of("bn254"))).view(40, 64)

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
        call(reqs, n_total, "bn254")
        torch.cuda.synchronize()
        return sum(c for _, _, c in mx.profile_get()) - before

    launches(1)                                                  # (tables and workspaces built outside the count)
    mx.profile_enable(1)
    try:
        one, eight = launches(1), launches(8)
    finally:
        mx.profile_enable(0)
    assert one == eight and one >= 1 + 1 + 1 + 8 + 1 + 1          # store, one data pass, MAC load, eight stages, the Y scaling, the close


# ---- 4. a whole cycle of one file, KZG, n_total = 8: writes 1 .. 7 through the update batch, write 8 through the client's rebuild call
# and then this one, both on one non-default stream, this call reading the client call's output buffers with nothing in between
def test_a_whole_cycle_behind_the_client_rebuild_call():
    import torch
    from porla_amd import multiexp as mx
    from tests import test_client_rebuild_batch_gpu as cr, test_update_batch_gpu as ub
    from tests.client_rebuild_model import n_prf, rebuild_points
    n_total = 8
    S, client_call = cr.setup_of("bn254")
    server = S.server
    # the library's key, SRS and hiding point are process state, and the setups above are cached per process: a test module that ran
    # in between may have installed another key (tests/test_golden_gpu.py, tests/test_msm_small_gpu.py do), and every init_SRS draws a
    # new hiding point.  So the setup's key goes in again, and h is read from the library as it stands now
    mx.init_key(ub.TAU, ub.ALPHA)
    mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
    h = pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))                # 1 * h_MAC
    rnd = random.Random(77)
    m = RebuildFileModel(n_total, NCOLS, "bn254", server.base, fill=SENTINEL)
    d = ub.DevFile(m)                                             # every level of the six families, as the update batch takes them
    row = 32 * NCOLS
    d_u = torch.full((n_total * row + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_um = torch.full((n_total * 64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    writes = []
    for step in range(1, n_total):
        level = (step & -step).bit_length() - 1
        chunks, mac, comps = ub.random_write(rnd, server, level, step % 2 == 1)
        writes.append((step, level, chunks, mac, comps))
    last_chunks = [rnd.getrandbits(256) for _ in range(NCOLS)]
    prf = [rnd.getrandbits(128) for _ in range(n_prf(n_total))]
    d_block = _dev(block_bytes(last_chunks))
    d_prf = _dev(b"".join(cr.raw_of("bn254", v) for v in prf))
    d_mac = torch.full((64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_comp = torch.full((128 * n_total + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    top = m.height - 1
    with torch.cuda.stream(stream):
        reqs = [d.req(chunks, mac, comps, step, level) for step, level, chunks, mac, comps in writes]
        up = {step: (_dev(block_bytes(chunks)), _dev(pt_bytes(mac))) for step, level, chunks, mac, comps in writes}
        stream.synchronize()                                      # (the inputs are uploaded; from here on nothing waits on the host)
        for (step, level, chunks, mac, comps), req in zip(writes, reqs):
            d_u[(step - 1) * row:step * row].copy_(up[step][0], non_blocking=True)      # U and MAC_U as Server::update keeps them
            d_um[(step - 1) * 64:step * 64].copy_(up[step][1], non_blocking=True)
            server.call([req], n_total, stream.cuda_stream)
        client_call([(d_block.data_ptr(), d_prf.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), n_total)], n_total, stream.cuda_stream)
        call([(d_block.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), d_u.data_ptr(), d_um.data_ptr()) +
              tuple(d.t[f][top].data_ptr() for f in FAMILIES) + (n_total, n_total)], n_total, "bn254", stream.cuda_stream)
    for step, level, chunks, mac, comps in writes:
        assert m.update(chunks, mac, comps, index=step) == (step, level)
    mac8, out8 = rebuild_points("bn254", n_total, n_total, prf, h, S.block_commit(last_chunks))
    assert m.update(last_chunks, mac8, out8, index=n_total) == (n_total, top)
    stream.synchronize()
    assert _host(d_mac[:64]) == pt_bytes(mac8)
    got = d.bytes()
    for f in FAMILIES:
        assert got[f][top] == bytes(m.fam[f][top]), "%s of the top level differs" % f
        for lv in range(top):
            assert got[f][lv] == bytes(m.fam[f][lv]), "%s level %d was touched" % (f, lv)
    assert _host(d_u) == bytes(m.u_blocks) + bytes([SENTINEL]) * GUARD and _host(d_um) == bytes(m.u_macs) + bytes([SENTINEL]) * GUARD


# ---- 5. PORLA_MAC_QUAD_MAX=0 (one lane per butterfly and per scaled point) gives the same bytes at n_total = 64
def digest_of(curve, n_total):
    """sha256 over every buffer of the three requests of make_requests (without the model's negative) after the call"""
    h = hashlib.sha256()
    for d in run_on_device(curve, n_total, make_requests(curve, n_total, False)):
        got = d.bytes()
        for f in FAMILIES + STORES:
            h.update(got[f])
    return h.hexdigest()


def test_mac_quad_max_0_gives_the_same_bytes():
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" \
           "from tests import test_server_rebuild_batch_gpu as t\n" \
           "print('digests', t.digest_of('bn254', 64), t.digest_of('secp256k1', 64))\n" % (common.ROOT, os.path.join(common.ROOT, "oracle"))
    env = dict(os.environ, PORLA_MAC_QUAD_MAX="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=common.ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("digests ")][-1].split()
    assert line[1:] == [digest_of("bn254", 64), digest_of("secp256k1", 64)]

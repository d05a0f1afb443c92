"""GPU box: the client's rebuild write (porla_kzg_client_rebuild_batch_device / porla_ipa_client_rebuild_batch_device) -- Client::CRebuild's
step for K writes in one asynchronous call -- bit-exact against the two restatements of tests/client_rebuild_model.py (both curves):
every byte against the point-domain model at n_total = 2, 4, 64, and MAC plus 64 sampled outputs against the scalar-domain model at
n_total = T, 2 T, 4 T (T = multiexp.CLIENT_REBUILD_TILE: the last in-tile stage, the first global stage, two global stages), where the
KZG build is also compared byte for byte with the composition of the entry points the call replaces.  128 columns.
The point-domain model costs about 640 scalar multiplications in Python per request at n_total = 64: those two cases take a few
seconds each, the others about one."""
import random

import pytest

from tests.client_rebuild_model import n_prf, rebuild_points, scalar_points
from tests.client_update_model import prf_scalar
from tests.update_model import pt_bytes

pytestmark = pytest.mark.gpu
NCOLS = 128
SENTINEL = 0xA5
CURVES = ["bn254", "secp256k1"]
MASK = (1 << 128) - 1


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy())


def setup_of(curve):
    """the client update test's setup (hiding point, alpha, the IPA bases, the block's commitment for the model) with this call"""
    from porla_amd import multiexp as mx
    from tests import test_client_update_batch_gpu as t
    S = t.setup_of(curve)
    if curve == "bn254":
        call = lambda reqs, n_total, stream=0: mx.kzg_client_rebuild_batch_device(reqs, n_total, stream)
    else:
        call = lambda reqs, n_total, stream=0: S.afb.ipa_client_rebuild_batch_device(S.hfb, reqs, n_total, stream)
    return S, call


def raw_of(curve, value):
    """the 16 raw bytes the library reads as `value`"""
    return value.to_bytes(16, "big" if curve == "bn254" else "little")


class Write:
    """one write: chunks, the PRF values in d_prf's order, and what a model makes of them (full = the point domain, every output;
    otherwise the scalar domain at the indices `sample`)"""

    def __init__(self, S, n_total, step, chunks, prf, sample=None):
        assert len(prf) == n_prf(n_total)
        self.n, self.step, self.chunks, self.prf = n_total, step, chunks, prf
        self.prf_raw = b"".join(raw_of(S.curve, v) for v in prf)
        assert all(prf_scalar(S.curve, self.prf_raw[16 * i:16 * i + 16]) == v for i, v in enumerate(prf[:3]))
        bc = S.block_commit(chunks)
        if sample is None:
            self.mac, out = rebuild_points(S.curve, n_total, step, prf, S.h, bc)
            self.want = dict(enumerate(out))
        else:
            self.mac, self.want = scalar_points(S.curve, n_total, step, prf, S.h, bc, sample)

    def block_bytes(self):
        return b"".join(c.to_bytes(32, "little") for c in self.chunks)


class DevWrite:
    """a write's buffers on the device; the outputs pre-filled with the sentinel, `extra` points past the call's"""

    def __init__(self, w, extra=2):
        import torch
        self.w = w
        self.block, self.prf = _dev(w.block_bytes()), _dev(w.prf_raw)
        self.mac = torch.full((64 * (1 + extra),), SENTINEL, dtype=torch.uint8, device="cuda")
        self.comp = torch.full((64 * (2 * w.n + extra),), SENTINEL, dtype=torch.uint8, device="cuda")

    def req(self):
        return (self.block.data_ptr(), self.prf.data_ptr(), self.mac.data_ptr(), self.comp.data_ptr(), self.w.step)

    def got(self):
        return _host(self.mac), _host(self.comp)

    def check(self, what=""):
        mac, comp = self.got()
        n = 128 * self.w.n
        assert mac[:64] == pt_bytes(self.w.mac), "%s MAC" % what
        for g, p in sorted(self.w.want.items()):
            assert comp[64 * g:64 * g + 64] == pt_bytes(p), "%s output %d of %d" % (what, g, 2 * self.w.n)
        assert mac[64:] == bytes([SENTINEL]) * (len(mac) - 64) and comp[n:] == bytes([SENTINEL]) * (len(comp) - n), "%s sentinel" % what


def random_write(rnd, S, n_total, step, sample=None):
    return Write(S, n_total, step, [rnd.getrandbits(256) for _ in range(NCOLS)], [rnd.getrandbits(128) for _ in range(n_prf(n_total))], sample)


# ---- 1. every byte against the point-domain model: one call of three requests, one write_step a multiple of n_total, two not
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n_total", [2, 4, 64])
def test_every_byte_equals_the_point_model(curve, n_total):
    import torch
    S, call = setup_of(curve)
    rnd = random.Random(100 + n_total)
    writes = [random_write(rnd, S, n_total, step) for step in (3 * n_total, n_total + 1, 5 * n_total + (n_total // 2 | 1))]
    assert [w.step % n_total == 0 for w in writes] == [True, False, False]
    devs = [DevWrite(w) for w in writes]
    torch.cuda.synchronize()
    call([d.req() for d in devs], n_total)
    torch.cuda.synchronize()
    for a, d in enumerate(devs):
        d.check("n_total %d, request %d:" % (n_total, a))


# ---- 2. around the tile: MAC and 64 sampled outputs against the scalar-domain model; KZG: every byte against the composition
def sample_of(rnd, n_total, tile):
    must = {0, tile - 1, tile, n_total - 1, n_total, 2 * n_total - 1}
    must = {g for g in must if g < 2 * n_total}
    rest = [g for g in range(2 * n_total) if g not in must]
    return sorted(must | set(rnd.sample(rest, 64 - len(must))))


def kzg_composition(w):
    """what a caller had before: complements of the old values, porla_icc_mac_encode_xy_device on them, complements of the new
    values, host point subtractions.  Returns the 2 * n_total * 64 bytes."""
    import torch
    from porla_amd import icc, multiexp as mx
    n = w.n
    sc = _dev(b"".join(v.to_bytes(32, "big") for v in w.prf[1:]))
    pts = torch.zeros(64 * 3 * n, dtype=torch.uint8, device="cuda")
    mx.kzg_complement_batch_device(sc.data_ptr(), 3 * n, pts.data_ptr())
    xy = torch.zeros(64 * 2 * n, dtype=torch.uint8, device="cuda")
    icc.mac_crebuild_xy_device(pts.data_ptr(), n, "bn254", w.step, xy.data_ptr(), xy.data_ptr() + 64 * n)
    torch.cuda.synchronize()
    new, t = _host(pts)[64 * n:], _host(xy)
    return b"".join(mx.bn254_add(new[64 * g:64 * g + 64], mx.bn254_neg(t[64 * g:64 * g + 64])) for g in range(2 * n))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("tiles", [1, 2, 4])
def test_sampled_outputs_around_the_tile_equal_the_scalar_model(curve, tiles):
    import torch
    from porla_amd import multiexp as mx
    S, call = setup_of(curve)
    tile = mx.CLIENT_REBUILD_TILE
    n_total = tiles * tile
    rnd = random.Random(200 + tiles)
    writes = [random_write(rnd, S, n_total, step, sample_of(rnd, n_total, tile)) for step in (n_total, 7 * n_total + 5)]
    for w in writes:
        assert len(w.want) == 64 and {0, tile - 1, tile, n_total - 1, n_total, 2 * n_total - 1} <= set(w.want)
    devs = [DevWrite(w) for w in writes]
    torch.cuda.synchronize()
    call([d.req() for d in devs], n_total)
    torch.cuda.synchronize()
    for a, d in enumerate(devs):
        d.check("n_total %d, request %d:" % (n_total, a))
    if curve == "bn254":
        for a, d in enumerate(devs):
            want = kzg_composition(d.w)
            got = d.got()[1][:128 * n_total]
            assert got == want, "request %d differs from the composition at output %d" % (
                a, next(g for g in range(2 * n_total) if got[64 * g:64 * g + 64] != want[64 * g:64 * g + 64]))


# ---- 3. edge values
@pytest.mark.parametrize("curve", CURVES)
def test_edge_values(curve):
    import torch
    S, call = setup_of(curve)
    rnd = random.Random(303)
    chunks = lambda: [rnd.getrandbits(256) for _ in range(NCOLS)]
    zeros = [0] * NCOLS
    r = lambda: rnd.getrandbits(128)
    s0, s1 = rnd.getrandbits(127), rnd.getrandbits(127)
    two = [
        Write(S, 2, 3, chunks(), [r(), s0, s1, s0 + s1, r(), r(), r()]),           # new_X[0] = s_0 + s_1: out[0] = infinity
        Write(S, 2, 2, zeros, [0, r(), r(), r(), r(), r(), r()]),                  # an all-zero block, comp0 = infinity: MAC = infinity
    ]
    assert two[0].want[0] is None and two[0].want[1] is not None and two[1].mac is None
    four = [
        Write(S, 4, 5, chunks(), [r()] + [0] * 4 + [MASK] * 8),                    # every old complement infinity, every new value 2^128 - 1
        Write(S, 4, 8, zeros, [MASK] + [MASK] * 4 + [0] * 8),                      # an all-zero block: MAC = comp0; every new complement infinity
        Write(S, 4, 6, chunks(), [0, MASK, 0, r(), MASK] + [r(), 0, MASK, r()] * 2),
    ]
    assert four[1].mac == __import__("icc_py").ec_mul(curve, S.h, MASK)
    for n_total, writes in ((2, two), (4, four)):
        devs = [DevWrite(w) for w in writes]
        torch.cuda.synchronize()
        call([d.req() for d in devs], n_total)
        torch.cuda.synchronize()
        for a, d in enumerate(devs):
            d.check("n_total %d, edge %d:" % (n_total, a))
        if n_total == 2:
            assert devs[0].got()[1][:64] == bytes(64) and devs[1].got()[0][:64] == bytes(64)


# ---- 4. the launch sequence depends on n_total, not on K
class BareWrite:
    """a request whose outputs are not compared (no model behind it)"""

    def __init__(self, rnd, n_total, step):
        import torch
        self.block = _dev(rnd.randbytes(32 * NCOLS))
        self.prf = _dev(rnd.randbytes(16 * n_prf(n_total)))
        self.mac = torch.zeros(64, dtype=torch.uint8, device="cuda")
        self.comp = torch.zeros(128 * n_total, dtype=torch.uint8, device="cuda")
        self.req = (self.block.data_ptr(), self.prf.data_ptr(), self.mac.data_ptr(), self.comp.data_ptr(), step)


@pytest.mark.parametrize("curve", CURVES)
def test_launch_count_does_not_depend_on_k(curve):
    import torch
    from porla_amd import multiexp as mx
    S, call = setup_of(curve)
    rnd = random.Random(606)
    n_total = 2 * mx.CLIENT_REBUILD_TILE                         # one global stage behind the tile's

    def launches(k):
        ws = [BareWrite(rnd, n_total, n_total * (a + 1) + (a % 3)) for a in range(k)]
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        call([w.req for w in ws], n_total)
        torch.cuda.synchronize()
        return sum(c for _, _, c in mx.profile_get()) - before

    launches(1)                                                  # (tables and workspaces built outside the count)
    mx.profile_enable(1)
    try:
        one, eight = launches(1), launches(8)
    finally:
        mx.profile_enable(0)
    assert one == eight and one >= 7                             # expand, two passes, the tile's stages, one global stage, close, place


# ---- 5. a larger call on another stream while the first is in flight (the pattern of tests/test_batch_scaffold_gpu.py)
@pytest.mark.parametrize("curve", CURVES)
def test_a_larger_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    S, call = setup_of(curve)
    rnd = random.Random(707)
    a = [DevWrite(random_write(rnd, S, 4, step)) for step in (4, 7)]
    b = [DevWrite(random_write(rnd, S, 16, step)) for step in (16, 21, 40)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ballast = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            ballast.normal_()                       # a few milliseconds ahead of A on its stream: A is in flight when B comes
    call([d.req() for d in a], 4, s1.cuda_stream)
    call([d.req() for d in b], 16, s2.cuda_stream)
    torch.cuda.synchronize()
    for d in a + b:
        d.check("n_total %d:" % d.w.n)


def test_ipa_bad_bases_are_refused():
    from porla_amd import multiexp as mx
    from tests import common, test_update_batch_gpu as t
    S, _ = setup_of("secp256k1")
    w = BareWrite(random.Random(808), 4, 4)
    short = mx.FixedBase("secp256k1", S.server.base[:64 * 100], 100, t.WINDOW)
    with pytest.raises(RuntimeError, match="128"):
        short.ipa_client_rebuild_batch_device(S.hfb, [w.req], 4)
    with pytest.raises(RuntimeError, match="exactly one"):
        S.afb.ipa_client_rebuild_batch_device(short, [w.req], 4)
    bn = mx.FixedBase("bn254", common.synth_points(NCOLS), NCOLS, 8)
    with pytest.raises(RuntimeError, match="secp256k1"):
        bn.ipa_client_rebuild_batch_device(S.hfb, [w.req], 4)
    with pytest.raises(RuntimeError, match="secp256k1"):
        S.afb.ipa_client_rebuild_batch_device(bn, [w.req], 4)
    assert _host(w.mac) == bytes(64) and _host(w.comp) == bytes(512)               # nothing was written

"""GPU box: the batched client update (porla_kzg_client_update_batch_device / porla_ipa_client_update_batch_device) -- Client::update's
preprocessing for K writes in one asynchronous call -- bit-exact against the Python restatement tests/client_update_model.py (both
curves), against the composition of the entry points it replaces, and as the input of the batched server update, audit and verify.
n_total = 16, 128 columns, levels 0 .. 3: the smallest shapes that reach every step of the pyramid."""
import random

import pytest

from tests import common
from tests.client_update_model import client_update, n_prf, prf_scalar
from tests.update_model import FAMILIES, FileModel, pt_bytes, pt_tuple, row_vals

pytestmark = pytest.mark.gpu
NCOLS = 128
SENTINEL = 0xA5
CURVES = ["bn254", "secp256k1"]
IPA_ALPHA = 5                       # the IPA twin's alpha: alpha_generators[i] = alpha * generators[i]
N_TOTAL = 16


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    return bytes(t.cpu().numpy())


class Setup:
    """per curve: the server side of tests/test_update_batch_gpu.py (commitment base, the server call) and the client's: the hiding
    point, alpha, the client call, the block's commitment for the model"""

    def __init__(self, curve):
        import icc_py
        from porla_amd import multiexp as mx
        from tests import test_update_batch_gpu as t
        self.curve, self.server = curve, t.setup_of(curve)
        self.q = icc_py.Q[curve]
        if curve == "bn254":
            self.alpha = int.from_bytes(t.ALPHA, "big")
            self.h = pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))       # 1 * h_MAC
            self.call = lambda reqs, n_total, stream=0: mx.kzg_client_update_batch_device(reqs, n_total, stream)
        else:
            self.alpha = IPA_ALPHA
            gens = [pt_tuple(self.server.base[64 * i:64 * i + 64]) for i in range(NCOLS)]
            self.afb = mx.FixedBase("secp256k1", b"".join(pt_bytes(icc_py.ec_mul(curve, g, IPA_ALPHA)) for g in gens), NCOLS, t.WINDOW)
            self.h = self.server.points[7]
            self.hfb = mx.FixedBase("secp256k1", pt_bytes(self.h), 1, t.WINDOW)
            self.call = lambda reqs, n_total, stream=0: self.afb.ipa_client_update_batch_device(self.hfb, reqs, n_total, stream)

    def commit(self, scalars):
        rows = b"".join(c.to_bytes(32, "big") for c in scalars)
        return pt_tuple(common.oracle_commit_batch(self.curve, rows, 1, NCOLS, self.server.base))

    def block_commit(self, chunks):
        import icc_py
        return icc_py.ec_mul(self.curve, self.commit([c % self.q for c in chunks]), self.alpha)


_SETUPS = {}


def setup_of(curve):
    if curve not in _SETUPS:
        _SETUPS[curve] = Setup(curve)
    return _SETUPS[curve]


class Write:
    """one write: chunks, the raw PRF bytes in d_prf's order, and what the model makes of them"""

    def __init__(self, S, n_total, step, level, chunks, prf_raw):
        assert len(prf_raw) == n_prf(level)
        self.step, self.level, self.chunks, self.prf_raw = step, level, chunks, prf_raw
        self.prf = [prf_scalar(S.curve, r) for r in prf_raw]
        self.new = self.prf[-(2 << level):]
        self.mac, self.out = client_update(S.curve, n_total, step, level, self.prf, S.h, S.block_commit(chunks))
        self.want_mac, self.want_out = pt_bytes(self.mac), b"".join(pt_bytes(p) for p in self.out)

    def block_bytes(self):
        return b"".join(c.to_bytes(32, "little") for c in self.chunks)


class DevWrite:
    """a write's buffers on the device; the outputs pre-filled with the sentinel, `extra` points past the call's"""

    def __init__(self, w, extra=2, prf_raw=None):
        import torch
        self.w = w
        self.block = _dev(w.block_bytes())
        self.prf = _dev(b"".join(prf_raw if prf_raw is not None else w.prf_raw))
        self.mac = torch.full((64 * (1 + extra),), SENTINEL, dtype=torch.uint8, device="cuda")
        self.comp = torch.full((64 * ((2 << w.level) + extra),), SENTINEL, dtype=torch.uint8, device="cuda")

    def req(self):
        return (self.block.data_ptr(), self.prf.data_ptr(), self.mac.data_ptr(), self.comp.data_ptr(), self.w.step, self.w.level)

    def got(self):
        return _host(self.mac), _host(self.comp)

    def check(self, what=""):
        mac, comp = self.got()
        n = 64 * (2 << self.w.level)
        assert mac[:64] == self.w.want_mac, "%s MAC" % what
        assert comp[:n] == self.w.want_out, "%s complements (first byte %d)" % (what, next(i for i in range(n) if comp[i] != self.w.want_out[i]))
        assert mac[64:] == bytes([SENTINEL]) * (len(mac) - 64) and comp[n:] == bytes([SENTINEL]) * (len(comp) - n), "%s sentinel" % what


def raw16(rnd):
    return rnd.getrandbits(128).to_bytes(16, "big")


def random_write(rnd, S, n_total, step, level):
    return Write(S, n_total, step, level, [rnd.getrandbits(256) for _ in range(NCOLS)], [raw16(rnd) for _ in range(n_prf(level))])


# ---- the 15 writes of a full cycle of one file, computed once per curve and shared (tests 1, 4, 5)
_CYCLES = {}


def cycle_of(curve):
    if curve not in _CYCLES:
        S = setup_of(curve)
        rnd = random.Random(101)
        slots, writes = {}, []
        for step in range(1, N_TOTAL):
            level = (step & -step).bit_length() - 1
            raw = [raw16(rnd)]
            for i in range(level):
                raw += slots.pop(i)                          # the PRF reproduces level i's values: X part, then Y part
            new = [raw16(rnd) for _ in range(2 << level)]
            slots[level] = new
            writes.append(Write(S, N_TOTAL, step, level, [rnd.getrandbits(256) for _ in range(NCOLS)], raw + new))
        _CYCLES[curve] = writes
    return _CYCLES[curve]


# ---- 1. one file, the 15 writes of a full cycle, one request per call on one side stream with no host synchronisation in between
@pytest.mark.parametrize("curve", CURVES)
def test_one_file_a_full_cycle_of_sequential_writes(curve):
    import torch
    S = setup_of(curve)
    writes = cycle_of(curve)
    devs = [DevWrite(w) for w in writes]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for d in devs:
        S.call([d.req()], N_TOTAL, stream.cuda_stream)
    stream.synchronize()
    for d in devs:
        d.check("write %d (level %d):" % (d.w.step, d.w.level))


def test_kzg_outputs_equal_the_composition_of_the_entry_points_they_replace():
    import icc_py
    import torch
    from porla_amd import multiexp as mx
    S = setup_of("bn254")
    writes = [w for w in cycle_of("bn254") if w.level <= 1][:4]
    devs = [DevWrite(w) for w in writes]
    torch.cuda.synchronize()
    S.call([d.req() for d in devs], N_TOTAL)
    # the MACs: porla_kzg_mac_batch_device on the big-endian form of the same chunks
    rows = _dev(b"".join(c.to_bytes(32, "big") for w in writes for c in w.chunks))
    sc = _dev(b"".join(w.prf_raw[0].rjust(32, b"\0") for w in writes))
    d_mac = torch.zeros(64 * len(writes), dtype=torch.uint8, device="cuda")
    mx.kzg_mac_batch_device(rows.data_ptr(), sc.data_ptr(), len(writes), d_mac.data_ptr())
    torch.cuda.synchronize()
    macs = _host(d_mac)
    sub = lambda a, b: mx.bn254_add(a, mx.bn254_neg(b))
    for a, (w, d) in enumerate(zip(writes, devs)):
        mac, comp = d.got()
        assert mac[:64] == macs[64 * a:64 * a + 64]
        cdc = [mx.compute_digest_complement(r) for r in w.prf_raw]
        wt = pow(icc_py.root_w(N_TOTAL), icc_py.reverse_bits(w.step % N_TOTAL, icc_py.height_of(N_TOTAL) - 1), icc_py.P_ICC)
        y = mx.bn254_mult(cdc[0], wt.to_bytes(32, "big"))
        if w.level == 0:
            want = [sub(cdc[1], cdc[0]), sub(cdc[2], y)]
        else:                                                   # one butterfly per part, v^0 = 1
            tx = [mx.bn254_add(cdc[1], cdc[0]), sub(cdc[1], cdc[0])]
            ty = [mx.bn254_add(cdc[2], y), sub(cdc[2], y)]
            want = [sub(cdc[3], tx[0]), sub(cdc[4], tx[1]), sub(cdc[5], ty[0]), sub(cdc[6], ty[1])]
        assert comp[:64 * len(want)] == b"".join(want), (w.step, w.level)


# ---- 2. mixed levels in one call: each output equals its single-request call's, and nothing past it is touched
@pytest.mark.parametrize("curve", CURVES)
def test_mixed_levels_in_one_call(curve):
    import torch
    S = setup_of(curve)
    rnd = random.Random(202)
    shapes = [(3, 8), (0, 1), (2, 4), (0, 3), (1, 2), (3, 24)]                     # (level, write_step), unsorted
    writes = [random_write(rnd, S, N_TOTAL, ws, level) for level, ws in shapes]
    batch = [DevWrite(w, extra=3) for w in writes]
    single = [DevWrite(w, extra=3) for w in writes]
    torch.cuda.synchronize()
    S.call([d.req() for d in batch], N_TOTAL)
    for d in single:
        S.call([d.req()], N_TOTAL)
    torch.cuda.synchronize()
    for a, (b, s) in enumerate(zip(batch, single)):
        assert b.got() == s.got(), a
        b.check("request %d:" % a)


# ---- 3. edge values, one call of four requests
@pytest.mark.parametrize("curve", CURVES)
def test_edge_values(curve):
    import torch
    S = setup_of(curve)
    rnd = random.Random(303)
    chunks = lambda: [rnd.getrandbits(256) for _ in range(NCOLS)]
    zero, s, t = bytes(16), raw16(rnd), raw16(rnd)
    big = [S.q + 5, (1 << 256) - 1, S.q, S.q - 1] + [rnd.getrandbits(256) | (1 << 255) for _ in range(NCOLS - 4)]
    writes = [
        Write(S, N_TOTAL, 1, 0, chunks(), [zero, zero, s]),                        # comp0 = infinity: X[0] = Y[0] = infinity, out[0] too
        Write(S, N_TOTAL, 3, 0, chunks(), [s, s, t]),                              # new X[0] == comp0: out[0] = infinity
        Write(S, N_TOTAL, 2, 1, chunks(), [s, s, t, raw16(rnd), raw16(rnd), raw16(rnd), raw16(rnd)]),   # a0 == a1 in X's butterfly
        Write(S, N_TOTAL, 5, 0, big, [raw16(rnd), raw16(rnd), raw16(rnd)]),        # chunks >= the group order
    ]
    assert writes[0].out[0] is None and writes[0].mac == S.block_commit(writes[0].chunks)
    assert writes[1].out[0] is None and writes[1].out[1] is not None
    devs = [DevWrite(w) for w in writes]
    torch.cuda.synchronize()
    S.call([d.req() for d in devs], N_TOTAL)
    torch.cuda.synchronize()
    for a, d in enumerate(devs):
        d.check("edge %d:" % a)
    assert devs[0].got()[1][:64] == bytes(64) and devs[1].got()[1][:64] == bytes(64)


# ---- 4. / 5. the closed loop on the device: client batch -> server update batch on the same stream and buffers, no synchronisation
def run_loop(curve, writes, flip=None):
    """the cycle's writes through both calls; flip = (step, prf index): one PRF byte of that write differs from what `writes` says.
    Returns the server-side device file."""
    import torch
    from tests import test_update_batch_gpu as t
    S = setup_of(curve)
    m = FileModel(N_TOTAL, NCOLS, curve, S.server.base, fill=SENTINEL)
    d = t.DevFile(m)
    devs = []
    for w in writes:
        raw = list(w.prf_raw)
        if flip and flip[0] == w.step:
            raw[flip[1]] = bytes([raw[flip[1]][0] ^ 1]) + raw[flip[1]][1:]
        devs.append(DevWrite(w, prf_raw=raw))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for dw in devs:
        w = dw.w
        S.call([dw.req()], N_TOTAL, stream.cuda_stream)
        sreq = (dw.block.data_ptr(), dw.mac.data_ptr(), dw.comp.data_ptr(), w.step, w.level) + \
            tuple([x.data_ptr() for x in d.t[f][:w.level + 1]] for f in FAMILIES)
        S.server.call([sreq], N_TOTAL, stream.cuda_stream)
    stream.synchronize()
    d.keep += devs
    return d


def final_slots(writes):
    """level -> (X scalars, Y scalars) of the complements resident after the cycle"""
    slots = {}
    for w in writes:
        for i in range(w.level):
            slots.pop(i)
        slots[w.level] = (w.new[:1 << w.level], w.new[1 << w.level:])
    return slots


def check_identity(S, got, writes, mul, add, digest, complement):
    """mac + alpha * align == alpha * Commit(row mod q) + s_new * h for every resident row of every level, X and Y"""
    n = 0
    for lv, (sx, sy) in final_slots(writes).items():
        for part, s in (("x", sx), ("y", sy)):
            for r in range(1 << lv):
                row = row_vals(got["data_" + part][lv][r * 64 * NCOLS:(r + 1) * 64 * NCOLS])
                mac_r = got["mac_" + part][lv][64 * r:64 * r + 64]
                al_r = got["align_" + part][lv][64 * r:64 * r + 64]
                assert add(mac_r, mul(al_r)) == add(digest([v % S.q for v in row]), complement(s[r])), (lv, part, r)
                n += 1
    assert n == 2 * (N_TOTAL - 1)


def test_kzg_closed_loop_update_audit_verify():
    import numpy as np
    import torch
    from porla_amd import multiexp as mx
    from tests import test_update_batch_gpu as t
    S = setup_of("bn254")
    writes = cycle_of("bn254")
    alpha32 = t.ALPHA.rjust(32, b"\0")
    d = run_loop("bn254", writes)
    check_identity(S, d.bytes(), writes, lambda p: mx.bn254_mult(p, alpha32), mx.bn254_add,
                   lambda vals: mx.compute_digest(b"".join(v.to_bytes(32, "big") for v in vals)),
                   lambda s: mx.compute_digest_complement(s.to_bytes(16, "big")))
    # a second file whose write 8 drew another PRF value for level 3's X slot 5 than the client's complement store holds
    lv, nrow = 3, 8
    bad = run_loop("bn254", writes, flip=(8, n_prf(3) - 2 * nrow + 5))
    comp_store = _dev(b"".join(mx.compute_digest_complement(s.to_bytes(16, "big")) for s in final_slots(writes)[lv][0]))
    idx = torch.tensor(list(range(nrow)), dtype=torch.int64).cuda()
    coef = torch.tensor(np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.uint32).view(np.int32)).cuda()
    audits = [(f.t["data_x"][lv].data_ptr(), idx.data_ptr(), coef.data_ptr(), nrow, 0, 0, 0, 0, f.t["mac_x"][lv].data_ptr(),
               f.t["align_x"][lv].data_ptr(), idx.data_ptr(), coef.data_ptr(), nrow, 777 + a) for a, f in enumerate((d, bad))]
    d_rec = torch.zeros(320 * 2, dtype=torch.uint8, device="cuda")
    mx.kzg_audit_batch_device(audits, d_rec.data_ptr())
    torch.cuda.synchronize()
    status = mx.kzg_verify_batch_device([(comp_store.data_ptr(), idx.data_ptr(), coef.data_ptr(), nrow, t.ALPHA)] * 2, d_rec.data_ptr())
    assert status[0] == mx.KZG_VERIFY_FULL | mx.KZG_VERIFY_PROOF
    assert status[1] == mx.KZG_VERIFY_PROOF                                        # the flipped PRF byte: FULL is lost, the opening holds


def test_ipa_closed_loop_update():
    import icc_py
    S = setup_of("secp256k1")
    writes = cycle_of("secp256k1")
    d = run_loop("secp256k1", writes)
    c = "secp256k1"
    check_identity(S, d.bytes(), writes, lambda p: pt_bytes(icc_py.ec_mul(c, pt_tuple(p), S.alpha)),
                   lambda a, b: pt_bytes(icc_py.ec_add(c, pt_tuple(a), pt_tuple(b))),
                   lambda vals: pt_bytes(icc_py.ec_mul(c, S.commit(vals), S.alpha)),
                   lambda s: pt_bytes(icc_py.ec_mul(c, S.h, s)))


# ---- 6. the launch sequence depends on the highest level, not on K
class BareWrite:
    """a request whose outputs are not compared (no model behind it)"""

    def __init__(self, rnd, step, level):
        import torch
        self.block = _dev(bytes(rnd.getrandbits(8) for _ in range(32 * NCOLS)))
        self.prf = _dev(bytes(rnd.getrandbits(8) for _ in range(16 * n_prf(level))))
        self.mac = torch.zeros(64, dtype=torch.uint8, device="cuda")
        self.comp = torch.zeros(64 * (2 << level), dtype=torch.uint8, device="cuda")
        self.req = (self.block.data_ptr(), self.prf.data_ptr(), self.mac.data_ptr(), self.comp.data_ptr(), step, level)


@pytest.mark.parametrize("curve", CURVES)
def test_launch_count_does_not_depend_on_k(curve):
    import torch
    from porla_amd import multiexp as mx
    S = setup_of(curve)
    rnd = random.Random(606)
    n_total, level = 256, 4

    def launches(k):
        ws = [BareWrite(rnd, 16 * (a + 1) + (0 if a == 0 else 1), level if a == 0 else rnd.randrange(level + 1)) for a in range(k)]
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        S.call([w.req for w in ws], n_total)
        torch.cuda.synchronize()
        return sum(c for _, _, c in mx.profile_get()) - before

    launches(1)                                                  # (tables and workspaces built outside the count)
    mx.profile_enable(1)
    try:
        one, eight = launches(1), launches(8)
    finally:
        mx.profile_enable(0)
    assert one == eight and one >= 6 + level                     # expand, two passes, scatter, place, `level` mixes, close


# ---- 7. a larger call on another stream while the first is in flight (the pattern of tests/test_batch_scaffold_gpu.py)
@pytest.mark.parametrize("curve", CURVES)
def test_a_larger_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    S = setup_of(curve)
    rnd = random.Random(707)
    a = [DevWrite(random_write(rnd, S, N_TOTAL, ws, level)) for level, ws in ((1, 2), (0, 5))]
    b = [DevWrite(random_write(rnd, S, N_TOTAL, ws, level)) for level, ws in ((0, 7), (2, 4), (1, 6), (2, 12), (0, 9))]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ballast = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            ballast.normal_()                       # a few milliseconds ahead of A on its stream: A is in flight when B comes
    S.call([d.req() for d in a], N_TOTAL, s1.cuda_stream)
    S.call([d.req() for d in b], N_TOTAL, s2.cuda_stream)
    torch.cuda.synchronize()
    for d in a + b:
        d.check("level %d:" % d.w.level)


def test_ipa_bad_bases_are_refused():
    from porla_amd import multiexp as mx
    from tests import test_update_batch_gpu as t
    S = setup_of("secp256k1")
    rnd = random.Random(808)
    w = BareWrite(rnd, 1, 0)
    short = mx.FixedBase("secp256k1", S.server.base[:64 * 100], 100, t.WINDOW)
    with pytest.raises(RuntimeError, match="128"):
        short.ipa_client_update_batch_device(S.hfb, [w.req], 16)
    with pytest.raises(RuntimeError, match="exactly one"):
        S.afb.ipa_client_update_batch_device(short, [w.req], 16)
    bn = mx.FixedBase("bn254", common.synth_points(NCOLS), NCOLS, 8)
    with pytest.raises(RuntimeError, match="secp256k1"):
        bn.ipa_client_update_batch_device(S.hfb, [w.req], 16)
    with pytest.raises(RuntimeError, match="secp256k1"):
        S.afb.ipa_client_update_batch_device(bn, [w.req], 16)
    assert _host(w.mac) == bytes(64) and _host(w.comp) == bytes(128)               # nothing was written

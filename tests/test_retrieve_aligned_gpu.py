"""GPU box: the aligned verified retrieval (porla_{kzg,ipa}_retrieve_aligned_batch_device and their host forms) -- every stored row
of ANY half checked against its MAC row and its alignment row, status_j = (stored MAC == E_j - alpha A_j), then the data decode in
the call's form -- against porla_*_retrieve_batch_device where the alignments are at infinity (byte for byte), against the Python
model tests/retrieve_aligned_model.py on residue halves of 64- and 32-byte rows, on chosen alignment points, and in the flow the call
exists for: seven writes through the client and server update batches, then the rebuild write, every half of every level retrieved on
the same stream.  Every comparison is byte equality; a 256-byte guard behind every output keeps its sentinel.

The aligned compare kernel (retrieve_batch.hip.h: k_rt_compare_aligned) takes RT_ALIGNED_ROWS = MACQ_BF = 64 rows per block of 256
lanes, a quad of lanes per row: BLOCK_ROWS below."""
import functools
import random

import pytest

from tests import common  # noqa: F401  (puts oracle/ on the path)
import icc_py
from tests import mac_decode_model as mdm
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model
from tests import test_retrieve_gpu as tr

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
SENTINEL, GUARD, IPA_COLS = tr.SENTINEL, tr.GUARD, tr.IPA_COLS
BLOCK_ROWS = 64
IPA_ALPHA = 0x6a09e667f3bcc908b2fb1366ea957d3e3adec17512775099da2f590b0667322a
P = icc_py.P_ICC
_dev, _host = tr._dev, tr._host


class Setup(tr.Setup):
    """the exact call's setup with the aligned call beside it; the key carries alpha (IPA: any scalar serves -- the generators are
    alpha^-1 times the alpha generators, whatever they are, and the call never sees them)"""

    def __init__(self, curve, ncols=128):
        from porla_amd import multiexp as mx
        super().__init__(curve, ncols)
        if curve == "bn254":
            self.aligned = lambda reqs, n_rows, n_total, form, stream=0: mx.kzg_retrieve_aligned_batch_device(reqs, n_rows, n_total, form, stream)
            self.aligned_host = lambda rows, macs, prf, n_rows, n_total, form, **kw: mx.kzg_retrieve_aligned_host(rows, macs, prf, n_rows, n_total,
                                                                                                             form, **kw)
        else:
            _, afb, hfb = tr.ipa_bases()
            self.key = dict(self.key, alpha=IPA_ALPHA)
            self.aligned = lambda reqs, n_rows, n_total, form, stream=0: afb.ipa_retrieve_aligned_batch_device(hfb, IPA_ALPHA, reqs, n_rows,
                                                                                                         n_total, form, stream)
            self.aligned_host = lambda rows, macs, prf, n_rows, n_total, form, **kw: afb.ipa_retrieve_aligned_host(hfb, IPA_ALPHA, rows, macs, prf,
                                                                                                              n_rows, n_total, form, **kw)

    def alpha_times(self, align):
        """alpha A_j from the alignments' logarithms (None = infinity): one full multiplication, alpha G, then short ones"""
        aG = icc_py.ec_mul(self.curve, mdm.GEN[self.curve], self.key["alpha"])
        return [icc_py.ec_mul(self.curve, aG, a) if a else None for a in align]

    def expected_aligned(self, commits, prf, align):
        neg = [icc_py.ec_neg(self.curve, p) if p is not None else None for p in self.alpha_times(align)]
        return [icc_py.ec_add(self.curve, e, n) for e, n in zip(self.expected(commits, prf), neg)]


def run(S, items, n_rows, n_total, form, stream=None, want_out=True, want_counts=True, call=None):
    """one aligned call.  items: (rows bytes, macs bytes, prf bytes, align bytes or None, write steps or None) per request.  Returns per
    request (status bytes, [counts] or None, blocks or None); the guards behind every output are checked."""
    import torch
    k, ncols = len(items), S.ncols
    out_b = n_rows * ncols * 32
    ins = [tuple(_dev(b) if b is not None else None for b in it[:4]) for it in items]
    steps = [torch.tensor(it[4], dtype=torch.int64).cuda() if it[4] is not None else None for it in items]
    outs = [torch.full((out_b + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") if want_out else None for _ in range(k)]
    sts = [torch.full((n_rows + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(k)]
    cns = [torch.full((8 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") if want_counts else None for _ in range(k)]
    ptr = lambda t: t.data_ptr() if t is not None else 0
    reqs = [(ptr(ins[a][0]), ptr(ins[a][1]), ptr(ins[a][2]), ptr(ins[a][3]), ptr(steps[a]), ptr(outs[a]), ptr(sts[a]), ptr(cns[a])) for a in range(k)]
    torch.cuda.synchronize()
    (call or S.aligned)(reqs, n_rows, n_total, form, stream.cuda_stream if stream is not None else 0)
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


def stand_alone_decode(rows_b, n_rows, ncols, n_total, curve, form, steps=None):
    from porla_amd import icc
    return icc.decode_host(rows_b, n_rows, ncols, n_total, curve, form, steps)[0]


# ---- 1. the exact call is a special case
@pytest.mark.parametrize("curve,n_rows,n_total,ncols", [("bn254", 2, 2, 8), ("bn254", 4, 4, 9), ("bn254", 64, 64, 128), ("secp256k1", 2, 2, 128),
                                                        ("secp256k1", 64, 64, 128)])
def test_without_alignments_the_call_is_the_exact_call(curve, n_rows, n_total, ncols):
    """form exact with d_align NULL (k_rt_compare itself) and with d_align = n_rows x 64 zero bytes (the aligned compare's block skip): status,
    blocks and both counters are byte for byte the exact call's on the same inputs, one MAC row swapped for its neighbour"""
    S = Setup(curve, ncols)
    L = tr.coded_level(curve, n_rows, ncols)
    macs = bytearray(model.points_to_bytes(S.expected(L.commits, L.prf)))
    macs[64:128] = macs[:64]
    old, = tr.run(S, [(L.rows_b, bytes(macs), L.prf_b)], n_rows, n_total)
    assert old[0] == bytes([1, 0] + [1] * (n_rows - 2)) and old[1][0] == 1
    for align in (None, bytes(64 * n_rows)):
        new, = run(S, [(L.rows_b, bytes(macs), L.prf_b, align, None)], n_rows, n_total, "exact")
        assert new == old, "d_align %s" % ("NULL" if align is None else "all infinity")


# ---- 2. statuses equal the model on residue halves
@functools.lru_cache(maxsize=None)
def residue_level(curve, n_rows, ncols, form, seed=0):
    """random stored rows of the form's width (below LCM / below p_icc), random 128-bit PRF values, alignments a_j G with a_j below
    2^40 and one row at infinity in the middle: computed once, shared, left unchanged.  Returns (tr.Level-like pieces, align logs)"""
    rng = random.Random(9000 + 131 * n_rows + ncols + 7 * seed + (form == "residue32"))
    bound = P if form == "residue32" else icc_py.LCM[curve]
    rows = [[rng.randrange(bound) for _ in range(ncols)] for _ in range(n_rows)]
    prf = [rng.getrandbits(128) for _ in range(n_rows)]
    commits = [model.alpha_commit(r, tr.commit_key(curve)) for r in rows]
    logs = [rng.randrange(1, 1 << 40) for _ in range(n_rows)]
    logs[n_rows // 2] = 0
    align_b = model.points_to_bytes([icc_py.ec_mul(curve, mdm.GEN[curve], a) if a else None for a in logs])
    return rows, am.rows_bytes(rows, form), prf, model.prf_bytes(curve, prf), commits, logs, align_b


RESIDUE_SHAPES = [("bn254", 2, 2, 8, "residue32"), ("bn254", 4, 4, 9, "residue32"), ("bn254", 4, 4, 9, "residue64"), ("bn254", 2, 2, 128, "residue32"),
                  ("bn254", 2, 2, 1024, "residue32"), ("bn254", 2, 2, 1032, "residue32"), ("bn254", 2, 2, 1032, "residue64"),
                  ("bn254", 4, 8, 128, "residue64"), ("bn254", BLOCK_ROWS // 2, BLOCK_ROWS // 2, 128, "residue64"),
                  ("bn254", 2 * BLOCK_ROWS, 2 * BLOCK_ROWS, 128, "residue32"),
                  ("secp256k1", 2, 2, 128, "residue64"), ("secp256k1", 4, 8, 128, "residue32"),
                  ("secp256k1", BLOCK_ROWS // 2, BLOCK_ROWS // 2, 128, "residue32"), ("secp256k1", 2 * BLOCK_ROWS, 2 * BLOCK_ROWS, 128, "residue64")]


@pytest.mark.parametrize("curve,n_rows,n_total,ncols,form", RESIDUE_SHAPES)
def test_statuses_equal_the_model_on_residue_halves(curve, n_rows, n_total, ncols, form):
    """KZG SRS sizes 8 and 9 (a ragged eight-lane step), 128, 1024 (the largest LDS table) and 1032 (the Horner path) in the 32-byte width;
    row counts 2, 4, BLOCK_ROWS / 2 and 2 * BLOCK_ROWS (n_rows is a power of two: the powers below and above the kernel's 64 rows per
    block), n_total above n_rows once per build.  The MAC rows are the model's E_j - alpha A_j, one replaced by its neighbour; the blocks
    are the stand-alone decode's of the same rows, form and write steps"""
    S = Setup(curve, ncols)
    rows, rows_b, prf, prf_b, commits, logs, align_b = residue_level(curve, n_rows, ncols, form)
    want_pts = S.expected_aligned(commits, prf, logs)
    if n_rows <= 4:                                                # (the short way through the logarithms is the model's relation)
        assert want_pts == am.expected_macs_aligned(rows, prf, mdm.bytes_to_points(align_b, curve), S.key)
    want_macs = model.points_to_bytes(want_pts)
    macs = bytearray(want_macs)
    macs[64:128] = want_macs[:64]
    want = am.statuses_of(want_pts, bytes(macs))
    assert want == bytes([1, 0] + [1] * (n_rows - 2))
    steps = [n_total + 1 + 3 * j for j in range(n_rows)] if n_rows == 4 else None
    (st, counts, out), = run(S, [(rows_b, bytes(macs), prf_b, align_b, steps)], n_rows, n_total, form)
    assert st == want
    assert counts == [1, 0]
    assert out == stand_alone_decode(rows_b, n_rows, ncols, n_total, curve, form, steps)
    # without the alignment store the finite rows fail: the term is exercised
    (st, _, _), = run(S, [(rows_b, want_macs, prf_b, None, None)], n_rows, n_total, form, want_out=False)
    assert st == bytes(0 if a else 1 for a in logs)


# ---- 3. chosen alignment points
def commit_log(row, key):
    """e with alpha Commit(row) = e G"""
    q = icc_py.Q[key["curve"]]
    if key["curve"] == "bn254":
        e = 0
        for c in reversed(row):
            e = (e * key["tau"] + c) % q
        return e * key["alpha"] % q
    return sum(c * d for c, d in zip(row, key["dlogs"])) % q


@pytest.mark.parametrize("curve", CURVES)
def test_chosen_alignment_points(curve):
    """n_rows = 4, PRF values 0 (KZG's h has no known logarithm), E_j = e_j G.  Row 0: alpha A = E, the expected MAC is infinity and 64
    zero bytes are OK.  Row 1: alpha A = -E, the subtraction is a doubling.  Row 2: A = infinity between finite neighbours of the same
    block.  Row 3: A with x + p in its bytes, read reduced like the other stores.  Then row 2's A replaced by bytes that are no point of
    the curve: status 0 on that row alone, no fault, the guards intact (run checks them)."""
    from tests import ec_vectors as ev
    from tests import mac_decode_vectors as mv
    n, ncols, form = 4, 128, "residue64"
    S = Setup(curve, ncols)
    q, G, alpha = icc_py.Q[curve], mdm.GEN[curve], S.key["alpha"]
    rows, rows_b, _, _, commits, _, _ = residue_level(curve, n, ncols, form, seed=3)
    prf = [0] * n
    prf_b = model.prf_bytes(curve, prf)
    e = [commit_log(r, S.key) for r in rows]
    assert [icc_py.ec_mul(curve, G, x) for x in e] == commits
    inv = pow(alpha, -1, q)
    raw, pt = mv.noncanonical_bytes(ev.CURVES[curve])
    a0, a1 = icc_py.ec_mul(curve, G, e[0] * inv % q), icc_py.ec_mul(curve, G, (q - e[1]) * inv % q)
    align_b = model.point_bytes(a0) + model.point_bytes(a1) + bytes(64) + raw
    want = [None, icc_py.ec_mul(curve, G, 2 * e[1] % q), commits[2],
            icc_py.ec_add(curve, commits[3], icc_py.ec_neg(curve, icc_py.ec_mul(curve, pt, alpha)))]
    macs = model.points_to_bytes(want)
    assert macs[:64] == bytes(64)
    assert want == am.expected_macs_aligned(rows, prf, [a0, a1, None, pt], S.key)
    (st, counts, out), = run(S, [(rows_b, macs, prf_b, align_b, None)], n, n, form)
    assert st == bytes([1] * n) and counts == [0, 0]
    assert out == stand_alone_decode(rows_b, n, ncols, n, curve, form)
    # the canonical bytes of the same A in row 3 give the same answer; a nonzero MAC row 0 is not OK
    canon = align_b[:192] + model.point_bytes(pt)
    bad0 = model.point_bytes(commits[0]) + macs[64:]
    got = run(S, [(rows_b, macs, prf_b, canon, None), (rows_b, bad0, prf_b, align_b, None)], n, n, form, want_out=False)
    assert got[0][0] == bytes([1] * n) and got[1][0] == bytes([0, 1, 1, 1]) and got[1][1] == [1, 0]
    # no point of the curve
    assert not ev.on_curve(ev.CURVES[curve], (5, 7))
    garbage = align_b[:128] + (5).to_bytes(32, "big") + (7).to_bytes(32, "big") + align_b[192:]
    (st, counts, _), = run(S, [(rows_b, macs, prf_b, garbage, None)], n, n, form, want_out=False)
    assert st == bytes([1, 1, 0, 1]) and counts == [1, 0]


# ---- 4. the flow: seven writes through the client and the server update batch, then the rebuild write, one stream
def raw_prf(curve, values):
    return b"".join(model.prf_raw(curve, v) for v in values)


class Flow:
    """a file of n_total = 8 blocks in HBM: writes 1 .. 7 through porla_*_client_update_batch_device -> porla_*_update_batch_device, all on
    one stream.  What the host keeps is what a client keeps: the PRF values every resident row is hidden with, and the write steps"""

    def __init__(self, curve, stream, seed=4100):
        import torch
        from porla_amd import multiexp as mx
        from tests import test_client_update_batch_gpu as cu, test_update_batch_gpu as ub
        from tests.client_update_model import n_prf
        from tests.update_model import FAMILIES, FileModel
        self.curve, self.n, self.ncols = curve, 8, 128
        self.C = C = cu.setup_of(curve)
        if curve == "bn254":                                      # the key, SRS and hiding point are process state: put ours in again
            mx.init_key(ub.TAU, ub.ALPHA)
            mx.init_SRS_from_data(self.ncols, mx.init_SRS(self.ncols))
        rnd = random.Random(seed)
        shape = FileModel(self.n, self.ncols, curve, C.server.base, fill=SENTINEL)
        self.d = ub.DevFile(shape)                                # every level of the six families, pre-filled with the sentinel
        self.hold, self.blocks, self.keep = {}, {}, []
        for step in range(1, self.n):
            level = (step & -step).bit_length() - 1
            chunks = [rnd.getrandbits(256) for _ in range(self.ncols)]
            self.blocks[step] = chunks
            new_x, new_y = ([rnd.getrandbits(128) for _ in range(1 << level)] for _ in range(2))
            prf = [rnd.getrandbits(128)]
            for i in range(level):
                prf += self.hold[i][0] + self.hold[i][1]
                del self.hold[i]
            prf += new_x + new_y
            assert len(prf) == n_prf(level)
            self.hold[level] = (new_x, new_y, list(range(step - (1 << level) + 1, step + 1)))
            d_block, d_prf = _dev(b"".join(c.to_bytes(32, "little") for c in chunks)), _dev(raw_prf(curve, prf))
            d_mac = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
            d_comp = torch.full((64 * (2 << level),), SENTINEL, dtype=torch.uint8, device="cuda")
            self.keep += [d_block, d_prf, d_mac, d_comp]
            torch.cuda.synchronize()                              # (the uploads are torch's; the calls below wait for nothing)
            C.call([(d_block.data_ptr(), d_prf.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), step, level)], self.n, stream.cuda_stream)
            C.server.call([(d_block.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), step, level) +
                           tuple([t.data_ptr() for t in self.d.t[f][:level + 1]] for f in FAMILIES)], self.n, stream.cuda_stream)
        self.S = Setup.__new__(Setup)                              # the retrieval calls on this state (no second init of the KZG state)
        self.S.curve, self.S.ncols = curve, self.ncols
        if curve == "bn254":
            self.S.aligned = lambda reqs, n_rows, n_total, form, s=0: mx.kzg_retrieve_aligned_batch_device(reqs, n_rows, n_total, form, s)
            self.exact = lambda reqs, n_rows, n_total, s=0: mx.kzg_retrieve_batch_device(reqs, n_rows, n_total, s)
        else:
            self.S.aligned = lambda reqs, n_rows, n_total, form, s=0: C.afb.ipa_retrieve_aligned_batch_device(C.hfb, C.alpha, reqs, n_rows, n_total,
                                                                                                            form, s)
            self.exact = lambda reqs, n_rows, n_total, s=0: C.afb.ipa_retrieve_batch_device(C.hfb, reqs, n_rows, n_total, s)

    def half(self, level, part):
        """(rows, macs, align) device tensors of the resident half, its PRF values, its blocks' write steps and the blocks"""
        n = 1 << level
        new_x, new_y, steps = self.hold[level]
        t = lambda f, row: self.d.t[f + "_" + part][level][:n * row]
        return t("data", 64 * self.ncols), t("mac", 64), t("align", 64), new_x if part == "x" else new_y, steps


def retrieve_half(F, rows, macs, prf, align, steps, n_rows, form, stream, call=None, want_out=True):
    """the aligned call (or the exact one: call = F.exact) on device tensors, on `stream`: (status, counts, blocks)"""
    import torch
    out_b = n_rows * F.ncols * 32
    d_prf = _dev(raw_prf(F.curve, prf)) if not hasattr(prf, "is_cuda") else prf
    d_steps = torch.tensor(steps, dtype=torch.int64).cuda() if steps is not None else None
    out = torch.full((out_b + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.full((n_rows + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    cn = torch.full((8 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if call is None:
        F.S.aligned([(rows.data_ptr(), macs.data_ptr(), d_prf.data_ptr(), align.data_ptr() if align is not None else 0,
                      d_steps.data_ptr() if d_steps is not None else 0, out.data_ptr() if want_out else 0, st.data_ptr(), cn.data_ptr())],
                    n_rows, F.n, form, stream.cuda_stream)
    else:
        call([(rows.data_ptr(), macs.data_ptr(), d_prf.data_ptr(), out.data_ptr() if want_out else 0, st.data_ptr(), cn.data_ptr())], n_rows, F.n,
             stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.all(st[n_rows:] == SENTINEL)) and bool(torch.all(out[out_b:] == SENTINEL)) and bool(torch.all(cn[8:] == SENTINEL))
    return _host(st[:n_rows]), list(cn[:8].cpu().view(torch.int32).tolist()), _host(out[:out_b])


def chunk_bytes(blocks, mod=None):
    return b"".join((c % mod if mod else c).to_bytes(32, "little") for chunks in blocks for c in chunks)


@pytest.mark.parametrize("curve", CURVES)
def test_every_half_of_a_written_file_checks_clean(curve):
    """after the seventh write levels 0, 1 and 2 are resident: every X half (exact) and every Y half (residue64, the blocks' write steps,
    the half's alignment store) is all OK, X decodes to the written blocks and Y to the chunks mod p_icc.  The exact call on the Y half
    gives 0 on every row whose alignment is finite -- the gap the aligned call closes -- and there is such a row in every Y half"""
    import torch
    stream = torch.cuda.Stream()
    F = Flow(curve, stream)
    assert sorted(F.hold) == [0, 1, 2]
    for level in (0, 1, 2):
        n = 1 << level
        if n < 2:
            continue                                               # (one row: below the call's smallest level)
        for part, form in (("x", "exact"), ("y", "residue64")):
            rows, macs, align, prf, steps = F.half(level, part)
            blocks = [F.blocks[s] for s in steps]
            st, counts, out = retrieve_half(F, rows, macs, prf, align, steps if part == "y" else None, n, form, stream)
            assert st == bytes([1] * n), "level %d %s" % (level, part)
            assert counts == [0, 0]
            assert out == chunk_bytes(blocks, None if part == "x" else P), "level %d %s does not decode to its blocks" % (level, part)
            finite = [_host(align[64 * j:64 * j + 64]) != bytes(64) for j in range(n)]
            st_old, _, _ = retrieve_half(F, rows, macs, prf, None, None, n, None, stream, call=F.exact, want_out=False)
            assert st_old == bytes(0 if f else 1 for f in finite), "level %d %s: the exact call" % (level, part)
            assert any(finite) == (part == "y")


@pytest.mark.parametrize("curve", CURVES)
def test_the_aligned_top_level_checks_clean(curve):
    """one client rebuild batch, then the aligned server rebuild batch, at n_total = 4, then the top level's X and Y halves with
    residue32 on the same stream: all rows OK, the blocks are the chunks mod p_icc (X; Y with the write's step as every block's)"""
    import torch
    from porla_amd import multiexp as mx
    from tests import test_client_rebuild_batch_gpu as cr, test_server_rebuild_aligned_batch_gpu as sra, test_update_batch_gpu as ub
    from tests.client_rebuild_model import n_prf
    from tests.update_model import FAMILIES, pt_bytes
    n, ncols, index, step = 4, 128, 3, 4 + 1
    sra.server_of(curve)
    C, client_call = cr.setup_of(curve)
    h = C.h
    if curve == "bn254":
        from tests.update_model import pt_tuple
        h = pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))
    rnd = random.Random(4400)
    u = [[rnd.getrandbits(256) for _ in range(ncols)] for _ in range(n)]
    block = [rnd.getrandbits(256) for _ in range(ncols)]
    prf = [rnd.getrandbits(128) for _ in range(n_prf(n))]
    prf[index] = prf[0]                                                       # complements_U of the written slot is the block's own
    old, new_x, new_y = prf[1:1 + n], prf[1 + n:1 + 2 * n], prf[1 + 2 * n:]
    u_macs = [None if i == index - 1 else icc_py.ec_add(curve, C.block_commit(u[i]), icc_py.ec_mul(curve, h, old[i])) for i in range(n)]
    d = sra.DevFile(n, b"".join(sra.block_bytes(c) for c in u), b"".join(pt_bytes(p) for p in u_macs))
    d_block, d_prf = _dev(sra.block_bytes(block)), _dev(raw_prf(curve, prf))
    d_mac = torch.full((64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_comp = torch.full((128 * n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    client_call([(d_block.data_ptr(), d_prf.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), step)], n, stream.cuda_stream)
    sra.call(curve, [d.req(d_block, d_mac, d_comp, step, index)], n, stream.cuda_stream)
    F = Flow.__new__(Flow)
    F.curve, F.n, F.ncols = curve, n, ncols
    F.S = Setup.__new__(Setup)
    if curve == "bn254":
        F.S.aligned = lambda reqs, n_rows, n_total, form, s=0: mx.kzg_retrieve_aligned_batch_device(reqs, n_rows, n_total, form, s)
    else:
        F.S.aligned = lambda reqs, n_rows, n_total, form, s=0: C.afb.ipa_retrieve_aligned_batch_device(C.hfb, C.alpha, reqs, n_rows, n_total, form, s)
    u[index - 1] = block
    finite = 0
    for part, new in (("x", new_x), ("y", new_y)):
        rows, macs, align = d.t["data_" + part][:n * ncols * 32], d.t["mac_" + part][:64 * n], d.t["align_" + part][:64 * n]
        st, counts, out = retrieve_half(F, rows, macs, new, align, [step] * n if part == "y" else None, n, "residue32", stream)
        assert st == bytes([1] * n), part
        assert counts == [0, 0]
        assert out == chunk_bytes(u, P), "data_%s does not decode to U mod p_icc" % part
        finite += sum(_host(align[64 * j:64 * j + 64]) != bytes(64) for j in range(n))
    assert finite > 0 and FAMILIES


# ---- 5. the tamper sweep on one Y half of that flow
@pytest.mark.parametrize("curve", CURVES)
def test_tamper_sweep_on_a_y_half(curve):
    """level 2's Y half (4 rows) after the seven writes: one bit in one symbol, in one MAC row, in one alignment row and in one PRF value
    each fail exactly their row, d_counts[0] counts them, and the decode still runs (the blocks are the stand-alone decode's)"""
    import torch
    stream = torch.cuda.Stream()
    F = Flow(curve, stream)
    n, level = 4, 2
    rows, macs, align, prf, steps = F.half(level, "y")
    stream.synchronize()
    only = lambda *js: bytes(0 if i in js else 1 for i in range(n))

    def flipped(t, byte, bit):
        c = t.clone()
        c[byte] ^= bit
        return c

    prf_b = bytearray(raw_prf(curve, prf))
    prf_b[16 * 2 + 5] ^= 0x20
    cases = [((rows, macs, prf, align), only()),
             ((flipped(rows, 64 * (1 * F.ncols + 77) + 3, 1), macs, prf, align), only(1)),
             ((rows, flipped(macs, 64 * 3 + 40, 0x80), prf, align), only(3)),
             ((rows, macs, prf, flipped(align, 64 * 0 + 63, 2)), only(0)),
             ((rows, macs, _dev(bytes(prf_b)), align), only(2)),
             ((flipped(rows, 64 * (1 * F.ncols + 77) + 3, 1), flipped(macs, 64 * 3 + 40, 0x80), prf, align), only(1, 3))]
    for a, ((r, m, p, al), want) in enumerate(cases):
        st, counts, out = retrieve_half(F, r, m, p, al, steps, n, "residue64", stream)
        assert st == want, "case %d" % a
        assert counts == [want.count(0), 0], "case %d" % a
        assert out == stand_alone_decode(_host(r), n, F.ncols, F.n, curve, "residue64", steps), "case %d" % a


# ---- 6. K and streams
def sixteen_rows(S, curve, form, seed):
    rows, rows_b, prf, prf_b, commits, logs, align_b = residue_level(curve, 16, 128, form, seed)
    return rows_b, model.points_to_bytes(S.expected_aligned(commits, prf, logs)), prf_b, align_b, model.points_to_bytes(S.expected(commits, prf))


@pytest.mark.parametrize("curve", CURVES)
def test_three_requests_one_tampered_one_without_alignments(curve):
    """16 rows a request: one block of the aligned compare holds the rows of all three.  The first request has no d_align (its MAC rows are
    the E_j), the middle one has a flipped symbol; every request gives what it gives alone"""
    import torch
    form = "residue64"
    S = Setup(curve)
    lv = [sixteen_rows(S, curve, form, seed) for seed in (0, 1, 2)]
    mid = bytearray(lv[1][0])
    mid[64 * (11 * 128 + 127) + 63 - 8] ^= 0x40
    items = [(lv[0][0], lv[0][4], lv[0][2], None, None), (bytes(mid), lv[1][1], lv[1][2], lv[1][3], None), (lv[2][0], lv[2][1], lv[2][2], lv[2][3], None)]
    got = run(S, items, 16, 16, form, stream=torch.cuda.Stream())
    for a in range(3):
        assert got[a] == run(S, [items[a]], 16, 16, form)[0], "request %d against its single call" % a
    assert got[0][0] == got[2][0] == bytes([1] * 16)
    assert got[1][0] == bytes(0 if i == 11 else 1 for i in range(16)) and got[1][1] == [1, 0]


@pytest.mark.parametrize("curve", CURVES)
def test_two_streams_host_form_and_optional_outputs(curve):
    import torch
    form, n = "residue32", 16
    S = Setup(curve)
    rows_b, macs, prf_b, align_b, _ = sixteen_rows(S, curve, form, 0)
    bad = bytearray(macs)
    bad[64 * 6 + 40] ^= 0x80
    steps = [17 + j for j in range(n)]
    item = (rows_b, bytes(bad), prf_b, align_b, steps)
    want = bytes(0 if i == 6 else 1 for i in range(n))
    blocks = stand_alone_decode(rows_b, n, 128, 32, curve, form, steps)
    blocks64 = stand_alone_decode(rows_b, n, 128, 64, curve, form, steps)         # (the unscale by the write steps depends on n_total)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = run(S, [item] * 2, n, 32, form, stream=s1)
    second = run(S, [item] * 3, n, 64, form, stream=s2)
    third = run(S, [item], n, 32, form, stream=s1)
    for res in first + third:
        assert res == (want, [1, 0], blocks)
    for res in second:
        assert res == (want, [1, 0], blocks64)
    # the host form
    kw = dict(align=align_b, write_steps=steps)
    assert S.aligned_host(rows_b, bytes(bad), prf_b, n, 32, form, **kw) == (want, [1, 0], blocks)
    assert S.aligned_host(rows_b, bytes(bad), prf_b, n, 32, form, want_blocks=False, **kw) == (want, [1, 0], None)
    e_macs = sixteen_rows(S, curve, form, 0)[4]
    assert S.aligned_host(rows_b, e_macs, prf_b, n, 32, form)[0] == bytes([1] * n)                       # align None: the E_j themselves
    # optional outputs
    (st, counts, out), = run(S, [item], n, 32, form, want_out=False)
    assert st == want and counts == [1, 0] and out is None
    (st, counts, out), = run(S, [item], n, 32, form, want_counts=False)
    assert st == want and counts is None and out == blocks
    (st, _, _), = run(S, [item], n, 32, form, want_out=False, want_counts=False)
    assert st == want


def test_ipa_rows_beyond_one_workspace_group_with_32_byte_rows():
    """K = 3 levels of 2^15 rows of 32-byte symbols share their inputs: the second group of the IPA build's coefficient workspace (2^16
    rows) starts inside request 2.  Every row's alignment is the same finite point A, so the expected MACs come from the device's own
    fixed-base commit over the 128 alpha generators, h and -alpha A (coefficient 1); symbols below 2^248 < p_icc, so sym mod n = sym"""
    import torch
    from porla_amd import multiexp as mx
    n, ncols, k = 1 << 15, IPA_COLS, 3
    key, afb, hfb = tr.ipa_bases()
    c, G = "secp256k1", mdm.GEN["secp256k1"]
    A = icc_py.ec_mul(c, G, 0xabcdef12345)
    minus = icc_py.ec_neg(c, icc_py.ec_mul(c, A, IPA_ALPHA))
    three = mx.FixedBase(c, model.points_to_bytes(key["alpha_generators"] + [key["h"], minus]), ncols + 2, window_bits=8)
    g = torch.Generator(device="cuda")
    g.manual_seed(12)
    rows = torch.randint(0, 256, (n * ncols, 32), dtype=torch.uint8, device="cuda", generator=g)
    rows[:, 31] = 0
    prf = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=g)            # r.d[0], r.d[1]: little-endian
    one = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    one[:, 31] = 1
    coeffs = torch.cat([rows.flip(1).reshape(n, ncols * 32), torch.zeros((n, 16), dtype=torch.uint8, device="cuda"), prf.flip(1), one], dim=1).contiguous()
    macs = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    three.commit_device(coeffs.data_ptr(), n, ncols + 2, macs.data_ptr())
    align = _dev(model.point_bytes(A)).repeat(n)
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
    afb.ipa_retrieve_aligned_batch_device(hfb, IPA_ALPHA, [(rows.data_ptr(), macs_of[a].data_ptr(), prf.data_ptr(), align.data_ptr(), 0, 0,
                                                            sts[a].data_ptr(), cns[a].data_ptr()) for a in range(k)], n, n, "residue32")
    torch.cuda.synchronize()
    for a in range(k):
        want = torch.ones(n, dtype=torch.uint8, device="cuda")
        want[tampered[a]] = 0
        assert torch.equal(sts[a][:n], want), "request %d" % a
        assert bool(torch.all(sts[a][n:] == SENTINEL)) and cns[a].tolist() == [1, 0], "request %d" % a

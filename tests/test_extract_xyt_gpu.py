"""GPU box: the file extraction with the top level's Y half (porla_{kzg,ipa}_extract_xyt_batch_device) -- a top level with damaged X
rows is rebuilt row by row from wt^-1 times its Y rows and decoded once -- against the Python model tests/extract_xyt_model.py (every
output byte, the patched half included), against the extraction with the lower levels' Y halves on the same stores, and in the flow the
call exists for: a top level left by a rebuild write with BOTH halves kept, then up to seven writes through the client and server update
batches on one stream.  Every comparison is byte equality; every output is pre-filled with a sentinel and a 256-byte guard behind it
keeps it.

The KZG build draws its hiding base anew at every init_SRS, so every test builds its own file and installs no key after that."""
import functools
import random
import types

import pytest

from tests import common  # noqa: F401  (puts oracle/ on the path)
import icc_py
from tests import extract_model as em
from tests import extract_xy_model as xm
from tests import extract_xyt_model as tm
from tests import retrieve_model as model
from tests import test_extract_gpu as te
from tests import test_extract_xy_gpu as txy
from tests import test_retrieve_aligned_gpu as ta
from tests import test_retrieve_gpu as tr

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
FORMS = ["exact", "residue32"]
SENTINEL, GUARD = tr.SENTINEL, tr.GUARD
_dev, _host = tr._dev, tr._host
N, NCOLS = te.N, te.NCOLS
P = xm.P
ALL = txy.ALL
flipped = txy.flipped
SYMB = {"exact": 64, "residue32": 32}


def xyt_call_of(curve, afb=None, hfb=None, alpha=None):
    from porla_amd import multiexp as mx
    if curve == "bn254":
        return lambda reqs, n, form, s=0: mx.kzg_extract_xyt_batch_device(reqs, n, form, s)
    return lambda reqs, n, form, s=0: afb.ipa_extract_xyt_batch_device(hfb, alpha, reqs, n, form, s)


class XytFlow(txy.XyFlow):
    """txy.XyFlow whose rebuild keeps the top level's Y half too -- top_y = (data_y, mac_y, the client's new-Y PRF values prf[1 + 2n :
    1 + 3n], align_y or None) -- and may run at any write step (`step`: wt = 1 iff it is a multiple of n) and n_total (`n`, with no
    writes after it).  file(t)["top_y"] / ["top_step"] go with every file"""

    def __init__(self, curve, stream, indices=txy.INDICES, top="exact", seed=5300, step=None, n=N, **kw):
        self.n_top, self.step = n, n if step is None else step
        assert n == N or not indices
        super().__init__(curve, stream, indices=indices, top=top, seed=seed, **kw)
        if curve == "bn254":
            self.xyt = xyt_call_of(curve)
        else:
            self.xyt = xyt_call_of(curve, self.C.afb, self.C.hfb, self.C.alpha)

    def _rebuild(self, top, cr):
        import torch
        from tests import test_server_rebuild_aligned_batch_gpu as sra, test_server_rebuild_batch_gpu as sr
        from tests.client_rebuild_model import n_prf
        from tests.update_model import pt_bytes
        self.n = n = self.n_top
        curve, rnd, C, step = self.curve, self.rnd, self.C, self.step
        _, client_call = cr.setup_of(curve)
        rebuilt = min(te.REBUILT, n)
        u = [te.block_of(rnd, b + 1) for b in range(n)]
        block = te.block_of(rnd, rebuilt)
        prf = [rnd.getrandbits(128) for _ in range(n_prf(n))]
        prf[rebuilt] = prf[0]                                     # complements_U of the written slot is the block's own
        old, new_x, new_y = prf[1:1 + n], prf[1 + n:1 + 2 * n], prf[1 + 2 * n:1 + 3 * n]
        u_macs = [None if i == rebuilt - 1 else icc_py.ec_add(curve, C.block_commit(u[i]), icc_py.ec_mul(curve, self.h, old[i])) for i in range(n)]
        mod = sr if top == "exact" else sra
        d = mod.DevFile(n, b"".join(sr.block_bytes(c) for c in u), b"".join(pt_bytes(p) for p in u_macs))
        d_block, d_prf = _dev(sr.block_bytes(block)), _dev(ta.raw_prf(curve, prf))
        d_mac = torch.full((64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_comp = torch.full((128 * n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.keep += [d, d_block, d_prf, d_mac, d_comp]
        torch.cuda.synchronize()
        client_call([(d_block.data_ptr(), d_prf.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), step)], n, self.stream.cuda_stream)
        req = d.req(d_block, d_mac, d_comp, step, rebuilt)
        if top == "exact":
            sr.call([req], n, curve, self.stream.cuda_stream)
        else:
            sra.call(curve, [req], n, self.stream.cuda_stream)
        self.stream.synchronize()
        u[rebuilt - 1] = block
        self.u = u
        symb = SYMB[top]
        half = lambda part, prf_part: (d.t["data_" + part][:n * NCOLS * symb].clone(), d.t["mac_" + part][:64 * n].clone(), prf_part,
                                       d.t["align_" + part][:64 * n].clone() if top != "exact" else None)
        self.top, self.top_y = half("x", new_x), half("y", new_y)

    def file(self, t, top=True, write_step=None, top_step=None):
        f = super().file(t, top, write_step)
        return dict(f, top_y=self.top_y if top else None, top_step=self.step if top_step is None else top_step)

    def u_bytes(self):
        mod = P if self.top_form == "residue32" else None
        return ta.chunk_bytes(self.u, mod)


def run_xyt(F, files, masks, tops, stream=None, call=None, n=N, ncols=NCOLS, top_form=None, null_y=False, null_top_y=False):
    """one call.  files: txy.run_xy's dictionaries with "top_y": None or (rows, MAC tensor, PRF integers, alignment tensor or None) and
    "top_step" beside them; masks: y_levels per file; tops: top_y per file.  null_y / null_top_y: every pointer of that family NULL.
    Returns a function giving, per file, the outputs as tm.extract_xyt names them; the guards behind every output are checked"""
    import torch
    logn = n.bit_length() - 1
    bb = ncols * 32
    form = top_form or F.top_form
    full = lambda size: torch.full((size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    ptr = lambda x: x.data_ptr() if x is not None else 0
    bufs, reqs, keep = [], [], []
    for f, mask, ty in zip(files, masks, tops):
        t = f["write_step"] % n
        rows = t + (n if f["top"] else 0)
        prf = [v for i in sorted(f["lower"]) for v in f["lower"][i][2]] + (f["top"][2] if f["top"] else [])
        assert len(prf) == rows and sorted(f["lower"]) == [i for i, _, _ in em.resident_levels(t, n)]
        d_prf = _dev(ta.raw_prf(F.curve, prf)) if rows else None
        sizes = {"work": t * bb, "blocks": n * bb, "steps": 4 * n, "flags": n, "row_status": rows, "counts": 32}
        if not null_y:
            sizes.update({"work_y": t * bb, "row_status_y": t})
        if not null_top_y:
            sizes.update({"top_patch": n * ncols * SYMB[form], "row_status_top_y": n})
        b = {name: full(size) for name, size in sizes.items()}
        b["sizes"] = sizes
        fam = lambda k: [ptr(f["lower"][i][k]) if i in f["lower"] else 0 for i in range(logn)] if t else None
        top = f["top"] or (None, None, None, None)
        req = (f["write_step"], fam(0), fam(1), ptr(top[0]), ptr(top[1]), ptr(top[3]), ptr(d_prf), b["work"].data_ptr() if t else 0,
               b["blocks"].data_ptr(), b["steps"].data_ptr(), b["flags"].data_ptr(), b["row_status"].data_ptr() if rows else 0,
               b["counts"].data_ptr())
        d_prf_y = d_prf_ty = None
        if null_y:
            req += (None, None, None, 0, 0, 0, mask)
        else:
            y = f["y"]
            assert sorted(y) == sorted(f["lower"])
            d_prf_y = _dev(ta.raw_prf(F.curve, [v for i in sorted(y) for v in y[i][2]])) if t else None
            famy = lambda k: [ptr(y[i][k]) if i in y else 0 for i in range(logn)]
            req += (famy(0), famy(1), famy(3), ptr(d_prf_y), b["work_y"].data_ptr() if t else 0, b["row_status_y"].data_ptr() if t else 0, mask)
        if null_top_y:
            req += (0, 0, 0, 0, 0, 0, f["top_step"], ty)
        else:
            topy = f["top_y"] or (None, None, None, None)
            d_prf_ty = _dev(ta.raw_prf(F.curve, topy[2])) if f["top_y"] else None
            req += (ptr(topy[0]), ptr(topy[1]), ptr(topy[3]), ptr(d_prf_ty), b["top_patch"].data_ptr(), b["row_status_top_y"].data_ptr(),
                    f["top_step"], ty)
        reqs.append(req)
        bufs.append(b)
        keep += [d_prf, d_prf_y, d_prf_ty]
    torch.cuda.synchronize()
    (call or F.xyt)(reqs, n, form, stream.cuda_stream if stream is not None else 0)
    return lambda: collect(bufs, tops, files, stream, n, keep)


def collect(bufs, tops, files, stream, n, keep=None):
    import torch
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res = []
    for a, b in enumerate(bufs):
        for name, size in b["sizes"].items():
            assert bool(torch.all(b[name][size:] == SENTINEL)), "file %d: the guard behind %s changed" % (a, name)
        cut = lambda name: _host(b[name][:b["sizes"][name]])
        tried = tops[a] == 1 and files[a]["top"] is not None
        if "top_patch" in b and not tried:                        # an untried half leaves its scratch alone
            assert bool(torch.all(b["top_patch"] == SENTINEL)), "file %d: d_top_patch written without a half to try" % a
        res.append({"blocks": cut("blocks"), "steps": [s & 0xffffffff for s in b["steps"][:4 * n].cpu().view(torch.int32).tolist()],
                    "flags": cut("flags"), "row_status": cut("row_status"),
                    "row_status_y": cut("row_status_y") if "row_status_y" in b else None,
                    "row_status_top_y": cut("row_status_top_y") if "row_status_top_y" in b else None,
                    "top_patch": cut("top_patch") if "top_patch" in b and tried else None,
                    "counts": b["counts"][:32].cpu().view(torch.int32).tolist()})
    return res


def extract_xyt(F, files, masks, tops, **kw):
    return run_xyt(F, files, masks, tops, **kw)()


def model_of(F, f, mask, ty, statuses, status_y, status_top_y, n=N, ncols=NCOLS, top_form=None):
    """tm.extract_xyt on the stores as they lie on the device, the row statuses of all halves given"""
    lower = {i: (_host(d[:(1 << i) * ncols * 64]), _host(m[:64 << i]), prf) for i, (d, m, prf) in f["lower"].items()}
    y = {i: (_host(d[:(1 << i) * ncols * 64]), _host(m[:64 << i]), prf, _host(a[:64 << i]) if a is not None else None)
         for i, (d, m, prf, a) in f["y"].items()}
    host = lambda h: (_host(h[0]), _host(h[1]), h[2], _host(h[3]) if h[3] is not None else None) if h else None
    form = top_form or F.top_form
    return tm.extract_xyt(em.File(n, ncols, F.curve, f["write_step"], lower, host(f["top"]), form), y, mask, host(f["top_y"]), f["top_step"],
                          ty, statuses=statuses, status_y=status_y, status_top_y=status_top_y)


def as_xy(got):
    """the outputs the call without the top level's Y half has"""
    return {"blocks": got["blocks"], "steps": got["steps"], "flags": got["flags"], "row_status": got["row_status"],
            "row_status_y": got["row_status_y"], "counts": got["counts"][:6]}


def with_top(f, **kw):
    """f with the top level's X half (data=, macs=) or Y half (data_y=, macs_y=, prf_y=, align_y=) replaced"""
    d, m, p, a = f["top"]
    dy, my, py, ay = f["top_y"]
    return dict(f, top=(kw.get("data", d), kw.get("macs", m), p, a),
                top_y=(kw.get("data_y", dy), kw.get("macs_y", my), kw.get("prf_y", py), kw.get("align_y", ay)))


def top_statuses(t, rows_bad, n=N):
    return bytes([1] * t) + bytes(0 if j in rows_bad else 1 for j in range(n))


def top_won(form):
    return xm.FOUND | xm.FROM_Y | (xm.RESIDUE if form == "residue32" else 0)


# ---- 1. top_y = 0: the call with the lower levels' Y halves
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_without_the_top_y_half_the_call_is_the_xy_call(curve, form):
    """top_y = 0 and NULL new pointers, t = 0 .. 7: every output and counts[0 .. 5] are porla_*_extract_xy_batch_device's on the same
    stores, also under a damaged lower level and a damaged top level; with the pointers given the statuses say NOT_TRIED"""
    import torch
    F = XytFlow(curve, torch.cuda.Stream(), top=form)
    for t in range(0, 8):
        f = F.file(t)
        got, = extract_xyt(F, [f], [ALL], [0], stream=F.stream, null_top_y=True)
        want, = txy.extract_xy(F, [f], [ALL], stream=F.stream)
        assert as_xy(got) == want and got["counts"][6:] == [0, 0], "t = %d" % t
        assert want["counts"] == [0] * 6 and want["row_status"] == bytes([1] * (t + N))
    f = F.file(7)
    g = with_top(txy.with_lower(f, 1, data=flipped(f["lower"][1][0], 64 * (NCOLS + 5) + 1)), data=flipped(f["top"][0], SYMB[form] * (3 * NCOLS + 9) + 2))
    for mask in (0, 2):
        want, = txy.extract_xy(F, [g], [mask], stream=F.stream)
        got, = extract_xyt(F, [g], [mask], [0], stream=F.stream, null_top_y=True)
        assert as_xy(got) == want and want["counts"][0] == 2 and got["counts"][6:] == [0, 0]
        got, = extract_xyt(F, [g], [mask], [0], stream=F.stream)
        assert as_xy(got) == want and got["row_status_top_y"] == bytes([xm.NOT_TRIED] * N) and got["counts"][6:] == [0, 0]
    # no top level: nothing to try whatever top_y says
    h = F.file(5, top=False, write_step=5)
    want, = txy.extract_xy(F, [h], [ALL], stream=F.stream)
    for kw in (dict(null_top_y=True), dict()):
        got, = extract_xyt(F, [h], [ALL], [1], stream=F.stream, **kw)
        assert as_xy(got) == want and got["counts"][6:] == [0, 0]
        assert got["row_status_top_y"] in (None, bytes([xm.NOT_TRIED] * N))


# ---- 2. a clean file with the top Y half tried
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_clean_file_with_the_top_y_half_tried(curve, form):
    import torch
    F = XytFlow(curve, torch.cuda.Stream(), top=form)
    for t in (7, 0):
        f = F.file(t)
        got, = extract_xyt(F, [f], [ALL], [1], stream=F.stream)
        want, = txy.extract_xy(F, [f], [ALL], stream=F.stream)
        assert as_xy(got) == want and got["row_status_top_y"] == bytes([1] * N) and got["counts"] == [0] * 8, "t = %d" % t
        assert got["top_patch"] == _host(f["top"][0]), "t = %d" % t
        assert got == model_of(F, f, ALL, 1, bytes([1] * (t + N)), bytes([1] * t), bytes([1] * N)), "t = %d" % t
    # the statuses are the aligned retrieval's on that half
    shim = types.SimpleNamespace(S=F.S, curve=curve, ncols=NCOLS, n=N)
    dy, my, py, ay = F.top_y
    st = ta.retrieve_half(shim, dy, my, py, ay, None, N, form, F.stream, want_out=False)[0]
    assert st == bytes([1] * N)


# ---- 3. one flipped symbol in a top X row
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_top_x_row_is_replaced_by_its_y_row(curve, form):
    """one symbol flipped in top X row 5 at t = 7 and t = 0.  top_y = 1: every slot has the bytes and steps of the clean extraction,
    the slots the top level wins carry FOUND | FROM_Y (| RESIDUE in the 32-byte form), none is UNSURE, counts = [1, 0, 0, 0, 0, 0, 0, 1].
    top_y = 0: the xy call's result with the top level failed"""
    import torch
    F = XytFlow(curve, torch.cuda.Stream(), top=form)
    for t in (7, 0):
        what = "t = %d" % t
        f = F.file(t)
        clean, = txy.extract_xy(F, [f], [0], stream=F.stream)
        g = with_top(f, data=flipped(f["top"][0], SYMB[form] * (5 * NCOLS + 77) + 3))
        st = top_statuses(t, {5})
        got, = extract_xyt(F, [g], [0], [1], stream=F.stream)
        assert got["row_status"] == st and got["row_status_top_y"] == bytes([1] * N), what
        assert got["counts"] == [1, 0, 0, 0, 0, 0, 0, 1], what
        assert got["blocks"] == clean["blocks"] and got["steps"] == clean["steps"], what
        assert got["top_patch"] == _host(f["top"][0]), what
        assert not any(x & xm.UNSURE for x in got["flags"]), what
        for slot in range(N):
            assert got["flags"][slot] == (top_won(form) if clean["steps"][slot] == 0 else clean["flags"][slot]), "%s slot %d" % (what, slot)
        assert top_won(form) in got["flags"], what
        assert got == model_of(F, g, 0, 1, st, bytes([1] * t), bytes([1] * N)), what
        if t == 0:
            assert got["blocks"] == F.u_bytes()
        want, = txy.extract_xy(F, [g], [0], stream=F.stream)
        lost, = extract_xyt(F, [g], [0], [0], stream=F.stream)
        assert as_xy(lost) == want and want["counts"][0] == 1 and lost["counts"][6:] == [0, 0], what
        assert all(x & xm.UNSURE or s != 0 and s != em.NONE for x, s in zip(want["flags"], want["steps"])), what


# ---- 4. both halves damaged
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_both_halves_damaged(curve, form):
    """X row 2 and Y row 5: every row still has a source, the file comes back.  X row 2 and Y row 2: the top level is failed, blocks,
    steps and flags are the xy call's"""
    import torch
    F = XytFlow(curve, torch.cuda.Stream(), top=form)
    f = F.file(7)
    w = SYMB[form]
    clean, = txy.extract_xy(F, [f], [0], stream=F.stream)
    bad_x = flipped(f["top"][0], w * (2 * NCOLS + 9) + 1)
    g = with_top(f, data=bad_x, data_y=flipped(f["top_y"][0], w * (5 * NCOLS + 100) + 7, 0x40))
    st, sty = top_statuses(7, {2}), bytes(0 if j == 5 else 1 for j in range(N))
    got, = extract_xyt(F, [g], [0], [1], stream=F.stream)
    assert got["row_status"] == st and got["row_status_top_y"] == sty and got["counts"] == [1, 0, 0, 0, 0, 0, 1, 1]
    assert got["blocks"] == clean["blocks"] and got["steps"] == clean["steps"] and got["top_patch"] == _host(f["top"][0])
    assert got == model_of(F, g, 0, 1, st, bytes([1] * 7), sty)
    g = with_top(f, data=bad_x, data_y=flipped(f["top_y"][0], w * (2 * NCOLS + 100) + 7, 0x40))
    sty = bytes(0 if j == 2 else 1 for j in range(N))
    got, = extract_xyt(F, [g], [0], [1], stream=F.stream)
    want, = txy.extract_xy(F, [g], [0], stream=F.stream)
    assert got["row_status"] == st and got["row_status_top_y"] == sty and got["counts"][6:] == [1, 0] and got["counts"][0] == 1
    assert got["blocks"] == want["blocks"] and got["steps"] == want["steps"] and got["flags"] == want["flags"]
    assert got["counts"][:6] == want["counts"] and want["counts"][3] == sum(1 for s in want["steps"] if s == em.NONE)
    assert got == model_of(F, g, 0, 1, st, bytes([1] * 7), sty)


# ---- 5. the tamper sweep on the top Y half
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_top_y_tamper_sweep(curve, form):
    """one bit in a symbol, a MAC row, an alignment row (32-byte form) and a PRF value of the top Y half each fail exactly their Y row,
    counts[6] is 1 and nothing else changes while the X half is clean"""
    import torch
    F = XytFlow(curve, torch.cuda.Stream(), top=form)
    f = F.file(7)
    dy, my, py, ay = f["top_y"]
    clean, = txy.extract_xy(F, [f], [ALL], stream=F.stream)
    prf_bad = list(py)
    prf_bad[6] ^= 1 << 45
    cases = [(1, dict(data_y=flipped(dy, SYMB[form] * (1 * NCOLS + 77) + 3))), (3, dict(macs_y=flipped(my, 64 * 3 + 40, 0x80))), (6, dict(prf_y=prf_bad))]
    if form == "residue32":
        finite = [j for j in range(N) if _host(ay[64 * j:64 * j + 64]) != bytes(64)]
        assert finite
        cases.append((finite[0], dict(align_y=flipped(ay, 64 * finite[0] + 63, 2))))
    for row, change in cases:
        what = "row %d %s" % (row, sorted(change))
        sty = bytes(0 if j == row else 1 for j in range(N))
        g = with_top(f, **change)
        got, = extract_xyt(F, [g], [ALL], [1], stream=F.stream)
        assert got["row_status_top_y"] == sty and got["counts"] == [0, 0, 0, 0, 0, 0, 1, 0], what
        assert as_xy(got) == clean and got["top_patch"] == _host(f["top"][0]), what
        assert got == model_of(F, g, ALL, 1, bytes([1] * 15), bytes([1] * 7), sty), what


# ---- 6. wt != 1
@pytest.mark.parametrize("n", [N, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_top_level_rebuilt_at_a_step_with_a_true_twiddle(curve, form, n):
    """the rebuild at write step n_total + 3: Y_j = wt X_j with wt = w^e, e != 0.  A top-only file (t = 0): clean, the patched half is
    the X half; an X row damaged, it is wt^-1 times the Y row byte for byte and the blocks are U (mod p_icc in the 32-byte form); with
    the wrong top_step the decode does not give U"""
    import torch
    F = XytFlow(curve, torch.cuda.Stream(), indices=[], top=form, step=n + 3, n=n)
    assert tm.top_exponent(n, n + 3) != 0
    f = F.file(0, write_step=2 * n)
    assert _host(f["top"][0]) != _host(f["top_y"][0])
    got, = extract_xyt(F, [f], [0], [1], stream=F.stream, n=n)
    assert got["row_status"] == got["row_status_top_y"] == bytes([1] * n) and got["counts"] == [0] * 8
    assert got["blocks"] == F.u_bytes() and got["top_patch"] == _host(f["top"][0])
    for rows in ([n - 1], list(range(n))):
        what = "rows %s" % rows
        bad = f["top"][0]
        for j in rows:
            bad = flipped(bad, SYMB[form] * (j * NCOLS + 3 + j) + 5, 0x20)
        g = with_top(f, data=bad)
        st = top_statuses(0, set(rows), n)
        got, = extract_xyt(F, [g], [0], [1], stream=F.stream, n=n)
        assert got["row_status"] == st and got["row_status_top_y"] == bytes([1] * n), what
        assert got["counts"] == [len(rows), 0, 0, 0, 0, 0, 0, len(rows)], what
        assert got["top_patch"] == _host(f["top"][0]), what
        assert got["blocks"] == F.u_bytes() and got["steps"] == [0] * n and got["flags"] == bytes([top_won(form)] * n), what
        assert got == model_of(F, g, 0, 1, st, b"", bytes([1] * n), n=n), what
    # top_step is the rebuild's: another one unscales by another factor
    wrong, = extract_xyt(F, [dict(g, top_step=n + 2)], [0], [1], stream=F.stream, n=n)
    assert wrong["top_patch"] != _host(f["top"][0]) and wrong["blocks"] != F.u_bytes()
    assert wrong == model_of(F, dict(g, top_step=n + 2), 0, 1, st, b"", bytes([1] * n), n=n)


# ---- 7. a mixed batch, and the launch count
@pytest.mark.parametrize("curve", CURVES)
def test_three_files_with_top_y_1_0_1_equal_three_calls_and_the_launch_count(curve):
    import torch
    from porla_amd import multiexp as mx
    F = XytFlow(curve, torch.cuda.Stream())
    f7 = F.file(7)
    bad_top = flipped(f7["top"][0], 64 * (6 * NCOLS + 1) + 9)
    files = [with_top(txy.with_lower(f7, 1, data=flipped(f7["lower"][1][0], 64 * 9 + 1)), data=bad_top), with_top(F.file(5), data=bad_top),
             with_top(F.file(6), data_y=flipped(f7["top_y"][0], 64 * 17 + 2))]
    masks, tops = [2, 0, ALL], [1, 0, 1]
    got = extract_xyt(F, files, masks, tops, stream=F.stream)
    for a, (f, mask, ty) in enumerate(zip(files, masks, tops)):
        assert got[a] == extract_xyt(F, [f], [mask], [ty], stream=F.stream)[0], "file %d against its single call" % a
    assert got[0]["counts"] == [2, 0, 0, 0, 0, 0, 0, 1] and txy.Y_WON in got[0]["flags"] and top_won("exact") in got[0]["flags"]
    assert got[1]["counts"][0] == 1 and got[1]["counts"][6:] == [0, 0] and got[1]["row_status_top_y"] == bytes([xm.NOT_TRIED] * N)
    assert all(x & xm.UNSURE or s not in (0, em.NONE) for x, s in zip(got[1]["flags"], got[1]["steps"]))
    assert got[2]["counts"] == [0, 0, 0, 0, 0, 0, 1, 0] and got[2]["row_status_top_y"] == bytes([0] + [1] * (N - 1))

    def launches(fs, ms, ts):
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        res = extract_xyt(F, fs, ms, ts)
        return sum(c for _, _, c in mx.profile_get()) - before, res

    mx.profile_enable(1)
    try:
        three, got3 = launches(files, masks, tops)
        more = [a % 3 for a in range(5)]
        eight, got8 = launches(files + [files[a] for a in more], masks + [masks[a] for a in more], tops + [tops[a] for a in more])
        none, _ = launches([files[0]], [2], [0])
        tried, _ = launches([files[0]], [2], [1])
    finally:
        mx.profile_enable(0)
    assert three == eight and got3 == got and got8[:3] == got and got8[3:] == [got[a] for a in more]
    assert tried > none                                           # the patch kernel


# ---- 8. the seams of the check's blocks: the synthetic file of n_total = 64, t = 63, with a top Y half by the model
TOP_STEP_64 = 64 + 37


@functools.lru_cache(maxsize=None)
def synthetic_top_y(curve, n=64):
    """the top level's Y half of te.synthetic's U by the model's network at write step 64 + 37 (wt != 1), its rows' alpha-commitments and
    PRF values, alignments at infinity: computed once, shared, left unchanged"""
    u, _, _, _, _ = te.synthetic(curve)
    rnd = random.Random(6600)
    key = tr.commit_key(curve)
    rows = icc_py.crebuild(u, curve, TOP_STEP_64)[1]
    return rows, [model.alpha_commit(r, key) for r in rows], [rnd.getrandbits(128) for _ in rows]


@pytest.mark.parametrize("curve", CURVES)
def test_254_rows_across_the_block_seams(curve):
    """levels 0 .. 5 in both halves and the top level in both halves: the one 64-byte pass holds 63 X rows, 63 Y rows, the top level's
    64 X rows and its 64 Y rows -- rows 189 | 190 are the seam between the top halves.  Clean, then the last top X row (row 189) and
    the first top Y row (row 190) damaged: exactly those rows fail, every row keeps a source and the file comes back"""
    import torch
    n = 64
    S = ta.Setup(curve)
    u, blocks, levels, commits, prf = te.synthetic(curve)
    ys = txy.synthetic_y(curve)
    ty_rows, ty_commits, ty_prf = synthetic_top_y(curve)
    mdm = ta.mdm
    if curve == "bn254":
        call, aligned = te.calls_of(curve)
        xy, xyt = txy.xy_call_of(curve), xyt_call_of(curve)
    else:
        _, afb, hfb = tr.ipa_bases()
        call, aligned = te.calls_of(curve, afb, hfb, ta.IPA_ALPHA)
        xy, xyt = txy.xy_call_of(curve, afb, hfb, ta.IPA_ALPHA), xyt_call_of(curve, afb, hfb, ta.IPA_ALPHA)
    F = types.SimpleNamespace(curve=curve, call=call, xy=xy, xyt=xyt, top_form="exact", stream=torch.cuda.Stream(),
                              S=types.SimpleNamespace(aligned=aligned))
    dev = {i: (_dev(model.rows_bytes(levels[i])), _dev(model.points_to_bytes(S.expected(commits[i], prf[i]))), prf[i]) for i in levels}
    dev_y = {}
    for i, (rows, cm, pv, logs) in ys.items():
        align_b = model.points_to_bytes([icc_py.ec_mul(curve, mdm.GEN[curve], a) if a else None for a in logs])
        dev_y[i] = (_dev(model.rows_bytes(rows)), _dev(model.points_to_bytes(S.expected_aligned(cm, pv, logs))), pv, _dev(align_b))
    top_y = (_dev(model.rows_bytes(ty_rows)), _dev(model.points_to_bytes(S.expected(ty_commits, ty_prf))), ty_prf, None)
    f = {"write_step": 2 * n + 63, "lower": {i: dev[i] for i in range(6)}, "y": dev_y, "top": dev["top"] + (None,), "top_y": top_y,
         "top_step": TOP_STEP_64}
    got, = extract_xyt(F, [f], [ALL], [1], stream=F.stream, n=n)
    assert got["row_status"] == bytes([1] * 127) and got["row_status_y"] == bytes([1] * 63) and got["row_status_top_y"] == bytes([1] * n)
    assert got["counts"] == [0] * 8
    clean, = txy.extract_xy(F, [f], [ALL], stream=F.stream, n=n)
    assert as_xy(got) == clean
    bad_x = flipped(dev["top"][0], 64 * (63 * NCOLS + 100) + 2, 4)
    bad_y = flipped(top_y[0], 64 * 5 + 1)
    g = with_top(f, data=bad_x, data_y=bad_y)
    st, sty = bytes([1] * 126 + [0]), bytes([0] + [1] * 63)
    got, = extract_xyt(F, [g], [ALL], [1], stream=F.stream, n=n)
    assert got["row_status"] == st and got["row_status_y"] == bytes([1] * 63) and got["row_status_top_y"] == sty
    assert got["counts"] == [1, 0, 0, 0, 0, 0, 1, 1]
    assert got["top_patch"] == _host(dev["top"][0])
    assert got["blocks"] == clean["blocks"] and got["steps"] == clean["steps"]
    assert got == model_of(F, g, ALL, 1, st, bytes([1] * 63), sty, n=n)


# ---- 9. a second call on another stream while the first is in flight
@pytest.mark.parametrize("curve", CURVES)
def test_a_second_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    F = XytFlow(curve, torch.cuda.Stream())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f7 = F.file(7)
    g = with_top(f7, data=flipped(f7["top"][0], 64 * (4 * NCOLS + 5) + 1))
    one, = extract_xyt(F, [g], [ALL], [1], stream=F.stream)
    clean, = txy.extract_xy(F, [f7], [ALL], stream=F.stream)
    first = run_xyt(F, [g for _ in range(6)], [ALL] * 6, [1] * 6, stream=s1)
    second = run_xyt(F, [F.file(t) for t in (5, 0, 6)], [ALL, ALL, 0], [1, 1, 0], stream=s2)
    third = run_xyt(F, [g], [4], [0], stream=s1)
    assert one["counts"] == [1, 0, 0, 0, 0, 0, 0, 1] and one["blocks"] == clean["blocks"] and one["steps"] == clean["steps"]
    for got in first():
        assert got == one
    for got, t in zip(second(), (5, 0, 6)):
        assert got["row_status"] == bytes([1] * (t + N)) and got["counts"] == [0] * 8
        assert got["steps"] == [r for _, r in F.want(t)] and got["blocks"] == ta.chunk_bytes([c for c, _ in F.want(t)])
    lost = third()[0]
    assert lost["counts"][0] == 1 and lost["counts"][6:] == [0, 0] and lost["flags"] != one["flags"]

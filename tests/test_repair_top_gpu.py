"""GPU box: the top-level repair (porla_{kzg,ipa}_repair_top_batch_device) -- the rows of a top level that fail their check while their
sibling in the other half passes are written back in place, data row and MAC row -- against the Python model
tests/repair_top_model.py (statuses, actions, counts and the final bytes of all four stores), against the pristine stores, against the
aligned retrieval's check before and after, and in the flow the call exists for: repair, then the extraction without the Y half.  The
stores are the ones tests/test_extract_xyt_gpu.py builds: a top level left by a rebuild write with BOTH halves kept (n_total 8 and 2,
both forms), and the synthetic file of n_total = 64.  Every comparison is byte equality; every store and output lies in front of a
256-byte sentinel guard that must survive.  No test damages anything but copies of its own buffers.

The KZG build draws its hiding base anew at every init_SRS, so every test builds its own file and installs no key after that."""
import types

import pytest

from tests import common  # noqa: F401  (puts oracle/ on the path)
import icc_py
from tests import repair_top_model as rm
from tests import retrieve_model as model
from tests import test_extract_gpu as te
from tests import test_extract_xy_gpu as txy
from tests import test_extract_xyt_gpu as xt
from tests import test_retrieve_aligned_gpu as ta
from tests import test_retrieve_gpu as tr
from tests.update_model import pt_tuple

pytestmark = pytest.mark.gpu
CURVES, FORMS = xt.CURVES, xt.FORMS
SENTINEL, GUARD = tr.SENTINEL, tr.GUARD
_dev, _host = tr._dev, tr._host
N, NCOLS = te.N, te.NCOLS
SYMB = xt.SYMB
DATA, MAC, LOST = rm.DATA, rm.MAC, rm.LOST
flipped = txy.flipped
STORES = ("rows_x", "macs_x", "rows_y", "macs_y")


def repair_call_of(curve, afb=None, hfb=None, alpha=None):
    from porla_amd import multiexp as mx
    if curve == "bn254":
        return lambda reqs, n, form, s=0: mx.kzg_repair_top_batch_device(reqs, n, form, s)
    return lambda reqs, n, form, s=0: afb.ipa_repair_top_batch_device(hfb, alpha, reqs, n, form, s)


def flow(curve, form, n=N, step=None):
    """xt.XytFlow without writes: the top level alone, both halves kept, rebuilt at write step `step` (n + 3: a true twiddle)"""
    import torch
    F = xt.XytFlow(curve, torch.cuda.Stream(), indices=[], top=form, step=n + 3 if step is None else step, n=n)
    F.repair = repair_call_of(curve) if curve == "bn254" else repair_call_of(curve, F.C.afb, F.C.hfb, F.C.alpha)
    F.alpha = F.C.alpha
    return F


def file_of(F, n=N):
    """the top level as the repair takes it: "x" / "y" = (rows, MAC tensor, PRF integers, alignment tensor or None), "pristine" = the same"""
    f = F.file(0, write_step=2 * n)
    g = {"x": f["top"], "y": f["top_y"], "top_step": f["top_step"], "xyt": f}
    return dict(g, pristine=(g["x"], g["y"]))


def damaged(f, half, rows=None, macs=None, align=None):
    r, m, p, a = f[half]
    return dict(f, **{half: (r if rows is None else rows, m if macs is None else macs, p, a if align is None else align)})


def run_repair(F, files, n=N, form=None, stream=None, work=None):
    """one call on working copies of the files' stores (or on `work`, the copies of an earlier call, in place).  Returns a function
    giving (per file the statuses, actions, counts and the bytes of the four stores; the working copies); the guards behind every
    store and output are checked, and the alignment stores are as they were"""
    import torch
    form = form or F.top_form
    sizes = {"rows_x": n * NCOLS * SYMB[form], "macs_x": 64 * n, "rows_y": n * NCOLS * SYMB[form], "macs_y": 64 * n, "status_x": n, "status_y": n,
             "action_x": n, "action_y": n, "counts": 32}
    src = lambda f, name: f[name[-1]][0 if name.startswith("rows") else 1]
    ptr = lambda t: t.data_ptr() if t is not None else 0
    works, reqs, keep, aligns = [], [], [], []
    for a, f in enumerate(files):
        wk = dict(work[a]) if work else {}
        for name, size in sizes.items():
            if name in STORES and work:
                continue
            wk[name] = torch.full((size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
            if name in STORES:
                wk[name][:size] = src(f, name)[:size]
        prf = [_dev(ta.raw_prf(F.curve, f[h][2])) for h in "xy"]
        al = [f[h][3] for h in "xy"]
        aligns.append([(t, _host(t)) for t in al if t is not None])
        reqs.append((ptr(wk["rows_x"]), ptr(wk["macs_x"]), ptr(al[0]), ptr(prf[0]), ptr(wk["rows_y"]), ptr(wk["macs_y"]), ptr(al[1]), ptr(prf[1]),
                     ptr(wk["status_x"]), ptr(wk["status_y"]), ptr(wk["action_x"]), ptr(wk["action_y"]), ptr(wk["counts"]), f["top_step"]))
        works.append(wk)
        keep.append(prf)
    torch.cuda.synchronize()
    F.repair(reqs, n, form, stream.cuda_stream if stream is not None else 0)

    def done():
        if stream is not None:
            stream.synchronize()
        torch.cuda.synchronize()
        res = []
        for a, wk in enumerate(works):
            for name, size in sizes.items():
                assert bool(torch.all(wk[name][size:] == SENTINEL)), "file %d: the guard behind %s changed" % (a, name)
            for t, before in aligns[a]:
                assert _host(t) == before, "file %d: an alignment store was written" % a
            got = {name: _host(wk[name][:size]) for name, size in sizes.items() if name != "counts"}
            got["counts"] = wk["counts"][:32].cpu().view(torch.int32).tolist()
            res.append(got)
        del keep[:]
        return res, works
    return done


def host_half(h):
    return _host(h[0]), _host(h[1]), h[2], _host(h[3]) if h[3] is not None else None


def model_of(F, f, got, n=N, form=None):
    """rm.repair_top on the stores as they lie on the device, with the statuses the call gave.  The expected MAC of a repaired row: the
    pristine row's MAC M_j satisfies M_j = E_j - alpha A_j, so over the pristine row and an alignment A' it is M_j + alpha (A_j - A')"""
    form = form or F.top_form
    curve = F.curve
    w = SYMB[form]
    pristine = [host_half(h) for h in f["pristine"]]

    def mac_of(h, js, rows, prf, align):
        p_rows, p_macs, _, p_align = pristine[h]
        out = []
        for j, row, a in zip(js, rows, align):
            assert row == [int.from_bytes(p_rows[w * (j * NCOLS + c):w * (j * NCOLS + c + 1)], "little") for c in range(NCOLS)]
            m = pt_tuple(p_macs[64 * j:64 * j + 64])
            a0 = pt_tuple(p_align[64 * j:64 * j + 64]) if p_align else None
            if a != a0:
                d = icc_py.ec_add(curve, a0, icc_py.ec_neg(curve, a) if a is not None else None)
                m = icc_py.ec_add(curve, m, icc_py.ec_mul(curve, d, F.alpha))
            out.append(m)
        return out

    return rm.repair_top(host_half(f["x"]), host_half(f["y"]), n, NCOLS, curve, form, f["top_step"], status_x=got["status_x"],
                         status_y=got["status_y"], mac_of=mac_of)


def check_half(F, rows, macs, prf, align, n, form, stream):
    """the aligned retrieval's statuses of one half, check only"""
    shim = types.SimpleNamespace(S=F.S, curve=F.curve, ncols=NCOLS, n=n)
    return ta.retrieve_half(shim, rows, macs, prf, align, None, n, form, stream, want_out=False)[0]


def repair_and_settle(F, f, n=N, form=None, stream=None, lost=()):
    """one file through the call, then everything that holds for every call: the statuses are the aligned retrieval's on the stores
    as they lay, everything equals the model, every row not lost passes the aligned retrieval's check afterwards, and a second call on
    the repaired stores writes nothing.  Returns (the call's outputs, the working copies)"""
    form = form or F.top_form
    stream = stream or F.stream
    (got,), works = run_repair(F, [f], n, form, stream)()
    for h in "xy":
        assert got["status_" + h] == check_half(F, f[h][0], f[h][1], f[h][2], f[h][3], n, form, stream), "the statuses of half " + h
    want = model_of(F, f, got, n, form)
    for name in want:
        assert got[name] == want[name], name
    wk = works[0]
    after = bytes(0 if j in lost else 1 for j in range(n))
    for h in "xy":
        size = n * NCOLS * SYMB[form]
        assert check_half(F, wk["rows_" + h][:size], wk["macs_" + h][:64 * n], f[h][2], f[h][3], n, form, stream) == after, "after, half " + h
    (again,), _ = run_repair(F, [f], n, form, stream, work=works)()
    assert again["status_x"] == again["status_y"] == after
    assert again["action_x"] == again["action_y"] == bytes(LOST if j in lost else 0 for j in range(n))
    assert again["counts"] == [len(lost), len(lost), 0, 0, 0, 0, len(lost), 0]
    for name in STORES:
        assert again[name] == got[name], "the second call wrote " + name
    return got, wk


def pristine_stores(f):
    return {"rows_x": _host(f["pristine"][0][0]), "macs_x": _host(f["pristine"][0][1]), "rows_y": _host(f["pristine"][1][0]),
            "macs_y": _host(f["pristine"][1][1])}


def only(j, bits, n=N):
    return bytes(bits if i == j else 0 for i in range(n))


def bad(j, n=N):
    return bytes(0 if i == j else 1 for i in range(n))


# ---- 1. a clean file
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_clean_file_is_left_alone(curve, form):
    F = flow(curve, form)
    f = file_of(F)
    got, _ = repair_and_settle(F, f)
    assert got["status_x"] == got["status_y"] == bytes([1] * N) and got["action_x"] == got["action_y"] == bytes(N)
    assert got["counts"] == [0] * 8
    assert {k: got[k] for k in STORES} == pristine_stores(f)


# ---- 2. one damaged data row, in X and in Y; 8. the flow
@pytest.mark.parametrize("n", [N, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_data_row_comes_back_from_the_other_half(curve, form, n):
    """rebuilt at write step n + 3 (wt != 1): one symbol of the last X row flipped, then one of Y row 0 -- the new direction, wt X_j.
    The store is the pristine clone again, the action exactly DATA, the other half untouched.  Then the flow: the repaired stores
    through the extraction with top_y = 0 give every block back with no failed row"""
    F = flow(curve, form, n)
    assert rm.top_exponent(n, F.step) != 0
    f = file_of(F, n)
    assert _host(f["x"][0]) != _host(f["y"][0])
    w = SYMB[form]
    for h, j in (("x", n - 1), ("y", 0)):
        g = damaged(f, h, rows=flipped(f[h][0], w * (j * NCOLS + 3 + j) + 5, 0x20))
        got, wk = repair_and_settle(F, g, n)
        o = "y" if h == "x" else "x"
        assert got["status_" + h] == bad(j, n) and got["status_" + o] == bytes([1] * n), h
        assert got["action_" + h] == only(j, DATA, n) and got["action_" + o] == bytes(n), h
        assert {k: got[k] for k in STORES} == pristine_stores(f), h
        hy = 1 if h == "y" else 0
        assert got["counts"] == [1 - hy, hy, 1 - hy, 0, hy, 0, 0, 0], h
        size = n * NCOLS * w
        top = xt.with_top(f["xyt"], data=wk["rows_x"][:size], macs=wk["macs_x"][:64 * n], data_y=wk["rows_y"][:size], macs_y=wk["macs_y"][:64 * n])
        ex, = xt.extract_xyt(F, [top], [0], [0], stream=F.stream, n=n)
        assert ex["counts"][0] == 0 and ex["blocks"] == F.u_bytes(), h


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_y_row_with_wt_1_is_the_x_row_copied(curve, form):
    F = flow(curve, form, step=2 * N)
    assert rm.top_exponent(N, F.step) == 0
    f = file_of(F)
    assert _host(f["x"][0]) == _host(f["y"][0])
    g = damaged(f, "y", rows=flipped(f["y"][0], SYMB[form] * (6 * NCOLS + 127) + SYMB[form] - 1, 0x80))
    got, _ = repair_and_settle(F, g)
    assert got["status_y"] == bad(6) and got["action_y"] == only(6, DATA) and got["action_x"] == bytes(N)
    assert {k: got[k] for k in STORES} == pristine_stores(f) and got["counts"] == [0, 1, 0, 0, 1, 0, 0, 0]


# ---- 3. only the MAC row; 4. data and MAC of the same row
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_mac_row_and_a_row_damaged_in_data_and_mac(curve, form):
    F = flow(curve, form)
    f = file_of(F)
    w = SYMB[form]
    g = damaged(f, "x", macs=flipped(f["x"][1], 64 * 2 + 40, 0x80))
    got, _ = repair_and_settle(F, g)
    assert got["status_x"] == bad(2) and got["action_x"] == only(2, MAC) and got["action_y"] == bytes(N)
    assert {k: got[k] for k in STORES} == pristine_stores(f) and got["counts"] == [1, 0, 0, 1, 0, 0, 0, 0]
    g = damaged(f, "y", rows=flipped(f["y"][0], w * (5 * NCOLS + 64) + 1), macs=flipped(f["y"][1], 64 * 5 + 63))
    got, _ = repair_and_settle(F, g)
    assert got["status_y"] == bad(5) and got["action_y"] == only(5, DATA | MAC) and got["action_x"] == bytes(N)
    assert {k: got[k] for k in STORES} == pristine_stores(f) and got["counts"] == [0, 1, 0, 0, 1, 1, 0, 0]


# ---- 5. a row index damaged in both halves
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_a_row_index_damaged_in_both_halves_is_lost_and_the_others_are_repaired(curve, form):
    """row 3 in both halves, row 0 in X, row 7 in Y: row 3 is LOST on both sides and stays as damaged, the other two are repaired"""
    F = flow(curve, form)
    f = file_of(F)
    w = SYMB[form]
    bad_x = flipped(flipped(f["x"][0], w * (3 * NCOLS + 1) + 2), w * 9 + 1, 4)
    bad_y = flipped(flipped(f["y"][0], w * (3 * NCOLS + 90) + 3, 2), w * (7 * NCOLS + 127) + 7)
    g = damaged(damaged(f, "x", rows=bad_x), "y", rows=bad_y)
    got, _ = repair_and_settle(F, g, lost={3})
    assert got["status_x"] == bytes([0, 1, 1, 0, 1, 1, 1, 1]) and got["status_y"] == bytes([1, 1, 1, 0, 1, 1, 1, 0])
    assert got["action_x"] == bytes([DATA, 0, 0, LOST, 0, 0, 0, 0]) and got["action_y"] == bytes([0, 0, 0, LOST, 0, 0, 0, DATA])
    assert got["counts"] == [2, 2, 1, 0, 1, 0, 1, 0]
    rb = NCOLS * w
    p = pristine_stores(f)
    for name, dam in (("rows_x", _host(bad_x)), ("rows_y", _host(bad_y))):
        assert got[name][3 * rb:4 * rb] == dam[3 * rb:4 * rb] != p[name][3 * rb:4 * rb]
        assert got[name][:3 * rb] == p[name][:3 * rb] and got[name][4 * rb:] == p[name][4 * rb:]
    assert got["macs_x"] == p["macs_x"] and got["macs_y"] == p["macs_y"]


# ---- 6. residue32 with finite alignments
@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_alignment_row_gets_the_mac_of_the_alignment_as_stored(curve):
    """the Y half of the aligned top level has finite alignments.  A data row damaged there comes back pristine (the tests above); an
    alignment row replaced by another row's -- a point, not the row's own -- fails the row with intact data: the MAC is rewritten to
    E_j - alpha A'_j, the data row is left alone, the alignment store is not restored"""
    F = flow(curve, "residue32")
    f = file_of(F)
    ay = _host(f["y"][3])
    finite = [j for j in range(N) if ay[64 * j:64 * j + 64] != bytes(64)]
    assert len(finite) >= 2
    j, other = finite[0], next(i for i in finite[1:] if ay[64 * i:64 * i + 64] != ay[64 * finite[0]:64 * finite[0] + 64])
    g = damaged(f, "y", align=_dev(ay[:64 * j] + ay[64 * other:64 * other + 64] + ay[64 * (j + 1):]))
    got, _ = repair_and_settle(F, g)
    p = pristine_stores(f)
    assert got["status_y"] == bad(j) and got["action_y"] == only(j, MAC) and got["action_x"] == bytes(N)
    assert got["rows_y"] == p["rows_y"] and got["rows_x"] == p["rows_x"] and got["macs_x"] == p["macs_x"]
    assert got["macs_y"][:64 * j] == p["macs_y"][:64 * j] and got["macs_y"][64 * (j + 1):] == p["macs_y"][64 * (j + 1):]
    assert got["macs_y"][64 * j:64 * (j + 1)] != p["macs_y"][64 * j:64 * (j + 1)]
    assert got["counts"] == [0, 1, 0, 0, 0, 1, 0, 0]
    # and a damaged data row of the same half, the alignments as they were
    g = damaged(f, "y", rows=flipped(f["y"][0], 32 * (j * NCOLS + 17) + 31, 0x10))
    got, _ = repair_and_settle(F, g)
    assert got["action_y"] == only(j, DATA) and {k: got[k] for k in STORES} == p


# ---- 9. three files, and the launch count
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("curve", CURVES)
def test_three_files_equal_three_calls_and_the_launch_count(curve, form):
    import torch
    from porla_amd import multiexp as mx
    F = flow(curve, form)
    f = file_of(F)
    w = SYMB[form]
    bad_x = flipped(f["x"][0], w * (6 * NCOLS + 1) + 9)
    files = [f, damaged(f, "x", rows=bad_x), damaged(damaged(f, "x", rows=bad_x), "y", rows=flipped(f["y"][0], w * 17 + 2))]
    got, _ = run_repair(F, files, stream=F.stream)()
    for a, g in enumerate(files):
        single, _ = run_repair(F, [g], stream=F.stream)()
        assert got[a] == single[0], "file %d against its single call" % a
        assert got[a] == dict(model_of(F, g, got[a]), **{k: got[a][k] for k in ()}), "file %d against the model" % a
        assert {k: got[a][k] for k in STORES} == pristine_stores(f)
    assert got[0]["counts"] == [0] * 8 and got[1]["counts"] == [1, 0, 1, 0, 0, 0, 0, 0] and got[2]["counts"] == [1, 1, 1, 0, 1, 0, 0, 0]
    assert got[2]["action_x"] == only(6, DATA) and got[2]["action_y"] == only(0, DATA)

    def launches(fs):
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        res, _ = run_repair(F, fs)()
        return sum(c for _, _, c in mx.profile_get()) - before, res

    mx.profile_enable(1)
    try:
        three, got3 = launches(files)
        eight, got8 = launches(files + [files[a % 3] for a in range(5)])
        clean, _ = launches([f])
        hurt, _ = launches([files[2]])
    finally:
        mx.profile_enable(0)
    assert three == eight == clean == hurt and three > 0
    assert got3 == got and got8[:3] == got and got8[3:] == [got[a % 3] for a in range(5)]


# ---- 10. the seams of the check's blocks: the synthetic top level of n_total = 64, two files
@pytest.mark.parametrize("curve", CURVES)
def test_256_rows_across_the_half_seam_and_the_file_seam(curve):
    """K = 2, n_total = 64: the pass holds rows 0 .. 255, X | Y of file 0 at 63 | 64, the file seam at 127 | 128, the quad compare's
    blocks are 64 rows.  The last X row and the first Y row of file 0 and the MAC of the first X row of file 1 are damaged: exactly
    those rows act, everything is pristine after"""
    import torch
    n = 64
    S = ta.Setup(curve)
    u, blocks, levels, commits, prf = te.synthetic(curve)
    ty_rows, ty_commits, ty_prf = xt.synthetic_top_y(curve)
    if curve == "bn254":
        _, aligned = te.calls_of(curve)
        call = repair_call_of(curve)
    else:
        _, afb, hfb = tr.ipa_bases()
        _, aligned = te.calls_of(curve, afb, hfb, ta.IPA_ALPHA)
        call = repair_call_of(curve, afb, hfb, ta.IPA_ALPHA)
    F = types.SimpleNamespace(curve=curve, repair=call, top_form="exact", stream=torch.cuda.Stream(), S=types.SimpleNamespace(aligned=aligned),
                              alpha=None)
    x = (_dev(model.rows_bytes(levels["top"])), _dev(model.points_to_bytes(S.expected(commits["top"], prf["top"]))), prf["top"], None)
    y = (_dev(model.rows_bytes(ty_rows)), _dev(model.points_to_bytes(S.expected(ty_commits, ty_prf))), ty_prf, None)
    f = {"x": x, "y": y, "top_step": xt.TOP_STEP_64, "pristine": (x, y)}
    f0 = damaged(damaged(f, "x", rows=flipped(x[0], 64 * (63 * NCOLS + 100) + 2, 4)), "y", rows=flipped(y[0], 64 * 5 + 1))
    f1 = damaged(f, "x", macs=flipped(x[1], 17, 0x10))
    got, works = run_repair(F, [f0, f1], n, "exact", F.stream)()
    assert got[0]["status_x"] == bad(63, n) and got[0]["status_y"] == bad(0, n)
    assert got[1]["status_x"] == bad(0, n) and got[1]["status_y"] == bytes([1] * n)
    assert got[0]["action_x"] == only(63, DATA, n) and got[0]["action_y"] == only(0, DATA, n)
    assert got[1]["action_x"] == only(0, MAC, n) and got[1]["action_y"] == bytes(n)
    assert got[0]["counts"] == [1, 1, 1, 0, 1, 0, 0, 0] and got[1]["counts"] == [1, 0, 0, 1, 0, 0, 0, 0]
    for a, g in enumerate((f0, f1)):
        assert {k: got[a][k] for k in STORES} == pristine_stores(f), a
        assert got[a] == model_of(F, g, got[a], n, "exact"), a
    clean, _ = run_repair(F, [f0, f1], n, "exact", F.stream, work=works)()
    for a in range(2):
        assert clean[a]["status_x"] == clean[a]["status_y"] == bytes([1] * n) and clean[a]["counts"] == [0] * 8
        assert clean[a]["action_x"] == clean[a]["action_y"] == bytes(n)
        assert {k: clean[a][k] for k in STORES} == pristine_stores(f), a


# ---- 11. a second call on another stream, on disjoint stores, while the first is in flight
@pytest.mark.parametrize("curve", CURVES)
def test_a_second_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    F = flow(curve, "exact")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f = file_of(F)
    g = damaged(f, "x", rows=flipped(f["x"][0], 64 * (4 * NCOLS + 5) + 1))
    h = damaged(f, "y", macs=flipped(f["y"][1], 64 * 1 + 3))
    (one,), _ = run_repair(F, [g], stream=F.stream)()
    (two,), _ = run_repair(F, [h], stream=F.stream)()
    first = run_repair(F, [g] * 6, stream=s1)
    second = run_repair(F, [h, f, h], stream=s2)
    third = run_repair(F, [f], stream=s1)
    assert one["counts"] == [1, 0, 1, 0, 0, 0, 0, 0] and two["counts"] == [0, 1, 0, 0, 0, 1, 0, 0]
    for got in first()[0]:
        assert got == one
    got = second()[0]
    assert got[0] == two and got[2] == two and got[1]["counts"] == [0] * 8
    assert third()[0][0] == got[1]
    assert {k: one[k] for k in STORES} == {k: two[k] for k in STORES} == pristine_stores(f)

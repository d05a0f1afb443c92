"""GPU box: the file extraction with the Y halves (porla_{kzg,ipa}_extract_xy_batch_device) -- a lower level whose X half fails is
recovered from its Y half mod p_icc -- against the Python model tests/extract_xy_model.py (every output byte), against the existing
extraction and the aligned retrieval on the same stores, and in the flow the call exists for: a top level left by a rebuild write,
then up to seven writes through the client and server update batches on one stream, all six families and both PRF halves of every
level kept per write.  Every comparison is byte equality; every output is pre-filled with a sentinel and a 256-byte guard behind it
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
from tests import icc_decode_model as dm
from tests import retrieve_model as model
from tests import test_extract_gpu as te
from tests import test_retrieve_aligned_gpu as ta
from tests import test_retrieve_gpu as tr

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
SENTINEL, GUARD = tr.SENTINEL, tr.GUARD
_dev, _host = tr._dev, tr._host
N, NCOLS = te.N, te.NCOLS
INDICES = te.INDICES
P, D = xm.P, xm.D
ALL = (1 << 64) - 1
Y_WON = xm.FOUND | xm.RESIDUE | xm.FROM_Y


def certain(rnd, step, index):
    return xm.chunk0_certain(rnd, index)


def xy_call_of(curve, afb=None, hfb=None, alpha=None):
    from porla_amd import multiexp as mx
    if curve == "bn254":
        return lambda reqs, n, form, s=0: mx.kzg_extract_xy_batch_device(reqs, n, form, s)
    return lambda reqs, n, form, s=0: afb.ipa_extract_xy_batch_device(hfb, alpha, reqs, n, form, s)


class XyFlow(te.ExFlow):
    """te.ExFlow keeping BOTH halves: after every write the resident X and Y data, MAC and alignment stores and the PRF values of both
    halves are cloned in stream order.  chunk0(rnd, step, index): chunk 0 of the block written at `step` (default: certain, in [D,
    p_icc)).  file(t)["y"] = {level: (data_y, mac_y, PRF integers, align_y)}"""

    def __init__(self, curve, stream, indices=INDICES, top="exact", seed=5200, chunk0=certain):
        import torch
        from porla_amd import multiexp as mx
        from tests import test_client_rebuild_batch_gpu as cr, test_client_update_batch_gpu as cu, test_update_batch_gpu as ub
        from tests.client_update_model import n_prf
        from tests.update_model import FAMILIES, FileModel, pt_tuple
        self.curve, self.n, self.ncols, self.stream, self.top_form, self.indices = curve, N, NCOLS, stream, top or "exact", list(indices)
        self.C = C = cu.setup_of(curve)
        self.h = C.h
        if curve == "bn254":                                      # the key, SRS and hiding point are process state: put ours in again
            mx.init_key(ub.TAU, ub.ALPHA)
            mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
            self.h = pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))
            self.call, aligned = te.calls_of(curve)
            self.xy = xy_call_of(curve)
        else:
            self.call, aligned = te.calls_of(curve, C.afb, C.hfb, C.alpha)
            self.xy = xy_call_of(curve, C.afb, C.hfb, C.alpha)
        self.S = types.SimpleNamespace(aligned=aligned)           # (what ta.retrieve_half calls)
        self.rnd = rnd = random.Random(seed)
        self.keep, self.top, self.u, self.base = [], None, None, 0
        if top:
            self._rebuild(top, cr)
            self.base = self.n                                    # the server's counter goes on from the rebuild's step
        self.d = ub.DevFile(FileModel(self.n, NCOLS, curve, C.server.base, fill=SENTINEL))
        self.hold, self.blocks, self.snap = {}, {}, {0: {}}
        for s, index in enumerate(indices, 1):
            step = self.base + s
            level = (s & -s).bit_length() - 1
            chunks = te.block_of(rnd, index)
            chunks[0] = chunk0(rnd, s, index)
            self.blocks[s] = chunks
            new_x, new_y = ([rnd.getrandbits(128) for _ in range(1 << level)] for _ in range(2))
            prf = [rnd.getrandbits(128)]
            for i in range(level):
                prf += self.hold[i][0] + self.hold[i][1]
                del self.hold[i]
            prf += new_x + new_y
            assert len(prf) == n_prf(level)
            self.hold[level] = (new_x, new_y)
            d_block, d_prf = _dev(ta.chunk_bytes([chunks])), _dev(ta.raw_prf(curve, prf))
            d_mac = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
            d_comp = torch.full((64 * (2 << level),), SENTINEL, dtype=torch.uint8, device="cuda")
            self.keep += [d_block, d_prf, d_mac, d_comp]
            torch.cuda.synchronize()                              # (the uploads are torch's; the calls below wait for nothing)
            C.call([(d_block.data_ptr(), d_prf.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), step, level)], self.n, stream.cuda_stream)
            C.server.call([(d_block.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), step, level) +
                           tuple([t.data_ptr() for t in self.d.t[f][:level + 1]] for f in FAMILIES)], self.n, stream.cuda_stream)
            with torch.cuda.stream(stream):                       # the resident halves as they stand now, cloned in stream order
                self.snap[s] = {i: tuple(self.d.t[f][i].clone() for f in ("data_x", "mac_x", "data_y", "mac_y", "align_y")) +
                                (list(self.hold[i][0]), list(self.hold[i][1])) for i in self.hold}
        stream.synchronize()

    def file(self, t, top=True, write_step=None):
        lower = {i: (dx, mx_, px) for i, (dx, mx_, dy, my, ay, px, py) in self.snap[t].items()}
        y = {i: (dy, my, py, ay) for i, (dx, mx_, dy, my, ay, px, py) in self.snap[t].items()}
        return {"write_step": self.base + t if write_step is None else write_step, "lower": lower, "y": y, "top": self.top if top else None}

    def want(self, t, top=True):
        """(chunks or None, rank or None) per slot, exact: the last write of the index among the steps 1 .. t, else U, else nothing"""
        out = [(list(self.u[b]), 0) if top and self.u else (None, None) for b in range(self.n)]
        for s in range(1, t + 1):
            if 1 <= self.indices[s - 1] <= self.n:
                out[self.indices[s - 1] - 1] = (self.blocks[s], s)
        return out


def run_xy(F, files, masks, stream=None, call=None, n=N, ncols=NCOLS, top_form=None, null_y=False):
    """one call.  files: te.run_extract's dictionaries with "y": {level: (data tensor, MAC tensor, PRF integers, alignment tensor or
    None)} beside them; masks: y_levels per file.  null_y: every Y pointer NULL.  Returns a function giving, per file, the outputs as
    xm.extract_xy names them; the guards behind every output are checked"""
    import torch
    logn = n.bit_length() - 1
    bb = ncols * 32
    full = lambda size: torch.full((size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    ptr = lambda x: x.data_ptr() if x is not None else 0
    bufs, reqs, keep = [], [], []
    for f, mask in zip(files, masks):
        t = f["write_step"] % n
        rows = t + (n if f["top"] else 0)
        prf = [v for i in sorted(f["lower"]) for v in f["lower"][i][2]] + (f["top"][2] if f["top"] else [])
        assert len(prf) == rows and sorted(f["lower"]) == [i for i, _, _ in em.resident_levels(t, n)]
        d_prf = _dev(ta.raw_prf(F.curve, prf)) if rows else None
        sizes = {"work": t * bb, "blocks": n * bb, "steps": 4 * n, "flags": n, "row_status": rows, "counts": 24}
        if not null_y:
            sizes.update({"work_y": t * bb, "row_status_y": t})
        b = {name: full(size) for name, size in sizes.items()}
        b["sizes"] = sizes
        fam = lambda k: [ptr(f["lower"][i][k]) if i in f["lower"] else 0 for i in range(logn)] if t else None
        top = f["top"] or (None, None, None, None)
        req = (f["write_step"], fam(0), fam(1), ptr(top[0]), ptr(top[1]), ptr(top[3]), ptr(d_prf), b["work"].data_ptr() if t else 0,
               b["blocks"].data_ptr(), b["steps"].data_ptr(), b["flags"].data_ptr(), b["row_status"].data_ptr() if rows else 0,
               b["counts"].data_ptr())
        if null_y:
            req += (None, None, None, 0, 0, 0, mask)
            d_prf_y = None
        else:
            y = f["y"]
            assert sorted(y) == sorted(f["lower"])
            d_prf_y = _dev(ta.raw_prf(F.curve, [v for i in sorted(y) for v in y[i][2]])) if t else None
            famy = lambda k: [ptr(y[i][k]) if i in y else 0 for i in range(logn)]
            req += (famy(0), famy(1), famy(3), ptr(d_prf_y), b["work_y"].data_ptr() if t else 0, b["row_status_y"].data_ptr() if t else 0, mask)
        reqs.append(req)
        bufs.append(b)
        keep += [d_prf, d_prf_y]
    torch.cuda.synchronize()
    (call or F.xy)(reqs, n, top_form or F.top_form, stream.cuda_stream if stream is not None else 0)
    return lambda: collect(bufs, stream, n, keep)


def collect(bufs, stream, n, keep=None):
    import torch
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res = []
    for a, b in enumerate(bufs):
        for name, size in b["sizes"].items():
            assert bool(torch.all(b[name][size:] == SENTINEL)), "file %d: the guard behind %s changed" % (a, name)
        cut = lambda name: _host(b[name][:b["sizes"][name]])
        res.append({"blocks": cut("blocks"), "steps": [s & 0xffffffff for s in b["steps"][:4 * n].cpu().view(torch.int32).tolist()],
                    "flags": cut("flags"), "row_status": cut("row_status"),
                    "row_status_y": cut("row_status_y") if "row_status_y" in b else None,
                    "counts": b["counts"][:24].cpu().view(torch.int32).tolist()})
    return res


def extract_xy(F, files, masks, **kw):
    return run_xy(F, files, masks, **kw)()


def model_of(F, f, mask, statuses, status_y, n=N, ncols=NCOLS, top_form=None):
    """xm.extract_xy on the stores as they lie on the device, the row statuses of both halves given"""
    lower = {i: (_host(d[:(1 << i) * ncols * 64]), _host(m[:64 << i]), prf) for i, (d, m, prf) in f["lower"].items()}
    y = {i: (_host(d[:(1 << i) * ncols * 64]), _host(m[:64 << i]), prf, _host(a[:64 << i]) if a is not None else None)
         for i, (d, m, prf, a) in f["y"].items()}
    top = None
    if f["top"]:
        rows, macs, prf, align = f["top"]
        top = (_host(rows), _host(macs), prf, _host(align) if align is not None else None)
    return xm.extract_xy(em.File(n, ncols, F.curve, f["write_step"], lower, top, top_form or F.top_form), y, mask, statuses=statuses,
                         status_y=status_y)


def as_existing(got):
    """the outputs the call without Y halves has"""
    return {"blocks": got["blocks"], "steps": got["steps"], "flags": got["flags"], "row_status": got["row_status"], "counts": got["counts"][:4]}


def flipped(t, byte, bit=1):
    c = t.clone()
    c[byte] ^= bit
    return c


def with_lower(f, level, **kw):
    """f with level's X half (data=, macs=) or Y half (data_y=, macs_y=, prf_y=, align_y=) replaced"""
    d, m, p = f["lower"][level]
    dy, my, py, ay = f["y"][level]
    return dict(f, lower={**f["lower"], level: (kw.get("data", d), kw.get("macs", m), p)},
                y={**f["y"], level: (kw.get("data_y", dy), kw.get("macs_y", my), kw.get("prf_y", py), kw.get("align_y", ay))})


def level_statuses(t, n, level, rows_in_level, total):
    off, _ = em.row_offsets(t, n, True)
    return bytes(0 if r - off[level] in rows_in_level and off[level] <= r < off[level] + (1 << level) else 1 for r in range(total))


# ---- 1. no level to try: the existing call
@pytest.mark.parametrize("curve", CURVES)
def test_without_a_level_to_try_the_call_is_the_existing_one(curve):
    """y_levels = 0 and NULL Y pointers, t = 0 .. 7: every output and counts[0 .. 3] are porla_*_extract_batch_device's on the same stores,
    also under a damaged level; y_levels with no bit of t likewise"""
    import torch
    F = XyFlow(curve, torch.cuda.Stream(), chunk0=lambda rnd, s, i: em.with_index(i, [rnd.getrandbits(256)])[0])
    for t in range(0, 8):
        f = F.file(t)
        got, = extract_xy(F, [f], [0], stream=F.stream, null_y=True)
        want, = te.extract(F, [f], stream=F.stream)
        assert as_existing(got) == want and got["counts"][4:] == [0, 0], "t = %d" % t
        assert want["counts"] == [0, 0, 0, 0] and want["row_status"] == bytes([1] * (t + N))
    f = F.file(7)
    d, m, prf = f["lower"][1]
    g = dict(f, lower={**f["lower"], 1: (flipped(d, 64 * (NCOLS + 5) + 1), m, prf)})
    want, = te.extract(F, [g], stream=F.stream)
    got, = extract_xy(F, [g], [8], stream=F.stream, null_y=True)              # (level 3 is not resident: y_levels & t == 0)
    assert as_existing(got) == want and want["counts"][0] == 1
    got, = extract_xy(F, [g], [0], stream=F.stream)                            # with the Y pointers given: the statuses say NOT_TRIED
    assert as_existing(got) == want and got["row_status_y"] == bytes([xm.NOT_TRIED] * 7) and got["counts"][4:] == [0, 0]


# ---- 2. a clean file, every Y half tried
@pytest.mark.parametrize("curve", CURVES)
def test_a_clean_file_with_every_y_half_tried(curve):
    import torch
    F = XyFlow(curve, torch.cuda.Stream())
    f = F.file(7)
    got, = extract_xy(F, [f], [ALL], stream=F.stream)
    assert got["row_status_y"] == bytes([1] * 7) and got["row_status"] == bytes([1] * 15) and got["counts"] == [0] * 6
    shim = types.SimpleNamespace(S=F.S, curve=curve, ncols=NCOLS, n=N)
    off, _ = em.row_offsets(7, N, True)
    for i, lo, hi in em.resident_levels(7, N):
        if i == 0:
            continue                                               # (one row: below the aligned retrieval's smallest level)
        dy, my, py, ay = f["y"][i]
        k = 1 << i
        st, _, out = ta.retrieve_half(shim, dy[:k * NCOLS * 64], my[:64 * k], py, ay[:64 * k], [N + s for s in range(lo, hi + 1)], k,
                                      "residue64", F.stream)
        assert got["row_status_y"][off[i]:off[i] + k] == st, "level %d" % i
        assert out == ta.chunk_bytes([F.blocks[s] for s in range(lo, hi + 1)], P), "level %d" % i
        assert any(_host(ay[64 * j:64 * j + 64]) != bytes(64) for j in range(k))
    want, = te.extract(F, [f], stream=F.stream)
    assert as_existing(got) == want
    assert got == model_of(F, f, ALL, bytes([1] * 15), bytes([1] * 7))
    te_check = [(c, r) for c, r in F.want(7)]
    assert got["steps"] == [r for _, r in te_check] and got["blocks"] == ta.chunk_bytes([c for c, _ in te_check])


# ---- 3. a level whose X half fails comes back from its Y half
@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_x_half_is_recovered_from_the_y_half(curve):
    """one X symbol flipped in level 0, 1 and 2 in turn at t = 7, chunk 0 of every block in [D, p_icc): with the bit set the level's
    blocks come back mod p_icc with FROM_Y, no slot is UNSURE and counts = [1, 0, 0, 0, 0, 0]; with it clear, the existing call's outputs"""
    import torch
    F = XyFlow(curve, torch.cuda.Stream())
    f = F.file(7)
    clean, = te.extract(F, [f], stream=F.stream)
    for level, row in ((0, 0), (1, 1), (2, 2)):
        what = "level %d" % level
        g = with_lower(f, level, data=flipped(f["lower"][level][0], 64 * (row * NCOLS + 77) + 3))
        st = level_statuses(7, N, level, {row}, 15)
        for mask in (1 << level, ALL):
            got, = extract_xy(F, [g], [mask], stream=F.stream)
            assert got["row_status"] == st and got["row_status_y"].count(1) == (7 if mask == ALL else 1 << level), what
            assert got["row_status_y"].count(xm.NOT_TRIED) == (0 if mask == ALL else 7 - (1 << level)), what
            assert got == model_of(F, g, mask, st, bytes([1] * 7)), what
            assert got["counts"] == [1, 0, 0, 0, 0, 0] and got["steps"] == clean["steps"], what
            assert not any(x & xm.UNSURE for x in got["flags"]), what
            lo, hi = [(lo, hi) for i, lo, hi in em.resident_levels(7, N) if i == level][0]
            for slot, (chunks, rank) in enumerate(F.want(7)):
                y_won = lo <= rank <= hi
                assert got["flags"][slot] == (Y_WON if y_won else xm.FOUND), "%s slot %d" % (what, slot)
                assert got["blocks"][slot * 32 * NCOLS:(slot + 1) * 32 * NCOLS] == ta.chunk_bytes([chunks], P if y_won else None), "%s slot %d" % (what, slot)
            assert Y_WON in got["flags"], what
        want, = te.extract(F, [g], stream=F.stream)
        for mask in (0, 7 & ~(1 << level)):
            got, = extract_xy(F, [g], [mask], stream=F.stream)
            assert as_existing(got) == want and want["counts"][0] == 1 and got["counts"][4:] == [0, 0], what


# ---- 4. the Y tamper sweep on level 2
@pytest.mark.parametrize("curve", CURVES)
def test_y_tamper_sweep(curve):
    """one bit in a symbol, a MAC row, an alignment row and a PRF value of level 2's Y half each fail exactly their Y row, counts[4] is 1
    and nothing else changes while the X half is clean; with the X half damaged too the level is failed"""
    import torch
    F = XyFlow(curve, torch.cuda.Stream())
    f = F.file(7)
    dy, my, py, ay = f["y"][2]
    clean, = te.extract(F, [f], stream=F.stream)
    prf_bad = list(py)
    prf_bad[2] ^= 1 << 45
    cases = [(1, dict(data_y=flipped(dy, 64 * (1 * NCOLS + 77) + 3))), (3, dict(macs_y=flipped(my, 64 * 3 + 40, 0x80))),
             (0, dict(align_y=flipped(ay, 64 * 0 + 63, 2))), (2, dict(prf_y=prf_bad))]
    bad_x = flipped(f["lower"][2][0], 64 * (2 * NCOLS + 9) + 1)
    st_x = level_statuses(7, N, 2, {2}, 15)
    for row, change in cases:
        what = "row %d %s" % (row, sorted(change))
        sy = bytes(0 if r == 3 + row else 1 for r in range(7))
        g = with_lower(f, 2, **change)
        got, = extract_xy(F, [g], [ALL], stream=F.stream)
        assert got["row_status_y"] == sy and got["counts"] == [0, 0, 0, 0, 1, 0], what
        assert as_existing(got) == clean and got == model_of(F, g, ALL, bytes([1] * 15), sy), what
        # the X half damaged as well: no source is left, the level is failed as in the call without Y halves
        g = with_lower(f, 2, data=bad_x, **change)
        got, = extract_xy(F, [g], [4], stream=F.stream)
        want, = te.extract(F, [g], stream=F.stream)
        sy4 = bytes(sy[r] if r >= 3 else xm.NOT_TRIED for r in range(7))
        assert got["row_status"] == st_x and got["row_status_y"] == sy4 and got["counts"][4:] == [1, 0], what
        assert as_existing(got) == want and got == model_of(F, g, 4, st_x, sy4), what
        assert not set(got["steps"]) & {1, 2, 3, 4} and Y_WON not in got["flags"], what


# ---- 5. the ambiguous index
def ambiguous_chunk0(shape):
    """chunk 0 per step of the three-write files of tests/test_extract_xy_cpu.py:ambiguity_case at n_total = 8: step 2 is ambiguous"""
    def chunk0(rnd, step, index):
        if step != 2:
            return xm.chunk0_certain(rnd, index) if step == 1 else em.with_index(index, [rnd.getrandbits(256)])[0]
        if shape == "wrap":
            return P + (rnd.randrange(1, D >> 64) << 64)                      # names index 1; mod p_icc its low 64 bits are 0
        return (rnd.randrange(1, D >> 64) << 64) | index
    return chunk0


AMBIGUOUS = {"wrap": ([1, 1, 2], [1, 3] + [em.NONE] * 6, {0}), "last": ([3, N, N], [em.NONE, em.NONE, 1] + [em.NONE] * 4 + [3], set()),
             "interior": ([3, 2, 2], [em.NONE, 3, 1] + [em.NONE] * 5, {2})}


@pytest.mark.parametrize("shape", sorted(AMBIGUOUS))
@pytest.mark.parametrize("curve", CURVES)
def test_an_ambiguous_block_is_set_aside(curve, shape):
    """three writes, no top level, level 1 (steps 1, 2) damaged in X and taken from Y: the block of step 2 is never taken, counts[5] is 1
    and UNSURE sits on exactly the doubted slots whose winner is older than step 2"""
    import torch
    indices, steps, unsure = AMBIGUOUS[shape]
    F = XyFlow(curve, torch.cuda.Stream(), indices=indices, top=None, chunk0=ambiguous_chunk0(shape))
    f = F.file(3, top=False)
    assert F.blocks[2][0] % P < D and (F.blocks[2][0] & xm.M64) == indices[1]
    g = with_lower(f, 1, data=flipped(f["lower"][1][0], 64 * 3 + 2))
    got, = extract_xy(F, [g], [2], stream=F.stream)
    assert got == model_of(F, g, 2, bytes([1, 0, 1]), bytes([1, 1, 1]))
    assert got["steps"] == steps and 2 not in got["steps"]
    assert got["counts"] == [1, 0, 0, N - 2 + len(unsure), 0, 1]
    assert {s for s in range(N) if got["flags"][s] & xm.UNSURE} == unsure
    assert got["flags"][steps.index(1)] & ~xm.UNSURE == Y_WON and got["flags"][steps.index(3)] == xm.FOUND
    # undamaged, the block is exact and bids for the slot it names
    got, = extract_xy(F, [f], [2], stream=F.stream)
    assert got["counts"] == [0, 0, 0, N - 2, 0, 0] and (2 in got["steps"]) == (shape == "wrap")


# ---- 6. a mixed batch, and the launch count
@pytest.mark.parametrize("curve", CURVES)
def test_three_files_with_different_masks_equal_three_calls_and_the_launch_count(curve):
    import torch
    from porla_amd import multiexp as mx
    F = XyFlow(curve, torch.cuda.Stream())
    f7 = F.file(7)
    files = [with_lower(f7, 1, data=flipped(f7["lower"][1][0], 64 * 9 + 1)), F.file(5, top=False, write_step=5), F.file(6)]
    files[1] = with_lower(files[1], 0, data=flipped(files[1]["lower"][0][0], 64 * 3 + 1, 0x10))
    masks = [2, 0, ALL]
    got = extract_xy(F, files, masks, stream=F.stream)
    for a, (f, mask) in enumerate(zip(files, masks)):
        assert got[a] == extract_xy(F, [f], [mask], stream=F.stream)[0], "file %d against its single call" % a
    assert got[0]["counts"] == [1, 0, 0, 0, 0, 0] and Y_WON in got[0]["flags"]
    assert got[1]["counts"][0] == 1 and got[1]["counts"][4:] == [0, 0] and got[1]["row_status_y"] == bytes([xm.NOT_TRIED] * 5)
    assert got[2]["counts"] == [0] * 6 and got[2]["row_status_y"] == bytes([1] * 6)

    def launches(fs, ms):
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        res = extract_xy(F, fs, ms)
        return sum(c for _, _, c in mx.profile_get()) - before, res

    mx.profile_enable(1)
    try:
        one, got1 = launches(files, masks)
        eight, got8 = launches(files + [files[a % 3] for a in range(5)], masks + [masks[a % 3] for a in range(5)])
        none, _ = launches([files[0]], [0])
        tried, _ = launches([files[0]], [2])
    finally:
        mx.profile_enable(0)
    assert one == eight and got1 == got and got8[:3] == got and got8[3:] == [got[a % 3] for a in range(5)]
    assert tried > none                                           # the step array and the Y decode of one level size


# ---- 7. the seams of the check's blocks: one synthetic file of n_total = 64, t = 63, every Y half tried
@functools.lru_cache(maxsize=None)
def synthetic_y(curve, n=64, ncols=NCOLS):
    """the Y halves of te.synthetic's levels by the model's networks, their rows' alpha-commitments, PRF values and alignments a_j G with
    known logarithms (one row of every half of four rows or more at infinity): computed once, shared, left unchanged"""
    _, blocks, _, _, _ = te.synthetic(curve)
    rnd = random.Random(6500)
    key = tr.commit_key(curve)
    out = {}
    for i, lo, hi in em.resident_levels(n - 1, n):
        rows = dm.level_y([blocks[s] for s in range(lo, hi + 1)], list(range(lo, hi + 1)), n, curve)
        logs = [rnd.randrange(1, 1 << 40) for _ in rows]
        if len(logs) >= 4:
            logs[len(logs) // 2] = 0
        out[i] = (rows, [model.alpha_commit(r, key) for r in rows], [rnd.getrandbits(128) for _ in rows], logs)
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_190_rows_across_the_block_seams(curve):
    """levels 0 .. 5 in both halves and the top level: the one 64-byte pass holds 63 X rows, 63 Y rows and 64 top rows -- row 62 is the
    last X row (level 5), row 63 level 0's Y row: the seam lies on a boundary of the 32-row evaluation blocks and the 64-row compare
    blocks; rows 125 | 126 are the seam between the Y halves and the top level inside a block.  Clean, then an X symbol of row 62 and a Y
    MAC byte of row 63 altered: exactly those rows fail"""
    import torch
    mdm = ta.mdm
    n = 64
    S = ta.Setup(curve)
    u, blocks, levels, commits, prf = te.synthetic(curve)
    ys = synthetic_y(curve)
    if curve == "bn254":
        call, aligned = te.calls_of(curve)
        xy = xy_call_of(curve)
    else:
        _, afb, hfb = tr.ipa_bases()
        call, aligned = te.calls_of(curve, afb, hfb, ta.IPA_ALPHA)
        xy = xy_call_of(curve, afb, hfb, ta.IPA_ALPHA)
    F = types.SimpleNamespace(curve=curve, call=call, xy=xy, top_form="exact", stream=torch.cuda.Stream(), S=types.SimpleNamespace(aligned=aligned))
    dev = {i: (_dev(model.rows_bytes(levels[i])), _dev(model.points_to_bytes(S.expected(commits[i], prf[i]))), prf[i]) for i in levels}
    dev_y = {}
    for i, (rows, cm, pv, logs) in ys.items():
        align_b = model.points_to_bytes([icc_py.ec_mul(curve, mdm.GEN[curve], a) if a else None for a in logs])
        dev_y[i] = (_dev(model.rows_bytes(rows)), _dev(model.points_to_bytes(S.expected_aligned(cm, pv, logs))), pv, _dev(align_b))
    f = {"write_step": 2 * n + 63, "lower": {i: dev[i] for i in range(6)}, "y": dev_y, "top": dev["top"] + (None,)}
    got, = extract_xy(F, [f], [ALL], stream=F.stream, n=n)
    assert got["row_status"] == bytes([1] * 127) and got["row_status_y"] == bytes([1] * 63) and got["counts"] == [0] * 6
    want, = te.extract(F, [f], stream=F.stream, n=n)
    assert as_existing(got) == want
    bad_x = flipped(dev[5][0], 64 * (31 * NCOLS + 100) + 2, 4)      # level 5 starts at row 31: its row 31 is row 62 of the pass
    bad_my = flipped(dev_y[0][1], 33)                               # level 0's Y row is row 63 of the pass
    g = with_lower(with_lower(f, 5, data=bad_x), 0, macs_y=bad_my)
    st, sy = bytes(0 if r == 62 else 1 for r in range(127)), bytes(0 if r == 0 else 1 for r in range(63))
    got, = extract_xy(F, [g], [ALL], stream=F.stream, n=n)
    assert got["row_status"] == st and got["row_status_y"] == sy
    assert got == model_of(F, g, ALL, st, sy, n=n)
    # level 5 is taken from its Y half: its blocks carry random chunks 0, so some are set aside; newer steps hold all their slots
    assert got["counts"][0] == 1 and got["counts"][4] == 1 and got["counts"][5] > 0 and got["steps"] == want["steps"]


# ---- 8. a second call on another stream while the first is in flight
@pytest.mark.parametrize("curve", CURVES)
def test_a_second_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    F = XyFlow(curve, torch.cuda.Stream())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    f7 = F.file(7)
    g = with_lower(f7, 2, data=flipped(f7["lower"][2][0], 64 * 5 + 1))
    one, = extract_xy(F, [g], [ALL], stream=F.stream)
    first = run_xy(F, [g for _ in range(6)], [ALL] * 6, stream=s1)
    second = run_xy(F, [F.file(t) for t in (5, 0, 6)], [ALL, ALL, 0], stream=s2)
    third = run_xy(F, [g], [4], stream=s1)
    assert one["counts"] == [1, 0, 0, 0, 0, 0] and one["flags"].count(Y_WON) == 1
    for got in first():
        assert got == one
    for got, t in zip(second(), (5, 0, 6)):
        assert got["row_status"] == bytes([1] * (t + N)) and got["counts"] == [0] * 6
        assert got["steps"] == [r for _, r in F.want(t)] and got["blocks"] == ta.chunk_bytes([c for c, _ in F.want(t)])
    assert as_existing(third()[0]) == as_existing(one)

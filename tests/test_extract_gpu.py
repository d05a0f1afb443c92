"""GPU box: the verified file extraction (porla_{kzg,ipa}_extract_batch_device) -- every resident level of a file checked row by row,
its X half decoded, the blocks merged per slot by "newest authentic copy wins" -- against the Python model tests/extract_model.py
(every output byte), against the existing per-level retrieval calls on the same stores (the row statuses), and in the flow the call
exists for: a top level left by a rebuild write, then up to seven writes through the client and server update batches with the block
index in chunk 0, everything on one stream.  Every comparison is byte equality; every output is pre-filled with a sentinel and a
256-byte guard behind it keeps it.

The KZG build draws its hiding base anew at every init_SRS, so every test builds its own file and installs no key after that."""
import functools
import random
import types

import pytest

from tests import common  # noqa: F401  (puts oracle/ on the path)
import icc_py
from tests import extract_model as em
from tests import icc_decode_model as dm
from tests import retrieve_model as model
from tests import test_retrieve_aligned_gpu as ta
from tests import test_retrieve_gpu as tr
from tests.update_model import pt_bytes, pt_tuple

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
SENTINEL, GUARD = tr.SENTINEL, tr.GUARD
_dev, _host = tr._dev, tr._host
N, NCOLS = 8, 128
INDICES = [3, 5, 3, 1, 5, 5, 3]           # writes 1 .. 7: 3 in levels 0, 1 and 2 at t = 7; 5 twice inside level 1 (steps 5, 6); 2, 4, 6, 7 never
REBUILT = 8                               # the index the rebuild write itself carries


def block_of(rnd, index, ncols=NCOLS):
    return em.with_index(index, [rnd.getrandbits(256) for _ in range(ncols)])


def calls_of(curve, afb=None, hfb=None, alpha=None):
    """(the extraction, the aligned retrieval) of a build, as calls that take a stream"""
    from porla_amd import multiexp as mx
    if curve == "bn254":
        return (lambda reqs, n, form, s=0: mx.kzg_extract_batch_device(reqs, n, form, s),
                lambda reqs, n_rows, n, form, s=0: mx.kzg_retrieve_aligned_batch_device(reqs, n_rows, n, form, s))
    return (lambda reqs, n, form, s=0: afb.ipa_extract_batch_device(hfb, alpha, reqs, n, form, s),
            lambda reqs, n_rows, n, form, s=0: afb.ipa_retrieve_aligned_batch_device(hfb, alpha, reqs, n_rows, n, form, s))


class ExFlow:
    """a file of n_total = 8 in HBM.  top: "exact" (client rebuild batch -> porla_server_rebuild_batch_device), "residue32" (... ->
    porla_*_server_rebuild_aligned_batch_device) or None; then one write per entry of `indices` through the client update batch and the
    server update batch, all on `stream`.  What the host keeps is what a client keeps: the PRF values every resident row is hidden
    with.  file(t) is the file as it stood after write t (the resident stores cloned then), file(0) the top level alone."""

    def __init__(self, curve, stream, indices=INDICES, top="exact", seed=5100):
        import torch
        from porla_amd import multiexp as mx
        from tests import test_client_rebuild_batch_gpu as cr, test_client_update_batch_gpu as cu, test_update_batch_gpu as ub
        from tests.client_update_model import n_prf
        from tests.update_model import FAMILIES, FileModel
        self.curve, self.n, self.ncols, self.stream, self.top_form = curve, N, NCOLS, stream, top or "exact"
        self.C = C = cu.setup_of(curve)
        self.h = C.h
        if curve == "bn254":                                      # the key, SRS and hiding point are process state: put ours in again
            mx.init_key(ub.TAU, ub.ALPHA)
            mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
            self.h = pt_tuple(mx.compute_digest_complement((1).to_bytes(16, "big")))
            self.call, aligned = calls_of(curve)
        else:
            self.call, aligned = calls_of(curve, C.afb, C.hfb, C.alpha)
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
            chunks = block_of(rnd, index)
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
            with torch.cuda.stream(stream):                       # the resident X halves as they stand now, cloned in stream order
                self.snap[s] = {i: (self.d.t["data_x"][i].clone(), self.d.t["mac_x"][i].clone(), list(self.hold[i][0])) for i in self.hold}
        stream.synchronize()

    def _rebuild(self, top, cr):
        import torch
        from tests import test_server_rebuild_aligned_batch_gpu as sra, test_server_rebuild_batch_gpu as sr
        from tests.client_rebuild_model import n_prf
        n, curve, rnd, C = self.n, self.curve, self.rnd, self.C
        _, client_call = cr.setup_of(curve)
        u = [block_of(rnd, b + 1) for b in range(n)]
        block = block_of(rnd, REBUILT)
        prf = [rnd.getrandbits(128) for _ in range(n_prf(n))]
        prf[REBUILT] = prf[0]                                     # complements_U of the written slot is the block's own
        old, new_x = prf[1:1 + n], prf[1 + n:1 + 2 * n]
        u_macs = [None if i == REBUILT - 1 else icc_py.ec_add(curve, C.block_commit(u[i]), icc_py.ec_mul(curve, self.h, old[i])) for i in range(n)]
        mod = sr if top == "exact" else sra
        d = mod.DevFile(n, b"".join(sr.block_bytes(c) for c in u), b"".join(pt_bytes(p) for p in u_macs))
        d_block, d_prf = _dev(sr.block_bytes(block)), _dev(ta.raw_prf(curve, prf))
        d_mac = torch.full((64 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_comp = torch.full((128 * n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.keep += [d, d_block, d_prf, d_mac, d_comp]
        torch.cuda.synchronize()
        client_call([(d_block.data_ptr(), d_prf.data_ptr(), d_mac.data_ptr(), d_comp.data_ptr(), n)], n, self.stream.cuda_stream)
        req = d.req(d_block, d_mac, d_comp, n, REBUILT)
        if top == "exact":
            sr.call([req], n, curve, self.stream.cuda_stream)
        else:
            sra.call(curve, [req], n, self.stream.cuda_stream)
        u[REBUILT - 1] = block
        self.u = u
        symb = 64 if top == "exact" else 32
        self.top = (d.t["data_x"][:n * NCOLS * symb], d.t["mac_x"][:64 * n], new_x, d.t["align_x"][:64 * n] if top != "exact" else None)

    def file(self, t, top=True, write_step=None):
        return {"write_step": self.base + t if write_step is None else write_step, "lower": dict(self.snap[t]), "top": self.top if top else None}

    def want(self, t, top=True):
        """(chunks or None, rank or None) per slot: the last write of the index among the steps 1 .. t, else U (mod p_icc from an aligned
        top level), else nothing"""
        mod = icc_py.P_ICC if self.top_form == "residue32" else None
        out = [([c % mod if mod else c for c in self.u[b]], 0) if top and self.u else (None, None) for b in range(self.n)]
        for s in range(1, t + 1):
            out[INDICES[s - 1] - 1] = (self.blocks[s], s)
        return out


def run_extract(F, files, stream=None, call=None, n=N, ncols=NCOLS, top_form=None, want_counts=True):
    """one call.  files: dicts {"write_step", "lower": {level: (data tensor, MAC tensor, PRF integers)}, "top": None or (rows, macs, PRF
    integers, align or None)}.  Returns per file the outputs as em.extract names them; the guards behind every output are checked"""
    import torch
    logn = n.bit_length() - 1
    bb = ncols * 32
    full = lambda size: torch.full((size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    bufs, reqs, keep = [], [], []
    for f in files:
        t = f["write_step"] % n
        rows = t + (n if f["top"] else 0)
        prf = [v for i in sorted(f["lower"]) for v in f["lower"][i][2]] + (f["top"][2] if f["top"] else [])
        assert len(prf) == rows and sorted(f["lower"]) == [i for i, _, _ in em.resident_levels(t, n)]
        d_prf = _dev(ta.raw_prf(F.curve, prf)) if rows else None
        b = {"work": full(t * bb), "blocks": full(n * bb), "steps": full(4 * n), "flags": full(n), "row_status": full(rows),
             "counts": full(16) if want_counts else None, "sizes": {"work": t * bb, "blocks": n * bb, "steps": 4 * n, "flags": n, "row_status": rows,
                                                                      "counts": 16}}
        ptr = lambda x: x.data_ptr() if x is not None else 0
        fam = lambda k: [ptr(f["lower"][i][k]) if i in f["lower"] else 0 for i in range(logn)] if t else None
        top = f["top"] or (None, None, None, None)
        reqs.append((f["write_step"], fam(0), fam(1), ptr(top[0]), ptr(top[1]), ptr(top[3]), ptr(d_prf), b["work"].data_ptr() if t else 0,
                     b["blocks"].data_ptr(), b["steps"].data_ptr(), b["flags"].data_ptr(), b["row_status"].data_ptr() if rows else 0,
                     ptr(b["counts"])))
        bufs.append(b)
        keep.append(d_prf)
    torch.cuda.synchronize()
    (call or F.call)(reqs, n, top_form or F.top_form, stream.cuda_stream if stream is not None else 0)
    return lambda: collect(bufs, stream, n, want_counts)


def collect(bufs, stream, n, want_counts=True):
    import torch
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    res = []
    for a, b in enumerate(bufs):
        for name, size in b["sizes"].items():
            if b[name] is not None:
                assert bool(torch.all(b[name][size:] == SENTINEL)), "file %d: the guard behind %s changed" % (a, name)
        res.append({"blocks": _host(b["blocks"][:b["sizes"]["blocks"]]), "steps": b["steps"][:4 * n].cpu().view(torch.int32).tolist(),
                    "flags": _host(b["flags"][:n]), "row_status": _host(b["row_status"][:b["sizes"]["row_status"]]),
                    "counts": b["counts"][:16].cpu().view(torch.int32).tolist() if want_counts else None})
        res[-1]["steps"] = [s & 0xffffffff for s in res[-1]["steps"]]
    return res


def extract(F, files, **kw):
    return run_extract(F, files, **kw)()


def model_of(F, f, statuses, n=N, ncols=NCOLS, top_form=None):
    """em.extract on the stores as they lie on the device, the row statuses given"""
    lower = {i: (_host(d[:(1 << i) * ncols * 64]), _host(m[:64 << i]), prf) for i, (d, m, prf) in f["lower"].items()}
    top = None
    if f["top"]:
        rows, macs, prf, align = f["top"]
        top = (_host(rows), _host(macs), prf, _host(align) if align is not None else None)
    return em.extract(em.File(n, ncols, F.curve, f["write_step"], lower, top, top_form or F.top_form), statuses=statuses)


def existing_statuses(F, f, level0=1, n=N, ncols=NCOLS, top_form=None):
    """the row statuses the per-level aligned retrieval gives on the same stores, in d_row_status's order; level 0 (one row: below that
    call's smallest level) is `level0`"""
    shim = types.SimpleNamespace(S=F.S, curve=F.curve, ncols=ncols, n=n)
    out = b""
    for i in sorted(f["lower"]):
        d, m, prf = f["lower"][i]
        if i == 0:
            out += bytes([level0])
            continue
        out += ta.retrieve_half(shim, d[:(1 << i) * ncols * 64], m[:64 << i], prf, None, None, 1 << i, "exact", F.stream, want_out=False)[0]
    if f["top"]:
        rows, macs, prf, align = f["top"]
        out += ta.retrieve_half(shim, rows, macs, prf, align, None, n, top_form or F.top_form, F.stream, want_out=False)[0]
    return out


def check_against_written(F, got, t, top=True):
    for slot, (chunks, rank) in enumerate(F.want(t, top)):
        blk = got["blocks"][slot * 32 * NCOLS:(slot + 1) * 32 * NCOLS]
        if chunks is None:
            assert blk == bytes(32 * NCOLS) and got["steps"][slot] == em.NONE and got["flags"][slot] == 0, "slot %d" % slot
        else:
            residue = em.RESIDUE if rank == 0 and F.top_form == "residue32" else 0
            assert blk == ta.chunk_bytes([chunks]) and got["steps"][slot] == rank and got["flags"][slot] == em.FOUND | residue, "slot %d" % slot


# ---- 1. a clean file after each of its writes
@pytest.mark.parametrize("curve", CURVES)
def test_a_clean_file_after_each_write(curve):
    """exact top level, then t = 1 .. 7: all occupancy patterns of three levels, level 0 alone included.  Every output byte is the
    model's, the statuses are the per-level calls', and the blocks are what was written"""
    import torch
    F = ExFlow(curve, torch.cuda.Stream())
    for t in range(0, 8):
        f = F.file(t)
        got, = extract(F, [f], stream=F.stream)
        st = existing_statuses(F, f)
        assert got["row_status"] == st == bytes([1] * (t + N)), "t = %d" % t
        assert got == dict(model_of(F, f, st)), "t = %d" % t
        assert got["counts"] == [0, 0, 0, 0]
        check_against_written(F, got, t)


# ---- 2. no top level
@pytest.mark.parametrize("curve", CURVES)
def test_without_a_top_level_unwritten_slots_are_empty(curve):
    import torch
    F = ExFlow(curve, torch.cuda.Stream(), top=None)
    for t in (7, 4):
        f = F.file(t, top=False)
        got, = extract(F, [f], stream=F.stream)
        assert got == model_of(F, f, bytes([1] * t)), "t = %d" % t
        check_against_written(F, got, t, top=False)
        assert got["counts"] == [0, 0, 0, N - len(set(INDICES[:t]))]
    # nothing resident at all: every slot empty, no row, no status
    got, = extract(F, [F.file(0, top=False)], stream=F.stream)
    assert got["blocks"] == bytes(N * NCOLS * 32) and got["steps"] == [em.NONE] * N and got["flags"] == bytes(N) and got["counts"] == [0, 0, 0, N]


# ---- 3. the tamper sweep at t = 7
@pytest.mark.parametrize("curve", CURVES)
def test_tamper_sweep(curve):
    """one data symbol in level 0, 1, 2 and the top level, one MAC row in level 1: exactly that row's status is 0, no block of that level
    is taken, the slots whose winner is newer than the failed level carry no UNSURE and all others carry it"""
    import torch
    F = ExFlow(curve, torch.cuda.Stream())
    f = F.file(7)
    off, rows = em.row_offsets(7, N, True)
    hi = {0: 7, 1: 6, 2: 4, "top": 0}
    steps_of = {0: {7}, 1: {5, 6}, 2: {1, 2, 3, 4}, "top": {0}}

    def flipped(t, byte):
        c = t.clone()
        c[byte] ^= 1
        return c

    cases = []                                                    # (level, row in the level, the tampered file)
    for level, row in ((0, 0), (1, 1), (2, 2)):
        d, m, prf = f["lower"][level]
        cases.append((level, row, dict(f, lower={**f["lower"], level: (flipped(d, 64 * (row * NCOLS + 77) + 3), m, prf)})))
    rt, mt, pt, at = f["top"]
    cases.append(("top", 5, dict(f, top=(flipped(rt, 64 * (5 * NCOLS + 1) + 9), mt, pt, at))))
    d, m, prf = f["lower"][1]
    cases.append((1, 0, dict(f, lower={**f["lower"], 1: (d, flipped(m, 40), prf)})))
    for level, row, g in cases:
        what = "level %s row %d" % (level, row)
        got, = extract(F, [g], stream=F.stream)
        want_st = bytes(0 if r == off[level] + row else 1 for r in range(rows))
        assert got["row_status"] == want_st, what
        assert existing_statuses(F, g, level0=0 if level == 0 else 1) == want_st, what
        assert got == model_of(F, g, want_st), what
        assert not set(got["steps"]) & steps_of[level], what
        for slot in range(N):
            rank = -1 if got["steps"][slot] == em.NONE else got["steps"][slot]
            assert bool(got["flags"][slot] & em.UNSURE) == (hi[level] > rank), "%s slot %d" % (what, slot)
        assert got["counts"][0] == 1 and got["counts"][2] == 0, what


# ---- 4. indices out of range
@pytest.mark.parametrize("curve", CURVES)
def test_indices_out_of_range_are_counted_and_dropped(curve):
    import torch
    F = ExFlow(curve, torch.cuda.Stream(), indices=[0, N + 1, 2], top=None)
    f = F.file(3, top=False)
    got, = extract(F, [f], stream=F.stream)
    assert got == model_of(F, f, bytes([1] * 3))
    assert got["counts"] == [0, 0, 2, N - 1]
    assert got["steps"] == [em.NONE, 3] + [em.NONE] * (N - 2) and got["flags"] == bytes([0, em.FOUND] + [0] * (N - 2))
    assert got["blocks"][32 * NCOLS:64 * NCOLS] == ta.chunk_bytes([F.blocks[3]])


# ---- 5. the aligned top level
@pytest.mark.parametrize("curve", CURVES)
def test_an_aligned_top_level_under_lower_level_writes(curve):
    """RESIDUE32 from the aligned rebuild write, finite alignments among its rows, three writes on top: the top level's slots are the
    chunks mod p_icc with RESIDUE, the lower levels' winners exact without it"""
    import torch
    F = ExFlow(curve, torch.cuda.Stream(), indices=INDICES[:3], top="residue32")
    assert any(_host(F.top[3][64 * j:64 * j + 64]) != bytes(64) for j in range(N))
    for t in (0, 3):
        f = F.file(t)
        got, = extract(F, [f], stream=F.stream)
        st = existing_statuses(F, f)
        assert got["row_status"] == st == bytes([1] * (t + N)), "t = %d" % t
        assert got == model_of(F, f, st), "t = %d" % t
        check_against_written(F, got, t)
        assert got["flags"].count(em.FOUND | em.RESIDUE) == N - len(set(INDICES[:t]))
    # without the alignment store the rows with a finite alignment fail, and with them the top level
    rows, macs, prf, align = F.top
    g = dict(F.file(3), top=(rows, macs, prf, None))
    got, = extract(F, [g], stream=F.stream)
    finite = bytes(0 if _host(align[64 * j:64 * j + 64]) != bytes(64) else 1 for j in range(N))
    assert got["row_status"] == bytes([1] * 3) + finite and got == model_of(F, g, bytes([1] * 3) + finite)
    assert all(x in (em.UNSURE, em.FOUND) for x in got["flags"])


# ---- 6. a mixed batch
@pytest.mark.parametrize("curve", CURVES)
def test_three_files_in_one_call_equal_three_calls(curve):
    """write_step 7, 5 and 8 (t = 0), the middle one without a top level and with a tampered level 0: every output is byte-identical to
    the one-file calls"""
    import torch
    F = ExFlow(curve, torch.cuda.Stream())
    mid = F.file(5, top=False, write_step=5)
    d, m, prf = mid["lower"][0]
    bad = d.clone()
    bad[64 * 3 + 1] ^= 0x10
    mid["lower"][0] = (bad, m, prf)
    files = [F.file(7, write_step=7), mid, F.file(0, write_step=8)]
    got = extract(F, files, stream=F.stream)
    for a, f in enumerate(files):
        assert got[a] == extract(F, [f], stream=F.stream)[0], "file %d against its single call" % a
    assert got[0]["counts"] == [0, 0, 0, 0] and got[2]["counts"] == [0, 0, 0, 0] and got[1]["counts"][0] == 1
    assert got[1]["row_status"] == bytes([0, 1, 1, 1, 1]) and got[1] == model_of(F, mid, bytes([0, 1, 1, 1, 1]))
    check_against_written(F, got[0], 7)
    check_against_written(F, got[2], 0)


# ---- 7. the seams of the check's blocks: one synthetic file of n_total = 64, t = 63
@functools.lru_cache(maxsize=None)
def synthetic(curve, n=64, ncols=NCOLS):
    """blocks of the steps 1 .. 63 and U, their levels by the model's networks, the rows' alpha-commitments (they do not depend on the
    hiding base): computed once, shared, left unchanged"""
    rnd = random.Random(6400)
    u = [block_of(rnd, b + 1, ncols) for b in range(n)]
    blocks = {s: block_of(rnd, 1 + (5 * s) % 40, ncols) for s in range(1, n)}
    levels = {i: dm.level_x([blocks[s] for s in range(lo, hi + 1)], n, curve) for i, lo, hi in em.resident_levels(n - 1, n)}
    levels["top"] = icc_py.crebuild(u, curve, 0)[0]
    key = tr.commit_key(curve)
    commits = {i: [model.alpha_commit(r, key) for r in rows] for i, rows in levels.items()}
    prf = {i: [rnd.getrandbits(128) for _ in rows] for i, rows in levels.items()}
    return u, blocks, levels, commits, prf


@pytest.mark.parametrize("curve", CURVES)
def test_127_rows_across_the_block_seams(curve):
    """levels 0 .. 5 and the top level: the rows 0 .. 126 of the one 64-byte pass cross the 32-row evaluation blocks and the 64-row
    compare blocks; rows 31 | 32 lie inside level 5, 63 | 64 is the seam between the top level's rows 0 and 1.  Clean, then a symbol of row 32
    and a MAC byte of row 64 altered"""
    import torch
    n = 64
    S = tr.Setup(curve)
    u, blocks, levels, commits, prf = synthetic(curve)
    if curve == "bn254":
        call, aligned = calls_of(curve)
    else:
        _, afb, hfb = tr.ipa_bases()
        call, aligned = calls_of(curve, afb, hfb, ta.IPA_ALPHA)   # (no alignment is finite here: alpha is never used)
    F = types.SimpleNamespace(curve=curve, call=call, top_form="exact", stream=torch.cuda.Stream(), S=types.SimpleNamespace(aligned=aligned))
    dev = {i: (_dev(model.rows_bytes(levels[i])), _dev(model.points_to_bytes(S.expected(commits[i], prf[i]))), prf[i]) for i in levels}
    f = {"write_step": 2 * n + 63, "lower": {i: dev[i] for i in range(6)}, "top": dev["top"] + (None,)}
    got, = extract(F, [f], stream=F.stream, n=n)
    assert got["row_status"] == bytes([1] * 127) and got == model_of(F, f, bytes([1] * 127), n=n)
    want = [(u[b], 0) for b in range(n)]
    for s in range(1, n):
        want[(5 * s) % 40] = (blocks[s], s)
    assert got["steps"] == [r for _, r in want] and got["blocks"] == ta.chunk_bytes([c for c, _ in want])
    d5, m5, p5 = dev[5]
    bad_rows = d5.clone()
    bad_rows[64 * (1 * NCOLS + 100) + 2] ^= 4                      # level 5 starts at row 31: its row 1 is row 32 of the pass
    bad_macs = dev["top"][1].clone()
    bad_macs[64 * 1 + 33] ^= 1                                    # the top level starts at row 63
    g = {"write_step": f["write_step"], "lower": {**f["lower"], 5: (bad_rows, m5, p5)}, "top": (dev["top"][0], bad_macs, dev["top"][2], None)}
    st = bytes(0 if r in (32, 64) else 1 for r in range(127))
    got, = extract(F, [g], stream=F.stream, n=n)
    assert got["row_status"] == st and got == model_of(F, g, st, n=n)
    assert got["counts"][0] == 2 and all(s == em.NONE or s > 32 for s in got["steps"])      # (level 5 holds the steps 1 .. 32)


# ---- 8. the launch count
@pytest.mark.parametrize("curve", CURVES)
def test_launch_count_depends_on_the_sizes_present_only(curve):
    import torch
    from porla_amd import multiexp as mx
    F = ExFlow(curve, torch.cuda.Stream())

    def launches(files):
        torch.cuda.synchronize()
        before = sum(c for _, _, c in mx.profile_get())
        got = extract(F, files)
        return sum(c for _, _, c in mx.profile_get()) - before, got

    launches([F.file(7)])                                        # (tables and workspaces built outside the count)
    mx.profile_enable(1)
    try:
        one, got1 = launches([F.file(7)])
        eight, got8 = launches([F.file(7) for _ in range(8)])
        mixed, gotm = launches([F.file(t) for t in (7, 3, 5, 6)])
    finally:
        mx.profile_enable(0)
    assert one == eight == mixed and one >= 6                     # clear, evaluation / pack, compare, decodes, level 0, merge
    assert all(g == got1[0] for g in got8) and gotm[0] == got1[0]
    for g, t in zip(gotm, (7, 3, 5, 6)):
        check_against_written(F, g, t)


# ---- 9. a second call on another stream while the first is in flight (the pattern of tests/test_batch_scaffold_gpu.py)
@pytest.mark.parametrize("curve", CURVES)
def test_a_second_call_on_another_stream_while_the_first_is_in_flight(curve):
    import torch
    F = ExFlow(curve, torch.cuda.Stream())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = run_extract(F, [F.file(7) for _ in range(6)], stream=s1)
    second = run_extract(F, [F.file(t) for t in (5, 0, 6)], stream=s2)
    third = run_extract(F, [F.file(3)], stream=s1)
    for g in first():
        check_against_written(F, g, 7)
        assert g["counts"] == [0, 0, 0, 0]
    for g, t in zip(second(), (5, 0, 6)):
        check_against_written(F, g, t)
        assert g["row_status"] == bytes([1] * (t + N))
    check_against_written(F, third()[0], 3)

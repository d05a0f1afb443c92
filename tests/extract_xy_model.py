"""MODEL (test infrastructure only) of the file extraction with the Y halves (include/porla_gpu.h: porla_kzg_extract_xy_batch_device /
porla_ipa_extract_xy_batch_device) on top of tests/extract_model.py: the same File, beside it the resident Y halves of the lower levels
as the stores hold them, and the mask of the levels to try.

  1y. every row of a tried Y half gets the aligned retrieval's status (RESIDUE64, the half's alignment store); untried rows NOT_TRIED
  2y. the source of a level: X if its X half is clean, else Y if tried and clean, else the level is failed
  3y. a tried Y half decodes mod p_icc with the write steps of its blocks (one row: the unscale alone)
  4y. a block of a Y-sourced level bids with its epoch write step; a winner gives chunks mod p_icc and FOUND | RESIDUE | FROM_Y
  5y. r0 = chunk 0 mod p_icc, D = 2^256 - p_icc: r0 >= D names low64(r0); r0 < D names low64(r0) or low64(r0) + 1 -- none in range:
      dropped; otherwise set aside, counted, and a doubt of its step on every candidate slot in range
  6y. UNSURE iff a failed level's hi_i or the slot's doubt is greater than the winner's rank (none: -1)
  7y. counts = [X / top rows with status 0, bad symbols of the exact decodes, dropped blocks, slots not FOUND or UNSURE,
                tried Y rows with status 0, blocks set aside]

A helper of tests/test_extract_xy_*.py, not a test module."""
import icc_py
from tests import extract_model as em
from tests import icc_decode_model as dm
from tests import retrieve_aligned_model as am
from tests.update_model import pt_tuple

FOUND, UNSURE, RESIDUE, FROM_Y = em.FOUND, em.UNSURE, em.RESIDUE, 8
NOT_TRIED = 2
NONE = em.NONE
P = icc_py.P_ICC
D = (1 << 256) - P
M64 = (1 << 64) - 1
assert D == 49 * (1 << 248) - 1 and P & M64 == 1


def chunk0_certain(rng, index):
    """a chunk 0 naming `index` whose residue mod p_icc is certain: in [D, p_icc)"""
    while True:
        c = (rng.randrange(D >> 64, P >> 64) << 64) | index
        if D <= c < P:
            return c


def candidates(r0, n_total):
    """(certain, [indices in 1 .. n_total the block may name])"""
    a = r0 & M64
    cand = [a] if r0 >= D else [a, (a + 1) & M64]
    return r0 >= D, [x for x in cand if 1 <= x <= n_total]


def statuses_y(f, y, tried, key):
    """d_row_status_y by the aligned retrieval's relation on the tried halves; y: {level: (rows bytes, MAC bytes, [PRF integers],
    alignment bytes or None)}"""
    out = bytearray([NOT_TRIED] * f.t)
    for i, _, _ in em.resident_levels(f.t, f.n_total):
        if not tried >> i & 1:
            continue
        rows_b, macs, prf, align_b = y[i]
        align = [pt_tuple(align_b[64 * j:64 * j + 64]) if align_b else None for j in range(1 << i)]
        o = f.t & ((1 << i) - 1)
        out[o:o + (1 << i)] = am.statuses_aligned(am.rows_of(rows_b, f.n_cols, "residue64"), macs, prf, align, key)
    return bytes(out)


def decode_y(rows_b, n_rows, n_cols, n_total, steps):
    """the blocks of a Y half as lists of chunks mod p_icc"""
    rows = am.rows_of(rows_b, n_cols, "residue64")
    if n_rows == 1:
        return [[v % P * dm.unscale_factor(steps[0], n_total) % P for v in rows[0]]]
    return dm.decode_residue(rows, n_total, steps)


def extract_xy(f, y, y_levels, key=None, statuses=None, status_y=None):
    """em.extract's dictionary with six counts and "row_status_y".  status_y: t bytes given instead of computed (the entries of
    untried levels are not looked at)"""
    n, nc, t = f.n_total, f.n_cols, f.t
    tried = y_levels & t
    st = statuses if statuses is not None else em.row_statuses(f, key)
    off, rows = em.row_offsets(t, n, f.top is not None)
    assert len(st) == rows
    if status_y is None:
        sy = statuses_y(f, y, tried, key) if tried else bytes([NOT_TRIED] * t)
    else:
        assert len(status_y) == t
        sy = bytes(status_y[r] if tried >> i & 1 else NOT_TRIED for i, _, _ in em.resident_levels(t, n)
                   for r in range(off[i], off[i] + (1 << i)))
    best = [(-1, None, 0)] * n                                   # (rank, chunks, flags beside FOUND)
    doubt = [-1] * n
    failed_hi, bad, dropped, aside = [], 0, 0, 0
    if f.top:
        blocks, b = em.decode_level(f.top[0], n, nc, n, f.curve, f.top_form)
        bad += b
        if 0 in st[off["top"]:off["top"] + n]:
            failed_hi.append(0)
        else:
            best = [(0, blocks[s], RESIDUE if f.top_form == "residue32" else 0) for s in range(n)]
    for i, lo, hi in em.resident_levels(t, n):
        blocks, b = em.decode_level(f.lower[i][0], 1 << i, nc, n, f.curve)
        bad += b
        if 0 not in st[off[i]:off[i] + (1 << i)]:
            for p, chunks in enumerate(blocks):
                idx = chunks[0] & M64
                if not 1 <= idx <= n:
                    dropped += 1
                elif lo + p > best[idx - 1][0]:
                    best[idx - 1] = (lo + p, chunks, 0)
            continue
        if not tried >> i & 1 or 0 in sy[off[i]:off[i] + (1 << i)]:
            failed_hi.append(hi)
            continue
        epoch = f.write_step - t
        for p, chunks in enumerate(decode_y(y[i][0], 1 << i, nc, n, [epoch + lo + q for q in range(1 << i)])):
            certain, cand = candidates(chunks[0], n)
            if not cand:
                dropped += 1
            elif not certain:
                aside += 1
                for idx in cand:
                    doubt[idx - 1] = max(doubt[idx - 1], lo + p)
            elif lo + p > best[cand[0] - 1][0]:
                best[cand[0] - 1] = (lo + p, chunks, RESIDUE | FROM_Y)
    blocks_b, steps, flags = b"", [], []
    for slot, (rank, chunks, extra) in enumerate(best):
        unsure = any(hi > rank for hi in failed_hi) or doubt[slot] > rank
        blocks_b += b"".join(c.to_bytes(32, "little") for c in chunks) if chunks is not None else bytes(32 * nc)
        steps.append(rank if rank >= 0 else NONE)
        flags.append((FOUND if rank >= 0 else 0) | (UNSURE if unsure else 0) | extra)
    counts = [st.count(0), bad, dropped, sum(1 for x in flags if not x & FOUND or x & UNSURE), sy.count(0), aside]
    return {"blocks": blocks_b, "steps": steps, "flags": bytes(flags), "row_status": bytes(st), "row_status_y": sy, "counts": counts}


def y_from_model(m, prf_of):
    """the `y` of extract_xy from a FileModel's stores as they are: the resident Y halves with their alignment stores; prf_of(level) =
    that half's PRF integers"""
    y = {}
    for i, is_empty in enumerate(m.empty):
        if not is_empty:
            k = 1 << i
            y[i] = (bytes(m.fam["data_y"][i][:k * m.n_cols * 64]), bytes(m.fam["mac_y"][i][:64 * k]), prf_of(i),
                    bytes(m.fam["align_y"][i][:64 * k]))
    return y

"""MODEL (test infrastructure only) of the verified file extraction (include/porla_gpu.h: porla_kzg_extract_batch_device /
porla_ipa_extract_batch_device) on top of tests/retrieve_aligned_model.py (the row check), tests/icc_decode_model.py (the decodes) and
the hierarchy of tests/update_model.py:FileModel.

A file is a `File`: t = write_step % n_total, the resident X halves of the lower levels as the stores hold them (bytes), the top level
or None.  extract() gives every output of the call as bytes and lists:

  1. every resident row gets the aligned retrieval's status (or the caller passes the statuses in, where another call has made them)
  2. a level with a status-0 row is failed; no block of a failed level is taken
  3. a block of a clean lower level with index id in 1 .. n_total bids for slot id - 1 with its epoch write step as rank; block b of a
     clean top level bids for slot b with rank 0; the highest rank wins
  4. blocks / steps / flags per slot; UNSURE iff a failed level's highest write step is greater than the winner's rank (none: -1)
  5. indices 0 and above n_total are counted and dropped
  6. counts = [rows with status 0, bad symbols of the exact decodes, dropped blocks, slots not FOUND or UNSURE]

A helper of tests/test_extract_*.py, not a test module."""
import icc_py
from tests import icc_decode_model as dm
from tests import retrieve_aligned_model as am
from tests.update_model import pt_tuple

FOUND, UNSURE, RESIDUE = 1, 2, 4
NONE = 0xffffffff


def resident_levels(t, n_total):
    """[(level, first write step, highest write step hi_i)] of the resident lower levels, ascending; the steps are those of the epoch"""
    out = []
    for i in range(n_total.bit_length() - 1):
        if t >> i & 1:
            hi = t >> i << i
            out.append((i, hi - (1 << i) + 1, hi))
    return out


def row_offsets(t, n_total, has_top):
    """{level or "top": offset} in d_prf / d_row_status: resident levels ascending, 2^i rows each, then the top level; and the row count"""
    off, o = {}, 0
    for i, _, _ in resident_levels(t, n_total):
        off[i] = o
        o += 1 << i
    if has_top:
        off["top"] = o
        o += n_total
    return off, o


class File:
    def __init__(self, n_total, n_cols, curve, write_step, lower, top=None, top_form="exact"):
        """lower: {level: (X half bytes: 2^level rows of n_cols 64-byte symbols, MAC bytes, [PRF integers])} for every resident level;
        top: None or (rows bytes in top_form, MAC bytes, [PRF integers], alignment bytes or None)"""
        self.n_total, self.n_cols, self.curve, self.write_step = n_total, n_cols, curve, write_step
        self.t = write_step % n_total
        self.lower, self.top, self.top_form = lower, top, top_form
        assert sorted(lower) == [i for i, _, _ in resident_levels(self.t, n_total)]

    def prf_values(self):
        """the PRF values in the order of d_prf"""
        out = []
        for i, _, _ in resident_levels(self.t, self.n_total):
            out += self.lower[i][2]
        return out + (self.top[2] if self.top else [])


def row_statuses(f, key):
    """d_row_status by the aligned retrieval's relation"""
    out = b""
    for i, _, _ in resident_levels(f.t, f.n_total):
        rows_b, macs, prf = f.lower[i]
        out += am.statuses_aligned(am.rows_of(rows_b, f.n_cols, "exact"), macs, prf, [None] * (1 << i), key)
    if f.top:
        rows_b, macs, prf, align_b = f.top
        align = [pt_tuple(align_b[64 * j:64 * j + 64]) if align_b else None for j in range(f.n_total)]
        out += am.statuses_aligned(am.rows_of(rows_b, f.n_cols, f.top_form), macs, prf, align, key)
    return out


def decode_level(rows_b, n_rows, n_cols, n_total, curve, form="exact"):
    """(blocks as lists of chunks, bad symbols).  One row: the identity on the low 32 bytes, a nonzero upper half counted"""
    if n_rows == 1:
        vals = am.rows_of(rows_b, n_cols, "exact")[0]
        return [[v & ((1 << 256) - 1) for v in vals]], sum(1 for v in vals if v >> 256)
    if form == "exact":
        return dm.decode_exact(am.rows_of(rows_b, n_cols, "exact"), curve)
    return dm.decode_residue(am.rows_of(rows_b, n_cols, form), n_total), 0


def extract(f, key=None, statuses=None):
    """{"blocks": bytes, "steps": [..], "flags": bytes, "row_status": bytes, "counts": [4]}"""
    n, nc = f.n_total, f.n_cols
    st = statuses if statuses is not None else row_statuses(f, key)
    off, rows = row_offsets(f.t, n, f.top is not None)
    assert len(st) == rows
    best = [(-1, None, False)] * n                               # (rank, chunks, from a residue top level)
    failed_hi, bad, dropped = [], 0, 0
    if f.top:
        blocks, b = decode_level(f.top[0], n, nc, n, f.curve, f.top_form)
        bad += b
        if 0 in st[off["top"]:off["top"] + n]:
            failed_hi.append(0)
        else:
            best = [(0, blocks[s], f.top_form == "residue32") for s in range(n)]
    for i, lo, hi in resident_levels(f.t, n):
        blocks, b = decode_level(f.lower[i][0], 1 << i, nc, n, f.curve)
        bad += b
        if 0 in st[off[i]:off[i] + (1 << i)]:
            failed_hi.append(hi)
            continue
        for p, chunks in enumerate(blocks):
            idx = chunks[0] & ((1 << 64) - 1)
            if not 1 <= idx <= n:
                dropped += 1
            elif lo + p > best[idx - 1][0]:
                best[idx - 1] = (lo + p, chunks, False)
    blocks_b, steps, flags = b"", [], []
    for rank, chunks, residue in best:
        unsure = any(hi > rank for hi in failed_hi)
        blocks_b += b"".join(c.to_bytes(32, "little") for c in chunks) if chunks is not None else bytes(32 * nc)
        steps.append(rank if rank >= 0 else NONE)
        flags.append((FOUND if rank >= 0 else 0) | (UNSURE if unsure else 0) | (RESIDUE if residue else 0))
    counts = [st.count(0), bad, dropped, sum(1 for x in flags if not x & FOUND or x & UNSURE)]
    return {"blocks": blocks_b, "steps": steps, "flags": bytes(flags), "row_status": bytes(st), "counts": counts}


def with_index(index, chunks):
    """the chunks of a block that names `index`: the low 8 bytes of chunk 0, little-endian"""
    return [(chunks[0] >> 64 << 64) | index] + list(chunks[1:])


def lower_from_model(m, prf_of):
    """the `lower` of a File from a FileModel's stores as they are: the resident X halves; prf_of(level) = that half's PRF integers, added
    to the stored MAC rows as complements by the caller where the model holds none"""
    lower = {}
    for i, is_empty in enumerate(m.empty):
        if not is_empty:
            n = 1 << i
            lower[i] = (bytes(m.fam["data_x"][i][:n * m.n_cols * 64]), bytes(m.fam["mac_x"][i][:64 * n]), prf_of(i))
    return lower


assert icc_py.P_ICC < 1 << 256

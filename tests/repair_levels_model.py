"""MODEL (test infrastructure only) of the lower-level repair (include/porla_gpu.h: porla_kzg_repair_levels_batch_device /
porla_ipa_repair_levels_batch_device) on Python integers and affine points, on top of oracle/icc_py.py, tests/icc_decode_model.py (the
exact decode) and tests/retrieve_aligned_model.py (the row check and the expected MACs).

The two facts the call rests on, as functions:
  y_half(chunks, steps, n_total, curve)      the resident Y half of a level = the one-shot network (icc_py.crebuild(rows, curve, 0)[0])
                                             over the rows y_p = chunk_p wt_p mod p_icc; level 0's one row is the input row itself
  align_scalars(chunks, steps, n_total, curve)   N mod q, N the same network over the rows c_p = (y_p - chunk_p wt_p) mod q: row j of
                                             the Y alignment store is Commit(N_j mod q)
and the rules 2 .. 7 of the header in repair_levels().  A level is {"x": (rows bytes, MAC bytes, [PRF integers]), "y": (rows bytes, MAC
bytes, [PRF integers], alignment bytes)}, 64-byte symbols.

A helper of tests/test_repair_levels_*.py, not a test module."""
import icc_py
from tests import icc_decode_model as dm
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model
from tests.update_model import pt_bytes, pt_tuple

DATA, MAC, ALIGN = 1, 2, 8
CLEAN, X_DAMAGED, INCONSISTENT, REPAIRED = 1, 2, 3, 4
NOT_TRIED = 2
P = icc_py.P_ICC
WORK_PER_SYMBOL = 200          # porla_repair_levels_work_bytes = 200 * n_cols * (levels & write_step % n_total)


def work_bytes(n_total, n_cols, write_step, levels):
    if n_total < 2 or n_total & (n_total - 1) or n_total > 1 << 16:
        return 0
    return WORK_PER_SYMBOL * n_cols * (levels & (write_step % n_total))


def level_steps(write_step, n_total, i):
    """rule 3y of the extraction: the write steps of the entries of level i, oldest first"""
    t = write_step % n_total
    lo = write_step - t + (t & ~((2 << i) - 1)) + 1
    return [lo + p for p in range(1 << i)]


def wt_of(n_total, step):
    return pow(icc_py.root_w(n_total), icc_py.reverse_bits(step % n_total, n_total.bit_length() - 1), P)


def hadd_rows(chunks, steps, n_total, curve):
    """per block (y_p, c_p): chunk wt mod p_icc, and (y_p - chunk wt) mod q with the block's own wt"""
    q = icc_py.Q[curve]
    ys, cs = [], []
    for row, step in zip(chunks, steps):
        wt = wt_of(n_total, step)
        ys.append([c * wt % P for c in row])
        cs.append([(c * wt % P - c * wt) % q for c in row])
    return ys, cs


def network(rows, curve):
    """the one-shot forward network; one row is its own network"""
    return [list(r) for r in rows] if len(rows) == 1 else icc_py.crebuild(rows, curve, 0)[0]


def y_half(chunks, steps, n_total, curve):
    return network(hadd_rows(chunks, steps, n_total, curve)[0], curve)


def align_scalars(chunks, steps, n_total, curve):
    q = icc_py.Q[curve]
    return [[v % q for v in r] for r in network(hadd_rows(chunks, steps, n_total, curve)[1], curve)]


def decode_x(rows, curve):
    """(chunks, bad symbols) of an X half; level 0's row as it lies, a symbol with a nonzero upper half is bad"""
    if len(rows) == 1:
        return [[v & ((1 << 256) - 1) for v in rows[0]]], sum(1 for v in rows[0] if v >> 256)
    return dm.decode_exact(rows, curve)


def resident(write_step, n_total, levels):
    t = write_step % n_total
    return [i for i in range(n_total.bit_length() - 1) if (levels & t) >> i & 1]


def offsets(t, n_total):
    return {i: t & ((1 << i) - 1) for i in range(n_total.bit_length() - 1) if t >> i & 1}


def repair_levels(file_levels, n_total, n_cols, curve, write_step, levels, commit, key=None, statuses=None, mac_of=None):
    """one file.  file_levels: {level: {"x": ..., "y": ...}} as the stores lie (every resident level of the mask at least).  commit(row
    of scalars) -> the affine point Commit(row).  The statuses are computed with `key` or given as {level: (status_x, status_y)};
    mac_of(level, row indices, rows of integers, prf, alignment points) -> the expected MAC points, by default the aligned retrieval
    model's with `key`.  Returns {"status_x", "status_y", "action_y" (t bytes each), "level" (16 bytes), "counts", "y": {level: (rows
    bytes, MAC bytes, alignment bytes)}}"""
    t = write_step % n_total
    off = offsets(t, n_total)
    rb = 64 * n_cols
    st_x, st_y, action = bytearray([NOT_TRIED] * t), bytearray([NOT_TRIED] * t), bytearray(t)
    verdict, counts, out_y = bytearray(16), [0] * 8, {}
    for i in resident(write_step, n_total, levels):
        n = 1 << i
        x, y = file_levels[i]["x"], file_levels[i]["y"]
        rows_x, rows_y = am.rows_of(x[0][:n * rb], n_cols, "exact"), am.rows_of(y[0][:n * rb], n_cols, "exact")
        align_y = [pt_tuple(y[3][64 * j:64 * j + 64]) for j in range(n)]
        if statuses is not None:
            sx, sy = statuses[i]
        else:
            sx = am.statuses_aligned(rows_x, x[1][:64 * n], x[2], [None] * n, key)
            sy = am.statuses_aligned(rows_y, y[1][:64 * n], y[2], align_y, key)
        st_x[off[i]:off[i] + n], st_y[off[i]:off[i] + n] = sx, sy
        counts[0] += bytes(sx).count(0)
        counts[1] += bytes(sy).count(0)
        data, macs, align = bytearray(y[0][:n * rb]), bytearray(y[1][:64 * n]), bytearray(y[3][:64 * n])
        out_y[i] = (data, macs, align)
        if 0 not in sx and 0 not in sy:
            verdict[i] = CLEAN
            continue
        if 0 in sx:
            verdict[i] = X_DAMAGED
            counts[6] += 1
            continue
        chunks, bad = decode_x(rows_x, curve)
        steps = level_steps(write_step, n_total, i)
        cand_data = am.rows_bytes(y_half(chunks, steps, n_total, curve), "exact")
        cand_align = b"".join(pt_bytes(commit(r)) for r in align_scalars(chunks, steps, n_total, curve))
        differ = [j for j in range(n) if sy[j] == 1 and (bytes(data[j * rb:(j + 1) * rb]) != cand_data[j * rb:(j + 1) * rb] or
                                                          bytes(align[64 * j:64 * j + 64]) != cand_align[64 * j:64 * j + 64])]
        counts[7] += len(differ)
        if differ or bad:
            verdict[i] = INCONSISTENT
            counts[6] += 1
            continue
        verdict[i] = REPAIRED
        counts[5] += 1
        todo = [j for j in range(n) if sy[j] == 0]
        for j in todo:
            if bytes(data[j * rb:(j + 1) * rb]) != cand_data[j * rb:(j + 1) * rb]:
                data[j * rb:(j + 1) * rb] = cand_data[j * rb:(j + 1) * rb]
                action[off[i] + j] |= DATA
                counts[2] += 1
            if bytes(align[64 * j:64 * j + 64]) != cand_align[64 * j:64 * j + 64]:
                align[64 * j:64 * j + 64] = cand_align[64 * j:64 * j + 64]
                action[off[i] + j] |= ALIGN
                counts[3] += 1
        ints = am.rows_of(b"".join(bytes(data[j * rb:(j + 1) * rb]) for j in todo), n_cols, "exact")
        pts = [pt_tuple(align[64 * j:64 * j + 64]) for j in todo]
        prf = [y[2][j] for j in todo]
        want = mac_of(i, todo, ints, prf, pts) if mac_of else am.expected_macs_aligned(ints, prf, pts, key)
        for j, pt in zip(todo, want):
            mb = model.point_bytes(pt)
            if bytes(macs[64 * j:64 * j + 64]) != mb:
                macs[64 * j:64 * j + 64] = mb
                action[off[i] + j] |= MAC
                counts[4] += 1
    return {"status_x": bytes(st_x), "status_y": bytes(st_y), "action_y": bytes(action), "level": bytes(verdict), "counts": counts,
            "y": {i: tuple(bytes(b) for b in v) for i, v in out_y.items()}}

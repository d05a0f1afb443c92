"""MODEL (test infrastructure only) of the top-level repair (include/porla_gpu.h: porla_kzg_repair_top_batch_device /
porla_ipa_repair_top_batch_device) on top of tests/extract_xyt_model.py (the scale by wt^-1) and tests/retrieve_aligned_model.py (the
row check and the expected MACs).  A half is (rows bytes in the top form, MAC bytes, [PRF integers], alignment bytes or None).

  1. every row of both halves gets the aligned retrieval's status in the top form's symbol width
  2. row j of a half is repairable iff its own status is 0 and row j of the other half is OK; lost iff both are 0
  3. the candidate for an X row is wt^-1 Y_j, for a Y row wt X_j, canonical below LCM (exact) or below p_icc (residue32); wt = 1: the
     sibling row copied as it lies; DATA iff the stored bytes differed
  4. the MAC of a repairable row is E_j - alpha A_j over the row as repaired, the alignment as it lies; MAC iff the stored bytes differed
  5. lost rows: LOST on both sides, not one byte written
  6. OK rows, alignments and PRF values are never written
  7. counts = [X rows with status 0, Y rows with status 0, X data rewritten, X MACs rewritten, Y data, Y MACs, lost indices, 0]

A helper of tests/test_repair_top_*.py, not a test module."""
import icc_py
from tests import extract_xyt_model as tm
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model
from tests.update_model import pt_tuple

DATA, MAC, LOST = 1, 2, 4
P = icc_py.P_ICC
top_exponent = tm.top_exponent


def scale_symbol(v, e, n_total, curve, form):
    """wt v for a stored symbol v (any value of the symbol's width), canonical in the form's modulus: the p_icc plane by w^e mod p_icc,
    the q plane by the INTEGER (w^e mod p_icc) mod q, joined below LCM"""
    wt = pow(icc_py.root_w(n_total), e, P)
    rp = v % P * wt % P
    if form == "residue32":
        return rp
    q = icc_py.Q[curve]
    rq = v % q * (wt % q) % q
    return rp + P * ((rq - rp) * pow(P, -1, q) % q)


def candidate_row(sibling_row_b, to_y, e, n_total, curve, form):
    """the bytes a repairable row gets from its sibling's: wt X_j (to_y) or wt^-1 Y_j"""
    if e == 0:
        return sibling_row_b
    w = am.FORM_SYMBOL_BYTES[form]
    f = scale_symbol if to_y else tm.unscale_symbol
    return b"".join(f(int.from_bytes(sibling_row_b[i:i + w], "little"), e, n_total, curve, form).to_bytes(w, "little")
                    for i in range(0, len(sibling_row_b), w))


def actions_of(st_x, st_y):
    """rule 2 on two status vectors: per half, per row "repair", "lost" or None"""
    pick = lambda own, other: None if own else ("repair" if other == 1 else "lost")
    return [pick(x, y) for x, y in zip(st_x, st_y)], [pick(y, x) for x, y in zip(st_x, st_y)]


def align_points(align_b, n):
    return [pt_tuple(align_b[64 * j:64 * j + 64]) if align_b else None for j in range(n)]


def half_statuses(half, n_cols, form, key):
    rows_b, macs, prf, align_b = half
    n = len(prf)
    return am.statuses_aligned(am.rows_of(rows_b, n_cols, form), macs, prf, align_points(align_b, n), key)


def repair_top(x, y, n_total, n_cols, curve, form, top_step, key=None, status_x=None, status_y=None, mac_of=None):
    """one file.  x, y: the halves as they lie.  The statuses are computed with `key`, or given.  mac_of(half index, row indices, rows of
    integers, prf, alignment points) -> the expected MAC points of those rows; by default the aligned retrieval model's with `key`.
    Returns {"rows_x", "macs_x", "rows_y", "macs_y", "status_x", "status_y", "action_x", "action_y", "counts"}"""
    w = am.FORM_SYMBOL_BYTES[form]
    rb = n_cols * w
    halves = [x, y]
    st = [bytes(status_x) if status_x is not None else half_statuses(x, n_cols, form, key),
          bytes(status_y) if status_y is not None else half_statuses(y, n_cols, form, key)]
    assert len(st[0]) == len(st[1]) == n_total
    if mac_of is None:
        mac_of = lambda h, js, rows, prf, align: am.expected_macs_aligned(rows, prf, align, key)
    what = actions_of(st[0], st[1])
    e = top_exponent(n_total, top_step)
    rows = [bytearray(x[0]), bytearray(y[0])]
    macs = [bytearray(x[1]), bytearray(y[1])]
    action = [bytearray(n_total), bytearray(n_total)]
    counts = [st[0].count(0), st[1].count(0), 0, 0, 0, 0, 0, 0]
    for h in (0, 1):
        sib = halves[h ^ 1][0]
        todo = [j for j in range(n_total) if what[h][j] == "repair"]
        for j in range(n_total):
            if what[h][j] == "lost":
                action[h][j] = LOST
                counts[6] += 1 if h == 0 else 0
        for j in todo:
            cand = candidate_row(sib[j * rb:(j + 1) * rb], h == 1, e, n_total, curve, form)
            if bytes(rows[h][j * rb:(j + 1) * rb]) != cand:
                rows[h][j * rb:(j + 1) * rb] = cand
                action[h][j] |= DATA
                counts[2 + 2 * h] += 1
        if todo:
            prf, align_b = halves[h][2], halves[h][3]
            ints = am.rows_of(b"".join(bytes(rows[h][j * rb:(j + 1) * rb]) for j in todo), n_cols, form)
            align = align_points(align_b, n_total)
            want = mac_of(h, todo, ints, [prf[j] for j in todo], [align[j] for j in todo])
            for j, pt in zip(todo, want):
                mb = model.point_bytes(pt)
                if bytes(macs[h][64 * j:64 * j + 64]) != mb:
                    macs[h][64 * j:64 * j + 64] = mb
                    action[h][j] |= MAC
                    counts[3 + 2 * h] += 1
    return {"rows_x": bytes(rows[0]), "macs_x": bytes(macs[0]), "rows_y": bytes(rows[1]), "macs_y": bytes(macs[1]),
            "status_x": st[0], "status_y": st[1], "action_x": bytes(action[0]), "action_y": bytes(action[1]), "counts": counts}

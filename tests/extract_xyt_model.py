"""MODEL (test infrastructure only) of the file extraction with the top level's Y half (include/porla_gpu.h:
porla_kzg_extract_xyt_batch_device / porla_ipa_extract_xyt_batch_device) on top of tests/extract_xy_model.py: the same File and lower-level
Y halves, beside them the top level's resident Y half as the store holds it and the write step of the rebuild that wrote it.

  1t. every top-level Y row gets the aligned retrieval's status in the top form's symbol width; untried: NOT_TRIED
  2t. the source of a top-level row: X if its X status is OK, else Y if its Y status is OK, else none; the top level is failed iff some
      row has no source
  3t. the patched half: row j is X row j as it lies, or wt^-1 Y_j -- canonical below LCM (exact) or below p_icc (residue32), the p_icc
      plane by w^(N - e), the q plane by the inverse of (w^e mod p_icc) mod q, e = reverse_bits(top_step % N); wt = 1: the Y row copied;
      a row without a source keeps its X row
  4t. the top level's one decode reads the patched half
  5t. a slot the top level wins: FOUND, RESIDUE iff the top form is residue32, FROM_Y iff some row came from the Y half
  6t. counts = extract_xy's six (counts[0]: the X and top X rows with status 0), then [tried top Y rows with status 0, rows from Y]

A helper of tests/test_extract_xyt_*.py, not a test module."""
import icc_py
from tests import extract_model as em
from tests import extract_xy_model as xm
from tests import retrieve_aligned_model as am
from tests.update_model import pt_tuple

FOUND, UNSURE, RESIDUE, FROM_Y, NOT_TRIED = xm.FOUND, xm.UNSURE, xm.RESIDUE, xm.FROM_Y, xm.NOT_TRIED
P = icc_py.P_ICC


def top_exponent(n_total, top_step):
    return icc_py.reverse_bits(top_step % n_total, icc_py.height_of(n_total) - 1)


def unscale_symbol(v, e, n_total, curve, form):
    """wt^-1 v for a stored symbol v (any value of the symbol's width), canonical in the form's modulus"""
    w = icc_py.root_w(n_total)
    rp = v % P * pow(w, (n_total - e) % n_total, P) % P
    if form == "residue32":
        return rp
    q = icc_py.Q[curve]
    rq = v % q * pow(pow(w, e, P) % q, -1, q) % q
    return rp + P * ((rq - rp) * pow(P, -1, q) % q)


def statuses_top_y(f, top_y, key):
    """d_row_status_top_y by the aligned retrieval's relation; top_y: (rows bytes in the top form, MAC bytes, [PRF integers], alignment
    bytes or None)"""
    rows_b, macs, prf, align_b = top_y
    align = [pt_tuple(align_b[64 * j:64 * j + 64]) if align_b else None for j in range(f.n_total)]
    return am.statuses_aligned(am.rows_of(rows_b, f.n_cols, f.top_form), macs, prf, align, key)


def row_sources(st_top_x, st_top_y):
    """per top-level row "x", "y" or None"""
    return ["x" if x else ("y" if y == 1 else None) for x, y in zip(st_top_x, st_top_y)]


def patch(x_rows_b, y_rows_b, sources, n_total, n_cols, curve, form, top_step):
    """the bytes of d_top_patch"""
    w = am.FORM_SYMBOL_BYTES[form]
    e = top_exponent(n_total, top_step)
    out = b""
    for j, src in enumerate(sources):
        lo, hi = j * n_cols * w, (j + 1) * n_cols * w
        if src != "y":
            out += x_rows_b[lo:hi]
        elif e == 0:
            out += y_rows_b[lo:hi]
        else:
            out += b"".join(unscale_symbol(int.from_bytes(y_rows_b[i:i + w], "little"), e, n_total, curve, form).to_bytes(w, "little")
                            for i in range(lo, hi, w))
    return out


def extract_xyt(f, y, y_levels, top_y, top_step, tried, key=None, statuses=None, status_y=None, status_top_y=None):
    """xm.extract_xy's dictionary with eight counts, "row_status_top_y" and "top_patch" (None when the top Y half is not tried).
    tried: the request's top_y (0 or 1); it counts only with a top level"""
    n, nc = f.n_total, f.n_cols
    st = statuses if statuses is not None else em.row_statuses(f, key)
    if not (tried and f.top):
        got = xm.extract_xy(f, y, y_levels, key=key, statuses=st, status_y=status_y)
        return dict(got, counts=got["counts"] + [0, 0], row_status_top_y=bytes([NOT_TRIED] * n), top_patch=None)
    sty = bytes(status_top_y) if status_top_y is not None else statuses_top_y(f, top_y, key)
    assert len(sty) == n
    sources = row_sources(st[f.t:f.t + n], sty)
    from_y = sources.count("y")
    patched = patch(f.top[0], top_y[0], sources, n, nc, f.curve, f.top_form, top_step)
    g = em.File(n, nc, f.curve, f.write_step, f.lower, (patched,) + tuple(f.top[1:]), f.top_form)
    st_merge = bytes(st[:f.t]) + bytes(1 if s else 0 for s in sources)
    got = xm.extract_xy(g, y, y_levels, key=key, statuses=st_merge, status_y=status_y)
    flags = bytes(x | (FROM_Y if from_y and x & FOUND and got["steps"][s] == 0 else 0) for s, x in enumerate(got["flags"]))
    counts = [bytes(st).count(0)] + got["counts"][1:] + [sty.count(0), from_y]
    return dict(got, flags=flags, counts=counts, row_status=bytes(st), row_status_top_y=sty, top_patch=patched)

"""MODEL (test infrastructure only) of the aligned verified retrieval (include/porla_gpu.h: porla_kzg_retrieve_aligned_batch_device /
porla_ipa_retrieve_aligned_batch_device) on top of tests/retrieve_model.py.

The relation.  Every row of every non-empty level, X and Y, keeps MAC[j] + alpha align[j] == alpha Commit(row[j] mod q) (+ s_j h with
the complements), row[j] being the STORED symbol reduced mod q (tests/test_update_batch_cpu.py: check_identity), and so does the
aligned top level (tests/test_server_rebuild_aligned_batch_cpu.py).  The call therefore accepts row j iff its stored MAC bytes are
the canonical bytes of
    E_j - alpha A_j,      E_j = retrieve_model.expected_macs' point, A_j = the half's alignment row.

A key is retrieve_model's with "alpha" in both builds (IPA: the scalar with alpha_generators[c] = alpha generators[c]).  With known
logarithms everywhere -- the commitment base point c is g_c G, h = eta G -- a stored half costs one multiplication per row.
A helper of tests/test_retrieve_aligned_*.py, not a test module."""
import icc_py
from tests import mac_decode_model as mdm
from tests import retrieve_model as model
from tests.update_model import pt_bytes, pt_tuple

ROW_OK = model.ROW_OK
FORM_SYMBOL_BYTES = {"exact": 64, "residue64": 64, "residue32": 32}


def sub_alpha_align(curve, expected, align_points, alpha):
    """E_j - alpha A_j for every row"""
    q = icc_py.Q[curve]
    return [icc_py.ec_add(curve, e, icc_py.ec_neg(curve, icc_py.ec_mul(curve, a, alpha % q))) if a is not None else e
            for e, a in zip(expected, align_points)]


def expected_macs_aligned(rows, prf, align_points, key):
    """the affine points the aligned call compares d_macs with; align_points: affine tuples, None = infinity"""
    return sub_alpha_align(key["curve"], model.expected_macs(rows, prf, key), align_points, key["alpha"])


def statuses_of(want_points, macs_bytes):
    return bytes(ROW_OK if macs_bytes[64 * j:64 * j + 64] == model.point_bytes(w) else 0 for j, w in enumerate(want_points))


def statuses_aligned(rows, macs_bytes, prf, align_points, key):
    return statuses_of(expected_macs_aligned(rows, prf, align_points, key), macs_bytes)


def rows_bytes(rows, form):
    w = FORM_SYMBOL_BYTES[form]
    return b"".join(v.to_bytes(w, "little") for row in rows for v in row)


def rows_of(b, n_cols, form):
    w = FORM_SYMBOL_BYTES[form]
    vals = [int.from_bytes(b[i:i + w], "little") for i in range(0, len(b), w)]
    return [vals[i:i + n_cols] for i in range(0, len(vals), n_cols)]


# ---- a build with known logarithms: base point c = g_c G, h = eta G
def known_key(curve, n_cols, rng):
    """(key, base bytes for FileModel, alpha): KZG g_c = tau^c (G1[0] = G), IPA g_c random with alpha generators alpha g_c G"""
    q, G = icc_py.Q[curve], mdm.GEN[curve]
    alpha, eta = rng.randrange(1, q), rng.randrange(1, q)
    if curve == "bn254":
        tau = rng.randrange(1, q)
        g = [pow(tau, c, q) for c in range(n_cols)]
        key = {"curve": curve, "alpha": alpha, "tau": tau, "h": icc_py.ec_mul(curve, G, eta), "h_dlog": eta}
    else:
        g = [rng.randrange(1, q) for _ in range(n_cols)]
        dl = [alpha * x % q for x in g]
        key = {"curve": curve, "alpha": alpha, "alpha_generators": [icc_py.ec_mul(curve, G, d) for d in dl], "dlogs": dl,
               "h": icc_py.ec_mul(curve, G, eta), "h_dlog": eta}
    base = b"".join(pt_bytes(icc_py.ec_mul(curve, G, x)) for x in g)
    return key, base, g


def block_mac_known(chunks, key, g):
    """alpha Commit(chunks) of a written block: the MAC the client sends, without complement"""
    curve = key["curve"]
    q = icc_py.Q[curve]
    return icc_py.ec_mul(curve, mdm.GEN[curve], key["alpha"] * sum(c % q * x for c, x in zip(chunks, g)) % q)


def half_of(m, level, part, form="residue64"):
    """the resident half `part` ("x" / "y") of level `level` of a FileModel (or the aligned rebuild model's top level, form "residue32"):
    (rows as integers, MAC bytes, alignment points)"""
    n, w = 1 << level, FORM_SYMBOL_BYTES[form]
    rows = rows_of(bytes(m.fam["data_" + part][level][:n * m.n_cols * w]), m.n_cols, form)
    macs = bytes(m.fam["mac_" + part][level][:64 * n])
    align = [pt_tuple(m.fam["align_" + part][level][64 * j:64 * j + 64]) for j in range(n)]
    return rows, macs, align


def add_complements(macs_bytes, s, key):
    """mac_row_j += s_j h"""
    curve = key["curve"]
    return b"".join(pt_bytes(icc_py.ec_add(curve, pt_tuple(macs_bytes[64 * j:64 * j + 64]), model.hiding(sj, key))) for j, sj in enumerate(s))

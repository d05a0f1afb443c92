"""MODEL (test infrastructure only) of the verified retrieval (include/porla_gpu.h: porla_kzg_retrieve_batch_device /
porla_ipa_retrieve_batch_device) on Python integers and affine points, on top of oracle/icc_py.py and tests/mac_decode_model.py.

The relation.  The data network works mod LCM = p_icc q with integer multipliers vi < p_icc, the MAC network multiplies by the same vi
reduced mod q.  So coded row j of an exact half, reduced mod q, is the Z_q network of the chunks, and with per-block MACs
alpha Commit(block_i) + u_i h the half's MAC row j is alpha Commit(row_j mod q) + s_j h, s = the Z_q network of the u_i (of wt u_i for
the Y half).  The call checks every row against exactly that, s_j being the 128-bit PRF value the client holds for the row.

A key says what Commit, alpha and h are:
  KZG  {"curve": "bn254", "alpha": int, "tau": int, "h": point}: alpha Commit(c) = (alpha f_c(tau)) G1[0], G1[0] = (1, 2)
  IPA  {"curve": "secp256k1", "alpha_generators": [points], "h": point}: alpha Commit(c) = sum c_i alpha_generators[i]; with
       "dlogs" (alpha_generators[i] = dlogs[i] G) and "h_dlog" (h = h_dlog G) a row costs one scalar multiplication instead of 129
A helper of tests/test_retrieve_*.py, not a test module."""
import icc_py
from tests import mac_decode_model as mdm

P = icc_py.P_ICC
ROW_OK = 1
point_bytes, points_to_bytes = mdm.point_bytes, mdm.points_to_bytes


def prf_scalar(curve, raw16):
    """16 raw bytes as the reference reads them: KZG a big-endian integer, IPA r.d[0], r.d[1] as little-endian 64-bit words"""
    assert len(raw16) == 16
    return int.from_bytes(raw16, "big" if curve == "bn254" else "little")


def prf_raw(curve, value):
    return value.to_bytes(16, "big" if curve == "bn254" else "little")


def alpha_commit(coeffs, key):
    """alpha * Commit(coeffs) as an affine point; the coefficients are reduced mod the group order"""
    curve = key["curve"]
    q = icc_py.Q[curve]
    if curve == "bn254":
        e = 0
        for c in reversed(coeffs):
            e = (e * key["tau"] + c) % q
        return icc_py.ec_mul(curve, mdm.GEN[curve], e * key["alpha"] % q)
    if "dlogs" in key:
        return icc_py.ec_mul(curve, mdm.GEN[curve], sum(c * d for c, d in zip(coeffs, key["dlogs"])) % q)
    acc = None
    for c, g in zip(coeffs, key["alpha_generators"]):
        acc = icc_py.ec_add(curve, acc, icc_py.ec_mul(curve, g, c % q))
    return acc


def hiding(scalar, key):
    curve = key["curve"]
    if "h_dlog" in key:
        return icc_py.ec_mul(curve, mdm.GEN[curve], scalar * key["h_dlog"] % icc_py.Q[curve])
    return icc_py.ec_mul(curve, key["h"], scalar)


def block_mac(coeffs, hide, key):
    """alpha Commit(coeffs) + hide h: a block's MAC with the hiding scalar `hide`, and equally the expected MAC of a coded row"""
    return icc_py.ec_add(key["curve"], alpha_commit(coeffs, key), hiding(hide, key))


def expected_macs(rows, prf, key):
    """rows: lists of symbols (integers < LCM); prf: one integer per row.  The affine points the call compares d_macs with."""
    return [block_mac(row, s, key) for row, s in zip(rows, prf)]


def statuses(rows, macs_bytes, prf, key):
    """the status bytes: 1 iff the 64 stored bytes equal the canonical bytes of the expected MAC"""
    want = expected_macs(rows, prf, key)
    return bytes(ROW_OK if macs_bytes[64 * j:64 * j + 64] == point_bytes(w) else 0 for j, w in enumerate(want))


# ---- the MAC network on the hiding scalars, in Z_q
def zq_network(vals, curve, inverse=False):
    """the stages of icc_py.mac_crebuild on scalars mod q (multipliers (v^j mod p_icc) mod q); inverse: its inverse"""
    n, q = len(vals), icc_py.Q[curve]
    w = icc_py.root_w(n)
    x = [v % q for v in vals]
    stages = range(1, icc_py.height_of(n))
    for s in (reversed(stages) if inverse else stages):
        m, m2 = 1 << s, 1 << (s - 1)
        v = pow(w, n // m2, P)
        for j in range(m2):
            vi = pow(v, j, P) % q
            for k in range(j, n, m):
                a, b = x[k], x[k + m2]
                if inverse:
                    half = pow(2, -1, q)
                    x[k], x[k + m2] = (a + b) * half % q, (a - b) * half * pow(vi, -1, q) % q
                else:
                    t = vi * b % q
                    x[k], x[k + m2] = (a + t) % q, (a - t) % q
    return x


def wt_of(n, write_step):
    return pow(icc_py.root_w(n), icc_py.reverse_bits(write_step % n, icc_py.height_of(n) - 1), P)


def hiding_scalars_for(s, curve, part=0, write_step=0):
    """the per-block hiding scalars u_i with which half `part` (0 = X, 1 = Y) of the level's MAC rows hides exactly s_j in row j"""
    u = zq_network(s, curve, inverse=True)
    if part:
        q = icc_py.Q[curve]
        wt_inv = pow(wt_of(len(s), write_step) % q, -1, q)
        u = [x * wt_inv % q for x in u]
    return u


def build_half(blocks, s, key, part=0, write_step=0):
    """A half as the encodes leave it, whose MAC rows hide exactly s_j: (coded rows, MAC rows as points, hiding scalars u_i) from
    icc_py.crebuild on the blocks and icc_py.mac_crebuild on the per-block MACs alpha Commit(block_i) + u_i h"""
    curve = key["curve"]
    u = hiding_scalars_for(s, curve, part, write_step)
    macs = [block_mac(b, ui, key) for b, ui in zip(blocks, u)]
    rows = icc_py.crebuild(blocks, curve, write_step)[part]
    mac_rows = icc_py.mac_crebuild(macs, curve, write_step)[part]
    return rows, mac_rows, u


# ---- byte forms
def rows_bytes(rows):
    return b"".join(v.to_bytes(64, "little") for row in rows for v in row)


def prf_bytes(curve, values):
    return b"".join(prf_raw(curve, v) for v in values)

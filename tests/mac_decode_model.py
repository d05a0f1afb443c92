"""MODEL (test infrastructure only) of the ICC MAC decode (include/porla_gpu.h: porla_icc_mac_decode_batch_device) on Python integers
and affine points, on top of oracle/icc_py.py: the stages of icc_py.mac_crebuild run backwards, (A, B) <- (A + B, vi^-1 (A - B)) with
vi^-1 the inverse mod the group order q of the INTEGER (w^e mod p_icc) mod q the encode multiplies by, the subtraction of d_sub before
the network, one final factor n^-1 wt_i^-1 mod q per row, and the 64-byte big-endian affine byte form (64 zero bytes = infinity).  The
CPU tests check the model against the oracle's encode and mixes, the GPU tests check the device against the model."""
import icc_py

P = icc_py.P_ICC


def twiddle(e, n_total):
    """the scalar the encode multiplies by at exponent e of the table of n_total: (w^e mod p_icc) mod q is taken by the group"""
    return pow(icc_py.root_w(n_total), e, P)


def inverse_twiddle(e, n_total, curve):
    q = icc_py.Q[curve]
    return pow(twiddle(e, n_total) % q, -1, q)


def wt_of(step, n_total):
    """wt of a write step: w^reverse_bits(step % N, log2 N) mod p_icc (icc_py.hadd)"""
    return pow(icc_py.root_w(n_total), icc_py.reverse_bits(step % n_total, n_total.bit_length() - 1), P)


def row_scalar(n_rows, curve, step=None, n_total=None):
    """what the close multiplies row i by: n_rows^-1, times wt_i^-1 with a write step, mod q"""
    q = icc_py.Q[curve]
    s = pow(n_rows, -1, q)
    if step is not None:
        s = s * pow(wt_of(step, n_total) % q, -1, q) % q
    return s


def inverse_stage(X, s, curve, scalar_of):
    """one stage backwards, in place: (A, B) <- (A + B, scalar_of(j) (A - B)) on the rows k, k + 2^(s-1), j = k mod 2^(s-1)"""
    n = len(X)
    m, m2 = 1 << s, 1 << (s - 1)
    for j in range(m2):
        sc = scalar_of(j)
        for k in range(j, n, m):
            a, b = X[k], X[k + m2]
            X[k] = icc_py.ec_add(curve, a, b)
            X[k + m2] = icc_py.ec_mul(curve, icc_py.ec_add(curve, a, icc_py.ec_neg(curve, b)), sc)
    return X


def decode(macs, curve, n_total=None, write_steps=None, sub=None):
    """macs: n affine points (x, y) or None, the outputs of the network (plus sub).  Returns its inputs; with write steps position i
    is also multiplied by wt_i^-1 mod q"""
    n = len(macs)
    n_total = n_total or n
    assert n >= 2 and n & (n - 1) == 0 and n_total >= n and n_total & (n_total - 1) == 0
    X = list(macs)
    if sub is not None:
        X = [icc_py.ec_add(curve, a, icc_py.ec_neg(curve, b)) for a, b in zip(X, sub)]
    for s in range(n.bit_length() - 1, 0, -1):
        inverse_stage(X, s, curve, lambda j: inverse_twiddle(j * (n_total >> (s - 1)), n_total, curve))
    return [icc_py.ec_mul(curve, x, row_scalar(n, curve, None if write_steps is None else write_steps[i], n_total))
            for i, x in enumerate(X)]


# ---- the byte forms of the C ABI
def point_bytes(pt):
    return bytes(64) if pt is None else pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def points_to_bytes(pts):
    return b"".join(point_bytes(p) for p in pts)


def bytes_to_points(data, curve):
    """64-byte big-endian affine points, each coordinate reduced mod the base field as SetBytes does; 64 zero bytes (after the
    reduction: x = y = 0) = infinity"""
    p = icc_py.CURVE_P[curve]
    assert len(data) % 64 == 0
    out = []
    for i in range(0, len(data), 64):
        x, y = int.from_bytes(data[i:i + 32], "big") % p, int.from_bytes(data[i + 32:i + 64], "big") % p
        out.append(None if x == 0 and y == 0 else (x, y))
    return out


def decode_bytes(data, n_rows, n_total, curve, write_steps=None, sub=None):
    """what porla_icc_mac_decode_batch_device writes for one request: n_rows * 64 bytes"""
    assert len(data) == 64 * n_rows
    return points_to_bytes(decode(bytes_to_points(data, curve), curve, n_total, write_steps,
                                  None if sub is None else bytes_to_points(sub, curve)))


# ---- levels as the update path builds them
GEN = {"bn254": (1, 2),
       "secp256k1": (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
                     0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)}


def level_x(macs, n_total, curve):
    """the X half of a level's MACs as Server::mix builds it from the per-block MACs in write order (icc_py.mac_mix, recursively)"""
    if len(macs) == 1:
        return [macs[0]]
    half = len(macs) // 2
    return icc_py.mac_mix(level_x(macs[:half], n_total, curve), level_x(macs[half:], n_total, curve), n_total, curve)


def level_y(macs, steps, n_total, curve):
    """the Y half: level 0 holds wt * MAC (icc_py.hadd), the mixes are the X half's"""
    if len(macs) == 1:
        return [icc_py.hadd([], macs[0], n_total, steps[0], curve)[2]]
    half = len(macs) // 2
    return icc_py.mac_mix(level_y(macs[:half], steps[:half], n_total, curve), level_y(macs[half:], steps[half:], n_total, curve),
                          n_total, curve)

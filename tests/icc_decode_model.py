"""MODEL (test infrastructure only) of the ICC decode (include/porla_gpu.h: porla_icc_decode_batch_device) on Python integers, on top of
oracle/icc_py.py: the stages of icc_py.crebuild run backwards, (a, b) <- (a + b, (a - b) vi^-1) with one final factor n^-1, one residue
plane at a time, and the join of the two residues.  The three forms, the unscale by wt_i^-1, the output bytes of a symbol that cannot
be a chunk and the count of such symbols are stated here once; the CPU tests check the model against the encode, the GPU tests check
the device against the model."""
import icc_py

P = icc_py.P_ICC
EXACT, RESIDUE64, RESIDUE32 = 0, 1, 2
FORMS = {"exact": EXACT, "residue64": RESIDUE64, "residue32": RESIDUE32}
WIDTH = {EXACT: 64, RESIDUE64: 64, RESIDUE32: 32}


def edge_chunks(curve):
    """the chunks the issue names: around p_icc, the group order, and the ends of the 256-bit range"""
    return [0, 1, P - 1, P, P + 1, icc_py.Q[curve], 2**256 - 1]


def inverse_plane(rows, mod):
    """the network backwards modulo `mod` (p_icc, q or LCM): rows = its outputs, returns its inputs.  The twiddle of stage s, row j is
    the INTEGER vi = w^(j n / 2^(s-1)) mod p_icc, as the encode multiplies by it; its inverse is taken modulo `mod`."""
    n = len(rows)
    h = icc_py.height_of(n)
    w = icc_py.root_w(n)
    X = [[v % mod for v in r] for r in rows]
    for s in range(h - 1, 0, -1):
        m, m2 = 1 << s, 1 << (s - 1)
        v = pow(w, n // m2, P)
        vi = 1
        for j in range(m2):
            inv = pow(vi % mod, -1, mod)
            for k in range(j, n, m):
                a, b = X[k], X[k + m2]
                for c in range(len(a)):
                    a[c], b[c] = (a[c] + b[c]) % mod, (a[c] - b[c]) * inv % mod
            vi = vi * v % P
    ninv = pow(n, -1, mod)
    return [[v * ninv % mod for v in r] for r in X]


def join(r_p, r_q, curve):
    """(value, ok): the value below LCM with the two residues -- r_p + p_icc t, t = (r_q - r_p) p_icc^-1 mod q, no 512-bit product --
    and whether it is a 256-bit chunk: t = 0, or t = 1 with r_p + p_icc < 2^256"""
    q = icc_py.Q[curve]
    t = (r_q - r_p) * pow(P, -1, q) % q
    value = r_p + P * t
    ok = t == 0 or (t == 1 and r_p + P < 2**256)
    assert ok == (value < 2**256)
    return value, ok


def decode_exact(rows, curve):
    """rows: n lists of values below LCM.  Returns (out, bad): the chunks, a symbol whose joined value is >= 2^256 written as its residue
    mod p_icc, and the number of such symbols"""
    rp = inverse_plane(rows, P)
    rq = inverse_plane(rows, icc_py.Q[curve])
    out, bad = [], 0
    for a, b in zip(rp, rq):
        row = []
        for x, y in zip(a, b):
            value, ok = join(x, y, curve)
            row.append(value if ok else x)
            bad += 0 if ok else 1
        out.append(row)
    return out, bad


def unscale_factor(step, n_total):
    """wt^-1 of a write step: w^(N - reverse_bits(step % N, log2 N)) mod p_icc"""
    logn = n_total.bit_length() - 1
    e = icc_py.reverse_bits(step % n_total, logn)
    return pow(icc_py.root_w(n_total), (n_total - e) % n_total, P)


def decode_residue(rows, n_total, write_steps=None):
    """rows: n lists of values (below LCM, or the 32-byte rows below p_icc).  Returns chunk mod p_icc, canonical; with write steps
    position i is multiplied by wt_i^-1"""
    out = inverse_plane(rows, P)
    if write_steps is not None:
        out = [[v * unscale_factor(write_steps[i], n_total) % P for v in r] for i, r in enumerate(out)]
    return out


# ---- the byte forms of the C ABI
def rows_to_bytes(rows, width):
    return b"".join(v.to_bytes(width, "little") for r in rows for v in r)


def bytes_to_rows(data, n_rows, n_cols, width):
    assert len(data) == n_rows * n_cols * width
    return [[int.from_bytes(data[(i * n_cols + c) * width:(i * n_cols + c + 1) * width], "little") for c in range(n_cols)]
            for i in range(n_rows)]


def decode_bytes(form, data, n_rows, n_cols, n_total, curve, write_steps=None):
    """what porla_icc_decode_batch_device writes for one request: (n_rows * n_cols * 32 bytes, bad count or None)"""
    form = FORMS.get(form, form)
    rows = bytes_to_rows(data, n_rows, n_cols, WIDTH[form])
    if form == EXACT:
        assert write_steps is None
        out, bad = decode_exact(rows, curve)
        return rows_to_bytes(out, 32), bad
    return rows_to_bytes(decode_residue(rows, n_total, write_steps), 32), None


def level_x(blocks, n_total, curve):
    """the X half of a level as Server::mix builds it from its blocks in write order, oldest first (icc_py.mix, recursively)"""
    if len(blocks) == 1:
        return [list(blocks[0])]
    half = len(blocks) // 2
    return icc_py.mix(level_x(blocks[:half], n_total, curve), level_x(blocks[half:], n_total, curve), n_total, curve)


def level_y(blocks, steps, n_total, curve):
    """the Y half: level 0 holds (chunk * wt) mod p_icc (icc_py.hadd), the mixes are the X half's"""
    if len(blocks) == 1:
        return [icc_py.hadd(blocks[0], None, n_total, steps[0], curve)[0]]
    half = len(blocks) // 2
    return icc_py.mix(level_y(blocks[:half], steps[:half], n_total, curve), level_y(blocks[half:], steps[half:], n_total, curve),
                      n_total, curve)

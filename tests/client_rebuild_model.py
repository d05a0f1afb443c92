"""Two Python restatements of the client's side of ONE rebuild write -- the write on which the reference calls Client::CRebuild
(porla/Client/Client.hpp:483-502, :1040-1453, the wire loop :584-614) -- for tests/test_client_rebuild_batch_*.py; not a test module.

The PRF values come in the order of porla_client_rebuild_req.d_prf (include/porla_gpu.h): [0] the block's own complement, then
complements_U[0 .. n_total-1], then the 2 * n_total new ones, X then Y.

  rebuild_points    the point domain, the reference loop for loop: oracle/icc_py.py mac_crebuild on the complements s_i * h, then
                    new - rebuilt with ec_mul / ec_add / ec_neg.
  rebuild_scalars   the scalar domain the library computes in: every point is a known scalar times h and the network is linear over
                    Z_q, so out_j = (s'_j - T_j) * h with T the same butterflies on plain integers mod q; scalar_points then spends
                    one ec_mul per REQUESTED output index, which is what makes sizes past a few hundred affordable."""
import icc_py


def n_prf(n_total):
    return 3 * n_total + 1


def split_prf(n_total, values):
    """(own, complements_U's values, new X values, new Y values)"""
    assert len(values) == n_prf(n_total)
    n = n_total
    return values[0], values[1:1 + n], values[1 + n:1 + 2 * n], values[1 + 2 * n:]


def wt_of(n_total, write_step):
    return pow(icc_py.root_w(n_total), icc_py.reverse_bits(write_step % n_total, icc_py.height_of(n_total) - 1), icc_py.P_ICC)


def rebuild_points(curve, n_total, write_step, prf, h, block_commit):
    """prf: the 3 * n_total + 1 PRF values as integers; h: the hiding point; block_commit: Commit_alpha(block) as an affine tuple or
    None.  Returns (mac, out): the MAC and the 2 * n_total points sent beside it (X part, then Y part)."""
    assert n_total >= 2 and n_total & (n_total - 1) == 0
    own, old, new_x, new_y = split_prf(n_total, prf)
    mac = icc_py.ec_add(curve, block_commit, icc_py.ec_mul(curve, h, own))
    x, y = icc_py.mac_crebuild([icc_py.ec_mul(curve, h, s) for s in old], curve, write_step)
    out = []
    for new, t in ((new_x, x), (new_y, y)):
        for j in range(n_total):
            out.append(icc_py.ec_add(curve, icc_py.ec_mul(curve, h, new[j]), icc_py.ec_neg(curve, t[j])))
    return mac, out


def network_scalars(curve, n_total, values):
    """mac_crebuild's X-part network on plain integers mod q: the multipliers are the integers v^j mod p_icc, reduced mod q by the
    group itself"""
    q = icc_py.Q[curve]
    w = icc_py.root_w(n_total)
    x = [v % q for v in values]
    for s in range(1, icc_py.height_of(n_total)):
        m, m2 = 1 << s, 1 << (s - 1)
        v = pow(w, n_total // m2, icc_py.P_ICC)
        vi = 1
        for j in range(m2):
            for k in range(j, n_total, m):
                t = vi * x[k + m2] % q
                u = x[k]
                x[k], x[k + m2] = (u + t) % q, (u - t) % q
            vi = vi * v % icc_py.P_ICC
    return x


def rebuild_scalars(curve, n_total, write_step, prf):
    """the 2 * n_total scalars e with out[g] = e[g] * h"""
    q = icc_py.Q[curve]
    _, old, new_x, new_y = split_prf(n_total, prf)
    t = network_scalars(curve, n_total, old)
    wt = wt_of(n_total, write_step)
    return [(new_x[j] - t[j]) % q for j in range(n_total)] + [(new_y[j] - wt * t[j]) % q for j in range(n_total)]


def scalar_points(curve, n_total, write_step, prf, h, block_commit, indices=None):
    """(mac, {g: out[g]}) for the output indices asked for (all of them by default), through the scalar domain"""
    e = rebuild_scalars(curve, n_total, write_step, prf)
    mac = icc_py.ec_add(curve, block_commit, icc_py.ec_mul(curve, h, prf[0]))
    return mac, {g: icc_py.ec_mul(curve, h, e[g]) for g in (range(2 * n_total) if indices is None else indices)}

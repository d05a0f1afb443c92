"""A Python restatement of Client::update's preprocessing for ONE write (porla/Client/Client.hpp:457-614): the block's MAC, the
complements of every slot below the level the write lands on (compute_MAC_complement, :423-455), Client::HAdd -> HRebuildX / HRebuildY
on them (:978-1038, mix :921-976) and the differences "new complement - mixed complement" that go on the wire (:584-614), built from
oracle/icc_py.py (hrebuild(..., mac=True), ec_add, ec_neg, ec_mul).  The PRF values come in the order of porla_client_update_req.d_prf
(include/porla_gpu.h): [0] the block's own, then level i's resident ones (X part, then Y part) for i = 0 .. level - 1, then the
2 * 2^level new ones.  A helper of tests/test_client_update_batch_*.py, not a test module."""
import icc_py


def n_prf(level):
    return (4 << level) - 1


def prf_scalar(curve, raw16):
    """a 16-byte AES output as the reference reads it: KZG a big-endian integer (compute_digest_complement), IPA r.d[0], r.d[1] as
    little-endian 64-bit words (Client.hpp:435-436)"""
    assert len(raw16) == 16
    return int.from_bytes(raw16, "big" if curve == "bn254" else "little")


def split_prf(level, values):
    """(own, [(X values, Y values) of level i for i < level], new X values, new Y values)"""
    assert len(values) == n_prf(level)
    own, pos, resident = values[0], 1, []
    for i in range(level):
        ln = 1 << i
        resident.append((values[pos:pos + ln], values[pos + ln:pos + 2 * ln]))
        pos += 2 * ln
    top = 1 << level
    return own, resident, values[pos:pos + top], values[pos + top:pos + 2 * top]


def client_update(curve, n_total, write_step, level, prf, h, block_commit):
    """prf: the 2^(level+2) - 1 PRF values as integers; h: the hiding point; block_commit: Commit_alpha(block) as an affine tuple or
    None.  Returns (mac, out): the MAC sent to the server and the 2 * 2^level points sent beside it (X part, then Y part)."""
    assert write_step % n_total != 0 and 0 <= level and (1 << level) <= n_total // 2
    own, resident, new_x, new_y = split_prf(level, prf)
    comp0 = icc_py.ec_mul(curve, h, own)
    mac = icc_py.ec_add(curve, block_commit, comp0)
    wt = pow(icc_py.root_w(n_total), icc_py.reverse_bits(write_step % n_total, icc_py.height_of(n_total) - 1), icc_py.P_ICC)
    b2 = icc_py.ec_mul(curve, comp0, wt)
    t = []
    for part, b in ((0, comp0), (1, b2)):
        levels = [[None] * (2 << i) for i in range(level + 1)]
        for i in range(level):
            levels[i][:1 << i] = [icc_py.ec_mul(curve, h, s) for s in resident[i][part]]
        levels[0][1 if level else 0] = b                                   # Client::HAdd (:1016-1034)
        if level:
            icc_py.hrebuild(levels, level, n_total, curve, mac=True)
        t.append(levels[level][:1 << level])
    out = []
    for part, new in ((0, new_x), (1, new_y)):
        for j, s in enumerate(new):
            out.append(icc_py.ec_add(curve, icc_py.ec_mul(curve, h, s), icc_py.ec_neg(curve, t[part][j])))
    return mac, out

"""GPU: k_points_to_mont of porla_amd/csrc/msm.hip.h on wire coordinates over the whole 256-bit range -- G1Affine.Unmarshal's
SetBytes semantics at the edges of what the reduction in front of the field product, and that product's own last subtraction, have
to cover (whichever of the two does the work: the kernel was measured without the loops in front, profiles/README.md).  The points
stage of tools/sort_check.hip against the table-point model of tests/ec_vectors.py as tests/sort_vectors.py:expected_point_words
states it: the residue mod p times the factor of the reduced-radix form, with the split the pair (x, y), (beta x, y), and (0, 0) --
however it is sent -- all zero.

Coordinates: 0, 1, p - 1, p, p + 1, 2p and 5p where they fit 256 bits (2p does not on secp256k1, 5p only on BN254: 6p > 2^256),
floor(2^256 / p) p - 1 and + 1 (where the latter fits), 2^256 - 1.  Every pair (x, y) of them is a point; every one of them also
stands as x and as y against a random 256-bit value; then 300 points of two random 256-bit values.  Comparison is word-exact."""
import functools
import random

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests import sort_vectors as sv

pytestmark = pytest.mark.gpu

M256 = sv.M256
N_RANDOM = 300


def special_values(curve):
    p = ev.CURVES[curve].p
    q = M256 // p
    vals = [("0", 0), ("1", 1), ("p-1", p - 1), ("p", p), ("p+1", p + 1), ("2p", 2 * p), ("5p", 5 * p), ("qp-1", q * p - 1), ("qp+1", q * p + 1),
            ("2^256-1", M256)]
    out, seen = [], set()
    for name, v in vals:
        if v <= M256 and v not in seen:
            seen.add(v)
            out.append((name, v))
    return out


@functools.lru_cache(maxsize=None)
def cases(curve):
    """[(name, x, y)]"""
    rng = random.Random(4100 + len(curve))
    sp = special_values(curve)
    out = [("%s,%s" % (nx, ny), x, y) for nx, x in sp for ny, y in sp]
    for name, v in sp:
        out.append(("%s,random" % name, v, rng.getrandbits(256)))
        out.append(("random,%s" % name, rng.getrandbits(256), v))
    out += [("random%d" % i, rng.getrandbits(256), rng.getrandbits(256)) for i in range(N_RANDOM)]
    return out


@functools.lru_cache(maxsize=None)
def outputs(curve):
    """one driver run per curve: the points without and with the split"""
    pts = [x.to_bytes(32, "big") + y.to_bytes(32, "big") for _, x, y in cases(curve)]
    F = sv.File(curve, "points_bounds", [sv.Section(curve, "glv%d" % glv, "points", [1] * 4, glv, 2, 1, points=pts) for glv in (0, 1)])
    return F, sv.run(F, timeout=120)


def test_the_list_reaches_its_edges():
    for curve in sv.CURVE_NAMES:
        p = ev.CURVES[curve].p
        names = [n for n, _ in special_values(curve)]
        assert {"0", "1", "p-1", "p", "p+1", "2^256-1"} <= set(names)
        assert ("5p" in names) == (curve == "bn254") and ("2p" in names) == (curve == "bn254")
        assert 6 * ev.CURVES["bn254"].p > M256 >= 5 * ev.CURVES["bn254"].p and 2 * ev.CURVES["secp256k1"].p > M256
        vals = {v for _, v in special_values(curve)}
        q = M256 // p                                    # (on secp256k1 q = 1: q p - 1 and q p + 1 are p - 1 and p + 1)
        assert q * p - 1 in vals and q * p + 1 in vals and (q + 1) * p > M256
        got = {(x, y) for _, x, y in cases(curve)}
        assert {(0, 0), (p, 0), (0, p), (p, p)} <= got
        assert len(cases(curve)) > N_RANDOM + len(names) ** 2


@pytest.mark.parametrize("glv", [0, 1])
@pytest.mark.parametrize("curve", sv.CURVE_NAMES)
def test_points_over_the_whole_range(curve, glv):
    F, outs = outputs(curve)
    s, o = F.sections[glv], outs[glv]
    assert s.glv == glv
    p = ev.CURVES[curve].p
    rows = o["pts"].reshape(len(s.points), -1)
    zero_rows = 0
    for i, (name, x, y) in enumerate(cases(curve)):
        want = [w for row in sv.expected_point_words(curve, glv, s.points[i]) for w in row]
        assert [int(w) for w in rows[i]] == want, "%s glv %d point %d (%s)" % (curve, glv, i, name)
        if x % p == 0 and y % p == 0:
            assert not rows[i].any(), "%s glv %d point %d (%s): infinity is not all zero" % (curve, glv, i, name)
            zero_rows += 1
        # canonical: every coordinate the kernel stored is below p
        for at in range(0, rows.shape[1], 8):
            assert ev.words_value(rows[i][at:at + 8]) < p
    n_zero = sum(1 for _, v in special_values(curve) if v % p == 0)
    assert zero_rows == n_zero ** 2 >= 4
    assert len(rows) == len(cases(curve))

"""CPU: the vectors of tests/ladder_vectors.py hold what tests/test_ladder_gpu.py relies on -- the two recoder models over every
chosen magnitude, the scalar families (their halves come back from the model of glv_split exactly; their counts), the (n, s) shapes
derived from mac_stage_index, and the fixed-base multiple of G against the affine double-and-add."""
import random

import pytest

from tests import ec_vectors as ev
from tests import ladder_vectors as lv

CURVES = [ev.BN254, ev.SECP]
IDS = [C.name for C in CURVES]


def test_signed_digit_model_over_all_magnitudes():
    mags = lv.magnitudes()
    assert len(mags) == len(lv.pattern_magnitudes()) + 2000
    for m in mags:
        lv.check_signed_digits(m, lv.signed_digits(m))
    # the patterns do what they were chosen for
    assert lv.signed_digits(lv.REP8) == [8] * 32 + [0]                       # every window exactly 8: no carry anywhere
    assert lv.signed_digits(lv.REP8 + 1) == [-7] + [-7] * 31 + [1]           # one more: the carry ripples through every limb
    assert lv.signed_digits(lv.M128)[32] == 1 and lv.signed_digits(lv.REP8 - 1)[32] == 0
    assert lv.signed_digits(0x88888888 << 32)[8:16] == [8] * 8
    assert sum(1 for m in mags if 8 in lv.signed_digits(m)) > 100
    assert sum(1 for m in mags if lv.signed_digits(m)[32]) > 100


def test_wnaf5_model_over_all_magnitudes():
    for m in lv.magnitudes():
        d, left = lv.wnaf5(m)
        lv.check_wnaf5(m, d, left)
        for flip in (0, 1):
            codes = [lv.wnaf_code(x, flip) for x in d]
            assert [lv.decode_code(c) for c in codes] == [-x if flip else x for x in d]
    assert lv.wnaf5(lv.M128)[0][128] == 1 and lv.wnaf5(lv.M128)[0][0] == -1  # the carry into the fifth word: position 128
    assert lv.wnaf5(1 << 120)[0][:120] == [0] * 120                          # a long zero run before the first digit
    assert lv.wnaf_code(-15, 0) == 16 | 8 | 7 and lv.wnaf_code(-15, 1) == 16 | 7 and lv.wnaf_code(1, 0) == 16


@pytest.mark.parametrize("C", CURVES, ids=IDS)
def test_families(C):
    n, l = lv.order(C), lv.lam(C)
    assert (l * l + l + 1) % n == 0
    a = lv.family_a(C)
    assert len(a) == 12 + 16 + 16 and all(0 <= k < n for k in a)
    for m in range(1, 17):
        assert lv.halves_match(C, m * l % n, 0, 0, m, 0) and lv.halves_match(C, m, m, 0, 0, 0)
    b = lv.family_b(C)
    assert len(b) == 17 * 17 * 4 == 1156
    for k, ha, sa, hb, sb in b:
        assert 0 <= k < n and lv.halves_match(C, k, ha, sa, hb, sb), hex(k)
    assert len({k for k, *_ in b}) >= 1000                                   # (a zero half has one sign: some members coincide)
    c = lv.family_c(C)
    if C is ev.SECP:
        assert len(c) == 32
        for k in c:
            assert any(lv.signed_digits(m)[32] == 1 for m, _ in lv.split(C, k)), hex(k)
    else:
        assert len(c) == 0                                                   # BN254's halves stay below 2^126 < 0x88..8
        rng = random.Random(1)
        assert all(m < 1 << 126 for _ in range(2000) for m, _ in lv.split(C, rng.randrange(n)))
    d = lv.family_d(C)
    assert len(d) == 12
    for k, ha, sa, hb, sb in d:
        assert lv.halves_match(C, k, ha, sa, hb, sb), hex(k)
    assert len(lv.family_e(C)) == 256
    fam = lv.families(C)
    assert len(fam) == len(a) + len(b) + len(c) + len(d) + 256
    assert [f for f, _ in lv.families(C, "abcd")] == [f for f, _ in fam if f != "e"]


def test_shapes_follow_from_the_stage_index():
    pb = lv.per_butterfly_shape(256)
    assert (pb.n, pb.s, pb.total) == (512, 9, 256) and pb.entries == [2 * t for t in range(256)]
    assert [pb.bf[t][:2] for t in (0, 255)] == [(0, 256), (255, 256)]
    q = lv.uniform_shape(16, 64)
    assert (q.n, q.s) == (2048, 7) and q.entries == [32 * j for j in range(64)] and (q.n >> q.s) >= 16
    o = lv.uniform_shape(64, 16)
    assert (o.n, o.s) == (2048, 5) and o.entries == [128 * j for j in range(16)] and (o.n >> o.s) >= 64 and (o.n // 2) % 256 == 0
    # a butterfly count that is no multiple of either block's: padding quads and octets in the last block
    assert lv.PAD_TOTAL % lv.MACQ_BF and lv.PAD_TOTAL % lv.MACO_BF and lv.PAD_TOTAL < pb.total


@pytest.mark.parametrize("C", CURVES, ids=IDS)
def test_fixed_base_multiple_equals_double_and_add(C):
    n = lv.order(C)
    assert ev.ec_mul(C, n - 1, C.g) == ev.ec_neg(C, C.g)
    rng = random.Random(7)
    for k in [0, 1, 2, 255, 256, n - 1, n, n + 1, lv.lam(C)] + [rng.randrange(n) for _ in range(8)] + [rng.randrange(1 << 40) << 80]:
        assert lv.mul_g(C, k) == (ev.ec_mul(C, k % n, C.g) if k % n else None), hex(k)
    assert lv.mul_g(C, lv.lam(C)) == ev.ec_phi(C, C.g)


@pytest.mark.parametrize("C", CURVES, ids=IDS)
def test_butterfly_expectations(C):
    seen = set()
    for idx in range(16):
        for slot in range(2):
            b = lv.butterfly(C, lv.family_e(C)[idx], idx, slot)
            seen.add((b.case, b.p_kind))
            assert b.lo == ev.ec_add(C, b.um, ev.ec_mul(C, b.k, b.P)) and b.hi == ev.ec_add(C, b.um, ev.ec_neg(C, ev.ec_mul(C, b.k, b.P)))
            if b.case == "same":
                assert b.hi is None and b.lo == ev.ec_add(C, b.tm, b.tm)
            if b.case == "neg":
                assert b.lo is None
    assert {c for c, _ in seen} == set(lv.UM_CASES) and {k for _, k in seen} == set(lv.KINDS)
    t = lv.trivial_butterfly(C, 5)
    assert t.lo is None and t.hi is None and not any(t.p_words) and not any(t.um_words)
    # a ladder's result carries an addition's or a doubling's bound unless one table entry passed through
    n, l = lv.order(C), lv.lam(C)
    assert [lv.by_value_key(C, k) for k in (1, 3, 15, n - 1, l, n - l)] == ["operand"] * 6
    assert [lv.by_value_key(C, k) for k in (2, 17, 32, l + 1, 2 * l % n, lv.family_e(C)[0])] == ["add"] * 6

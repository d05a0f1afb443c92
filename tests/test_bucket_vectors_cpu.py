"""CPU: the bucket lists of tests/bucket_vectors.py hold what tests/test_bucket_sum_gpu.py relies on -- every named family, kind,
length and position is there whatever the seed, no position case is lost, every expected sum computed in the exponent equals the
sum of the bucket's points added one by one with the affine group law, and the heavy_stride pass sends k_bucket_combine round its
grid-stride loop a second time."""
import random

import pytest

from tests import bucket_vectors as bv
from tests import ec_vectors as ev
from tests import ladder_vectors as lv

CURVE_NAMES = ["bn254", "secp256k1"]


def test_position_grid():
    """the listed lengths, positions and kinds; 126..129 wherever the bucket reaches them"""
    assert bv.POSITION_L == [1, 2, 3, 4, 5, 64, 127, 128, 129, 130, 255, 256, 257, 385]
    assert bv.position_js(1) == [0] and bv.position_js(2) == [0, 1] and bv.position_js(5) == [0, 1, 2, 3, 4]
    assert bv.position_js(64) == [0, 1, 2, 3, 32, 62, 63]
    assert bv.position_js(128) == [0, 1, 2, 3, 64, 126, 127] and bv.position_js(129) == [0, 1, 2, 3, 64, 126, 127, 128]
    assert bv.position_js(385) == [0, 1, 2, 3, 126, 127, 128, 129, 192, 383, 384]
    cases = bv.position_cases()
    # positions per length, times five kinds in two forms; position 0 holds a point at infinity only
    n_pos = sum(len(bv.position_js(L)) for L in bv.POSITION_L)
    assert n_pos == 1 + 2 + 3 + 4 + 5 + 7 + 7 + 7 + 8 + 9 + 10 + 10 + 10 + 11
    assert len(cases) == len(set(cases)) == 2 * (5 * n_pos - 4 * len(bv.POSITION_L)) == 828


@pytest.mark.parametrize("seed", [None, 7])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_every_family_is_present(curve, seed):
    F = bv.single_pass_file(curve) if seed is None else bv.single_pass_file(curve, seed)
    got = [(c["kind"], c["L"], c["j"], c["form"]) for c in F.cases if c["family"] == "position"]
    assert got == bv.position_cases()                             # none dropped, none merged
    for c in F.cases:
        if c["family"] != "position":
            continue
        words, j, kind = c["passes"][0], c["j"], c["kind"]
        assert len(words) == c["L"] and bool(words[j] & bv.SIGN) == (c["form"] == "signbit")
        vals = [F.T.value(w) for w in words]
        first = j % bv.CHUNK == 0
        acc = sum(vals[:j] if first else vals[j - j % bv.CHUNK:j]) % F.T.n          # what the item's accumulator holds before j
        want = {"inf": 0, "prev": vals[j - 1], "negprev": -vals[j - 1], "runsum": acc, "negrunsum": -acc}[kind] % F.T.n
        assert vals[j] == want and (kind == "inf") == (want == 0), (kind, c["L"], j)
        assert all(v != 0 for i, v in enumerate(vals) if i != j)
        # every other entry is an ordinary distinct multiple of the generator
        small = [min(v, F.T.n - v) for i, v in enumerate(vals) if i != j]
        assert len(set(small)) == len(small) and all(1 <= s <= bv.SMALL for s in small)
    kinds = lambda fam: [c["kind"] for c in F.cases if c["family"] == fam]
    assert kinds("items") == bv.ITEMS_KINDS
    assert kinds("fill") == ["fill"] * bv.N_FILL and len({len(c["passes"][0]) for c in F.cases if c["family"] == "fill"}) > 20
    heavy = kinds("heavy_stride")
    assert heavy.count("heavy") == bv.N_HEAVY and heavy.count("single") == bv.N_HEAVY and heavy.count("empty") == bv.N_HEAVY // 3
    assert "heavy" in heavy[:3] and "single" in heavy[:3] and "empty" in heavy[:3]          # interleaved, not one after the other
    if seed is None:
        A, G = bv.accumulate_file(curve), bv.glv_file(curve)
        assert [c["kind"] for c in A.cases] == bv.ACC_KINDS2 + bv.ACC_KINDS3 + ["late:" + k for k in bv.ACC_KINDS2]
        assert sorted(set(c["kind"] for c in A.cases)) == sorted(bv.ACC_KINDS) and A.n_passes == 3
        assert set(c["kind"] for c in G.cases) == set(bv.GLV_KINDS) | {"fill"} and G.T.glv
        for kind in ("P,-phiP", "phiP,phiP", "phiP,-phiP,Q", "P,phiP", "phi_runsum", "phi_negrunsum"):
            assert {c["form"] for c in G.cases if c["kind"] == kind} == set(bv.FORMS)
        # both slots and both signs of the doubled table are in use
        seen = {(w & 1, bool(w & bv.SIGN)) for c in G.cases for w in c["passes"][0]}
        assert len(seen) == 4


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_items_and_accumulate_shapes(curve):
    """the compositions do what their names say, in the exponent"""
    F, A = bv.single_pass_file(curve), bv.accumulate_file(curve)
    n = F.T.n
    by = {c["kind"]: c for c in F.cases if c["family"] == "items"}

    def item_sums(T, words):
        v = [T.value(w) for w in words]
        return [sum(v[i:i + bv.CHUNK]) % n for i in range(0, len(v), bv.CHUNK)]
    for m in (1, 2, 3):
        assert len(by["full_%d" % (128 * m)]["passes"][0]) == 128 * m and len(by["full_plus_one_%d" % (128 * m + 1)]["passes"][0]) == 128 * m + 1
    for name, L in (("equal_sums", 256), ("equal_sums_copy", 129)):
        a, b = item_sums(F.T, by[name]["passes"][0])
        assert a == b != 0 and len(by[name]["passes"][0]) == L
    for name, L in (("opposite_sums", 256), ("opposite_sums_copy", 129)):
        a, b = item_sums(F.T, by[name]["passes"][0])
        assert (a + b) % n == 0 and a != 0 and len(by[name]["passes"][0]) == L
    for name, count in (("inf_item_between", 3), ("inf_item_between_plus_one", 4)):
        s = item_sums(F.T, by[name]["passes"][0])
        assert len(s) == count and s[1] == 0 and all(x != 0 for i, x in enumerate(s) if i != 1)
    for L in (1, 2, 129):
        assert [F.T.value(w) for w in by["all_inf_%d" % L]["passes"][0]] == [0] * L
    exp = bv.expected(A)
    kinds = [c["kind"] for c in A.cases]
    at = lambda kind, p: exp[p][kinds.index(kind)]
    assert at("P|P", 1)["exp"] == 2 * at("P|P", 0)["exp"] % n and at("P|-P", 1)["exp"] == 0 and at("P,-P|Q", 0)["exp"] == 0
    assert at("P|-P|Q", 0)["exp"] != 0 and at("P|-P|Q", 1)["exp"] == 0 and at("P|-P|Q", 2)["exp"] != 0
    assert at("multi|S", 1)["exp"] == 2 * at("multi|S", 0)["exp"] % n and at("multi|-S", 1)["exp"] == 0
    assert at("P|multi_total_P", 1)["exp"] == 2 * at("P|multi_total_P", 0)["exp"] % n and at("P|multi_total_-P", 1)["exp"] == 0
    assert at("P|multi_item0_P", 1)["key"] == "add" and at("multi|multi_total_-S", 1)["exp"] == 0
    assert at("P|inf", 1)["same"] and at("P|multi_inf", 1)["same"] and at("multi|multi_inf", 1)["same"] and at("P|empty", 1)["same"]
    assert at("late:P|P", 0)["exp"] == 0 and at("late:P|P", 2)["exp"] == 2 * at("late:P|P", 1)["exp"] % n
    # an odd and an even number of additions in the accumulating pass
    counts = {len(c["passes"][1]) for c in A.cases if 0 < len(c["passes"][1]) <= bv.CHUNK and c["passes"][0]}
    assert {1, 2, 3} <= counts
    # a bucket only one pass touches stands next to one both touch
    assert kinds.index("P|empty") + 1 == kinds.index("P,-P|Q") and kinds.index("empty|Q") + 1 == kinds.index("P|empty")


@pytest.mark.parametrize("name", ["single", "accumulate", "glv"])
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_exponent_sums_equal_one_by_one_sums(curve, name):
    C = ev.CURVES[curve]
    F = bv.FILES[name](curve)
    exp = bv.expected(F)
    checked = 0
    for b, c in enumerate(F.cases):
        total = None
        for p in range(F.n_passes):
            total = ev.ec_add(C, total, bv.sum_one_by_one(F, c["passes"][p]))
            assert bv.mul(C, exp[p][b]["exp"]) == total, "%s %s bucket %d (%s %s) pass %d" % (curve, name, b, c["family"], c["kind"], p)
            checked += 1
    assert checked == len(F.cases) * F.n_passes
    if name == "glv":
        assert lv.mul_g(C, lv.lam(C)) == ev.ec_phi(C, C.g)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_heavy_stride_makes_a_second_trip(curve):
    F = bv.single_pass_file(curve)
    multi = [len(c["passes"][0]) for c in F.cases if len(c["passes"][0]) > bv.CHUNK]
    assert len(multi) > bv.COMBINE_BLOCKS and sum(1 for c in F.cases if c["kind"] == "heavy") > bv.COMBINE_BLOCKS
    sums = {e["exp"] for e, c in zip(bv.expected(F)[0], F.cases) if c["kind"] == "heavy"}
    assert len(sums) == bv.N_HEAVY                                # no two of them have the same sum
    assert len(F.cases) > 1024                                    # more than one block of the scheduling kernels


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_table_points_are_the_stated_multiples(curve):
    C = ev.CURVES[curve]
    T = bv.single_pass_file(curve).T
    rng = random.Random(11)
    picks = [0, 1, 2, len(T.exps) - 1] + [rng.randrange(len(T.exps)) for _ in range(24)]
    wire = T.wire().tobytes()
    for i in picks:
        P = ev.ec_mul(C, T.exps[i], C.g) if T.exps[i] else None
        assert bv.mul(C, T.exps[i]) == P and (P is None or ev.on_curve(C, P))
        want = bytes(64) if P is None else P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big")
        assert wire[64 * i:64 * i + 64] == want
    assert T.exps[0] == 0 and len(set(T.exps)) == len(T.exps)
    assert any(k > bv.SMALL and T.n - k > bv.SMALL for k in (T.exps[i] for i in picks))       # a running sum, not a small multiple


def test_combine_model():
    n = 101
    assert bv.combine_model(n, 0, [5, 0]) == (5, "operand") and bv.combine_model(n, 0, [5, 96]) == (0, None)
    assert bv.combine_model(n, 0, [5, 5]) == (10, "add") and bv.combine_model(n, 7, [0, 0]) == (7, "operand")
    assert bv.combine_model(n, 7, [94, 3]) == (3, "operand") and bv.combine_model(n, 0, [1, 2, 100, 4]) == (6, "add")
    rng = random.Random(3)
    for _ in range(50):
        items = [rng.randrange(n) for _ in range(rng.randint(2, 64))]
        st = rng.randrange(n)
        assert bv.combine_model(n, st, items)[0] == (st + sum(items)) % n

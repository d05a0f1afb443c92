"""CPU: the bucket arrays of tests/tree_vectors.py hold what tests/test_tree_gpu.py relies on, and the reduction tree's schedule
(porla_amd/csrc/msm_tree.hip.h:tree_plan, printed by tree_check --plan, which needs no device) keeps its layout:
  completeness      every family and every (level, slot, kind, position) combination is in the files, with the operands it names
  self-consistency  sum (b + 1) e_b = S + sum 2^k M_k for every case; the roots and every M_k built bottom-up equal mul(C, exponent)
  layout            for c in 2..17, W in {1, 2, 3, 4, 5, 8, 15, 16, 17}, lone and not: every access inside the stated scratch sizes,
                    S ranges of levels and parts disjoint, no read range of a launch overlapping a write range, every node read
                    written before by the same part (or a bucket), the parts' fin ranges tiling [0, W c), and the plan equal to
                    tree_vectors.model_plan, the rules restated -- a change to the schedule is made in both places"""
import os

import numpy as np
import pytest

from tests import bucket_vectors as bv
from tests import ec_vectors as ev
from tests import ladder_vectors as lv
from tests import tree_vectors as tv

CURVE_NAMES = ["bn254", "secp256k1"]


def test_driver_is_built():
    assert os.path.exists(tv.EXE), "build it with make -C porla_amd/csrc"


def operand_sums(k, l, s, node, n):
    L, R = tv.operand_sets(l, s, node)
    return sum(k.exps[b] for b in L) % n, sum(k.exps[b] for b in R) % n, L, R


def test_operand_sets():
    """the S addition takes the node's halves, slot s the buckets with bit s set; the aliased slot's operands are the odd entries
    of S^(l-2) under the node"""
    assert tv.operand_sets(0, 0, 3) == ([6], [7])
    assert tv.operand_sets(2, 2, 1) == ([8, 9, 10, 11], [12, 13, 14, 15])
    assert tv.operand_sets(2, 0, 0) == ([1, 3], [5, 7])
    assert tv.operand_sets(2, 1, 0) == ([2, 3], [6, 7])              # S^0[1] and S^0[3]: entries 4i + 1 and 4i + 3 of S^(l-2)
    assert tv.operand_sets(3, 2, 1) == ([20, 21, 22, 23], [28, 29, 30, 31])
    assert tv.operand_sets(1, 0, 2) == ([9], [11])                   # the buckets 4i + 1 and 4i + 3


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_slot_family_is_complete(curve):
    C = ev.CURVES[curve]
    n = lv.order(C)
    grid, ballots = tv.slot_cases(curve)
    want = tv.slot_grid()
    assert [(k.meta["l"], k.meta["s"], k.meta["pos"], k.kind, k.meta["origin"] or "empty") for k in grid] == want
    # every level, every slot s <= l, three positions, five kinds; infinity by empty buckets everywhere, by cancellation wherever
    # an operand covers two buckets or more: that is every (l, s) but the S additions of level 0 and the slots of level 1
    levels = range(tv.SLOT_C - 1)
    assert {(l, s) for l, s, _, _, _ in want} == {(l, s) for l in levels for s in range(l + 1)}
    one_bucket = {(0, 0), (1, 0)}
    for l in levels:
        for s in range(l + 1):
            here = [(pos, kind, origin) for ll, ss, pos, kind, origin in want if (ll, ss) == (l, s)]
            origins = tv.ORIGINS[:1] if (l, s) in one_bucket else tv.ORIGINS
            assert sorted(here) == sorted((pos, kind, o) for pos in tv.POSITIONS for kind in tv.KINDS
                                          for o in (origins if kind.endswith("_inf") else tv.ORIGINS[:1])), (l, s)
    for k in grid:
        l, s, node = k.meta["l"], k.meta["s"], k.meta["node"]
        assert node == (0 if k.meta["pos"] == "first" else (k.B >> (l + 1)) - 1)
        sl, sr, L, R = operand_sums(k, l, s, node, n)
        if k.kind == "equal":
            assert sl == sr != 0, k
        elif k.kind == "opposite":
            assert (sl + sr) % n == 0 and sl != 0, k
        else:
            assert (sl == 0) == (k.kind in ("left_inf", "both_inf")) and (sr == 0) == (k.kind in ("right_inf", "both_inf")), k
            for side, name in ((L, "left_inf"), (R, "right_inf")):
                if k.kind in (name, "both_inf"):
                    empty = all(k.exps[b] == 0 for b in side)
                    assert empty == (k.meta["origin"] == "empty"), k
                    assert empty or all(k.exps[b] != 0 for b in side), k          # cancelled: non-empty buckets whose sum is zero
        # the rest of the window: ordinary, pairwise distinct buckets, so the exceptional quad sits among quads on the straight-line path
        rest = [min(k.exps[b], n - k.exps[b]) for b in range(k.B) if b not in L and b not in R]
        assert len(set(rest)) == len(rest) and all(1 <= x <= bv.SMALL for x in rest), k
        lev = tv.expected(C, k)["S"][0]
        assert all(lev[i][2] == "add" for i in range(len(lev)) if 2 * i not in L + R and 2 * i + 1 not in L + R), k
    assert [(k.meta["node"], k.kind) for k in ballots] == [(node, kind) for node in tv.BALLOT_NODES for kind in tv.KINDS]
    for k in ballots:
        sl, sr, _, _ = operand_sums(k, 0, 0, k.meta["node"], n)
        assert k.c == tv.BALLOT_C == 6 and k.B >> 1 == 16        # 16 nodes per window at level 0: node j is quad j of its wave
        if k.kind == "equal":
            assert sl == sr != 0
        elif k.kind == "opposite":
            assert (sl + sr) % n == 0 and sl
        else:
            assert (sl == 0) == (k.kind in ("left_inf", "both_inf")) and (sr == 0) == (k.kind in ("right_inf", "both_inf"))
    F = tv.slot_file(curve)
    assert [sc.label for sc in F.sections] == [label for label, _ in tv.FORCED_SLOT] + ["ballot_" + label for label, _ in tv.FORCED_6]
    assert [label for label, _ in tv.FORCED_SLOT] == ["default", "l0_2", "all_level", "all_level_quad", "front2_level", "front2_level_quad"]
    for sc in F.sections:
        flat = [k for r in sc.runs for k in r]
        if sc.label.startswith("ballot_"):
            assert (sc.c, sc.W) == (6, 3) and all(any(k is x for x in flat) for k in ballots)
            continue
        assert (sc.c, sc.W) == (tv.SLOT_C, 3)
        assert all(any(k is x for x in flat) for k in grid)                       # none dropped
        for r in sc.runs:
            assert all(k.meta["pos"] != "last_of_last_window" for k in r[:-1])
        assert sum(1 for r in sc.runs if r[-1].meta["pos"] == "last_of_last_window") == len(want) // 3
    # the plans: which kernel runs which level
    kinds = {sc.label: [(q["kind"], q["l"]) for q in p["launches"]] for sc, p in zip(F.sections, tv.file_plans(curve, "slot"))}
    assert kinds["default"] == [("tail", 0)] and kinds["l0_2"] == [("level_quad", 0), ("level_quad", 1), ("tail", 2)]
    assert kinds["all_level"] == [("level", 0), ("level", 1), ("level", 2), ("tail", 3)]
    assert kinds["all_level_quad"] == [("level_quad", 0), ("level_quad", 1), ("level_quad", 2), ("tail", 3)]
    assert kinds["front2_level"] == [("front2", 1), ("level", 2), ("tail", 3)]
    assert kinds["front2_level_quad"] == [("front2", 1), ("level_quad", 2), ("tail", 3)]
    assert kinds["ballot_default"] == [("tail", 0)] and kinds["ballot_all_level_quad"][0] == ("level_quad", 0)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_other_families_are_complete(curve):
    C = ev.CURVES[curve]
    n = lv.order(C)
    # copy
    F = tv.copy_file(curve)
    assert [sc.label for sc in F.sections] == ["c2", "c2_lone", "c2_W1", "c3", "c6", "c10"]
    assert [k.kind for k in F.sections[0].runs[0]] == ["ordinary", "copy_inf"] + tv.KINDS
    for sc in F.sections[3:]:
        by = {k.kind: k for k in sc.runs[0]}
        assert sorted(by) == ["copy_inf_cancel", "copy_inf_empty", "ordinary"]
        for kind, k in by.items():
            top = tv.expected(C, k)["fin"][k.c - 1][0]
            assert (top == 0) == (kind != "ordinary") and top == sum(k.exps[k.B // 2:]) % n
            assert all(e != 0 for e in k.exps[k.B // 2:]) == (kind != "copy_inf_empty")
    # sparse
    F = tv.sparse_file(curve)
    cs = [k for r in F.sections[0].runs for k in r]
    B = 32
    assert {k.kind for k in cs} == {"all_empty", "single", "all_equal", "alternating", "alternating_pairs"}
    assert sorted(k.meta["at"] for k in cs if k.kind == "single") == sorted({0, B - 1, 1, 2, 4, 8, 16})
    for k in cs:
        e = tv.expected(C, k)
        if k.kind == "all_empty":
            assert all(x[0] == 0 for x in e["fin"])
        if k.kind == "single":
            assert sum(1 for x in k.exps if x) == 1 and k.exps[k.meta["at"]] != 0
        if k.kind == "all_equal":                                 # a doubling at every S node and in every slot of the root
            assert all(x[2] == "double" for lev in e["S"] for x in lev)
        if k.kind == "alternating":
            assert all(x[0] == 0 for lev in e["S"] for x in lev) and e["fin"][1][0] != 0
    assert [sc.label for sc in F.sections] == [label for label, _ in tv.FORCED_6] and F.sections[0].c == 6
    # shape: the product's plan, lone and not lone
    F = tv.shape_file(curve)
    assert [(sc.c, sc.W, sc.lone) for sc in F.sections] == [(c, W, lone) for c in tv.SHAPE_C for W in tv.SHAPE_W for lone in (0, 1)]
    assert all(sc.default_plan() for sc in F.sections)
    for sc, plan in zip(F.sections, tv.file_plans(curve, "shape")):
        kinds = [q["kind"] for q in plan["launches"]]
        assert plan["parts_info"][0]["l0"] == tv.L0_BY_C[sc.c] and plan["parts"] == 1
        assert kinds == ["level_quad"] * tv.L0_BY_C[sc.c] + ["tail"]
        if sc.c == 9:       # 2 * 128 additions at level 0, four lanes each, in a block of 512 threads: two passes
            assert plan["launches"][-1]["block"] == 512 and 2 * (sc.c - 1 > 1) * (256 >> 1) * 4 > 512
    # forced plans
    F = tv.forced_file(curve)
    labels = {sc.label: (sc, p) for sc, p in zip(F.sections, tv.file_plans(curve, "forced"))}
    kinds = lambda label: [(q["part"], q["kind"], q["l"]) for q in labels[label][1]["launches"]]
    assert kinds("c6_W3_l0_3") == [(0, "level_quad", 0), (0, "level_quad", 1), (0, "level_quad", 2), (0, "tail", 3)]
    assert kinds("c6_W3_all_level") == [(0, "level", l) for l in range(4)] + [(0, "tail", 4)]
    assert kinds("c6_W3_all_level_quad") == [(0, "level_quad", l) for l in range(4)] + [(0, "tail", 4)]
    assert kinds("c6_W3_front2_level") == [(0, "front2", 1), (0, "level", 2), (0, "level", 3), (0, "tail", 4)]
    assert kinds("c6_W3_front2_level_quad") == [(0, "front2", 1), (0, "level_quad", 2), (0, "level_quad", 3), (0, "tail", 4)]
    for W in (2, 3, 5):
        sc, plan = labels["c6_W%d_parts2" % W]
        assert plan["parts"] == 2 and [p["Wp"] for p in plan["parts_info"]] == [W // 2, W - W // 2]
        assert plan["launches"][-1]["fin"] == (W // 2) * 6 and kinds("c6_W%d_parts2" % W) == [(0, "tail", 0), (1, "tail", 0)]
        assert [k[:2] for k in kinds("c6_W%d_parts2_front2_level" % W)] == [(p, kd) for p in (0, 1) for kd in ("front2", "level", "level", "tail")]
    for l0 in range(6):
        assert kinds("c7_W3_l0_%d_level" % l0) == [(0, "level", l) for l in range(l0)] + [(0, "tail", l0)]
        assert kinds("c7_W3_l0_%d_level_quad" % l0) == [(0, "level_quad", l) for l in range(l0)] + [(0, "tail", l0)]
    # bounds
    if curve == "bn254":
        F = tv.bounds_file(curve)
        assert all(k.top for k in F.cases())
        deep = [sc for sc in F.sections if sc.label.startswith("deep")]
        assert [(sc.c, sc.W) for sc in deep] == [(tv.DEEP_C, 1)] * 4
        k = deep[0].runs[0][0]
        assert 100 < sum(1 for e in k.exps if e) < 400 and tv.expected(C, k)["fin"][0][0] != 0
        kinds = [[q["kind"] for q in p["launches"]] for p in tv.file_plans(curve, "bounds")[-4:]]
        assert "level_quad" in kinds[0] and "level" in kinds[2] and kinds[3][0] == "front2"
        # the words: Y up to 4p, a residue within 2^-6 of a multiple of p in every other bucket
        w = tv.case_words(C, F.sections[0].runs[0][0])
        ys = [ev.get_words(row, 0)[1] for row in w]
        assert all(3 * C.p < y <= 4 * C.p for y in ys)
        assert sum(1 for row in w if any(v % C.p > C.p - (C.p >> 6) for v in ev.get_words(row, 0))) >= len(w) // 2
    else:
        assert "bounds" not in tv.FILE_NAMES[curve]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_cases_are_self_consistent(curve):
    """sum (b + 1) e_b = S + sum 2^k M_k in the exponent; the bottom-up points of the root, of every M_k and of the copied node
    are the stated multiples of G; the words decode to the stated buckets"""
    C = ev.CURVES[curve]
    n = lv.order(C)
    seen, checked = set(), 0
    for name in tv.FILE_NAMES[curve]:
        for k in tv.FILES[name](curve).cases():
            if id(k) in seen:
                continue
            seen.add(id(k))
            e = tv.expected(C, k)
            fin = [x[0] for x in e["fin"]]
            assert fin == tv.fin_exponents(k, n), k
            assert sum((b + 1) * x for b, x in enumerate(k.exps)) % n == (fin[0] + sum(m << j for j, m in enumerate(fin[1:]))) % n, k
            for x, P in e["fin"]:
                assert P == bv.mul(C, x), k
            for l, lev in enumerate(e["S"]):
                assert len(lev) == k.B >> (l + 1)
                for i in (0, len(lev) - 1):
                    assert lev[i][0] == sum(k.exps[i << (l + 1):(i + 1) << (l + 1)]) % n and lev[i][1] == bv.mul(C, lev[i][0]), k
            checked += 1
    assert checked == len(seen) > 250
    k = tv.slot_cases(curve)[0][17]
    w = tv.case_words(C, k)
    for b in (0, 5, k.B - 1):
        ev.check_point_mem(C, w[b], bv.mul(C, k.exps[b]), "operand", "bucket %d" % b)


# ================================================================ the layout, through --plan
GROUPS = [(c, W, lone, None, None, None, None) for c in tv.PLAN_C for W in tv.PLAN_W for lone in (0, 1)]


@pytest.fixture(scope="module")
def plans():
    return {"bn254": tv.dump_plans("bn254", GROUPS), "secp256k1": tv.dump_plans("secp256k1", GROUPS[:40])}


def test_default_plan_equals_the_restated_rules(plans):
    for g, plan in zip(GROUPS, plans["bn254"]):
        assert plan == tv.model_plan(*g[:3]), g
    for g, plan in zip(GROUPS, plans["secp256k1"]):               # both curves have the reduced-radix memory form: the same plans
        assert plan == tv.model_plan(*g[:3]), g
    # the paths the module's comment names, at the shapes the product takes them
    by = {g[:3]: p for g, p in zip(GROUPS, plans["bn254"])}
    assert by[(16, 16, 1)]["parts"] == 2 and by[(16, 16, 0)]["parts"] == 1 and by[(17, 3, 1)]["parts"] == 1 and by[(17, 4, 1)]["parts"] == 2
    assert by[(17, 17, 1)]["parts_info"][1] == dict(part=1, w0=8, Wp=9, l0=by[(17, 17, 1)]["parts_info"][0]["l0"], front2=0, quad_max=65536)
    assert by[(16, 16, 0)]["launches"][0]["kind"] == "front2" and by[(16, 16, 1)]["launches"][0]["kind"] == "level"
    assert by[(16, 1, 0)]["launches"][0]["kind"] == "level_quad" and by[(17, 1, 0)]["launches"][0]["kind"] == "front2"
    assert [tv.tail_start(1 << (c - 1), c - 1) for c in tv.SHAPE_C] == [tv.L0_BY_C[c] for c in tv.SHAPE_C]


@pytest.mark.parametrize("lone", [0, 1])
def test_layout_invariants(plans, lone):
    checked = 0
    for g, plan in zip(GROUPS, plans["bn254"]):
        if g[2] != lone:
            continue
        check_layout(plan)
        checked += 1
    assert checked == len(tv.PLAN_C) * len(tv.PLAN_W)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_layout_invariants_of_the_forced_plans(curve):
    """the plans the GPU module runs: nothing reaches the device that leaves its buffers"""
    for name in tv.FILE_NAMES[curve]:
        for plan in tv.file_plans(curve, name):
            check_layout(plan)


def check_layout(plan):
    c, W, B, nlev = plan["c"], plan["W"], plan["B"], plan["nlev"]
    lay = tv.Layout(plan)                                         # bounds, read-after-write, read / write overlap: asserted inside
    where = "c=%d W=%d lone=%d" % (c, W, plan["lone"])
    # fin: the parts tile [0, W c), every entry written once
    at = 0
    for info, q in zip(plan["parts_info"], [q for q in plan["launches"] if q["kind"] == "tail"]):
        assert q["fin"] == at == info["w0"] * c and q["part"] == info["part"], where
        at += info["Wp"] * c
    assert at == W * c == plan["fin_entries"] and lay.written["F"].all(), where
    assert sum(p["Wp"] for p in plan["parts_info"]) == W
    # S: the levels of the parts are disjoint ranges, written completely but for the even entries of S^0 under front2, and nothing else
    want = np.zeros(plan["s_entries"], dtype=bool)
    ranges = []
    for info in plan["parts_info"]:
        nbp = info["Wp"] * B
        for l in range(nlev - 1):                                 # the last level goes to fin
            lo = lay.s_entry(info["part"], l, 0)
            ranges.append((lo, lo + (nbp >> (l + 1))))
            want[lo:lo + (nbp >> (l + 1))] = True
            if l == 0 and info["front2"]:
                want[lo:lo + (nbp >> 1):2] = False
    ranges.sort()
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])) and (not ranges or ranges[-1][1] <= plan["s_entries"]), where
    assert np.array_equal(lay.written["S"], want), where
    # the slack entries: one behind each part's S levels, one behind each M half and each tail half
    assert not lay.written["S"][-1] and not lay.written["M"][-1] and not lay.written["T"][-1], where


def test_plan_refusals():
    """what the kernels do not support never becomes a plan"""
    import subprocess

    def refused(args, what):
        r = subprocess.run([tv.EXE, "--plan", "bn254"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
    refused([6, 3, 0, "-", 1, "-", 1], "front2 needs l0 >= 2")
    refused([6, 3, 0, "-", 1, "-", "-"], "front2 needs l0 >= 2")          # the product's l0 at c = 6 is 0
    refused([2, 3, 0, "-", 1, "-", 0], "front2 needs l0 >= 2")
    refused([6, 1, 0, 2, "-", "-", "-"], "two parts need at least two windows")
    refused([6, 3, 0, 3, "-", "-", "-"], "parts must be 1 or 2")
    refused([6, 3, 0, "-", "-", "-", 5], "l0 < nlev")
    refused([25, 1, 0], "shape out of range")
    refused([1, 1, 0], "shape out of range")
    refused([6, 0, 0], "shape out of range")
    refused([6, 3, 2], "header out of range")

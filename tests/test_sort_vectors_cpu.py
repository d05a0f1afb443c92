"""CPU: the scalars of tests/sort_vectors.py reach what tests/test_sort_gpu.py relies on, and the sort front's launch shape
(porla_amd/csrc/msm.hip.h:sort_front_plan, printed by sort_check --plan, which needs no device) keeps its values:
  completeness      every family and kind is in the files, and every edge is what the model sees: a partition with exactly STAGE_CAP + 1
                    entries, a run of exactly L items, a raw digit of 2^(c-1), an all-ones digit under a carry, ...
  self-consistency  for every model scalar sum_w digit_w 2^(wc) rebuilds the sub-scalar and k1 + lambda k2 = k (mod n); the array form
                    of the recode equals the one-scalar form
  plan              sort_check --plan equals tests/golden/sort_front_plan.txt -- recorded from the inline code of msm_launch that
                    sort_front_plan replaced -- and the rules restated in sort_vectors.plan_model
  refusals          malformed files end with a message and status 1 before any device call"""
import os
import subprocess

import numpy as np
import pytest

from tests import common
from tests import ec_vectors as ev
from tests import ladder_vectors as lv
from tests import sort_vectors as sv

CURVE_NAMES = sv.CURVE_NAMES


def test_driver_is_built():
    assert os.path.exists(sv.EXE), "build it with make -C porla_amd/csrc"


def run_lengths(sec, w=0):
    """items per (tile, partition) of window w, from the model"""
    m, P = sec.model, sec.plan["P"]
    cap = sec.plan["tile_cap"]
    live = np.nonzero(m.bucket[w] >= 0)[0]
    return np.bincount((live // cap) * P + (m.bucket[w][live] & (P - 1)), minlength=sec.plan["T_tiles"] * P).reshape(-1, P)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_edges_family_is_complete(curve):
    F = sv.file(curve, "edges")
    assert [(s.c, s.glv) for s in F.sections[:18]] == [(c, glv) for c in sv.SHAPE_C for glv in (0, 1)]
    assert [s.label for s in F.sections[18:]] == ["c17_glv1_fullW", "c16_glv1_W9"]
    r, q = lv.order(ev.CURVES[curve]), sv.MAX_Q[curve]
    checked = 0
    for s in F.sections:
        assert s.W == sv.SHORT_W.get(s.c, sv.full_W(curve, s.glv, s.c)) or s.label in ("c17_glv1_fullW", "c16_glv1_W9")
        assert s.forced == (None, None, None)
        # order edges: they lead the section
        want = [0, 1, r - 1, r, r + 1, 2 * r, q * r, q * r + 1, sv.M256]
        want += [v for w in range(1, s.W + 1) if w * s.c < 256 for v in (1 << (w * s.c), (1 << (w * s.c)) - 1)]
        want = [v for v in want if v <= sv.M256]
        assert s.scalars[:len(want)] == want
        assert [sv.reduce_order(curve, v) for v in want[:8 if 2 * r <= sv.M256 else 7]] == ([0, 1, r - 1, 0, 1, 0, 0, 1] if 2 * r <= sv.M256 else [0, 1, r - 1, 0, 1, 0, 1])
        assert sv.reduce_order(curve, sv.M256) == sv.M256 - q * r
        for kind, i, e, w in s.edges:
            assert sv.check_edge(s, kind, i, e, w), (s, kind, i, e, w)
            checked += 1
        kinds = {(kind, w) for kind, _, _, w in s.edges}
        per_window = {"last_positive", "first_negative"}
        top = 256 if not s.glv else sv.GLV_BITS[curve] - 3
        limit = r if not s.glv else 1 << top
        for w in range(s.W):                                      # every window whose edge value is a sub-scalar at all
            B = 1 << (s.c - 1)
            for kind, v in (("last_positive", B << (w * s.c)), ("first_negative", (B + 1) << (w * s.c))):
                assert ((kind, w) in kinds) == (v < limit), (s, kind, w)
            if w >= 1 and (((1 << s.c) - 1) << (w * s.c)) | ((B + 1) << ((w - 1) * s.c)) < limit:
                assert ("ones_with_carry", w) in kinds, (s, w)
        if (s.W - 1) * s.c < (254 if not s.glv else top):
            assert ("carry_run", s.W - 1) in kinds and ("carry_only_top", s.W - 1) in kinds, s
        if s.glv:
            assert sum(1 for kind, _, _, _ in s.edges if kind == "top_bit") >= 6
            if any(w * s.c <= sv.GLV_BITS[curve] - 1 and 128 < (w + 1) * s.c for w in range(s.W)):     # the top bit lies in that window
                assert any(kind == "straddle" for kind, _, _, _ in s.edges), s
            assert any(kind == "beyond" for kind, _, _, _ in s.edges) == (s.W * s.c > 128 + s.c - 1 or (s.W - 1) * s.c >= 128), s
        assert per_window <= {k for k, _ in kinds}
    assert checked > 1500
    # both curves reach a window behind limb 3 and a window across its end
    labels = {s.label: {kind for kind, _, _, _ in s.edges} for s in F.sections}
    assert "beyond" in labels["c16_glv1_W9"] and "straddle" in labels["c17_glv1_fullW" if curve == "secp256k1" else "c13_glv1"]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_run_families_are_complete(curve):
    F = sv.file(curve, "runs")
    by = {s.label: s for s in F.sections}
    assert list(by) == ["runs_glv0", "runs_glv1"] + ["stage_half%d_%+d" % (h, d) for h in (0, 1) for d in (-1, 0, 1)] + ["lanes"]
    # run lengths: partition 0 of tile t holds exactly L_t items of window 0, the tile's other items lie elsewhere
    for glv in (0, 1):
        s = by["runs_glv%d" % glv]
        Ls = sv.RUN_L + ([8192] if glv else [])
        assert [L for _, _, _, L in s.edges] == Ls and s.n == len(Ls) * sv.TILE
        rl = run_lengths(s)
        assert rl[:, 0].tolist() == Ls
        assert (rl.sum(axis=1) == s.plan["tile_cap"]).all()        # no window-0 digit is zero: every sub-scalar has its item
        assert s.plan["P"] >= 2 and s.plan["sort_half"] == glv
    # staging: (window 0, partition 0) receives exactly the staging area's size, one more, one less; the others are not empty
    for half in (0, 1):
        for d in (-1, 0, 1):
            s = by["stage_half%d_%+d" % (half, d)]
            cap = sv.STAGE_CAP // 2 if half else sv.STAGE_CAP
            assert s.stage_cap == cap and s.plan["sort_half"] == half and s.plan["lowbits"] == 10
            per_part = run_lengths(s).sum(axis=0)
            assert per_part[0] == cap + d == s.edges[0][3] and (per_part[1:] > 0).all()
            assert 5 <= s.plan["T_tiles"] <= 9
            assert (run_lengths(s, 1).sum(axis=0) < cap).all()     # window 1: staged blocks share `entries` with the unstaged one
    # lane sharing: a 64-item run made of k items of one bucket (and k of a second), strays in distinct buckets
    s = by["lanes"]
    assert [(k, two) for _, _, _, (k, two, _, _) in s.edges] == sv.LANE_COMPS * 2 and s.plan["T_tiles"] == 2 * len(sv.LANE_COMPS)
    assert [k for k, _ in sv.LANE_COMPS if k != 64] == [7, 7, 8, 8, 9, 9] and (64, 0) in sv.LANE_COMPS
    rl = run_lengths(s)
    m = s.model
    for _, t, _, (k, two, X, Y) in s.edges:
        assert rl[t, 0] == 64
        bk = m.bucket[0][t * sv.TILE:(t + 1) * sv.TILE]
        mult = np.bincount(bk[(bk & (s.plan["P"] - 1)) == 0], minlength=m.B)
        assert mult[X] == k and (mult[Y] == k if two else mult[Y] <= 1)
        assert sorted(mult[mult > 0].tolist(), reverse=True)[(2 if two else 1):] == [1] * (64 - (2 if two else 1) * k)
    front = [int(np.nonzero((m.bucket[0][t * sv.TILE:(t + 1) * sv.TILE] & (s.plan["P"] - 1)) == 0)[0][0]) for _, t, _, _ in s.edges]
    assert front == [0] * len(sv.LANE_COMPS) + [sv.TILE - 64] * len(sv.LANE_COMPS)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_tile_shape_and_fill_families_are_complete(curve):
    F = sv.file(curve, "tiles")
    by = {s.label: s for s in F.sections}
    assert [s.n for s in F.sections if s.family == "tiles"] == sv.TILE_N + [35 * 4096 - 5]
    big = by["n%d" % sv.BIG_N]
    assert big.plan["T_tiles"] == 35 > 32 and big.n % sv.TILE != 0         # tiles wv, wv + 16, wv + 32; the last one partial
    wgs = [s for s in F.sections if s.family == "wg"]
    assert [s.plan["wg"] for s in wgs] == [1, 2, 16, 5, 1, 5]
    assert all(s.scalars == wgs[0].scalars and s.plan["T_tiles"] == 2 for s in wgs[:4]) and wgs[0].W % 5 != 0
    assert wgs[4].scalars == wgs[5].scalars and wgs[4].glv == 1 and wgs[4].W % 5 != 0
    shapes = {s.label: s.plan for s in F.sections if s.family == "shapes"}
    assert shapes["P1"]["P"] == 1 and shapes["P1_c2"]["P"] == 1 and shapes["P128"]["P"] == 128 and shapes["P128_half"]["P"] == 128
    for label, lowbits, half in (("per4", 12, 0), ("per4_P16", 12, 0), ("per2", 11, 1), ("per2_P16", 11, 1)):
        assert (shapes[label]["lowbits"], shapes[label]["sort_half"]) == (lowbits, half)
    assert shapes["per4"]["P"] == 1 and shapes["per4_P16"]["P"] == 16 and shapes["per2_P16"]["P"] == 16
    assert {s.c for f in ("edges", "tiles") for s in sv.file(curve, f).sections} >= set(sv.SHAPE_C)
    # fill: the launch shape is the product's own
    F = sv.file(curve, "fill")
    assert all(s.forced == (None, None, None) for s in F.sections) and F.sections[0].n == (1 << 15) + 1 and F.sections[0].glv == 1
    assert F.sections[0].W == sv.full_W(curve, 1, sv.FILL_C_GLV)
    if curve == "secp256k1":
        s = F.sections[1]
        assert (s.n, s.glv, s.c, s.W) == (1 << 17, 0, 16, 17)
        top = s.model.digit[16]
        assert set(np.unique(top).tolist()) == {0, 1} and 0.3 < top.mean() < 0.7       # the 17th window: carries only, half of all scalars
    # scalar OR and points
    F = sv.file(curve, "or")
    assert [s.label for s in F.sections] == sv.OR_CASES and [s.n for s in F.sections[:4]] == [1, 255, 256, 257]
    by = {s.label: s for s in F.sections}
    assert by["stride"].n > 131072 + 256 and by["stride"].scalars[-1] == 1 << 255 and all(k < 1 << 64 for k in by["stride"].scalars[:-1])
    assert by["last_scalar"].scalars[-1] >> 200 and all(k < 1 << 64 for k in by["last_scalar"].scalars[:-1])
    high = [i for i, k in enumerate(by["lane63"].scalars) if k >> 64]
    assert len(high) == 1 and high[0] % 64 == 63
    C = ev.CURVES[curve]
    cases = sv.point_cases(curve)
    names = [name for name, _, _ in cases]
    for i in range(1, 9):
        x = ev.multiples(C)[i][0]
        assert sum(1 for nm in names if nm.startswith("%dG+" % i)) == (sv.M256 - x) // C.p + 1
    assert {"inf", "inf+p", "x0", "x=p-1", "small+p", "max"} <= set(names)
    assert all(0 <= x <= sv.M256 and 0 <= y <= sv.M256 for _, x, y in cases)
    assert len(sv.file(curve, "points").sections[0].points) > 256


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_model_is_self_consistent(curve):
    """every sub-scalar is rebuilt from its digits; the split satisfies k1 + lambda k2 = k (mod n); the array recode equals recode()"""
    C = ev.CURVES[curve]
    n, lam = lv.order(C), lv.lam(C)
    checked = 0
    for name in sv.FILE_NAMES:
        for s in sv.file(curve, name).sections:
            m = s.model
            step = 1 if s.n <= 7000 else s.n // 1500
            limbs = 4 if s.glv else 8
            for i in range(0, s.n, step):
                k = sv.reduce_order(curve, s.scalars[i])
                assert (s.scalars[i] - k) % n == 0 and (s.scalars[i] - k) // n <= sv.MAX_Q[curve]
                subs = m.subs[i * m.SUBS:(i + 1) * m.SUBS]
                signed = [-mag if neg else mag for mag, neg in subs]
                assert (signed[0] + (lam * signed[1] if s.glv else 0) - k) % n == 0, (s, i)
                for e, (mag, neg) in enumerate(subs):
                    assert mag < 1 << (sv.GLV_BITS[curve] if s.glv else 256)
                    dg, carry = sv.recode(mag, s.c, s.W, limbs)
                    assert [d for d, _, _ in dg] == m.digit[:, i * m.SUBS + e].tolist(), (s, i, e)
                    assert all(-(1 << (s.c - 1)) < d <= 1 << (s.c - 1) for d, _, _ in dg)
                    rebuilt = sum(d << (w * s.c) for w, (d, _, _) in enumerate(dg)) + (carry << (s.W * s.c))
                    assert rebuilt == mag & ((1 << (s.W * s.c)) - 1), (s, i, e)
                    if s.W == sv.full_W(curve, s.glv, s.c):       # the product's window count holds every sub-scalar: no carry leaves
                        assert carry == 0 and rebuilt == mag, (s, i, e)
                    checked += 1
    assert checked > 100000


# ================================================================ the launch shape, through --plan
PLAN_N = [1, 4096, 32769, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 21, 1 << 22]
FIELDS = ["n", "glv", "c", "W", "tile_cap", "T_tiles", "lowbits", "sort_half", "P", "wg"]


def plan_groups():
    return sorted({(n, glv, c, sv.full_W(curve, glv, c)) for curve in CURVE_NAMES for n in PLAN_N for glv in (0, 1) for c in range(2, 21)})


def test_plan_equals_the_recorded_inline_code():
    groups = plan_groups()
    assert len(groups) == 500
    with open(os.path.join(common.ROOT, "tests", "golden", "sort_front_plan.txt")) as f:
        rows = [dict(zip(FIELDS, map(int, line.split()))) for line in f if not line.startswith("#")]
    recorded = {(r["n"], r["glv"], r["c"], r["W"]): r for r in rows}
    assert sorted(recorded) == groups
    for g, got in zip(groups, sv.dump_plans(groups)):
        assert got == recorded[g], g
        assert got == sv.plan_model(*g), g
    # the rule for dropping to half: the widest half-size case and its neighbours, as the code before read
    by = lambda n, glv, c: recorded[(n, glv, c, sv.full_W("bn254", glv, c))]
    assert (by(1 << 20, 0, 16)["lowbits"], by(1 << 20, 0, 16)["sort_half"], by(1 << 20, 0, 16)["P"]) == (9, 1, 64)     # 64-item runs of a tile
    assert (by(1 << 21, 0, 16)["lowbits"], by(1 << 21, 0, 16)["sort_half"], by(1 << 22, 0, 17)["sort_half"]) == (10, 0, 0)    # 32-item runs: full size
    assert {r["sort_half"] for r in rows} == {0, 1} and {r["wg"] for r in rows} >= {1, 2, 4, 7, 16}
    assert by(1 << 20, 0, 16)["wg"] == 1 and by(1 << 18, 0, 16)["wg"] == 4 and by(1, 0, 2)["wg"] == 16 and by(1, 0, 20)["wg"] == 13


def test_plan_refusals():
    def refused(args, what):
        r = subprocess.run([sv.EXE, "--plan"] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr and r.stdout == "", (args, r.returncode, r.stderr)
    refused([0, 0, 16, 16], "header out of range")
    refused([4096, 2, 16, 16], "header out of range")
    refused([4096, 0, 1, 16], "shape out of range")
    refused([4096, 0, 21, 16], "shape out of range")
    refused([4096, 0, 16, 0], "shape out of range")
    refused([4096, 0, 16, "x"], "not a number")


def test_malformed_files_are_refused(tmp_path):
    """a shape outside the kernels' limits, a truncated file, words behind the last section: a message and status 1, before
    anything reaches the device (this test runs without one)"""
    s = sv.Section("bn254", "x", "x", list(range(1, 41)), 0, 13, 2, lowbits=10, sort_half=0, wg=2, points=[bytes(64)] * 3)
    good = s.words()
    assert int(good[0]) == sv.MAGIC and good.size == sv.HDR + 8 * 40 + 16 * 3

    def refused(words, what):
        fin = str(tmp_path / "in")
        words.tofile(fin)
        r = subprocess.run([sv.EXE, "bn254", fin, str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr and "HIP error" not in r.stderr, (what, r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / "out"))

    def with_(**kw):
        w = good.copy()
        for k, v in kw.items():
            w[{"magic": 0, "n": 1, "glv": 2, "c": 3, "W": 4, "lowbits": 5, "sort_half": 6, "wg": 7, "n_points": 8, "reserved": 9}[k]] = v
        return w
    refused(with_(magic=sv.MAGIC ^ 1), "not a sort_check file")
    refused(with_(c=1), "shape out of range")
    refused(with_(c=21), "shape out of range")
    refused(with_(W=0), "shape out of range")
    refused(with_(c=20, lowbits=12, W=5), "shape out of range")               # 5 * 2^19 buckets
    refused(with_(glv=2), "header out of range")
    refused(with_(n=0), "header out of range")
    refused(with_(n=(1 << 18) + 1), "header out of range")
    refused(with_(reserved=1), "header out of range")
    refused(with_(lowbits=13), "above c - 1")
    refused(with_(c=14, lowbits=13), "above the full sort's counters")
    refused(with_(lowbits=12, sort_half=1), "above the half sort's counters")
    refused(with_(lowbits=4), "more than 128 partitions")
    refused(with_(sort_half=2), "sort_half must be 0 or 1")
    refused(with_(wg=0), "wg 0 outside")
    refused(with_(wg=3), "wg 3 outside")                                       # W = 2
    refused(with_(wg=17, W=40), "wg 17 outside")
    refused(with_(n=41), "file ends inside")
    refused(with_(n_points=4), "file ends inside the points")
    refused(good[:-1], "file ends inside the points")
    refused(good[:sv.HDR + 17], "file ends inside the scalars")
    refused(np.concatenate([good, good[:5]]), "section 1: not a sort_check file")
    refused(good[:0], "not a sort_check file")

"""CPU: the models of tests/fb_vectors.py hold their own properties, the degenerate builders cover what they claim, the launch shapes
of fixed_base.hip.h (fb_check --plan, no device) equal tests/golden/fb_plan.txt -- generated from the formulas that stood inline in
FixedBase<C>::build, commit_device and commit_small before they moved into fb_table_plan, fb_commit_slices, fb_small_slices and
fb_finish_rows -- and the driver refuses a malformed file before it touches a device."""
import collections
import os

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests import fb_vectors as fv

CURVE_NAMES = ["bn254", "secp256k1"]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_constants(curve):
    C = ev.CURVES[curve]
    n = fv.order(C)
    assert fv.mul_g(C, n - 1) == ev.ec_neg(C, C.g) and fv.mul_g(C, n) is None and fv.mul_g(C, 5) == ev.multiples(C)[5]
    assert n.bit_length() == fv.SCALAR_BITS[curve]
    k = 0x1234567890abcdef1234567890abcdef1234567890abcdef
    assert fv.mul_g(C, k) == ev.ec_mul(C, k, C.g)
    pairs = [(ev.multiples(C)[a], ev.multiples(C)[b]) for a, b in ((1, 2), (3, 3), (0, 4), (5, 0), (7, 9))] + [(C.g, ev.ec_neg(C, C.g))]
    assert fv.ec_add_batch(C, pairs) == [ev.ec_add(C, a, b) for a, b in pairs]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_signed_digit_model(curve):
    """sum d_w 2^(cw) = k mod order, digits in [-(2^(c-1) - 1), 2^(c-1)], no carry out of window W - 1: every family, c = 2 .. 20"""
    C = ev.CURVES[curve]
    n = fv.order(C)
    total = 0
    for c in range(2, 21):
        fam = fv.families(curve, c)
        counts = collections.Counter(f for f, _ in fam)
        W, half = fv.windows(C, c), 1 << (c - 1)
        assert counts["edge"] == 4 and counts["half"] == 3 and counts["ripple"] == W and counts["random"] >= 1000
        assert counts["order"] == 3 * ((1 << 256) // n) and counts["win"] >= 2 * (W - 1)
        assert (counts["top"] > 0) == ((1 << (c * (W - 1))) < n)
        assert all(0 <= k < 1 << 256 for _, k in fam)
        for f, k in fam:
            d = fv.signed_digits(C, k, c)
            fv.check_signed_digits(C, k, c, d)
            if f == "top":
                assert all(x == 0 for x in d[:-1]) and d[-1] > 0
            total += 1
        allhalf = [k for f, k in fam if f == "half"][1]
        d = fv.signed_digits(C, allhalf, c)
        assert allhalf < n and all(x in (0, half) for x in d) and d[0] == half and sum(1 for x in d if x == half) >= W - 2
        # a ripple: 2^(cj) - 1 recodes to -1 in window 0 and +1 in window j
        for j in range(1, W):
            k = (1 << (c * j)) - 1
            if k < n:
                d = fv.signed_digits(C, k, c)
                assert d[0] == -1 and d[j] == 1 and not any(d[1:j]) and not any(d[j + 1:]), (c, j)
    assert total > 19 * 1000


def test_table_boundaries():
    for c in range(2, 21):
        ks, doubling = fv.boundaries(c)
        p = fv.table_plan(c, 1)
        H, lanes, K, runs = p["H"], p["lanes"], p["K"], p["runs"]
        assert lanes * K * runs == H and lanes * p["groups_per_wave"] == 64
        assert ks and ks[0] == 0 and ks[-1] == H - 1
        if K > 1:
            assert doubling == 2 * lanes - 1 and doubling in ks and lanes in ks and lanes - 1 in ks
        if runs > 1:
            assert lanes * K in ks and lanes * K - 1 in ks
    # the five lane-group geometries
    assert fv.table_plan(4, 1)["lanes"] == 1 and fv.table_plan(4, 1)["K"] == 8
    assert fv.table_plan(7, 1)["lanes"] == 4 and fv.table_plan(7, 1)["K"] == 16
    assert fv.table_plan(11, 1)["lanes"] == 64 and fv.table_plan(11, 1)["K"] == 16
    assert fv.table_plan(13, 1)["runs"] == 1 and fv.table_plan(14, 1)["runs"] == 2
    assert fv.table_plan(20, 13)["batch_pairs"] == 13 and fv.table_plan(20, 128 * 13)["batch_pairs"] == 16


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_commit_rows(curve):
    C = ev.CURVES[curve]
    rows, where = fv.commit_degenerate_rows(C)
    assert len(rows) == 300 and all(len(r) == len(fv.COMMIT_BASES) for r in rows)
    d = fv.signed_digits(C, rows[where["last_window"][0]][-1], fv.COMMIT_C)
    assert d[-1] == 1 and not any(d[:-1])
    for c in (2, 5, 8, 11, 13, 16, 20):
        bs = fv.recoder_bases(C, c)
        rws, fed = fv.recoder_rows(C, c)
        assert len(bs) * (fv.windows(C, c) << (c - 1)) <= fv.MAX_ENTRIES and len(set(bs)) == len(bs)
        chosen = [k for f, k in fv.families(curve, c) if f != "random"]
        for j in range(len(bs)):                                    # every chosen member at every coefficient position
            assert collections.Counter(r[j] for r in rws[:len(chosen)]) == collections.Counter(chosen)
        assert {k for f, k in fv.families(curve, c) if f == "random"} <= {k for r in rws[len(chosen):] for k in r}


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_small_degenerate_coverage(curve):
    """every LDS level and every slice-fold step has its equal and its opposite pair"""
    C = ev.CURVES[curve]
    bs, rows, labels = fv.small_degenerate(curve)
    assert len(rows) == fv.SMALL_MAX_ROWS and len(bs) == fv.SMALL_COEFFS
    for (label, kind), coeffs in zip(labels, rows):
        if kind is None:
            continue
        SL = {"lds": 1, "slice2": 2, "slice3": 3}[label[0]]
        total, slices, meetings = fv.small_model(C, fv.SMALL_C, bs, coeffs, SL)
        key = ("lds" if label[0] == "lds" else "slice", label[1], kind)
        assert meetings == [key], (label, kind, meetings)
        assert (total == 0) == (kind == "opp")
    assert sum(1 for l, k in labels if l[0] == "lds") == 16
    total, slices, meetings = fv.small_model(C, fv.SMALL_C, bs, rows[labels.index(("zero", None))], 3)
    assert total == 0 and slices == [0, 0, 0] and not meetings


def test_fold_rows_coverage():
    for S in (2, 4, 8, 16, 32, 64, 128):
        rows = fv.fold_layout(S)
        per_block = 128 // S
        assert per_block == 1 or len(rows) % per_block != 0
        assert isinstance(rows[-1][0], tuple)
        want = {(n, kind) for n in [S >> k for k in range(1, S.bit_length())] for kind in ("eq", "opp")}
        have = set()
        for label, a in rows:
            assert len(a) == S and all(abs(m) < 8192 for m in a)
            total, meetings = fv.fold_model(a, S)
            assert total == sum(a)
            if isinstance(label, tuple):
                assert label in meetings and a[label[1]] != 0 and a[label[1] + label[0]] != 0
                have.add((label[0], label[2]))
        assert have == want, S


def test_finish_rows():
    for R in (1, 2, 4):
        a = fv.finish_rows(R, 64 * R + 37)
        lanes = [[a[t + 64 * k] for k in range(R)] for t in range(64)]
        assert {tuple(i for i, v in enumerate(l) if v == 0) for l in lanes[:16]} == {(k,) for k in range(R)}
        assert not any(lanes[20]) and all(all(l) for l in lanes[21:])
        assert fv.finish_rows(R, 1) == [1]


# ================================================================ the launch shapes
def test_plan_equals_the_golden_file():
    assert os.path.exists(fv.EXE), "build it with make -C porla_amd/csrc"
    text = fv.dump_plan()
    assert text == open(fv.GOLDEN_PLAN).read()
    lines = text.splitlines()
    assert sum(1 for l in lines if l.startswith("table ")) == 2 * 19
    assert sum(1 for l in lines if l.startswith("commit ")) == 2 * len(fv.PLAN_COMMIT)
    assert sum(1 for l in lines if l.startswith("finish ")) == 2 * len(fv.PLAN_ROWS)
    # the restated table shapes say the same
    for l in lines:
        if l.startswith("table "):
            f = dict(kv.split("=") for kv in l.split()[1:])
            p = fv.table_plan(int(f["c"]), int(f["pairs"]))
            assert all(int(f[k]) == v for k, v in p.items()), l


# ================================================================ the driver's validation (no device is touched: it comes first)
def refused(words, what):
    r, out = fv.run_file("bn254", words, timeout=60)
    assert r.returncode == 1 and what in r.stderr and r.stdout == "", (r.returncode, r.stderr)


def test_driver_refuses_malformed_files():
    C = ev.BN254
    good = fv.table_section(C, 5, [C.g]).words
    bad_c = good.copy()
    bad_c[2] = 21
    refused(bad_c, "c = 21")
    refused(good[:-3], "file ends inside")
    refused(good[:7], "not an fb_check file")
    bad_magic = good.copy()
    bad_magic[0] ^= 1
    refused(bad_magic, "not an fb_check file")
    part = np.zeros((3 * 4, 32), dtype=np.uint32)
    fold3 = fv.fold_section(5, part, 4).words
    fold3[5] = 3
    refused(fold3, "S = 3")
    refused(np.concatenate([fv.header(fv.OP_FOLD, 5, n_rows=1, S=256), np.zeros(256 * 32, dtype=np.uint32)]), "S = 256")
    rows = [[1, 2]] * 3
    refused(fv.commit_section(5, rows, 1).words, "no resident table")
    two = fv.table_section(C, 5, [C.g, C.g]).words
    refused(np.concatenate([two, fv.commit_section(5, [[1, 2, 3]], 1).words]), "n_coeffs 3")
    refused(np.concatenate([two, fv.header(fv.OP_SMALL, 5, n=2, n_rows=1, S=9, row_stride=64), np.zeros(16, dtype=np.uint32)]), "SL = 9")
    refused(np.concatenate([two, fv.header(fv.OP_SMALL, 5, n=2, n_rows=65, S=1, row_stride=64), np.zeros(65 * 16, dtype=np.uint32)]), "n_rows = 65")
    refused(np.concatenate([fv.header(fv.OP_TABLE, 20, n=2), np.zeros(32, dtype=np.uint32)]), "more than 2^23")
    refused(np.concatenate([fv.header(fv.OP_TABLE, 5, n=1, flag=1), np.zeros(16, dtype=np.uint32), np.array([1 << 20], dtype=np.uint32)]), "outside the table")
    # a bad section BEHIND a good one: nothing is launched either (validation covers the whole file first)
    refused(np.concatenate([good, bad_c]), "c = 21")
    refused(np.concatenate([fv.header(fv.OP_FINISH, 5, n_rows=1, S=1, flag=3), np.zeros(32, dtype=np.uint32)]), "3 rows per lane")

"""CPU: the vectors of tests/small_vectors.py against themselves -- the model the GPU test of the single-launch MSM's block body
(tests/test_small_block_gpu.py) trusts.  For every section: the blocks' sums, weighted as the host fold weighs them, add up to
sum k_i m_i mod the order; the slices partition the scalars; the shape is the one the library's own shape function reports; and every
family contains what it claims -- the raw digit values at the carry threshold, the top windows of every width, equal and opposite
sums meeting at the stated level of the tree and of the slice fold (counted, as fb_vectors.small_model counts them).  No device."""
import random

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests import fb_vectors as fv
from tests import small_vectors as sv

CURVE_NAMES = ["bn254", "secp256k1"]


def all_sections(name):
    secs = list(sv.capacity(name))
    for fam in (sv.digits(name), sv.accumulate(name), sv.pairs(name)):
        secs += list(fam.values())
    return secs


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_endomorphism_of_the_model_is_multiplication_by_lambda(curve):
    C = ev.CURVES[curve]
    n, l = sv.order(C), sv.lam(C)
    assert (l * l + l + 1) % n == 0
    for m in (1, 2, sv.pool(curve)[100]):
        pt = fv.mul_g(C, m)
        assert ev.on_curve(C, pt) and sv.phi(C, pt) == fv.mul_g(C, l * m)
    assert sv.lin_point(C, 5, -3) == fv.mul_g(C, 5 - 3 * l) and sv.lin_point(C, 0, 0) is None and sv.lin_point(C, -7, 0) == ev.ec_neg(C, fv.mul_g(C, 7))
    assert len(set(sv.pool(curve))) == len(sv.pool(curve)) <= 512


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_every_section_sums_to_its_msm_and_its_slices_partition_the_scalars(curve):
    C = ev.CURVES[curve]
    secs = all_sections(curve)
    checked = 0
    for s in secs:
        m = sv.model(s)
        assert m.fits and m.W * m.S <= s.blocks, s.name
        assert m.bounds[0][0] == 0 and m.bounds[-1][1] == s.n and all(a[1] == b[0] for a, b in zip(m.bounds, m.bounds[1:])), s.name
        assert all(0 <= i1 - i0 and (i1 - i0) * m.subs <= sv.SMALL_MAX_SUB for i0, i1 in m.bounds), s.name
        for st in range(s.sets):
            assert sv.launch_value(C, m, st) == sv.msm_value(s, st), s.name
            # fin is the sum over the slices, and the sums beyond a window's own width are infinity
            assert (m.fin[st] == m.sums[st].reshape(m.W, m.S, sv.SMALL_MAX_C, 2).sum(axis=1)).all()
            assert not m.sums[st, (m.W - 1) * m.S:, m.top:].any() and not m.sums[st, :, m.c:].any(), s.name
        checked += 1
    assert checked == len(secs) >= 130


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_the_model_shape_is_the_exported_shape(curve):
    from porla_amd import multiexp as mx
    secs = all_sections(curve) + (sv.refusal(curve) if curve == "secp256k1" else [])
    eff = [s.hint if s.hint else s.used_bits for s in secs]
    # the driver passes the section's own block count: lone sections carry the lone call's, pairs the pair's
    form = [sv.LONE if s.sets == 1 else (sv.HINT if s.hint else sv.PAIR) for s in secs]
    out = mx.msm_small_shape([sv.CURVE_ID[curve]] * len(secs), [s.n for s in secs], eff, [s.c_flags for s in secs], form)
    for s, o in zip(secs, out):
        m = sv.model(s)
        assert list(o) == [int(m.fits), s.blocks, m.glv, m.c, m.W, m.S], s.name
        assert m.fits == (not s.refusal)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_capacity_sections_fill_a_slice_to_the_last_index(curve):
    got = {s.name: sv.model(s) for s in sv.capacity(curve)}
    full = [name for name, m in got.items() if max(i1 - i0 for i0, i1 in m.bounds) * m.subs == sv.SMALL_MAX_SUB]
    if curve == "bn254":
        assert full == ["pair 32768"]
    else:
        assert full == ["pair 28672 split on", "pair 24576 split off"] and "lone 32768" in got
    for s in sv.capacity(curve):
        assert s.used_bits == 256
        m = got[s.name]
        # the last entry of a full slice has a non-zero digit in some window: local index 8 191 is really used
        i_last = m.bounds[0][1] - 1
        assert m.digits[m.sid[i_last], m.subs - 1].any()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_digit_families_contain_what_they_claim(curve):
    C = ev.CURVES[curve]
    d = sv.digits(curve)
    n = sv.order(C)
    tops = set()
    for c in range(1, sv.SMALL_MAX_C + 1):
        s = d[("threshold", c)]
        m = sv.model(s)
        assert (m.c, m.glv, m.L, m.reduce) == (c, 0, sv.DIGIT_L, False), s.name
        B = 1 << (c - 1)
        full = sv.DIGIT_L // c                              # windows that lie wholly inside the scalar
        at = {k: j for j, k in enumerate(sorted(set(s.scalars)))}
        x0, x1 = sv.threshold_scalars(c, sv.DIGIT_L)
        assert (m.raws[at[x0], 0, :full] == B).all() and (m.digits[at[x0], 0, :full] == B).all()
        if c >= 2:                                          # (a one-bit window never carries: its raw value is at most 1 = B)
            assert (m.raws[at[x1], 0, :full] == B + 1).all() and (m.digits[at[x1], 0, :full] == B + 1 - (1 << c)).all()
            assert m.raws[at[x1], 0, full] >= 1             # the carry out of the last full window arrives
        s = d[("full", c)]
        m = sv.model(s)
        assert m.reduce and m.glv and m.L == sv.GLV_BITS[sv.CURVE_ID[curve]] and {0, n - 1, n, (1 << 256) - 1} <= set(s.scalars)
        assert m.c == (c if (m.L + c) // c <= s.blocks else sv.SMALL_MAX_C)
        for top in range(1, c + 1):
            m = sv.model(d[("top", c, top)])
            assert (m.c, m.top) == (c, top)
            assert m.raws[:, 0, -1].max() == (1 << (top - 1) if c >= 2 else 0)      # the widest top digit: all ones plus a carry
            tops.add((c, top))
    assert len(tops) == 36
    for bits in (128, 129, 249, 250):
        for flags in (0, 5, sv.NO_SPLIT, sv.NO_SPLIT | 5):
            s = d[("length", bits, flags)]
            m = sv.model(s)
            assert s.used_bits == bits and m.glv == (bits > 128 and not flags & sv.NO_SPLIT) and m.reduce == (bits >= 250)
            if flags & 0xff:
                assert m.c == 5
    m = sv.model(d[("w_is_blocks",)])
    assert m.W == d[("w_is_blocks",)].blocks == 192 and m.S == 1 and m.c == 1
    assert any(sv.model(s).W * sv.model(s).S < s.blocks for s in list(d.values())[:8])


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_accumulate_families_contain_what_they_claim(curve):
    C = ev.CURVES[curve]
    a = sv.accumulate(curve)
    for c in (4, 8):
        s = a[("one_bucket", c)]
        m = sv.model(s, keep_buckets=True)
        assert len(set(s.scalars)) == 1
        for bx in range(m.W * m.S):
            assert (m.buckets[(0, bx)] != 0).any(axis=1).sum() <= 1          # at most one bucket of a block holds anything
    s = a[("infinity",)]
    assert s.ms[0].count(0) >= 60 and s.ms[0][0] == s.ms[0][-1] == 0
    assert (len(s.lifts) >= 8) == (curve == "bn254")      # secp256k1's p leaves no room for x + p in 32 bytes
    # 3a: every window's one bucket holds 2 T equal entries: every lane sums to the same 2 P, equal operands at every level
    s = a[("lane", "eq")]
    m = sv.model(s)
    assert (m.c, m.S, m.W) == (1, 1, 128) and sv.lane_fold_levels(1) == [1, 2, 4, 8, 16, 32, 64, 128]
    assert (m.digits[0, 0, :127] == 1).all() and s.n == 2 * sv.SMALL_THREADS and len(set(s.ms[0])) == 1
    assert (m.sums[0, :127, 0, 0] == s.n * s.ms[0][0]).all()
    # P and -P at level k, for every order the sort can leave the entries in: one negative entry, the others positive, total zero, one
    # entry per lane -- so the two operands of level k are the two half sums X > 0 and -X, and no smaller group of lanes cancels
    rng = random.Random(0x1A7E)
    for k in range(1, 9):
        s = a[("lane", "opp", k)]
        m = sv.model(s)
        ms = s.ms[0]
        assert (m.c, m.S, m.W) == (1, 1, 128) and s.n == 1 << k <= sv.SMALL_THREADS and (m.digits[0, 0, :127] == 1).all()
        assert sum(ms) == 0 and sum(1 for x in ms if x < 0) == 1 and all(ms) and not m.sums.any()
        for trial in range(64):
            order_ = list(ms) if trial == 0 else rng.sample(ms, len(ms))
            if trial == 1:
                order_ = list(reversed(ms))
            lanes = order_ + [0] * (sv.SMALL_THREADS - len(ms))
            opp = [h for h, kind in sv.lane_fold_meetings(C, lanes) if kind == "opp"]
            assert opp == [1 << (k - 1)], (k, trial, opp)
    assert not sv.model(a[("lane", "cancel")]).sums.any()
    # 3b: the stated meeting at the stated level of the full 128-bucket tree
    for l in range(7):
        for kind in ("eq", "opp"):
            for slot in ("S", "M"):
                if slot == "M" and l == 0:
                    continue
                m = sv.model(a[("tree", slot, l, kind)], keep_buckets=True)
                assert (m.c, m.W, m.S, m.top) == (8, 2, 1, 1)
                assert (slot, l, kind) in sv.tree_meetings(C, m, 0, 0), (slot, l, kind)
    # 4: the stated meeting at the stated step of the slice fold, at every ragged S
    for S, (c, L, q) in sv.SLICE_SHAPES.items():
        assert sv.fold_steps(S) == {3: 2, 5: 3, 7: 3, 32: 5}[S]
        for step in range(sv.fold_steps(S)):
            for kind in ("eq", "opp"):
                m = sv.model(a[("slice", S, step, kind)])
                assert (m.S, m.c) == (S, c)
                hits = [w for w in range(m.W) if (step, kind) in sv.slice_meetings(C, m, 0, w)]
                assert len(hits) >= m.W // 2, (S, step, kind)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_pair_families_contain_what_they_claim(curve):
    C = ev.CURVES[curve]
    p = sv.pairs(curve)
    assert all(s.sets == 2 and s.blocks == 96 for s in p.values())
    s = p[("infinity",)]
    assert sv.msm_value(s, 1) == 0 and sv.msm_value(s, 0) != 0
    m = sv.model(s)
    assert not m.fin[1].any() and m.sums[1].any()          # set b: blocks with sums of their own that cancel across the slices
    assert p[("three",)].launches == 3 and p[("audit",)].hint == 32 and sv.model(p[("audit",)]).glv == 0

"""GPU: the single-launch MSM block by block -- k_small_msm, the product's own kernel, launched by the driver tools/small_check.hip in
the product's launch shapes on scalars and points the test chose.  Expected values: Python integers (tests/small_vectors.py, which
tests/test_small_vectors_cpu.py checks against itself; the group law of tests/ec_vectors.py).  Comparison is exact: every block's c
sums (S, M_0 .. M_(c-2)) decoded with their form and value bounds and compared as group elements, folded with the window's weights
against the digits' own sum, fin[w] against the sum over the slices, the header against the library's shape export, every counter
zero after every launch, and every word no block owns still the sentinel.  No record is skipped (checked == generated).

One driver process per curve and pytest session; a driver run that failed is never repeated and nothing more starts on the device."""
import functools
import os
import time

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests import fb_vectors as fv
from tests import small_vectors as sv

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "secp256k1"]
FAMILIES = {"capacity": lambda name: {(s.name,): s for s in sv.capacity(name)},
            "refusal": lambda name: {(s.name,): s for s in sv.refusal(name)} if name == "secp256k1" else {},
            "digits": sv.digits, "accumulate": sv.accumulate, "pairs": sv.pairs}
DRIVER_FAILED = []                       # a driver run that failed is never repeated, for either curve: nothing more starts on the device


def test_driver_is_built():
    assert os.path.exists(sv.EXE), "build it with make -C porla_amd/csrc"


@functools.lru_cache(maxsize=None)
def session(curve):
    """{(family, label): (Section, [Launch])}: every section of every family, one driver process"""
    C = ev.CURVES[curve]
    if DRIVER_FAILED:
        pytest.fail("not run: the driver failed before (%s)" % DRIVER_FAILED[0])
    t0 = time.time()
    keys, secs = [], []
    for fam, make in FAMILIES.items():
        for label, s in make(curve).items():
            keys.append((fam, label))
            secs.append(s)
    t1 = time.time()
    try:
        outs = sv.run(C, secs)
    except BaseException as e:
        DRIVER_FAILED.append("%s: %s" % (curve, str(e)[:300]))
        raise
    print("small_check session %s: %d sections, %.1f s to build the inputs, %.1f s in the driver" % (curve, len(secs), t1 - t0, time.time() - t1))
    return {k: (s, o) for k, s, o in zip(keys, secs, outs)}


def family(curve, fam):
    got = {k[1]: v for k, v in session(curve).items() if k[0] == fam}
    assert len(got) == len(FAMILIES[fam](curve))
    return got


def exported_shape(sec):
    """(single launch, blocks, glv, c, W, S) of the library's shape export for this section"""
    from porla_amd import multiexp as mx
    form = sv.LONE if sec.sets == 1 else (sv.HINT if sec.hint else sv.PAIR)
    return [int(v) for v in mx.msm_small_shape([sv.CURVE_ID[sec.C.name]], [sec.n], [sec.hint if sec.hint else sec.used_bits], [sec.c_flags], [form])[0]]


def all_sentinel(words):
    return bool((np.asarray(words) == sv.SENTINEL).all())


def fold_window(C, pts):
    """S + sum_j 2^j M_j of one block's decoded sums"""
    acc = None
    for pt in reversed(pts[1:]):
        acc = ev.ec_add(C, ev.ec_add(C, acc, acc), pt)
    return ev.ec_add(C, pts[0], acc)


def check_launch(sec, m, L, seq, counter):
    """one launch of a section that fits: every area against the model"""
    C = sec.C
    where = "%s %s" % (C.name, sec.name)
    fits, blocks, glv, c, W, S = exported_shape(sec)
    assert fits == 1 and blocks == sec.blocks and (glv, c, W, S) == (m.glv, m.c, m.W, m.S), where
    ms = [np.array(x, dtype=np.int64) for x in sec.ms]
    for st in range(sec.sets):
        # the header is (seq, W, c, glv) and nothing else; set b's lies one region further on
        assert [int(x) for x in L.hdr[st, :4]] == [seq, W, c, glv], "%s set %d: header %s" % (where, st, L.hdr[st, :4])
        assert all_sentinel(L.hdr[st, 4:]), where + ": header words 4 .. 31"
        for bx in range(sec.blocks):
            blk = L.part[st, bx]
            if bx >= W * S:
                assert all_sentinel(blk), "%s set %d: idle block %d wrote" % (where, st, bx)
                continue
            assert all_sentinel(blk[c:]), "%s set %d block %d: entries beyond its c sums" % (where, st, bx)
            w, s = bx // S, bx % S
            got = []
            for k in range(c):
                a, b = (int(v) for v in m.sums[st, bx, k])
                pt = fv.decode_mem(C, blk[k], "%s set %d block %d (window %d slice %d) sum %d" % (where, st, bx, w, s, k))
                assert pt == sv.lin_point(C, a, b), "%s set %d block %d (window %d slice %d) sum %d" % (where, st, bx, w, s, k)
                got.append(pt)
                counter.checked += 1
            # folded with one window's weights: sum over the slice of digit_w(k_i) m_i G, from the digits themselves
            i0, i1 = m.bounds[s]
            ab = [int((m.digits[m.sid[i0:i1], e, w] * ms[st][i0:i1]).sum()) for e in range(m.subs)] + [0]
            assert fold_window(C, got) == sv.lin_point(C, ab[0], ab[1]), "%s set %d block %d: folded sums" % (where, st, bx)
        for w in range(W):
            for k in range(c):
                a, b = (int(v) for v in m.fin[st, w, k])
                at = (w * c + k) * 32
                pt = fv.decode_mem(C, L.fin[st, at:at + 32], "%s set %d fin window %d sum %d" % (where, st, w, k), final=True)
                assert pt == sv.lin_point(C, a, b), "%s set %d fin window %d sum %d" % (where, st, w, k)
                counter.checked += 1
        assert all_sentinel(L.fin[st, W * c * 32:]), "%s set %d: words behind fin" % (where, st)
    assert not L.counters.any(), "%s: counters %s" % (where, np.nonzero(L.counters)[0][:8])
    assert all_sentinel(L.part_tail) and all_sentinel(L.pin_tail), where + ": the sentinel areas behind part and fin"
    return sec.sets * (W * S * c + W * c)


def check_family(curve, fam, labels=None):
    got = family(curve, fam)
    counter, generated = ev.Counter(), 0
    for label, (sec, launches) in got.items():
        if labels is not None and not labels(label):
            continue
        m = sv.model(sec)
        assert m.fits and len(launches) == sec.launches
        for l, L in enumerate(launches):
            generated += check_launch(sec, m, L, sec.seq + l, counter)
    assert counter.checked == generated > 0
    return counter.checked


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_capacity_a_slice_of_exactly_8192(curve):
    """BN254 pair of 32 768 full scalars; secp256k1 pair of 28 672 with the split, of 24 576 without, lone 32 768: local index 8 191
    beside the sign bit, the last word of ent[] and raw[]"""
    n = check_family(curve, "capacity")
    print("capacity %s: %d sums" % (curve, n))


def test_refusal_of_an_unfit_shape_writes_nothing():
    """secp256k1, 32 768 pairs of full scalars on 128 blocks per set: slices of 9 363 sub-scalars.  The kernel's admit refuses: every
    output area keeps its sentinel, the counters stay zero, no header is published (word 0 stays as the host cleared it)"""
    (sec, (L,)), = family("secp256k1", "refusal").values()
    m = sv.model(sec)
    assert not m.fits and (m.c, m.W, m.S) == (8, 17, 7) and exported_shape(sec)[0] == 0
    assert all_sentinel(L.part) and all_sentinel(L.part_tail) and all_sentinel(L.pin_tail)
    assert not L.counters.any()
    for st in range(2):
        assert int(L.hdr[st, 0]) == 0 and all_sentinel(L.hdr[st, 1:]) and all_sentinel(L.fin[st])


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("c", range(1, sv.SMALL_MAX_C + 1))
def test_digits_every_width(c, curve):
    """n = 300, window width c: raw digit values exactly B and B + 1 in every window and a scalar whose every window carries; 0,
    order - 1, order, 2^256 - 1; a top window of every width 1 .. c"""
    n = check_family(curve, "digits", lambda label: label[0] in ("threshold", "full", "top") and label[1] == c)
    print("digits %s c=%d: %d sums" % (curve, c, n))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_digits_length_thresholds_and_w_equal_blocks(curve):
    """scalar lengths 128 / 129 (split) and 249 / 250 (reduction), split on and off, automatic and forced width; W == blocks"""
    n = check_family(curve, "digits", lambda label: label[0] in ("length", "w_is_blocks"))
    print("lengths %s: %d sums" % (curve, n))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_accumulate_one_bucket_infinity_and_lane_fold(curve):
    """every entry in one bucket; infinity points and coordinates >= p; P and P, and P and -P, at every one of the 8 levels of the
    lane fold (the opposite pair of level k: 2^k entries whose two half sums are X and -X in whatever order the sort leaves them)"""
    n = check_family(curve, "accumulate", lambda label: label[0] in ("one_bucket", "infinity", "lane"))
    print("accumulate %s: %d sums" % (curve, n))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_tree_equal_and_opposite_at_every_level(curve):
    """P and P, P and -P meeting at every S level and in every new M slot of the 128-bucket tree (step 3b)"""
    n = check_family(curve, "accumulate", lambda label: label[0] == "tree")
    print("tree %s: %d sums" % (curve, n))


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("S", sorted(sv.SLICE_SHAPES))
def test_slice_fold_ragged(S, curve):
    """S = 3, 5, 7, 32 slices (half = (cnt + 1) / 2): equal and opposite slice sums at every step of the last block's fold"""
    n = check_family(curve, "accumulate", lambda label: label[0] == "slice" and label[1] == S)
    print("slice fold %s S=%d: %d sums" % (curve, S, n))


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_pair_form(curve):
    """set b's part offset, counters + 256 and result region; the audit's hint of 32 bits; one set summing to infinity; three launches
    in a row on one workspace (the counters reset themselves, the sequence number moves on)"""
    n = check_family(curve, "pairs")
    sec, launches = family(curve, "pairs")[("infinity",)]
    m = sv.model(sec)
    assert not launches[0].fin[1, :m.W * m.c * 32].any()          # every window sum of set b is the all-zero infinity
    sec, launches = family(curve, "pairs")[("three",)]
    assert [int(L.hdr[0, 0]) for L in launches] == [5, 6, 7] and [int(L.hdr[1, 0]) for L in launches] == [5, 6, 7]
    print("pair %s: %d sums" % (curve, n))

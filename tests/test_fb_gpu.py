"""GPU: the fixed-base commitment stage by stage -- table construction, both signed-digit recoders through both commit kernels, the
degenerate accumulations and folds, k_fb_fold_quad at every S and k_fb_finish at every width -- through the driver
tools/fb_check.hip, which launches fixed_base.hip.h's own kernels in the product's launch shapes on inputs the test chose.
Expected values: Python integers (tests/fb_vectors.py, the group law of tests/ec_vectors.py).  Comparison is exact: table entries
and output bytes word for word, projective results as group elements with their form and value bounds; areas no kernel owns keep
the sentinel.  No record is skipped (checked == generated)."""
import collections
import functools
import os
import random
import time

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests import fb_vectors as fv

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "secp256k1"]
FULL_C = list(range(2, 11))
BIG_C = [11, 12, 13, 14, 17, 20]
RECODER_C = [2, 5, 8, 11, 13, 16, 20]
COMMIT_S = [1, 2, 8]
SMALL_SL = [1, 3, 8]
FOLD_S = [2, 4, 8, 16, 32, 64, 128]
TABLE_BASE = [1, None, 7]                # G, infinity, 7 G
BIG_BASE = 0xB5
SAMPLE = 4096


def test_driver_is_built():
    assert os.path.exists(fv.EXE), "build it with make -C porla_amd/csrc"


# ================================================================ one driver process per curve
JOBS = {}                                # name -> function(C) -> ([Section], what the check needs)


def job(name):
    def register(fn):
        JOBS[name] = fn
        return fn
    return register


DRIVER_FAILED = []                       # a driver run that failed is never repeated, for either curve: nothing more starts on the device


@functools.lru_cache(maxsize=None)
def session(curve):
    """{job name: ([output words of each section], what the check needs)}"""
    C = ev.CURVES[curve]
    if DRIVER_FAILED:
        pytest.fail("not run: the driver failed before (%s)" % DRIVER_FAILED[0])
    t0 = time.time()
    built = {n: fn(C) for n, fn in JOBS.items()}
    t1 = time.time()
    flat = [s for n in JOBS for s in built[n][0]]
    try:
        outs = fv.run(C, flat)
    except BaseException as e:
        DRIVER_FAILED.append("%s: %s" % (curve, str(e)[:300]))
        raise
    print("fb_check session %s: %d sections, %.1f s to build the inputs, %.1f s in the driver" % (curve, len(flat), t1 - t0, time.time() - t1))
    res, at = {}, 0
    for n in JOBS:
        k = len(built[n][0])
        res[n] = (outs[at:at + k], built[n][1])
        at += k
    return res


def one_entry():
    return [0]                           # (a table section that is only built for the sections behind it returns one entry)


# ================================================================ table
def full_table_job(c, C):
    return [fv.table_section(C, c, [fv.point(C, b) for b in TABLE_BASE])], None


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("c", FULL_C)
def test_table_every_entry(c, curve):
    """base G, infinity, 7 G: every entry (i, w, k) = (k + 1) 2^(cw) G_i in the stored form; the infinity point's are all-zero"""
    C = ev.CURVES[curve]
    (out,), _ = session(curve)["table_full_c%d" % c]
    W, H = fv.windows(C, c), 1 << (c - 1)
    tab = out.reshape(len(TABLE_BASE), W, H, 16)
    checked = 0
    for i, b in enumerate(TABLE_BASE):
        want = fv.expected_entries(C, c, b, {w: range(H) for w in range(W)})
        for w in range(W):
            exp = np.stack([fv.entry_words(C, pt) for pt in want[w]])
            bad = np.nonzero((tab[i, w] != exp).any(axis=1))[0]
            assert len(bad) == 0, "%s c=%d point %d window %d: entries %s differ" % (curve, c, i, w, bad[:8])
            assert b is not None or not tab[i, w].any()
            checked += H
    print("table %s c=%d: %d entries (plan %s)" % (curve, c, checked, fv.table_plan(c, len(TABLE_BASE) * W)))
    assert checked == len(TABLE_BASE) * W * H == tab.shape[0] * tab.shape[1] * tab.shape[2]


def big_table_indices(C, c):
    """[(w, k)]: every structural boundary of every pair, then a seeded sample"""
    W, H = fv.windows(C, c), 1 << (c - 1)
    ks, doubling = fv.boundaries(c)
    want = [(w, k) for w in range(W) for k in ks]
    rng = random.Random(0x7AB1E + c)
    want += [(rng.randrange(W), rng.randrange(H)) for _ in range(SAMPLE)]
    return want, len(ks), doubling


def big_table_job(c, C):
    want, _, _ = big_table_indices(C, c)
    H = 1 << (c - 1)
    return [fv.table_section(C, c, [fv.point(C, BIG_BASE)], idx=[w * H + k for w, k in want])], None


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("c", BIG_C)
def test_table_boundaries_and_sample(c, curve):
    """one finite base point: the entries at every structural boundary of every pair (first and last entry of each lane-group run, both
    sides of each k * lanes stride, the in-group doubling entry) and a seeded sample of 4096 entries"""
    C = ev.CURVES[curve]
    (out,), _ = session(curve)["table_big_c%d" % c]
    want, n_bound, doubling = big_table_indices(C, c)
    assert n_bound > 0 and doubling is not None and any(k == doubling for _, k in want)
    got = out.reshape(len(want), 16)
    by_w = collections.defaultdict(list)
    for at, (w, k) in enumerate(want):
        by_w[w].append((at, k))
    exp_pts = fv.expected_entries(C, c, BIG_BASE, {w: [k for _, k in lst] for w, lst in by_w.items()})
    checked = 0
    for w, lst in by_w.items():
        for (at, k), pt in zip(lst, exp_pts[w]):
            assert (got[at] == fv.entry_words(C, pt)).all(), "%s c=%d window %d entry %d" % (curve, c, w, k)
            checked += 1
    print("table %s c=%d: %d boundary entries per pair x %d pairs + %d sampled (plan %s)"
          % (curve, c, n_bound, fv.windows(C, c), SAMPLE, fv.table_plan(c, fv.windows(C, c))))
    assert checked == len(want) == n_bound * fv.windows(C, c) + SAMPLE


BATCH_C, BATCH_PAIRS = 5, 64


@job("table_batched")
def batched_job(C):
    pts = [fv.point(C, b) for b in TABLE_BASE]
    budget = BATCH_PAIRS * (1 << (BATCH_C - 1)) * fv.XYZZ_BYTES
    return [fv.table_section(C, BATCH_C, pts), fv.table_section(C, BATCH_C, pts, budget=budget)], budget


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_table_in_scratch_batches(curve):
    """the scratch budget lowered to 64 pairs per batch: three batches, the last one ragged, the same bits as the one-batch table"""
    C = ev.CURVES[curve]
    (one, many), budget = session(curve)["table_batched"]
    pairs = len(TABLE_BASE) * fv.windows(C, BATCH_C)
    plan = fv.table_plan(BATCH_C, pairs, budget)
    batches = -(-pairs // plan["batch_pairs"])
    assert batches >= 3 and pairs % plan["batch_pairs"] != 0 and fv.table_plan(BATCH_C, pairs)["batch_pairs"] == pairs
    assert one.shape == many.shape and (one == many).all()
    assert (one != fv.SENTINEL).any()
    print("table %s c=%d: %d entries in %d batches of %d pairs (last %d) = the one-batch table"
          % (curve, BATCH_C, len(one) // 16, batches, plan["batch_pairs"], pairs % plan["batch_pairs"]))


for _c in FULL_C:
    JOBS["table_full_c%d" % _c] = functools.partial(full_table_job, _c)
for _c in BIG_C:
    JOBS["table_big_c%d" % _c] = functools.partial(big_table_job, _c)


# ================================================================ recoders through both commit kernels
def chunks(rows, n):
    return [rows[at:at + n] for at in range(0, len(rows), n)]


def recoder_job(c, C):
    bs = fv.recoder_bases(C, c)
    rows, _ = fv.recoder_rows(C, c)
    secs = [fv.table_section(C, c, [fv.point(C, b) for b in bs], idx=one_entry())]
    for S in COMMIT_S:
        for guest in (0, 1):
            secs.append(fv.commit_section(c, rows, S, guest=guest, sentinel=1))
    for SL in SMALL_SL:
        for ch in chunks(rows, fv.SMALL_MAX_ROWS):
            secs.append(fv.small_section(c, ch, SL))
    return secs, None


def fold_by_model(C, pts):
    r = None
    for pt in pts:
        r = ev.ec_add(C, r, pt)
    return r


def check_small_output(C, out, n_rows, SL, want, where):
    """part, out_sums, counters, hdr of one k_fb_commit_small section; want: the rows' expected points"""
    part = out[:n_rows * SL * 32].reshape(n_rows, SL, 32)
    sums = out[n_rows * SL * 32:(n_rows * SL + n_rows) * 32].reshape(n_rows, 32)
    counters, hdr = out[(n_rows * SL + n_rows) * 32:-1], int(out[-1])
    assert len(counters) == fv.SMALL_MAX_ROWS + 1 and not counters.any(), "%s: the counters are not back at zero: %s" % (where, counters)
    assert hdr == 1, "%s: hdr[0] = %#x, seq 1 was not published" % (where, hdr)
    for r in range(n_rows):
        w = "%s row %d" % (where, r)
        assert fv.decode_mem(C, sums[r], w + " out_sums", final=True) == want[r], w + ": out_sums"
        slices = [fv.decode_mem(C, part[r, s], w + " part %d" % s) for s in range(SL)]
        assert fold_by_model(C, slices) == want[r], w + ": the slices' sums"


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("c", RECODER_C)
def test_recoders_through_both_commit_kernels(c, curve):
    """every family member at every coefficient position: k_fb_commit (S = 1, 2, 8, both template forms) and k_fb_commit_small
    (SL = 1, 3, 8) give sum (k_i mod order) G_i for every row"""
    C = ev.CURVES[curve]
    outs, _ = session(curve)["recoder_c%d" % c]
    bs = fv.recoder_bases(C, c)
    rows, fed = fv.recoder_rows(C, c)
    nc = len(bs)
    want = [fv.mul_g(C, fv.row_scalar(C, bs, r)) for r in rows]
    at, checked, generated = 1, 0, 0
    for S in COMMIT_S:
        assert nc % S != 0 or S == 1
        forms = []
        for guest in (0, 1):
            part = outs[at].reshape(len(rows) + 1, S, 32)
            at += 1
            assert (part[len(rows)] == fv.SENTINEL).all(), "c=%d S=%d form %d: the sentinel row was written" % (c, S, guest)
            elems = []
            for r in range(len(rows)):
                where = "%s c=%d S=%d form %d row %d" % (curve, c, S, guest, r)
                sl = [fv.decode_mem(C, part[r, s], where, final=(S == 1), key=ev.BOUNDS["flip_finish"]) for s in range(S)]
                for s, (i0, i1) in enumerate(fv.slice_ranges(nc, S)):
                    assert i0 < i1 or sl[s] is None, where + ": an empty slice is not infinity"
                assert fold_by_model(C, sl) == want[r], where + " coefficients %s" % [hex(k) for k in rows[r]]
                elems.append(sl)
                checked += 1
            generated += len(rows)
            forms.append(elems)
        assert forms[0] == forms[1], "c=%d S=%d: k_fb_commit<C> and k_fb_commit<C, true> differ as group elements" % (c, S)
    for SL in SMALL_SL:
        lo = 0
        for ch in chunks(rows, fv.SMALL_MAX_ROWS):
            check_small_output(C, outs[at], len(ch), SL, want[lo:lo + len(ch)], "%s c=%d SL=%d rows from %d" % (curve, c, SL, lo))
            at += 1
            lo += len(ch)
            checked += len(ch)
            generated += len(ch)
    counts = dict(collections.Counter(fed))
    print("recoders %s c=%d: %d rows of %d coefficients x (%d commit runs + %d commit_small runs) = %d row sums, families %s"
          % (curve, c, len(rows), nc, 2 * len(COMMIT_S), len(SMALL_SL), checked, counts))
    assert at == len(outs) and checked == generated == len(rows) * (2 * len(COMMIT_S) + len(SMALL_SL))
    assert counts["random"] >= 1000 and counts["edge"] == 4 and counts["half"] == 3 and counts["win"] >= fv.windows(C, c)


for _c in RECODER_C:
    JOBS["recoder_c%d" % _c] = functools.partial(recoder_job, _c)


# ================================================================ degenerate accumulation in k_fb_commit
COMMIT_STRIDE = 32 * len(fv.COMMIT_BASES) + 64
COMMIT_SENTINEL = 2


@job("commit_degenerate")
def commit_degenerate_job(C):
    rows, where = fv.commit_degenerate_rows(C)
    secs = [fv.table_section(C, fv.COMMIT_C, [fv.point(C, b) for b in fv.COMMIT_BASES], idx=one_entry())]
    for S in (1, 2):
        for guest in (0, 1):
            secs.append(fv.commit_section(fv.COMMIT_C, rows, S, stride=COMMIT_STRIDE, guest=guest, sentinel=COMMIT_SENTINEL))
    return secs, (rows, where)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_commit_degenerate_accumulation(curve):
    """base G, G, G, G, -G, 3 G, infinity, 7 G: a doubling on the second addition, infinity mid-row, a lone last window, a zero row, a
    coefficient on the infinity point; row_stride > 32 n_coeffs, 300 rows (a ragged last block), sentinel rows behind"""
    C = ev.CURVES[curve]
    outs, (rows, where) = session(curve)["commit_degenerate"]
    n = len(rows)
    assert n == 300 and n % 256 != 0 and all(len(v) == 2 and v[1] >= 256 for v in where.values())
    scal = [fv.row_scalar(C, fv.COMMIT_BASES, r) for r in rows]
    for label in ("zero", "order", "cancel_first", "cancel_end", "inf_only"):
        assert all(scal[i] == 0 for i in where[label]), label
    want = [fv.mul_g(C, s) for s in scal]
    at, checked = 1, 0
    for S in (1, 2):
        for guest in (0, 1):
            part = outs[at].reshape(n + COMMIT_SENTINEL, S, 32)
            at += 1
            assert (part[n:] == fv.SENTINEL).all(), "S=%d form %d: the sentinel rows were written" % (S, guest)
            for r in range(n):
                w = "%s S=%d form %d row %d" % (curve, S, guest, r)
                sl = [fv.decode_mem(C, part[r, s], w, final=(S == 1), key=ev.BOUNDS["flip_finish"]) for s in range(S)]
                assert fold_by_model(C, sl) == want[r], w
                checked += 1
    print("commit degenerate %s: %d rows x 4 runs, named rows %s" % (curve, n, {k: v for k, v in where.items()}))
    assert checked == 4 * n and at == len(outs)


# ================================================================ degenerate folds in k_fb_commit_small
SMALL_RUNS = [(1, fv.SMALL_MAX_ROWS), (2, fv.SMALL_MAX_ROWS), (3, fv.SMALL_MAX_ROWS), (1, 1), (8, 1)]     # (SL, rows)


@job("small_degenerate")
def small_degenerate_job(C):
    bs, rows, _ = fv.small_degenerate(C.name)
    secs = [fv.table_section(C, fv.SMALL_C, [fv.point(C, b) for b in bs], idx=one_entry())]
    for SL, n in SMALL_RUNS:
        secs.append(fv.small_section(fv.SMALL_C, rows[:n], SL))
    return secs, None


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_commit_small_degenerate_folds(curve):
    """equal (P + P) and opposite (P - P) lane sums at every one of the 8 LDS levels, and slice sums in the last block's fold; rows
    where most lanes hold infinity; 1 row and FB_SMALL_MAX_ROWS rows"""
    C = ev.CURVES[curve]
    outs, _ = session(curve)["small_degenerate"]
    bs, rows, labels = fv.small_degenerate(curve)
    checked, met = 0, collections.Counter()
    for (SL, n), out in zip(SMALL_RUNS, outs[1:]):
        models = [fv.small_model(C, fv.SMALL_C, bs, r, SL) for r in rows[:n]]
        for total, _, meetings in models:
            met.update((SL,) + m for m in meetings)
        check_small_output(C, out, n, SL, [fv.mul_g(C, total) for total, _, _ in models], "%s SL=%d" % (curve, SL))
        checked += n
    for h in (1, 2, 4, 8, 16, 32, 64, 128):
        assert met[(1, "lds", h, "eq")] > 0 and met[(1, "lds", h, "opp")] > 0, "no equal / opposite lane sums at LDS level %d" % h
    for key in ((2, "slice", 0), (3, "slice", 0), (3, "slice", 1)):
        assert met[key + ("eq",)] > 0 and met[key + ("opp",)] > 0, key
    print("commit_small degenerate %s: %d rows in %d launches, meetings %s" % (curve, checked, len(SMALL_RUNS), dict(met)))
    assert checked == sum(n for _, n in SMALL_RUNS) and len(outs) == 1 + len(SMALL_RUNS)


# ================================================================ k_fb_fold_quad
FOLD_SENTINEL = 2


@job("fold")
def fold_job(C):
    secs = []
    for S in FOLD_S:
        rows = fv.fold_layout(S)
        secs.append(fv.fold_section(5, fv.fold_partials(C, rows, S, 0xF0 + S), S, sentinel=FOLD_SENTINEL))
    return secs, None


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("S", FOLD_S)
def test_fold_quad(S, curve):
    """partials at the operand bounds of the lazy memory form: all distinct, infinity scattered, all infinity, slot q equal and
    opposite to slot q + n at every level n; a last block with padding quads.  Slot 0 is the row's sum in the final form, the slots from
    S / 2 up and the sentinel rows are untouched"""
    C = ev.CURVES[curve]
    outs, _ = session(curve)["fold"]
    out = outs[FOLD_S.index(S)]
    rows = fv.fold_layout(S)
    src = fv.fold_partials(C, rows, S, 0xF0 + S).reshape(len(rows), S, 32)
    got = out.reshape(len(rows) + FOLD_SENTINEL, S, 32)
    per_block = 128 // S
    assert per_block == 1 or len(rows) % per_block != 0, "no padding quads in the last block"
    assert (got[len(rows):] == fv.SENTINEL).all(), "the sentinel rows were written"
    seen, checked = set(), 0
    for r, (label, a) in enumerate(rows):
        total, meetings = fv.fold_model(a, S)
        if isinstance(label, tuple):
            assert label in meetings, (label, meetings)
            seen.add((label[0], label[2]))
        where = "%s S=%d row %d (%s)" % (curve, S, r, label)
        assert fv.decode_mem(C, got[r, 0], where, final=True) == fv.mul_g(C, total), where
        assert (got[r, S // 2:] == src[r, S // 2:]).all(), where + ": a slot from S / 2 up was written"
        checked += 1
    n = S // 2
    while n >= 1:
        assert (n, "eq") in seen and (n, "opp") in seen, n
        n //= 2
    print("fold_quad %s S=%d: %d rows (%d per block), levels with equal and opposite partners: %s"
          % (curve, S, checked, per_block, sorted({l for l, _ in seen})))
    assert checked == len(rows) and labels_present(rows)


def labels_present(rows):
    names = [l for l, _ in rows]
    return "distinct" in names and "scattered" in names and "all_inf" in names


# ================================================================ k_fb_finish
FINISH_RUNS = [(R, n, S) for R in (1, 2, 4) for n in (1, 64 * R + 37) for S in (1, 4)]
FINISH_SENTINEL = 3


@job("finish")
def finish_job(C):
    secs = []
    for i, (R, n, S) in enumerate(FINISH_RUNS):
        secs.append(fv.finish_section(5, fv.finish_partials(C, fv.finish_rows(R, n), S, 0xF1 + i), S, R, sentinel=FINISH_SENTINEL))
    return secs, None


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("R", [1, 2, 4])
def test_finish(R, curve):
    """k_fb_finish<C, R>: 1 row and 64 R + 37 rows at stride 1 and 4; an infinity row in each of a lane's R positions in turn, a lane whose
    rows are all infinity; 64 big-endian bytes per row, zero for infinity, the bytes behind the last row untouched"""
    C = ev.CURVES[curve]
    outs, _ = session(curve)["finish"]
    checked = generated = 0
    for i, (r_, n, S) in enumerate(FINISH_RUNS):
        if r_ != R:
            continue
        a = fv.finish_rows(R, n)
        if n > 1:
            assert all(a[t + 64 * (t % R)] == 0 for t in range(16)) and all(a[20 + 64 * k] == 0 for k in range(R))
            assert {t % R for t in range(16)} == set(range(R)) and sum(1 for v in a if v) > n // 2
        got = outs[i].reshape(n + FINISH_SENTINEL, 16)
        assert (got[n:] == fv.SENTINEL).all(), "R=%d n=%d S=%d: the bytes behind the last row were written" % (R, n, S)
        for r, m in enumerate(a):
            assert (got[r] == fv.out_bytes(C, fv.small_point(C, m) if m else None)).all(), "%s R=%d n=%d S=%d row %d" % (curve, R, n, S, r)
            checked += 1
        generated += n
    print("finish %s R=%d: %d rows in %d launches" % (curve, R, checked, sum(1 for r_, _, _ in FINISH_RUNS if r_ == R)))
    assert checked == generated == 2 * (1 + 64 * R + 37)

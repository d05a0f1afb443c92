"""GPU: the MAC side's scalar-multiplication ladders and their digit recoders per form, on scalars the test chooses, through the
driver tools/ladder_check.hip (which launches mac_fft.hip.h's own kernels with mac_fft.hip's launch helpers).  Expected values:
Python integers (tests/ladder_vectors.py).

Recoders (mac_signed_digit, mac_wnaf5_step, glv_split on the device): digits, codes and halves compare word for word with the
models.  Stage kernels: a scalar table of the test's stands in place of the twiddles -- stage s reads entry j (n >> (s-1))
(mac_stage_index), so (n, s) are chosen such that every butterfly, or every wave, multiplies by the scalar the test wants; both
outputs um + k P and um - k P compare as group elements with form and value bounds (ec_vectors.check_point_mem; infinity is
all-zero words); rows no live butterfly owns stay bit-identical.  The forms that read k_mac_wnaf_codes' table also check that its
entries decode to the halves of the table's scalars.  Comparison is exact; no record is skipped (checked == generated)."""
import collections
import functools
import os
import random

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests import ladder_vectors as lv

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "secp256k1"]
PER_BUTTERFLY = ["stage30", "stage30_quad", "stage30_oct"]
# wave-uniform stage forms: (butterflies that share a scalar, scalars per launch)
UNIFORM = {"stage30_uniform": (64, 16), "stage30_quad_uniform": (16, 64), "stage30_oct_uniform": (16, 64)}
BY_VALUE = ["scale30", "load30_wt", "load30_quad", "load30_quad_work"]
LIVE_PER_SCALAR = 2              # butterflies of a wave-uniform scalar with finite inputs (two of the four um cases, walking with the
                                 # scalar's index); the rest sit at infinity beside them


def test_driver_is_built():
    assert os.path.exists(lv.EXE), "build it with make -C porla_amd/csrc"


def family_minimums(C, fed):
    """fed: the family labels of the scalars a test ran"""
    n = collections.Counter(fed)
    assert n["b"] >= 1000, n
    assert n["c"] == (32 if C is ev.SECP else 0), n
    assert n["a"] >= 44 and n["d"] == 12, n
    return dict(n)


# ================================================================ one driver process per curve
# Starting the driver (a process, the device's initialisation) costs more than most of its jobs: every job of a curve -- the
# recoders' records and every form's launches -- goes to ONE process, run when the first test of that curve asks for an output;
# each test then checks its own job's output.
JOBS = {}                        # name -> function(C) -> (driver op, input words, what the check needs)


def job(name):
    def register(fn):
        JOBS[name] = fn
        return fn
    return register


@functools.lru_cache(maxsize=None)
def session(curve):
    """{job name: (output words, what the check needs)}"""
    C = ev.CURVES[curve]
    names = [n for n in JOBS if curve == "bn254" or n not in CURVE_FREE]
    built = [JOBS[n](C) for n in names]
    outs = lv.run(C, [(op, data) for op, data, _ in built])
    return {n: (out, ctx) for n, out, (_, _, ctx) in zip(names, outs, built)}


CURVE_FREE = ("mac_signed_digit", "mac_wnaf5_step")      # recoders that do not depend on the curve: run with BN254's jobs


# ================================================================ recoders
@job("mac_signed_digit")
def digit_job(C):
    mags = lv.magnitudes()
    recs = lv.recoder_records(len(mags))
    for i, m in enumerate(mags):
        recs[i, lv.A0:lv.A0 + 4] = ev.words(m)[:4]
    return "mac_signed_digit", recs.reshape(-1), recs


def test_mac_signed_digit():
    """(the recoder does not depend on the curve: one run)"""
    curve, mags = "bn254", lv.magnitudes()
    out, recs = session(curve)["mac_signed_digit"]
    out = out.reshape(-1, lv.REC)
    assert out.shape == recs.shape
    checked = 0
    for i, m in enumerate(mags):
        got = [int(x) for x in out[i, lv.O0:lv.O0 + 33].view(np.int32)]
        lv.check_signed_digits(m, got)
        assert got == lv.signed_digits(m), hex(m)
        assert (out[i, lv.O0 + 33:] == lv.SENTINEL).all() and (out[i, :lv.O0] == recs[i, :lv.O0]).all(), hex(m)
        checked += 1
    print("mac_signed_digit %s: %d records" % (curve, checked))
    assert checked == len(mags) > 2000


def wnaf_cases():
    return [(m, flip) for m in lv.magnitudes() for flip in (0, 1)]


@job("mac_wnaf5_step")
def wnaf_job(C):
    cases = wnaf_cases()
    recs = lv.recoder_records(len(cases))
    for i, (m, flip) in enumerate(cases):
        recs[i, lv.A0:lv.A0 + 4] = ev.words(m)[:4]
        recs[i, lv.F_FLIP] = flip
    return "mac_wnaf5_step", recs.reshape(-1), recs


def test_mac_wnaf5_step():
    """(the recoder does not depend on the curve: one run)"""
    curve, cases = "bn254", wnaf_cases()
    out, recs = session(curve)["mac_wnaf5_step"]
    out = out.reshape(-1, lv.REC)
    assert out.shape == recs.shape
    checked = 0
    for i, (m, flip) in enumerate(cases):
        codes = [int(x) for x in out[i, lv.O0:lv.O0 + lv.WNAF_LEN]]
        digits = [(-d if flip else d) for d in (lv.decode_code(c) for c in codes)]
        left = [int(x) for x in out[i, lv.O0 + lv.WNAF_LEN:lv.O0 + lv.WNAF_LEN + 5]]
        lv.check_wnaf5(m, digits, ev.words_value(left + [0, 0, 0]))
        assert codes == [lv.wnaf_code(d, flip) for d in lv.wnaf5(m)[0]], (hex(m), flip)
        assert left == [0] * 5, (hex(m), left)
        assert (out[i, lv.O0 + lv.WNAF_LEN + 5:] == lv.SENTINEL).all(), hex(m)
        checked += 1
    print("mac_wnaf5_step %s: %d records" % (curve, checked))
    assert checked == len(cases) > 4000


def glv_scalars(C):
    d, n, lam = lv.glv(C.name), lv.order(C), lv.lam(C)
    rnd = random.Random(11)
    ks = [0, 1, 2, n - 1, n - 2, lam, lam + 1, n - lam, lam * lam % n, (n - 1) // 2, (n + 1) // 2, (1 << 128) - 1, 1 << 128,
          abs(d["a1"]), abs(d["b1"]), abs(d["a2"]), abs(d["b2"]), n, n + 1, (1 << 256) - 1]
    ks += [rnd.randrange(1 << 256) for _ in range(20000)]
    return [k % n for k in ks] + [k for _, k in lv.families(C)]


@job("glv_split")
def glv_job(C):
    ks = glv_scalars(C)
    recs = lv.recoder_records(len(ks))
    for i, k in enumerate(ks):
        recs[i, lv.A0:lv.A0 + 8] = ev.words(k)
    return "glv_split", recs.reshape(-1), (ks, recs)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_glv_split_on_the_device(curve):
    """the vectors of tests/test_glv_cpu.py (reduced mod n, as every caller hands them over) and every family scalar"""
    C = ev.CURVES[curve]
    d, n, lam = lv.glv(curve), lv.order(C), lv.lam(C)
    out, (ks, recs) = session(curve)["glv_split"]
    out = out.reshape(-1, lv.REC)
    bits = max(((abs(d["a1"]) + abs(d["a2"])) // 2 + 2).bit_length(), ((abs(d["b1"]) + abs(d["b2"])) // 2 + 2).bit_length())
    assert out.shape == recs.shape
    checked = 0
    for i, k in enumerate(ks):
        o = out[i, lv.O0:]
        got = [(ev.words_value(o[0:4]), int(o[4])), (ev.words_value(o[5:9]), int(o[9]))]
        assert got == lv.split(C, k), hex(k)
        k1, k2 = [-m if neg else m for m, neg in got]
        assert (k1 + lam * k2 - k) % n == 0 and got[0][0] < 1 << bits and got[1][0] < 1 << bits, hex(k)
        assert (o[10:] == lv.SENTINEL).all()
        checked += 1
    print("glv_split %s: %d records" % (curve, checked))
    assert checked == len(ks) > 20000


# ================================================================ stage kernels
def untouched(work, owned, where):
    for r in range(work.shape[0]):
        if r not in owned:
            assert (work[r] == lv.SENTINEL).all(), "%s: row %d, which no live butterfly owns, was written" % (where, r)


def per_butterfly_job(form, C):
    sh = lv.per_butterfly_shape(256)
    fam = lv.families(C)
    launches = []                                   # (total, {t: Butterfly})
    for at in range(0, len(fam), sh.total):
        chunk = fam[at:at + sh.total]
        launches.append((len(chunk), {t: lv.butterfly(C, k, at + t, 0) for t, (_, k) in enumerate(chunk)}))
    pad = [k for _, k in lv.families(C, "e")][:lv.PAD_TOTAL]
    launches.append((lv.PAD_TOTAL, {t: lv.butterfly(C, k, t, 1) for t, k in enumerate(pad)}))
    data = np.concatenate([lv.stage_launch(C, sh, {sh.bf[t][2]: b.k for t, b in bfs.items()}, bfs, total) for total, bfs in launches])
    return form, data, launches


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("form", PER_BUTTERFLY)
def test_per_butterfly_form(form, curve):
    """one scalar per butterfly: families (a)-(e) over the last stage of tables of 512 rows; then a launch whose butterfly count
    fills neither the four- nor the eight-lane kernel's last block, sentinel rows behind the last live pair"""
    C = ev.CURVES[curve]
    sh, fam = lv.per_butterfly_shape(256), lv.families(C)
    raw, launches = session(curve)[form]
    outs = lv.split_stage_output(raw, [(sh.n, sh.n)] * len(launches), False)
    generated = sum(total for total, _ in launches)
    checked = 0
    for li, ((total, bfs), (work, _)) in enumerate(zip(launches, outs)):
        owned = set()
        for t in range(total):
            lv.check_butterfly(C, work, sh, t, bfs[t], "%s %s launch %d butterfly %d k = %#x" % (form, curve, li, t, bfs[t].k))
            owned |= {sh.bf[t][0], sh.bf[t][0] + sh.bf[t][1]}
            checked += 1
        untouched(work, owned, "%s %s launch %d" % (form, curve, li))
    counts = family_minimums(C, [f for f, _ in fam])
    print("%s %s: %d butterflies in %d launches, families %s + %d padded" % (form, curve, checked, len(launches), counts, lv.PAD_TOTAL))
    assert checked == generated == len(fam) + lv.PAD_TOTAL and counts["e"] == 256


def wave_uniform_job(form, C):
    share, per_launch = UNIFORM[form]
    sh = lv.uniform_shape(share, per_launch)
    fam = lv.families(C, "abcd")
    filler = [k for _, k in lv.families(C, "e")]
    launches = []                                   # ({entry: k}, {t: Butterfly}, entries that carry a family scalar)
    for at in range(0, len(fam), per_launch):
        chunk = [k for _, k in fam[at:at + per_launch]]
        fed = len(chunk)
        chunk += filler[:per_launch - fed]          # (a table entry that is read holds a scalar: the last launch is filled up)
        scalars, bfs = {}, {}
        for i, e in enumerate(sh.entries):
            scalars[e] = chunk[i]
            idle = lv.trivial_butterfly(C, chunk[i])
            for slot, t in enumerate(sh.readers[e]):
                bfs[t] = lv.butterfly(C, chunk[i], at + i, slot) if slot < LIVE_PER_SCALAR else idle
        launches.append((scalars, bfs, sh.entries[:fed]))
    data = np.concatenate([lv.stage_launch(C, sh, scalars, bfs) for scalars, bfs, _ in launches])
    return form, data, launches


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("form", sorted(UNIFORM))
def test_wave_uniform_form(form, curve):
    """one scalar per wave, its digit codes from k_mac_wnaf_codes run on the test's table: every scalar of families (a)-(d)"""
    C = ev.CURVES[curve]
    sh, fam = lv.uniform_shape(*UNIFORM[form]), lv.families(C, "abcd")
    raw, launches = session(curve)[form]
    outs = lv.split_stage_output(raw, [(sh.n, sh.n)] * len(launches), True)
    generated = sum(len(bfs) for _, bfs, _ in launches)
    checked = scalars_checked = 0
    for li, ((scalars, bfs, fed), (work, codes)) in enumerate(zip(launches, outs)):
        for e in sh.entries:
            lv.check_codes_entry(C, codes[e >> lv.CODES_EXP_SHIFT], scalars[e], "%s %s launch %d entry %d k = %#x" % (form, curve, li, e, scalars[e]))
            scalars_checked += e in fed
        for t in range(sh.total):
            lv.check_butterfly(C, work, sh, t, bfs[t], "%s %s launch %d butterfly %d k = %#x" % (form, curve, li, t, bfs[t].k))
            checked += 1
    counts = family_minimums(C, [f for f, _ in fam])
    print("%s %s: %d butterflies (%d with finite inputs) in %d launches, %d scalars, families %s"
          % (form, curve, checked, sum(1 for _, bfs, _ in launches for b in bfs.values() if b.case != "trivial"), len(launches),
             scalars_checked, counts))
    assert checked == generated == len(launches) * sh.total > 0 and scalars_checked == len(fam)


VALUE_ROWS, VALUE_LIVE = 4, 3


def by_value_job(form, C):
    fam = lv.families(C, "abcd")
    affine = form in ("load30_wt", "load30_quad")
    rows, live = VALUE_ROWS, VALUE_LIVE
    pad = [[lv.SENTINEL] * (16 if affine else 32)] * (rows - live)
    launches, blocks = [], []
    for (_, k), (ms, words) in zip(fam, lv.by_value_rows(C, affine)):
        launches.append((k, ms))
        blocks.append(lv.launch_words(n=live, rows=words + pad, wt=k))
    return form, np.concatenate(blocks), launches


for _form in PER_BUTTERFLY:
    JOBS[_form] = functools.partial(per_butterfly_job, _form)
for _form in sorted(UNIFORM):
    JOBS[_form] = functools.partial(wave_uniform_job, _form)
for _form in BY_VALUE:
    JOBS[_form] = functools.partial(by_value_job, _form)


@pytest.mark.parametrize("curve", CURVE_NAMES)
@pytest.mark.parametrize("form", BY_VALUE)
def test_by_value_form(form, curve):
    """wt handed over by value and recoded in the kernel: one launch per scalar of families (a)-(d) over two points and infinity;
    the output rows behind the last point keep what they held"""
    C = ev.CURVES[curve]
    fam, rows, live = lv.families(C, "abcd"), VALUE_ROWS, VALUE_LIVE
    raw, launches = session(curve)[form]
    outs = lv.split_stage_output(raw, [(0, rows)] * len(launches), False)
    checked = 0
    for li, ((k, ms), (work, _)) in enumerate(zip(launches, outs)):
        key = lv.by_value_key(C, k)
        for j, m in enumerate(ms):
            ev.check_point_mem(C, work[j], lv.scalar_multiples(C, k)[m], key, "%s %s k = %#x P = %d G" % (form, curve, k, m))
            checked += 1
        assert (work[live:] == lv.SENTINEL).all(), "%s %s launch %d: a row behind the last point was written" % (form, curve, li)
    counts = family_minimums(C, [f for f, _ in fam])
    print("%s %s: %d points in %d launches, families %s" % (form, curve, checked, len(launches), counts))
    assert checked == live * len(fam) > 0

"""GPU: the division-step inversion of inv30.hip.h, run by the driver tools/inv_check.hip (which calls f30_inv_safegcd_raw and
fe_inv_safegcd unchanged), against tests/inv_vectors.py.

raw: the nine limbs of every active lane equal, word for word, the limb model run for the rounds of the lane's WAVE -- the maximum of
the rounds the lanes that execute the call need: the active lanes when the others left before the call, all lanes with the dummy 1
(18 rounds) when they stayed.  The returned integer depends on that count, so a vote that counted the wrong lanes fails here and
nowhere else.  Independently of the model: limbs 0..7 below 2^30, the value in (0, 4 p) and value * V = 1 mod p.  Lanes without work
keep the sentinel; the input words come back unchanged.  All four moduli, inputs below and above them, blocks of 64 and 256.

fe (the two base fields): canonical bytes equal to the Fe-form inverse on Python integers, a * out = R1 under the field's own product,
and the same bytes for a value in whichever wave it sits.

Comparison is exact; no record is skipped (checked == generated).  One driver process per modulus."""
import functools
import os

import pytest

from tests import inv_vectors as iv

pytestmark = pytest.mark.gpu


def test_driver_is_built():
    assert os.path.exists(iv.EXE), "build it with make -C porla_amd/csrc"


@functools.lru_cache(maxsize=None)
def session(name):
    """{job name: (job, input records, output records)}"""
    js = iv.jobs(name)
    return {j.name: (j, recs, out) for j, (recs, out) in zip(js, iv.run(name, js))}


def limbs_value(limbs):
    return sum(int(l) << (30 * i) for i, l in enumerate(limbs))


def check_raw_job(name, job_name):
    p = iv.MODULI[name].p
    job, recs, out = session(name)[job_name]
    assert job.op == "raw" and out.shape == recs.shape
    expected = iv.expected_records(name, job)
    assert len(expected) == out.shape[0]
    checked = active_n = 0
    for i, (w, lane, V, active, rounds) in enumerate(expected):
        where = "%s %s: wave '%s' lane %d V = %#x, %d rounds" % (name, job_name, w.label, lane, V, rounds)
        assert (out[i, :iv.O0] == recs[i, :iv.O0]).all(), where + ": input words changed"
        o = [int(x) for x in out[i, iv.O0:]]
        if active:
            got = o[:9]
            # independent of the model
            assert all(l < 1 << 30 for l in got[:8]), where
            x = limbs_value(got)
            assert 0 < x < 4 * p, where + ": value %#x outside (0, 4 p)" % x
            assert x * V % p == 1, where
            # word for word
            want = list(iv.raw_limbs(V, p, rounds))
            assert got == want, where + ": got p-multiple %d, want %d" % (x // p, limbs_value(want) // p)
            assert o[9:] == [iv.SENTINEL] * 3, where
            active_n += 1
        else:
            assert o == [iv.SENTINEL] * (iv.REC - iv.O0), where + ": a lane without work wrote"
        checked += 1
    print("%s %s: checked %d == generated %d records (%d active) in %d waves" % (name, job_name, checked, len(expected), active_n, len(job.waves)))
    assert checked == len(expected) == len(job.waves) * iv.WAVE > 0
    return checked


RAW_JOBS = ["raw uniform", "raw mixed", "raw random", "raw masks leave", "raw masks stay", "raw block256 leave", "raw block256 stay"]
FE_JOBS = ["fe uniform", "fe mixed", "fe random", "fe masks stay", "fe block256 leave"]


@pytest.mark.parametrize("name", iv.NAMES)
@pytest.mark.parametrize("job_name", RAW_JOBS)
def test_raw_limbs(job_name, name):
    check_raw_job(name, job_name)


@pytest.mark.parametrize("name", iv.NAMES)
def test_every_job_ran(name):
    """the jobs of a modulus are exactly the ones the tests above and below read"""
    want = RAW_JOBS + (FE_JOBS if name in iv.FE_NAMES else [])
    s = session(name)
    assert list(s) == want
    generated = sum(len(j.waves) * iv.WAVE for j, _, _ in s.values())
    checked = sum(out.shape[0] for _, _, out in s.values())
    print("%s: checked %d == generated %d records in %d jobs" % (name, checked, generated, len(s)))
    assert checked == generated


@pytest.mark.parametrize("name", iv.FE_NAMES)
def test_fe_inverse(name):
    m = iv.MODULI[name]
    p, radix = m.p, m.fe_radix
    radix_inv = pow(radix, -1, p)
    seen = {}                                                   # V -> (bytes, where first seen)
    checked = generated = below = above = 0
    for job_name in FE_JOBS:
        job, recs, out = session(name)[job_name]
        assert job.op == "fe" and out.shape == recs.shape
        expected = iv.expected_records(name, job)
        generated += len(expected)
        assert len(expected) == out.shape[0]
        for i, (w, lane, V, active, rounds) in enumerate(expected):
            where = "%s %s: wave '%s' lane %d V = %#x" % (name, job_name, w.label, lane, V)
            assert (out[i, :iv.O0] == recs[i, :iv.O0]).all(), where + ": input words changed"
            o = [int(x) for x in out[i, iv.O0:]]
            if active:
                x = iv.words_value(o[:8])
                assert x < p, where + ": not canonical"
                assert V * x * radix_inv % p == radix % p, where + ": a * out is not R1"       # the field's product: a b / radix
                assert x == iv.fe_inverse(V, m), where
                assert o[8:] == [iv.SENTINEL] * 4, where
                first = seen.setdefault(V, (x, where))
                assert first[0] == x, where + ": other bytes than in " + first[1]
                below += V < p
                above += V >= p
            else:
                assert o == [iv.SENTINEL] * (iv.REC - iv.O0), where + ": a lane without work wrote"
            checked += 1
    repeated = sum(1 for j in FE_JOBS for w in session(name)[j][0].waves for v, a in zip(w.values, w.active) if a) - len(seen)
    print("%s fe: checked %d == generated %d records, %d distinct values (%d below p, %d at or above), %d repeats in other waves"
          % (name, checked, generated, len(seen), below, above, repeated))
    assert checked == generated > 0 and below >= 256 and above >= 256 and repeated > 1000

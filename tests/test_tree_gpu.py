"""GPU: the bucket reduction tree of porla_amd/csrc/msm.hip.h -- k_tree_front2, k_tree_level, k_tree_level_quad and k_tree_tail as
they are, issued by the product's schedule (msm_tree.hip.h) through tools/tree_check.hip on bucket arrays the test wrote
(tests/tree_vectors.py: the families slot, copy, bounds, sparse, shape and forced; tests/test_tree_vectors_cpu.py asserts that all of
them are there and that every plan run here stays inside its buffers).  Per curve and file, ONE driver run:
  nodes       every stored S node of every window through ec_vectors.check_point_mem with the bound key of the operation that
              produced it (add, double, or operand where a sum passed an infinite neighbour), every fin entry with final=True
              (canonical 2^256 form, infinity all-zero); exact; checked == generated
  untouched   every word of the S, M and tail areas the plan does not write still holds 0xA5A5A5A5: the slack entries and, under
              k_tree_front2, the even entries of S^0
  same        fin is bit-identical between lone and not lone and between every forced plan and the product's own over the same
              buckets; on secp256k1 (canonical memory form) the S nodes too
Then: malformed files are refused before anything reaches the device.

How to see the tests bite (on a scratch copy, not committed): in msm.hip.h:tree_op's aliased-slot branch write `o.pb = o.pa + 1`
for `o.pa + 2` -- the test_nodes cases with c >= 3 fail at fin[w][l] of the first level l >= 1 whose aliased slot it reaches; or in
msm_tree.hip.h drop the `+ 1` of `m_off + nbp / 4 + 1` -- test_tree_vectors_cpu.py::test_default_plan_equals_the_restated_rules
fails for every shape."""
import os
import subprocess

import numpy as np
import pytest

from tests import ec_vectors as ev
from tests import tree_vectors as tv

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "secp256k1"]
CURVE_FILES = [(c, f) for c in CURVE_NAMES for f in tv.FILE_NAMES[c]]


def groups(curve, name):
    """a file's sections in groups that take a few seconds of Python each: the shape file by c, the slot file by plan"""
    secs = tv.FILES[name](curve).sections
    if name == "shape":
        return [("c%d" % c, [i for i, sc in enumerate(secs) if sc.c == c]) for c in tv.SHAPE_C]
    if name == "slot":
        return [(sc.label, [i]) for i, sc in enumerate(secs)]
    return [("all", list(range(len(secs))))]


NODE_PARAMS = [(c, f, g) for c, f in CURVE_FILES for g, _ in groups(c, f)]


def test_driver_is_built():
    assert os.path.exists(tv.EXE), "build it with make -C porla_amd/csrc"


_RUNS = {}


def outputs(curve, name):
    """one driver run per curve and file, as a fresh child process under a time limit; the result is kept, a failed one too
    (functools.lru_cache would start a failing driver again for every test that asks)"""
    key = (curve, name)
    if key not in _RUNS:
        try:
            _RUNS[key] = (tv.run(tv.FILES[name](curve), timeout=60), None)
        except (AssertionError, subprocess.TimeoutExpired, OSError, ValueError) as e:
            _RUNS[key] = (None, "%s: %s" % (type(e).__name__, e))
    out, err = _RUNS[key]
    if err is not None:
        pytest.fail("the driver run of %s %s failed (not started again): %s" % (curve, name, err))
    return out


_LAYOUTS = {}


def layout(curve, name, si):
    key = (curve, name, si)
    if key not in _LAYOUTS:
        _LAYOUTS[key] = tv.Layout(tv.file_plans(curve, name)[si])
    return _LAYOUTS[key]


def stored_nodes(plan, info, k):
    """(level, node of the window) of every S node the plan stores for window case k: the levels below the last (that one goes
    to fin), without the even entries of S^0 where k_tree_front2 keeps them in registers"""
    return [(l, j) for l in range(k.c - 2) for j in range(k.B >> (l + 1)) if not (info["front2"] and l == 0 and j % 2 == 0)]


@pytest.mark.parametrize("curve,name,group", NODE_PARAMS)
def test_nodes(curve, name, group):
    C = ev.CURVES[curve]
    F = tv.FILES[name](curve)
    outs, plans = outputs(curve, name), tv.file_plans(curve, name)
    checked = generated = 0
    for si in dict(groups(curve, name))[group]:
        sc, plan, lay = F.sections[si], plans[si], layout(curve, name, si)
        for ri, (run, out) in enumerate(zip(sc.runs, outs[si])):
            for w, k in enumerate(run):
                part, info = tv.part_of(plan, w)
                e = tv.expected(C, k)
                where = "%s %s section %s run %d window %d (%r)" % (curve, name, sc.label, ri, w, k)
                generated += k.B - 2 - (k.B // 4 if info["front2"] else 0) + k.c
                for l, j in stored_nodes(plan, info, k):
                    _, P, key = e["S"][l][j]
                    row = out["S"][lay.s_entry(part, l, (w - info["w0"]) * (k.B >> (l + 1)) + j)]
                    ev.check_point_mem(C, row, P, key, "%s: S^%d[%d]" % (where, l, j))
                    checked += 1
                for i, (_, P) in enumerate(e["fin"]):
                    ev.check_point_mem(C, out["fin"][w * k.c + i], P, None, "%s: fin[%d][%d]" % (where, w, i), final=True)
                    checked += 1
    assert checked == generated > 0


@pytest.mark.parametrize("curve,name", CURVE_FILES)
def test_untouched_slots(curve, name):
    F = tv.FILES[name](curve)
    outs = outputs(curve, name)
    looked = 0
    for si, sc in enumerate(F.sections):
        lay = layout(curve, name, si)
        for ri, out in enumerate(outs[si]):
            for area in "SMT":
                rows = out[area]
                free = ~lay.written[area]
                assert free.any()                                 # at least the slack entry at the end
                bad = np.nonzero((rows[free] != tv.FILL).any(axis=1))[0]
                assert bad.size == 0, "%s %s section %s run %d: %s entries %s were written, the plan does not write them" % (
                    curve, name, sc.label, ri, area, np.nonzero(free)[0][bad][:8].tolist())
                # ... and what the plan writes was written: the fill is no value of either memory form (a ZZ of 0xA5A5.. exceeds p + eps)
                assert not (rows[lay.written[area]][:, 16:24] == tv.FILL).all(axis=1).any(), "%s %s section %s run %d: %s" % (curve, name, sc.label, ri, area)
                looked += int(free.sum())
            assert not (out["fin"] == tv.FILL).all(axis=1).any()
    assert looked > 0


@pytest.mark.parametrize("curve,name", CURVE_FILES)
def test_same_results_from_every_plan(curve, name):
    """sections over the same windows: fin bit for bit; secp256k1 stores canonical residues, so there every S node both plans store too"""
    F = tv.FILES[name](curve)
    outs, plans = outputs(curve, name), tv.file_plans(curve, name)
    by = {}
    for si, sc in enumerate(F.sections):
        by.setdefault(tuple(id(k) for r in sc.runs for k in r), []).append(si)
    compared = 0
    for members in by.values():
        a = members[0]
        for b in members[1:]:
            sa, sb = F.sections[a], F.sections[b]
            for ri, (oa, ob) in enumerate(zip(outs[a], outs[b])):
                where = "%s %s run %d: sections %s and %s" % (curve, name, ri, sa.label or a, sb.label or b)
                assert np.array_equal(oa["fin"], ob["fin"]), where + ": fin differs"
                compared += 1
                if curve != "secp256k1":
                    continue
                la, lb = layout(curve, name, a), layout(curve, name, b)
                for w, k in enumerate(sa.runs[ri]):
                    (pa, ia), (pb, ib) = tv.part_of(plans[a], w), tv.part_of(plans[b], w)
                    both = set(stored_nodes(plans[a], ia, k)) & set(stored_nodes(plans[b], ib, k))
                    for l, j in both:
                        nw = k.B >> (l + 1)
                        ra = oa["S"][la.s_entry(pa, l, (w - ia["w0"]) * nw + j)]
                        rb = ob["S"][lb.s_entry(pb, l, (w - ib["w0"]) * nw + j)]
                        assert np.array_equal(ra, rb), "%s: window %d S^%d[%d] differs" % (where, w, l, j)
    if name in ("slot", "sparse", "shape", "forced", "bounds"):
        assert compared >= len(F.sections) // 2
    if name == "shape":                                           # lone against not lone
        assert all(len(m) == 2 and F.sections[m[0]].lone != F.sections[m[1]].lone for m in by.values())
    if name in ("slot", "sparse", "forced", "bounds"):            # every forced plan against the product's own
        assert all(F.sections[m[0]].default_plan() for m in by.values())


def test_malformed_files_are_refused(tmp_path):
    """a wrong magic word, a truncated file, c out of range, front2 with l0 < 2, parts = 2 with W = 1, too many buckets: a message
    and status 1, before anything reaches the device"""
    sc = tv.copy_file("bn254").sections[3]                        # c = 3, W = 3, one run
    good = tv.File(ev.BN254, "x", [sc]).words()
    assert good.size == tv.HDR + 3 * 4 * 32 and (int(good[1]), int(good[2])) == (3, 3)

    def refused(words, what):
        fin = str(tmp_path / "in")
        words.tofile(fin)
        r = subprocess.run([tv.EXE, "bn254", fin, str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and what in r.stderr, (r.returncode, r.stderr)

    def header(**kw):
        bad = good.copy()
        for k, v in kw.items():
            bad[dict(magic=0, c=1, W=2, lone=3, parts=4, front2=5, quad=6, l0=7, runs=8, pad=9)[k]] = v
        return bad
    refused(header(magic=tv.MAGIC ^ 1), "not a tree_check file")
    refused(good[:-3], "file ends inside the buckets")
    refused(good[:tv.HDR - 2], "not a tree_check file")
    refused(np.concatenate([good, good[:5]]), "not a tree_check file")           # words behind the last run are no section
    refused(header(c=18), "header out of range")
    refused(header(c=1), "header out of range")
    refused(header(c=17, W=5), "header out of range")                             # more than 2^18 buckets
    refused(header(W=0), "header out of range")
    refused(header(lone=2), "header out of range")
    refused(header(runs=0), "header out of range")
    refused(header(pad=1), "header out of range")
    refused(header(c=4), "file ends inside the buckets")                          # the same words as larger windows
    refused(header(front2=1), "front2 needs l0 >= 2")                             # the product's l0 at c = 3 is 0
    refused(header(front2=1, l0=1), "front2 needs l0 >= 2")
    refused(header(W=1, parts=2), "two parts need at least two windows")
    refused(header(parts=3), "parts must be 1 or 2")
    refused(header(l0=2), "l0 < nlev")

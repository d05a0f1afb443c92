"""GPU: the MAC decode's inverse stage kernels per form (icc_mac_decode.hip.h: k_imd_stage_quad per-butterfly and wave-uniform,
k_imd_stage1_quad) through the driver tools/ladder_check.hip (istage_quad, istage_quad_uniform, istage1_quad), on the operands and
scalars of tests/mac_decode_vectors.py: a scalar table of the test's stands in place of the inverse twiddles, and both outputs
(A, B) -> (A + B, s (A - B)) compare as group elements with form and value bounds (ec_vectors.check_point_mem; infinity is all-zero
words).  Every operand case meets every scalar; rows no live butterfly owns stay bit-identical; padding quads (a butterfly count that
fills no block) and two tables end to end in one work array (the batch's layout) are launches of their own.  Comparison is exact."""
import functools
import os

import pytest

from tests import ec_vectors as ev
from tests import ladder_vectors as lv
from tests import mac_decode_vectors as mv

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bn254", "secp256k1"]


def pairs_for(C, shape, total, uniform, stage1=False):
    """{t: Pair}: butterfly t multiplies by the scalar its table entry holds; the operand case walks with the butterfly's position
    among the readers of that entry, so every scalar meets every case"""
    sc = mv.scalars(C)
    table = {e: sc[i % len(sc)] for i, e in enumerate(shape.entries)}
    seen, pairs = {}, {}
    for t in range(total):
        _, _, e = mv.rows_of(shape, t)
        label, k = table[e]
        i = seen.get(e, 0)
        seen[e] = i + 1
        # per-butterfly form: one reader per entry and table -- the case walks with the entry instead
        case = mv.CASES[(i + (0 if uniform else shape.entries.index(e) // len(sc))) % len(mv.CASES)]
        pairs[t] = mv.Pair(C, label, k, case, t, uniform, stage1)
    return pairs, {e: k for e, (_, k) in table.items()}


@functools.lru_cache(maxsize=None)
def session(curve):
    """one driver process per curve: [(name, output, what the check needs)]"""
    C = ev.CURVES[curve]
    jobs = []
    # per-butterfly form: 64 butterflies that read 64 different entries (8 scalars x 7 cases, and one more round), one whole block;
    # then 40 of them (padding quads), then two tables of 16 rows end to end
    full = lv.per_butterfly_shape(64)
    small = lv.per_butterfly_shape(8)
    for name, shape, tables, total in (("istage_quad full", full, 1, 64), ("istage_quad padded", full, 1, 40),
                                       ("istage_quad two tables", small, 2, 16)):
        pairs, table = pairs_for(C, shape, total, False)
        data, rows = mv.launch(C, shape, tables, pairs, total, table)
        jobs.append(("istage_quad", name, data, (shape, tables, total, pairs, rows, None)))
    # wave-uniform form: one table of 256 rows at the stage where a wave's 16 butterflies share one of 8 entries (16 readers each:
    # every case twice and more); two tables of 64 rows end to end at stage 2 (the smallest uniform launch: 2 entries, whole waves of
    # padding quads in the last block when the table count is odd -- here 64 butterflies, one block)
    for name, shape, tables in (("istage_quad_uniform 256", lv.uniform_shape(16, 8, 256), 1),
                                ("istage_quad_uniform 2 x 64", lv.uniform_shape(16, 2, 64), 2),
                                ("istage_quad_uniform 3 x 64", lv.uniform_shape(16, 2, 64), 3)):
        total = tables * shape.n // 2
        pairs, table = pairs_for(C, shape, total, True)
        data, rows = mv.launch(C, shape, tables, pairs, total, table)
        jobs.append(("istage_quad_uniform", name, data, (shape, tables, total, pairs, rows, table)))
    # stage 1: 24 pairs (no whole block), every case more than three times; the table is not read
    s1 = lv.Shape(16, 1, 8, 1)
    total = 24
    pairs = {t: mv.Pair(C, "stage1", 1, mv.CASES[t % len(mv.CASES)], t, False, True) for t in range(total)}
    data, rows = mv.launch(C, s1, 3, pairs, total, None)
    jobs.append(("istage1_quad", "istage1_quad", data, (s1, 3, total, pairs, rows, None)))
    outs = lv.run(C, [(op, data) for op, _, data, _ in jobs])
    return [(name, out, ctx) for (_, name, _, ctx), out in zip(jobs, outs)]


def test_driver_is_built():
    assert os.path.exists(lv.EXE), "build it with make -C porla_amd/csrc"


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_inverse_stage_forms(curve):
    C = ev.CURVES[curve]
    checked, cases_met = 0, set()
    for name, out, (shape, tables, total, pairs, rows, table) in session(curve):
        uniform = table is not None and name.startswith("istage_quad_uniform")
        (work, codes), = lv.split_stage_output(out, [(shape.n, tables * shape.n)], uniform)
        checked += mv.check(C, work, rows, shape, total, pairs)
        cases_met |= {(name.split()[0], p.label, p.case) for p in pairs.values()}
        if uniform:                                 # the digit codes the wave-uniform form read: the halves of the table's scalars
            for e, k in table.items():
                lv.check_codes_entry(C, codes[e >> lv.CODES_EXP_SHIFT], k, "%s entry %d" % (name, e))
        print("%s %s: %d butterflies" % (curve, name, total))
    labels = [label for label, _ in mv.scalars(C)]
    for form in ("istage_quad", "istage_quad_uniform"):
        for label in labels[:4] + labels[4:5]:      # 1, q - 1, the zero halves, a real inverse twiddle: every operand case
            for case in mv.CASES:
                assert (form, label, case) in cases_met, (form, label, case)
    assert {c for f, _, c in cases_met if f == "istage1_quad"} == set(mv.CASES)
    assert checked == 64 + 40 + 16 + 128 + 64 + 96 + 24

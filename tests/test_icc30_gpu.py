"""GPU: the reduced-radix field helpers of the ICC encode (porla_amd/csrc/icc30.hip.h, icc30_split.hip.h) per operation, at the
operand bounds their comments state, through the driver tools/icc30_check.hip.  Expected values: Python integers
(tests/icc_vectors.py, where the form and every bound are stated).  Comparison is exact -- limb for limb for the products (the value
(a b + m p) / 2^270 is unique), byte for byte for the finish step and the mix; limbs 0..7 of every residue are below 2^30; no record
is skipped (checked == generated is asserted and the count printed) and the named operand families are present whatever the seed."""
import functools
import os

import pytest

from tests import icc_vectors as iv

pytestmark = pytest.mark.gpu

SWEEP = 2000                                   # random records per operation, on top of the listed families
CASES = [(name, op) for name in iv.MODULI for op in iv.ops_of(name)]


def test_driver_is_built():
    assert os.path.exists(iv.EXE), "build it with make -C porla_amd/csrc"


@functools.lru_cache(maxsize=None)
def batch(name):
    """one process per modulus for every operation"""
    ops = iv.ops_of(name)
    gens = [iv.generate(name, op, SWEEP) for op in ops]
    outs = iv.run(name, [(op, recs) for op, (recs, _) in zip(ops, gens)])
    return {op: (recs, out, metas) for op, (recs, metas), out in zip(ops, gens, outs)}


@pytest.mark.parametrize("name,op", CASES, ids=["%s-%s" % c for c in CASES])
def test_helper(name, op):
    recs, out, metas = batch(name)[op]
    iv.assert_families_present(name, op, metas)
    counter = iv.Counter()
    iv.check(name, op, recs, out, metas, counter)
    print("%s %s: %d records checked" % (name, op, counter.checked))
    assert counter.checked == len(metas) == recs.shape[0] > 0

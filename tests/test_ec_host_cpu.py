"""CPU: the 8 x 32-bit group law of porla_amd/csrc/ec.hip.h (xyzz_madd, xyzz_add, xyzz_double, xyzz_double_affine, each with
CALL = false and true), run on the host by `ec30_check --host` -- no HIP call -- over the same vectors tests/test_ec30_gpu.py
feeds the device, against affine chord-and-tangent arithmetic on Python integers (tests/ec_vectors.py).  Exact comparison."""
import os

import numpy as np
import pytest

from tests import ec_vectors as ev

N = 1500


@pytest.mark.parametrize("op", ev.OPS32)
@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
def test_ec_hip_h_on_the_host(curve, op):
    if not os.path.exists(ev.EXE):
        pytest.skip("porla_amd/ec30_check has not been built (make -C porla_amd/csrc)")
    C = ev.CURVES[curve]
    recs, want = ev.gen32(C, op, N, seed=32)
    plain, call = ev.run(C, [(op, recs), (op + "_call", recs)], host=True)
    counter = ev.Counter()
    ev.check32(C, op, plain, want, counter)
    assert counter.checked == len(want) == recs.shape[0] >= N
    assert np.array_equal(plain, call), "CALL = false and CALL = true disagree"
    assert np.array_equal(plain[:, :ev.FO], recs[:, :ev.FO]), "the operands were changed"

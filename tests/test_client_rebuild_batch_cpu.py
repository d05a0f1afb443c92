"""CPU: the client's rebuild write (include/porla_gpu.h: porla_kzg_client_rebuild_batch_device / porla_ipa_client_rebuild_batch_device).
1. The two restatements of tests/client_rebuild_model.py -- the point domain, the reference loop for loop, and the scalar domain the
   library computes in -- agree on every output.  This pins the identity out_j = (s'_j - T_j) * h without the engine.
2. The C ABI: the symbols, the struct layout, every refusal that needs no device, k = 0; and the client update batch still refuses
   CRebuild's step.  Nothing here computes on a device: the pointer values are never dereferenced."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
FAKE = 0x1000
OFFSETS = dict(d_block=0, d_prf=8, d_mac_out=16, d_complements_out=24, write_step=32)
H = {"bn254": (1, 2), "secp256k1": (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
                                    0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)}


# ---- 1. the two models
@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
@pytest.mark.parametrize("n_total,write_step", [(2, 3), (4, 3), (8, 21), (16, 21), (16, 8), (4, 0)])
def test_the_scalar_model_equals_the_point_model(curve, n_total, write_step):
    import icc_py
    from tests.client_rebuild_model import n_prf, rebuild_points, scalar_points
    rnd = random.Random(1000 * n_total + write_step)
    h = icc_py.ec_mul(curve, H[curve], 9)
    block_commit = icc_py.ec_mul(curve, H[curve], rnd.getrandbits(200))
    prf = [rnd.getrandbits(128) for _ in range(n_prf(n_total))]
    mac, out = rebuild_points(curve, n_total, write_step, prf, h, block_commit)
    mac_s, out_s = scalar_points(curve, n_total, write_step, prf, h, block_commit)
    assert mac == mac_s and out == [out_s[g] for g in range(2 * n_total)]
    assert len(out) == 2 * n_total and None not in out


@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
def test_the_models_agree_where_the_first_output_is_infinity(curve):
    """n_total = 2: the network's X[0] is U_0 + U_1, so new_X[0] = s_0 + s_1 makes out[0] infinity"""
    import icc_py
    from tests.client_rebuild_model import rebuild_points, scalar_points
    rnd = random.Random(77)
    h = icc_py.ec_mul(curve, H[curve], 9)
    s0, s1 = rnd.getrandbits(127), rnd.getrandbits(127)
    prf = [rnd.getrandbits(128), s0, s1, s0 + s1] + [rnd.getrandbits(128) for _ in range(3)]
    mac, out = rebuild_points(curve, 2, 3, prf, h, None)
    mac_s, out_s = scalar_points(curve, 2, 3, prf, h, None)
    assert out[0] is None and out[1] is not None
    assert mac == mac_s and out == [out_s[g] for g in range(4)]


# ---- 2. the C ABI
def good(write_step=16, base=0x2000, **kw):
    r = dict(d_block=FAKE, d_prf=FAKE, d_mac_out=base, d_complements_out=base + 0x40, write_step=write_step)
    r.update(kw)
    return tuple(r[f] for f in OFFSETS)


def call(reqs, n_total=16, k=None, null_reqs=False, ipa=None):
    from porla_amd import lib, multiexp as mx
    arr = mx.client_rebuild_requests(reqs)
    a = None if null_reqs else arr
    n = len(reqs) if k is None else k
    if ipa is not None:
        return lib.porla_ipa_client_rebuild_batch_device(ctypes.c_void_p(ipa[0] or None), ctypes.c_void_p(ipa[1] or None), a, n, n_total,
                                                         ctypes.c_void_p(0))
    return lib.porla_kzg_client_rebuild_batch_device(a, n, n_total, ctypes.c_void_p(0))


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def refused(rc, *words):
    assert rc == ERR_ARG
    msg = last_error()
    assert msg and ("porla_kzg_client_rebuild_batch_device" in msg or "porla_ipa_client_rebuild_batch_device" in msg)
    for w in words:
        assert w in msg, msg


def test_the_symbols_are_exported():
    from porla_amd import lib
    assert hasattr(lib, "porla_kzg_client_rebuild_batch_device") and hasattr(lib, "porla_ipa_client_rebuild_batch_device")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_CLIENT_REBUILD_REQ_BYTES, ClientRebuildReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_CLIENT_REBUILD_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(ClientRebuildReq) == size == PORLA_CLIENT_REBUILD_REQ_BYTES == 40
    assert {f: getattr(ClientRebuildReq, f).offset for f, _ in ClientRebuildReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "client_rebuild_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_client_rebuild_req, %s) == %d" % (f, off) in src


def test_the_tile_constant_is_mirrored():
    from porla_amd import multiexp as mx
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "client_rebuild_batch.hip.h")).read()
    log = int(re.search(r"CR_TILE_LOG = (\d+)", src).group(1))
    assert mx.CLIENT_REBUILD_TILE == 1 << log <= 4096


def test_null_reqs_is_refused():
    refused(call([good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("field", ["d_block", "d_prf", "d_mac_out", "d_complements_out"])
def test_a_null_pointer_is_refused(field):
    refused(call([good(), good(base=0x4000, **{field: 0})]), "NULL", "request 1")


@pytest.mark.parametrize("field", ["d_block", "d_prf", "d_mac_out", "d_complements_out"])
def test_a_misaligned_pointer_is_refused(field):
    refused(call([good(**{field: 0x8008})]), "aligned", "request 0")


@pytest.mark.parametrize("n_total", [0, 1, 3, 12, 1000, (1 << 20) + 1])
def test_n_total_not_a_power_of_two_or_below_two_is_refused(n_total):
    refused(call([good()], n_total=n_total), "n_total")


def test_two_requests_naming_one_output_pointer_are_refused():
    a = good(base=0x2000)
    refused(call([a, good(base=0x4000, d_mac_out=a[2])]), "output pointer", "request 1")
    refused(call([a, good(base=0x4000, d_complements_out=a[3])]), "output pointer", "request 1")
    refused(call([a, good(base=0x4000, d_complements_out=a[2])]), "output pointer", "request 1")
    refused(call([good(d_mac_out=0x2000, d_complements_out=0x2000)]), "output pointer", "request 0")
    # the same block or PRF buffer in two requests is the caller's business
    assert call([a, good(base=0x4000)]) != ERR_ARG


def test_ipa_null_bases_are_refused():
    refused(call([good()], ipa=(0, 0)), "NULL base")
    refused(call([good()], ipa=(FAKE, 0)), "NULL base")
    refused(call([good()], ipa=(0, FAKE)), "NULL base")
    # and the shared checks come first on this entry point too
    refused(call([good()], ipa=(0, 0), n_total=12), "n_total")


@pytest.mark.parametrize("write_step", [0, 5, 16, 16 << 20])
def test_any_write_step_is_accepted(write_step):
    assert call([good(write_step=write_step)]) != ERR_ARG


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, null_reqs=True) == 0
    assert call([], k=0, null_reqs=True, ipa=(0, 0)) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments return PORLA_ERR_NO_DEVICE"""
    code = r"""
import sys
sys.path.insert(0, %r)
from porla_amd import lib, multiexp as mx
F = 0x1000
reqs = [(F, F, 0x2000, 0x2040, 16), (F, F, 0x4000, 0x4040, 5)]
print(lib.porla_kzg_client_rebuild_batch_device(mx.client_rebuild_requests(reqs), 2, 16, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(ERR_NO_DEVICE)


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr = mx.client_rebuild_requests([good(write_step=32)])
    assert arr[0].d_block == FAKE and arr[0].d_mac_out == 0x2000 and arr[0].d_complements_out == 0x2040 and arr[0].write_step == 32
    with pytest.raises(ValueError):
        mx.client_rebuild_requests([good()[:4]])
    with pytest.raises(RuntimeError, match="aligned"):
        mx.kzg_client_rebuild_batch_device([good(d_prf=0x1008)], 16)


@pytest.mark.parametrize("write_step", [0, 16, 32])
def test_the_client_update_batch_still_refuses_crebuilds_step(write_step):
    from porla_amd import lib, multiexp as mx
    arr = mx.client_update_requests([(FAKE, FAKE, 0x2000, 0x2040, write_step, 2)])
    assert lib.porla_kzg_client_update_batch_device(arr, 1, 16, None) == ERR_ARG
    assert "CRebuild" in last_error()

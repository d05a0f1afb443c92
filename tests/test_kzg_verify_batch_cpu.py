"""CPU: the batched KZG audit verifier's C ABI (include/porla_gpu.h: porla_kzg_verify_batch_device) -- the symbol is exported, the
ctypes mirror of porla_kzg_verify_req has the layout the library static_asserts, every bad argument is refused with PORLA_ERR_ARG
before the device is touched, k = 0 is a no-op, and valid arguments without a device give PORLA_ERR_NO_DEVICE.  Nothing here
computes on a device: the pointer values are never dereferenced."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from tests import common

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
FAKE = 0x1000
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")
# the offsets porla_kzg_verify_batch_device static_asserts (porla_amd/csrc/kzg_verify_batch.hip)
OFFSETS = dict(d_comp_store=0, d_idx=8, d_coef=16, n=24, alpha=32)


def good(**kw):
    a = dict(d_comp_store=FAKE, d_idx=FAKE, d_coef=FAKE, n=3200, alpha=ALPHA)
    a.update(kw)
    return tuple(a[f] for f in OFFSETS)


def call(verifs, k=None, records=FAKE, weights=None, status=True, reqs=True):
    from porla_amd import lib, multiexp as mx
    arr = mx.kzg_verify_requests(verifs) if reqs else None
    st = ctypes.create_string_buffer(b"\x77" * max(len(verifs), 1)) if status else None
    rc = lib.porla_kzg_verify_batch_device(arr, len(verifs) if k is None else k, ctypes.c_void_p(records or None), weights, st,
                                           ctypes.c_void_p(0))
    if st is not None:
        assert st.raw[:len(verifs)] == b"\x77" * len(verifs), "status written on a refused call"
    return rc


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def test_the_symbol_is_exported():
    from porla_amd import lib
    assert hasattr(lib, "porla_kzg_verify_batch_device")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd import multiexp as mx
    from porla_amd.loader import KzgVerifyReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_KZG_VERIFY_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(KzgVerifyReq) == size == 64
    assert {f: getattr(KzgVerifyReq, f).offset for f, _ in KzgVerifyReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "kzg_verify_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_kzg_verify_req, %s) == %d" % (f, off) in src
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PORLA_KZG_VERIFY_(\w+)\s+(\d+)", header)}
    assert consts == dict(REQ_BYTES=64, MAX_K=10922, FULL=1, PROOF=2, MALFORMED=4)
    assert (mx.KZG_VERIFY_FULL, mx.KZG_VERIFY_PROOF, mx.KZG_VERIFY_MALFORMED, mx.KZG_VERIFY_MAX_K) == (1, 2, 4, 10922)
    assert 3 * mx.KZG_VERIFY_MAX_K <= 32768 < 3 * (mx.KZG_VERIFY_MAX_K + 1)


@pytest.mark.parametrize("field", ["d_comp_store", "d_idx", "d_coef"])
def test_a_null_array_with_a_count_is_refused(field):
    assert call([good(), good(**{field: 0})]) == ERR_ARG
    assert "NULL" in last_error() and "porla_kzg_verify_batch_device" in last_error()
    # with its count 0 the same NULL is fine (the call then gets as far as the next check)
    assert call([good(**{field: 0, "n": 0})], records=0) == ERR_ARG and "d_records" in last_error()


def test_more_than_32768_complements_is_refused():
    assert call([good(n=32769)]) == ERR_ARG
    assert "32768" in last_error()
    assert call([good(n=32768)], records=0) == ERR_ARG and "d_records" in last_error()   # the limit itself passes


def test_null_reqs_records_or_status_is_refused():
    for kw in (dict(records=0), dict(status=False), dict(reqs=False)):
        assert call([good()], k=1, **kw) == ERR_ARG and "NULL" in last_error()


def test_an_all_zero_weight_is_refused():
    w = (1).to_bytes(16, "big") + bytes(16) + (1 << 127).to_bytes(16, "big")
    assert call([good(), good(), good()], weights=w) == ERR_ARG
    assert "zero weight" in last_error()
    assert call([good()], weights=bytes(16)) == ERR_ARG and "zero weight" in last_error()


def test_k_above_the_folded_entry_limit_is_refused():
    """P holds 3 pairs per reply in one batched-MSM entry of at most 32 768: k <= 10 922, checked before the array is read"""
    many = [good(n=0)] * 10923
    assert call(many) == ERR_ARG and "10922" in last_error()
    assert call(many[:10922], records=0) == ERR_ARG and "d_records" in last_error()   # the limit itself passes
    assert call([good()], k=(1 << 62), reqs=True) == ERR_ARG and "10922" in last_error()


def test_k_zero_returns_zero():
    from porla_amd import lib
    assert call([], k=0) == 0
    assert lib.porla_kzg_verify_batch_device(None, 0, None, None, None, None) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (an empty challenge and caller weights included) return
    PORLA_ERR_NO_DEVICE and leave status untouched"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, multiexp as mx
F = 0x1000
verifs = [(F, F, F, 3200, b"\x01" * 16), (0, 0, 0, 0, b""), (F, F, F, 32768, b"\xff" * 32)]
st = ctypes.create_string_buffer(b"\x77" * 3)
rc = lib.porla_kzg_verify_batch_device(mx.kzg_verify_requests(verifs), 3, ctypes.c_void_p(F), None, st, None)
rc2 = lib.porla_kzg_verify_batch_device(mx.kzg_verify_requests(verifs), 3, ctypes.c_void_p(F), b"\x05" * 48, st, None)
print(rc, rc2, st.raw[:3].hex())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE), str(ERR_NO_DEVICE), "777777"]


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr = mx.kzg_verify_requests([good(alpha=ALPHA), good(d_comp_store=0, d_idx=0, d_coef=0, n=0, alpha=b"\x01" * 32)])
    assert arr[0].d_comp_store == FAKE and arr[0].n == 3200
    assert bytes(arr[0].alpha) == bytes(16) + ALPHA                      # SECRET_KEY in bytes 16..31 (Client.hpp:851-853)
    assert arr[1].d_idx is None and arr[1].n == 0 and bytes(arr[1].alpha) == b"\x01" * 32
    with pytest.raises(ValueError):
        mx.kzg_verify_requests([good()[:4]])
    with pytest.raises(ValueError):
        mx.kzg_verify_requests([good(alpha=bytes(33))])
    with pytest.raises(ValueError):
        mx.kzg_verify_batch_device([good()], FAKE, weights=[1, 2])
    with pytest.raises(RuntimeError, match="32768"):
        mx.kzg_verify_batch_device([good(n=40000)], FAKE)
    with pytest.raises(RuntimeError, match="zero weight"):
        mx.kzg_verify_batch_device([good()], FAKE, weights=[0])

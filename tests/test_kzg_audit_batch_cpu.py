"""CPU: the batched KZG audit's C ABI (include/porla_gpu.h: porla_kzg_audit_batch_device) -- the symbol is exported, the ctypes
mirror of porla_kzg_audit_req has the layout the library static_asserts, every bad argument is refused with PORLA_ERR_ARG before
the device is touched, k = 0 is a no-op, and valid arguments without a device give PORLA_ERR_NO_DEVICE.  Nothing here computes on a
device: the pointer values are never dereferenced."""
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
# the offsets porla_kzg_audit_batch_device static_asserts (porla_amd/csrc/kzg_audit_batch.hip)
OFFSETS = dict(d_rows64=0, d_idx64=8, d_coef64=16, n64=24, d_rows32=32, d_idx32=40, d_coef32=48, n32=56, d_mac_store=64,
               d_align_store=72, d_mac_idx=80, d_mac_coef=88, n_macs=96, random_point=104)


def good(**kw):
    a = dict(d_rows64=FAKE, d_idx64=FAKE, d_coef64=FAKE, n64=100, d_rows32=FAKE, d_idx32=FAKE, d_coef32=FAKE, n32=20,
             d_mac_store=FAKE, d_align_store=FAKE, d_mac_idx=FAKE, d_mac_coef=FAKE, n_macs=120, random_point=7)
    a.update(kw)
    return tuple(a[f] for f in OFFSETS)


def call(audits, k=None, out=FAKE, b=0, reqs=True):
    from porla_amd import lib, multiexp as mx
    arr = mx.kzg_audit_requests(audits) if reqs else None
    return lib.porla_kzg_audit_batch_device(arr, len(audits) if k is None else k, ctypes.c_void_p(out or None), ctypes.c_void_p(b or None),
                                            ctypes.c_void_p(0))


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def test_the_symbol_is_exported():
    from porla_amd import lib
    assert hasattr(lib, "porla_kzg_audit_batch_device")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import KzgAuditReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_KZG_AUDIT_REQ_BYTES\s+(\d+)", header).group(1))
    record = int(re.search(r"#define PORLA_KZG_AUDIT_RECORD_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(KzgAuditReq) == size == 112 and record == 320
    assert {f: getattr(KzgAuditReq, f).offset for f, _ in KzgAuditReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "kzg_audit_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_kzg_audit_req, %s) == %d" % (f, off) in src


@pytest.mark.parametrize("field,counts", [
    ("d_rows64", "n64"), ("d_idx64", "n64"), ("d_coef64", "n64"),
    ("d_rows32", "n32"), ("d_idx32", "n32"), ("d_coef32", "n32"),
    ("d_mac_store", "n_macs"), ("d_align_store", "n_macs"), ("d_mac_idx", "n_macs"), ("d_mac_coef", "n_macs")])
def test_a_null_array_with_a_count_is_refused(field, counts):
    assert call([good(), good(**{field: 0})]) == ERR_ARG
    assert "NULL" in last_error() and "porla_kzg_audit_batch_device" in last_error()
    # with its count 0 the same NULL is fine (the call then needs a device)
    assert call([good(**{field: 0, counts: 0})], out=0) == ERR_ARG and "d_out" in last_error()


def test_more_than_32768_macs_is_refused():
    assert call([good(n_macs=32769)]) == ERR_ARG
    assert "32768" in last_error() and "porla_kzg_audit_device" in last_error()
    assert call([good(n_macs=32768)], out=0) == ERR_ARG and "d_out" in last_error()     # the limit itself passes the size check


def test_row_counts_at_or_above_2_to_32_are_refused():
    for n64, n32 in ((1 << 32, 0), (0, 1 << 32), ((1 << 31), (1 << 31)), ((1 << 32) - 1, 1), ((1 << 64) - 1, 2)):
        assert call([good(n64=n64, n32=n32)]) == ERR_ARG
        assert "2^32" in last_error()


def test_null_reqs_or_out_is_refused():
    assert call([good()], out=0) == ERR_ARG and "NULL" in last_error()
    assert call([good()], reqs=False, k=1) == ERR_ARG and "NULL" in last_error()


def test_a_batch_whose_byte_size_overflows_is_refused():
    # k records of 320 bytes past 2^64 (the count is checked before the array is read)
    assert call([good()], k=(1 << 62), reqs=False) == ERR_ARG
    assert call([good()], k=(1 << 62)) == ERR_ARG and "overflow" in last_error()


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, out=0, reqs=False) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (empty challenges and no MACs included) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, multiexp as mx
F = 0x1000
audits = [(F, F, F, 3200, 0, 0, 0, 0, F, F, F, F, 3200, 5), (0, 0, 0, 0, F, F, F, 10, 0, 0, 0, 0, 0, 0),
          (0, 0, 0, 0, 0, 0, 0, 0, F, F, F, F, 32768, (1 << 64) - 1)]
rc = lib.porla_kzg_audit_batch_device(mx.kzg_audit_requests(audits), 3, ctypes.c_void_p(F), None, None)
print(rc)
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(ERR_NO_DEVICE)


def test_python_mirror_builds_requests_and_splits_records():
    from porla_amd import multiexp as mx
    arr = mx.kzg_audit_requests([good(n64=5, random_point=(1 << 64) - 1), good(d_rows32=0, n32=0)])
    assert arr[0].n64 == 5 and arr[0].random_point == (1 << 64) - 1 and arr[0].d_rows64 == FAKE
    assert arr[1].d_rows32 is None and arr[1].n32 == 0
    with pytest.raises(ValueError):
        mx.kzg_audit_requests([good()[:13]])
    raw = b"".join(bytes([i]) * 320 for i in range(3))
    recs = mx.split_audit_records(raw, 3)
    assert [r["commitment"] for r in recs] == [bytes([i]) * 64 for i in range(3)]
    assert recs[2]["point"] == bytes([2]) * 32 and recs[1]["combined_align"] == bytes([1]) * 64
    with pytest.raises(RuntimeError, match="32768"):
        mx.kzg_audit_batch_device([good(n_macs=40000)], FAKE)

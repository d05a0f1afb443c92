"""CPU: the batched MSM's C ABI (include/porla_gpu.h: porla_*_msm_batch_device / _host) -- the four symbols are exported, every bad
argument is refused with PORLA_ERR_ARG before the device is touched, k = 0 is a no-op, and valid arguments without a device give
PORLA_ERR_NO_DEVICE; the Python mirror's offsets and output split.  Nothing here computes on a device: the argument cases use
pointer values that are never dereferenced."""
import ctypes
import os
import subprocess
import sys

import pytest

from tests import common

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
CURVES = ("bn254", "secp256k1")
FAKE = 0x1000          # a non-null pointer value for the device arguments (the checks refuse the call before any use)


def offs(*values):
    return (ctypes.c_uint64 * len(values))(*values)


def call_device(curve, offsets, k, sc=FAKE, pt=FAKE, out=FAKE):
    from porla_amd import lib
    fn = getattr(lib, "porla_%s_msm_batch_device" % curve)
    return fn(ctypes.c_void_p(sc), ctypes.c_void_p(pt), offsets, k, ctypes.c_void_p(out), ctypes.c_void_p(0))


def call_host(curve, offsets, k, n_pairs=0, out_len=None, sc=True, pt=True, out=True):
    from porla_amd import lib
    fn = getattr(lib, "porla_%s_msm_batch_host" % curve)
    buf = ctypes.create_string_buffer(out_len if out_len is not None else max(64 * k, 1))
    return fn(bytes(32 * n_pairs) if sc else None, bytes(64 * n_pairs) if pt else None, offsets, k, buf if out else None), buf


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def test_the_four_symbols_are_exported():
    from porla_amd import lib
    for curve in CURVES:
        for form in ("device", "host"):
            assert hasattr(lib, "porla_%s_msm_batch_%s" % (curve, form))


@pytest.mark.parametrize("curve", CURVES)
def test_offsets_not_starting_at_zero_are_refused(curve):
    assert call_device(curve, offs(1, 2, 3), 2) == ERR_ARG
    assert "start at 0" in last_error()
    assert call_host(curve, offs(1, 2, 3), 2, n_pairs=3)[0] == ERR_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_decreasing_offsets_are_refused(curve):
    assert call_device(curve, offs(0, 5, 4, 9), 3) == ERR_ARG
    assert "non-decreasing" in last_error()
    assert call_host(curve, offs(0, 5, 4, 9), 3, n_pairs=9)[0] == ERR_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_an_entry_above_32768_pairs_is_refused_and_names_the_large_msm_call(curve):
    assert call_device(curve, offs(0, 3, 3 + 32768, 3 + 32769 + 32768), 3) == ERR_ARG
    msg = last_error()
    assert "32768" in msg and ("porla_%s_msm_device" % curve) in msg and "entry 2" in msg
    # exactly the limit passes the checks (and then needs a device or is refused for another reason, never for its size)
    assert call_device(curve, offs(0, 32768), 1, out=0) == ERR_ARG and "null" in last_error()
    assert call_host(curve, offs(0, 32769), 1, n_pairs=32769)[0] == ERR_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_null_pointers_are_refused_when_there_is_work(curve):
    assert call_device(curve, offs(0, 1), 1, sc=0) == ERR_ARG
    assert call_device(curve, offs(0, 1), 1, pt=0) == ERR_ARG
    assert call_device(curve, offs(0, 1), 1, out=0) == ERR_ARG
    assert call_device(curve, offs(0, 0), 1, out=0) == ERR_ARG       # an empty entry still has an output to write
    assert call_device(curve, None, 1) == ERR_ARG
    assert call_host(curve, offs(0, 2), 1, n_pairs=2, sc=False)[0] == ERR_ARG
    assert call_host(curve, offs(0, 2), 1, n_pairs=2, pt=False)[0] == ERR_ARG
    assert call_host(curve, offs(0, 2), 1, n_pairs=2, out=False)[0] == ERR_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_offsets_near_the_top_of_the_range_are_refused_by_the_entry_limit(curve):
    # a total whose byte size (64 per pair) would overflow needs an entry above 32 768 pairs (or more than 2^43 entries): the entry
    # limit refuses it before any pointer is used
    for top in ((1 << 64) - 1, 1 << 60, 1 << 58):
        assert call_device(curve, offs(0, top), 1) == ERR_ARG
        assert "32768" in last_error() and "entry 0" in last_error()
    assert call_host(curve, offs(0, 1 << 58), 1)[0] == ERR_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_k_zero_returns_zero_and_writes_nothing(curve):
    assert call_device(curve, offs(0), 0) == 0
    assert call_device(curve, None, 0, sc=0, pt=0, out=0) == 0
    rc, buf = call_host(curve, offs(0), 0, out_len=16)
    assert rc == 0 and buf.raw == bytes(16)
    from porla_amd import multiexp as mx
    assert mx.msm_batch_host(curve, b"", b"", [0]) == []


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device (this machine may have one): every valid call returns PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib
offs = (ctypes.c_uint64 * 4)(0, 1, 1, 40)
rcs = []
for curve in ("bn254", "secp256k1"):
    rcs.append(getattr(lib, "porla_%%s_msm_batch_device" %% curve)(ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1000), offs, 3,
                                                                    ctypes.c_void_p(0x1000), ctypes.c_void_p(0)))
    out = ctypes.create_string_buffer(3 * 64)
    rcs.append(getattr(lib, "porla_%%s_msm_batch_host" %% curve)(bytes(32 * 40), bytes(64 * 40), offs, 3, out))
    assert out.raw == bytes(3 * 64)
print(rcs)
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str([ERR_NO_DEVICE] * 4)


def test_python_mirror_builds_offsets_and_splits_outputs():
    from porla_amd import multiexp as mx
    assert mx.batch_offsets([]) == [0]
    assert mx.batch_offsets([0, 1, 2, 3, 17]) == [0, 0, 1, 3, 6, 23]
    with pytest.raises(ValueError):
        mx.batch_offsets([3, -1])
    raw = b"".join(bytes([i]) * 64 for i in range(5))
    parts = mx.split_outputs(raw, 5)
    assert len(parts) == 5 and all(p == bytes([i]) * 64 for i, p in enumerate(parts))
    assert mx.split_outputs(raw, 0) == []
    with pytest.raises(ValueError):
        mx.split_outputs(raw, 6)
    # the mirror hands the C ABI the offsets it was given (checked there): a bad array is refused with the library's message
    with pytest.raises(RuntimeError, match="start at 0"):
        mx.msm_batch_host("bn254", bytes(32), bytes(64), [1, 1])
    with pytest.raises(RuntimeError, match="non-decreasing"):
        mx.msm_batch_device("secp256k1", FAKE, FAKE, [0, 2, 1], FAKE)

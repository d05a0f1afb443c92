"""CPU: the C ABI of the ragged ICC decode (include/porla_gpu.h: porla_icc_decode_ragged_batch_device) without a device: the symbol is
exported, the request has the layout the library static_asserts, every bad argument is refused with PORLA_ERR_ARG before the device is
touched -- n_rows judged per request, the overlap rule applied with each request's own byte sizes -- k = 0 returns 0 and valid
arguments without a device give PORLA_ERR_NO_DEVICE.  Nothing here computes on a device: the pointer values are never dereferenced."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from tests import common

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
WHO = "porla_icc_decode_ragged_batch_device"
FIELDS = ("d_rows", "d_out", "d_write_steps", "d_bad")


def good(base=0x1000000, n_rows=16, steps=False, bad=False):
    """one request as icc.decode_ragged_requests takes it: fake, far apart, aligned addresses"""
    return (base, base + 0x400000, base + 0x800000 if steps else 0, base + 0xa00000 if bad else 0, n_rows)


def call(reqs, n_cols=128, n_total=16, curve=0, form=0, k=None, null_reqs=False):
    from porla_amd import icc, lib
    arr = icc.decode_ragged_requests(reqs)
    return lib.porla_icc_decode_ragged_batch_device(None if null_reqs else arr, len(reqs) if k is None else k, n_cols, n_total, curve, form,
                                                    ctypes.c_void_p(0))


def refused(rc, *words):
    from porla_amd import lib
    assert rc == ERR_ARG
    msg = lib.porla_gpu_last_error().decode()
    assert msg and WHO in msg
    for w in words:
        assert w in msg, msg


def test_the_symbol_is_exported():
    from porla_amd import lib
    assert hasattr(lib, WHO)


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_ICC_DECODE_RAGGED_REQ_BYTES, IccDecodeRaggedReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_ICC_DECODE_RAGGED_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(IccDecodeRaggedReq) == size == PORLA_ICC_DECODE_RAGGED_REQ_BYTES == 40
    offsets = {f: 8 * i for i, f in enumerate(FIELDS + ("n_rows",))}
    assert offsets["n_rows"] == 32
    assert {f: getattr(IccDecodeRaggedReq, f).offset for f, _ in IccDecodeRaggedReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "icc_decode.hip")).read()
    for f, off in offsets.items():
        assert "offsetof(porla_icc_decode_ragged_req, %s) == %d" % (f, off) in src


def test_null_reqs_is_refused():
    refused(call([good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("field", ["d_rows", "d_out"])
def test_a_null_rows_or_out_pointer_is_refused(field):
    r = list(good(base=0x3000000, n_rows=4))
    r[FIELDS.index(field)] = 0
    refused(call([good(), tuple(r)]), "NULL", "request 1")


@pytest.mark.parametrize("field,off,form,word", [("d_rows", 8, 0, "16-byte"), ("d_out", 8, 0, "16-byte"), ("d_write_steps", 4, 1, "8-byte"),
                                                 ("d_bad", 2, 0, "4-byte")])
def test_a_misaligned_pointer_is_refused(field, off, form, word):
    r = list(good(base=0x3000000, n_rows=2, steps=form == 1, bad=form == 0))
    r[FIELDS.index(field)] += off
    refused(call([good(), tuple(r)], form=form), word, "request 1")
    assert call([good(), good(base=0x3000000, n_rows=2, steps=form == 1, bad=form == 0)], form=form) != ERR_ARG


@pytest.mark.parametrize("n_rows", [0, 1, 3, 12, 32, 1 << 17])
def test_a_bad_n_rows_is_refused(n_rows):
    """0, 1, 3 and 2 * n_total among them; judged per request: the request in front is fine"""
    refused(call([good(n_rows=8), good(base=0x3000000, n_rows=n_rows)], n_total=16), "n_rows", "request 1")
    refused(call([good(n_rows=n_rows)], n_total=16), "n_rows", "request 0")


def test_every_size_up_to_n_total_passes_the_checks():
    reqs = [good(base=0x100000000 * (l + 1), n_rows=1 << l) for l in range(1, 17)]
    assert call(reqs, n_cols=1, n_total=1 << 16) != ERR_ARG
    assert call([good(n_rows=2)], n_total=2) != ERR_ARG


@pytest.mark.parametrize("n_total", [0, 1, 3, 1000, (1 << 16) + 1, 1 << 17])
def test_a_bad_n_total_is_refused(n_total):
    refused(call([good(n_rows=2)], n_total=n_total), "n_total")


@pytest.mark.parametrize("n_cols", [0, 65536, 1 << 20])
def test_a_bad_n_cols_is_refused(n_cols):
    refused(call([(0x1000000, 0x4000000000, 0, 0, 16)], n_cols=n_cols), "n_cols")


@pytest.mark.parametrize("curve", [-1, 2, 7])
def test_a_bad_curve_is_refused(curve):
    refused(call([good()], curve=curve), "curve")


@pytest.mark.parametrize("form", [-1, 3, 9])
def test_a_bad_form_is_refused(form):
    refused(call([good()], form=form), "form")


def test_write_steps_and_bad_go_with_their_forms_only():
    refused(call([good(), good(base=0x3000000, n_rows=4, steps=True)], form=0), "d_write_steps", "request 1")
    for form in (1, 2):
        refused(call([good(bad=True)], form=form), "d_bad", "request 0")
        assert call([good(steps=True), good(base=0x3000000, n_rows=4)], form=form) != ERR_ARG
    assert call([good(bad=True), good(base=0x3000000, n_rows=4)], form=0) != ERR_ARG


def test_an_output_overlapping_anything_is_refused():
    n_cols = 128
    big, small = 16, 2                                            # rows of the two requests
    in_big, out_big = big * n_cols * 64, big * n_cols * 32
    in_small, out_small = small * n_cols * 64, small * n_cols * 32
    a = good(n_rows=big)
    b = good(base=0x5000000, n_rows=small)
    assert call([a, b]) != ERR_ARG
    # one request: in place, the tail of the input, the head of the output -- with its own sizes
    for n, in_b, out_b in ((big, in_big, out_big), (small, in_small, out_small)):
        refused(call([(a[0], a[0], 0, 0, n)]), "overlaps")
        refused(call([(a[0], a[0] + in_b - 16, 0, 0, n)]), "overlaps")
        refused(call([(a[0], a[0] - out_b + 16, 0, 0, n)]), "overlaps")
        assert call([(a[0], a[0] + in_b, 0, 0, n)]) != ERR_ARG    # back to back is fine
        assert call([(a[0], a[0] - out_b, 0, 0, n)]) != ERR_ARG
    # the small request's output inside the LARGE request's input: its last 16 bytes lie beyond what a request of the small size
    # would read there, so only the large request's own byte size sees the overlap ...
    inside = a[0] + in_big - 16
    assert inside >= a[0] + in_small
    refused(call([a, (b[0], inside, 0, 0, small)]), "overlaps")
    refused(call([(b[0], inside, 0, 0, small), a]), "overlaps")
    assert call([(a[0], a[1], 0, 0, small), (b[0], inside, 0, 0, small)]) != ERR_ARG     # (both small: nothing is read there)
    # ... and the large request's output over the small request's input, which begins inside its last bytes
    refused(call([(a[0], a[1], 0, 0, big), (a[1] + out_big - 16, b[1], 0, 0, small)]), "overlaps")
    assert call([(a[0], a[1], 0, 0, small), (a[1] + out_big - 16, b[1], 0, 0, small)]) != ERR_ARG
    # two outputs; the counter inside an output; two requests sharing a counter
    refused(call([a, (b[0], a[1] + out_big - 32, 0, 0, small)]), "overlaps")
    refused(call([a, (b[0], b[1], 0, a[1] + out_big - 4, small)]), "overlaps")
    refused(call([good(n_rows=big, bad=True), (b[0], b[1], 0, good(bad=True)[3], small)]), "overlaps")
    # the write steps are as long as their request: an output behind the small request's steps is fine, inside the large one's not
    st = 0x9000000
    assert call([(a[0], a[1], st, 0, small), (b[0], st + 8 * small, 0, 0, small)], form=1) != ERR_ARG
    refused(call([(a[0], a[1], st, 0, big), (b[0], st + 8 * small, 0, 0, small)], form=1), "overlaps")
    # two requests may read the same rows and the same steps
    assert call([a, (a[0], b[1], 0, 0, small)]) != ERR_ARG
    assert call([(a[0], a[1], st, 0, big), (b[0], b[1], st, 0, small)], form=1) != ERR_ARG
    # the 32-byte form's input is half as long
    assert call([(a[0], a[0] + out_big, 0, 0, big)], form=2) != ERR_ARG
    refused(call([(a[0], a[0] + out_big, 0, 0, big)], form=1), "overlaps")


def test_too_many_requests_are_refused():
    from porla_amd import lib
    from porla_amd.loader import IccDecodeRaggedReq
    k = 65536
    arr = (IccDecodeRaggedReq * k)()
    for i in range(k):
        arr[i] = IccDecodeRaggedReq(0x10000000 + 0x1000 * i, 0x40000000 + 0x1000 * i, None, None, 2)
    refused(lib.porla_icc_decode_ragged_batch_device(arr, k, 1, 2, 0, 0, None), "65535")
    assert lib.porla_icc_decode_ragged_batch_device(arr, k - 1, 1, 2, 0, 0, None) != ERR_ARG


def test_a_byte_size_that_overflows_is_refused():
    refused(call([good()], n_total=1 << 16, n_cols=1 << 60), "overflow")
    refused(call([good()], n_total=1 << 16, n_cols=(1 << 56) + 1), "overflow")
    refused(call([((1 << 64) - (1 << 16), 0x1000, 0, 0, 16)]), "overflow")        # the rows wrap around the address space
    refused(call([good(), (0x1000, (1 << 64) - (1 << 12), 0, 0, 2)]), "overflow", "request 1")


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, null_reqs=True) == 0
    assert call([], k=0, null_reqs=True, curve=1, form=2) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both curves, the three forms, mixed sizes) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, icc
def req(base, n, steps, bad):
    return (base, base + 0x400000, base + 0x800000 if steps else 0, base + 0xa00000 if bad else 0, n)
for curve in (0, 1):
    for form in (0, 1, 2):
        reqs = [req(0x1000000, 2, form != 0, form == 0), req(0x3000000, 32, False, False), req(0x5000000, 16, form == 2, False)]
        print(lib.porla_icc_decode_ragged_batch_device(icc.decode_ragged_requests(reqs), 3, 128, 32, curve, form, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 6


def test_python_mirror_builds_requests():
    from porla_amd import icc
    arr = icc.decode_ragged_requests([good(bad=True), good(base=0x3000000, n_rows=512, steps=True)])
    assert arr[0].d_rows == 0x1000000 and arr[0].d_out == 0x1400000 and arr[0].d_write_steps is None and arr[0].d_bad == 0x1a00000
    assert arr[0].n_rows == 16 and arr[1].n_rows == 512 and arr[1].d_write_steps == 0x3800000 and arr[1].d_bad is None
    with pytest.raises(ValueError):
        icc.decode_ragged_requests([good()[:4]])
    with pytest.raises(RuntimeError, match="n_rows"):
        icc.decode_ragged_batch_device([good(n_rows=3)], 128, 16, "bn254", "exact")
    with pytest.raises(KeyError):
        icc.decode_ragged_batch_device([good()], 128, 16, "bn254", "nearly")

"""CPU: the ICC MAC decode without a device.  The model the GPU tests compare against (tests/mac_decode_model.py) inverts the oracle's
MAC network (icc_py.mac_crebuild, both parts) and the chains of icc_py.mac_mix that build a level, with per-row write steps and
n_total > n_rows; every inverse twiddle times its twiddle is 1 mod q at n_total = 2^16; the vectors of the stage checks build; and the
C ABI (include/porla_gpu.h: porla_icc_mac_decode_batch_device / porla_icc_mac_decode_host) exports its symbols, has the layout the
library static_asserts, refuses every bad argument with PORLA_ERR_ARG before the device is touched, returns 0 for k = 0 and
PORLA_ERR_NO_DEVICE for valid arguments without a device.  Nothing here computes on a device: the pointer values are never
dereferenced."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
import icc_py
from tests import mac_decode_model as model

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
WHO = "porla_icc_mac_decode_batch_device"
CURVES = ("bn254", "secp256k1")
P = icc_py.P_ICC


def some_macs(n, curve, seed):
    """n points: small multiples of the generator, infinity at position 1 when there is room"""
    rng = random.Random(seed)
    g = model.GEN[curve]
    macs = [icc_py.ec_mul(curve, g, rng.randrange(1, 1 << 20)) for _ in range(n)]
    if n > 2:
        macs[1] = None
    return macs


# ---- the model against the oracle's encode
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_model_inverts_mac_crebuild(curve, n):
    macs = some_macs(n, curve, 31 * n)
    X, Y = icc_py.mac_crebuild(macs, curve, 0)
    assert model.decode(X, curve) == macs
    assert Y == X                                                   # write step 0: wt = 1
    # a write step with step % n != 0: the Y part is the network over wt * MAC, one wt for every row
    step = n + 1 if n > 2 else 3
    assert step % n != 0
    X, Y = icc_py.mac_crebuild(macs, curve, step)
    assert Y != X
    assert model.decode(X, curve) == macs
    assert model.decode(Y, curve, n, [step] * n) == macs
    # ... and the byte forms
    assert model.decode_bytes(model.points_to_bytes(Y), n, n, curve, [step] * n) == model.points_to_bytes(macs)
    assert model.bytes_to_points(model.points_to_bytes(macs), curve) == macs


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("level,n_total", [(1, 8), (2, 8), (3, 16), (2, 64)])
def test_model_on_levels(curve, level, n_total):
    """a level as the update path builds it (icc_py.mac_mix chains, n_total > n_rows): the X half decodes to the per-block MACs in
    write order, the Y half with the write steps hadd used too; without them to wt_i * MAC_i"""
    n = 1 << level
    macs = some_macs(n, curve, 7 * level + n_total)
    steps = [n_total + 3 + i for i in range(n)]
    X = model.level_x(macs, n_total, curve)
    Y = model.level_y(macs, steps, n_total, curve)
    assert len(X) == n and len(Y) == n
    assert model.decode(X, curve, n_total) == macs
    assert model.decode(Y, curve, n_total, steps) == macs
    assert model.decode(Y, curve, n_total) == [icc_py.hadd([], m, n_total, s, curve)[2] for m, s in zip(macs, steps)]
    # the network itself does not depend on n_total
    if level > 1:
        assert model.decode(X, curve, n_total) == model.decode(X, curve, n)


@pytest.mark.parametrize("curve", CURVES)
def test_model_subtracts_the_complements(curve):
    n = 8
    macs = some_macs(n, curve, 5)
    comp = some_macs(n, curve, 6)
    X, _ = icc_py.mac_crebuild(macs, curve, 0)
    stored = [icc_py.ec_add(curve, x, c) for x, c in zip(X, comp)]
    assert model.decode(stored, curve, sub=comp) == macs
    assert model.decode(stored, curve, sub=stored) == [None] * n


@pytest.mark.parametrize("curve", CURVES)
def test_model_sees_a_tampered_row(curve):
    """linearity: one altered row changes every row of the output"""
    n = 8
    macs = some_macs(n, curve, 9)
    X, _ = icc_py.mac_crebuild(macs, curve, 0)
    X[5] = icc_py.ec_add(curve, X[5], model.GEN[curve])
    out = model.decode(X, curve)
    assert all(o != m for o, m in zip(out, macs))


# ---- the twiddles
@pytest.mark.parametrize("curve", CURVES)
def test_every_inverse_twiddle_times_its_twiddle_is_one(curve):
    N, q = 1 << 16, icc_py.Q[curve]
    rng = random.Random(16)
    exps = [0, 1, 2, 31, 32, N // 2 - 1, N // 2, N // 2 + 1, N - 1] + [rng.randrange(N) for _ in range(200)]
    for e in exps:
        assert model.inverse_twiddle(e, N, curve) * (model.twiddle(e, N) % q) % q == 1
    assert model.inverse_twiddle(0, N, curve) == 1                  # j = 0 of every stage: the ladder multiplies by 1
    # the exponent of stage s, row j does not depend on which table it is read from
    for n in (4, 64, 1 << 10):
        for s in (1, 2, n.bit_length() - 1):
            j = (1 << (s - 1)) - 1
            assert model.twiddle(j * (n >> (s - 1)), n) == model.twiddle(j * (N >> (s - 1)), N)
    # the per-row scalar: one factor n^-1, times wt^-1
    for n, step in ((2, None), (1 << 16, None), (16, 21), (64, N + 5)):
        s = model.row_scalar(n, curve, step, N)
        assert s * n * (model.wt_of(step, N) % q if step is not None else 1) % q == 1


def test_the_stage_vectors_build():
    """tests/mac_decode_vectors.py: the scalars split as they are named, and an inverse butterfly's expectation is the butterfly's
    inverse"""
    from tests import ec_vectors as ev
    from tests import ladder_vectors as lv
    from tests import mac_decode_vectors as mv
    for C in ev.CURVES.values():
        sc = dict(mv.scalars(C))
        q = lv.order(C)
        assert sc["one"] == 1 and sc["minus_one"] == q - 1
        assert lv.split(C, sc["second_half_zero"])[1][0] == 0 and lv.split(C, sc["first_half_zero"])[0][0] == 0
        assert mv.passes_through(C, 1, False) and mv.passes_through(C, 1, True) and not mv.passes_through(C, sc["first_half_zero"], True)
        k = sc["inverse_twiddle_12345"]
        for i, case in enumerate(mv.CASES):
            p = mv.Pair(C, "t", k, case, i, False)
            # forward butterfly with the twiddle k^-1 on (sum / 2, prod / 2) gives (A, B) back
            half, tw = pow(2, -1, q), pow(k, -1, q)
            a2 = None if p.sum is None else ev.ec_mul(C, half, p.sum)
            b2 = None if p.prod is None else ev.ec_mul(C, half * tw % q, p.prod)
            assert ev.ec_add(C, a2, b2) == p.A and ev.ec_add(C, a2, ev.ec_neg(C, b2)) == p.B, case
        raw, pt = mv.noncanonical_bytes(C)
        assert ev.on_curve(C, pt) and int.from_bytes(raw[:32], "big") >= C.p
        assert model.bytes_to_points(raw, C.name) == [pt]


# ---- the C ABI
FIELDS = ("d_macs", "d_out", "d_write_steps", "d_sub")


def good(base=0x1000000, steps=False, sub=False):
    """one request as icc.mac_decode_requests takes it: fake, far apart, aligned addresses"""
    return (base, base + 0x400000, base + 0x800000 if steps else 0, base + 0xa00000 if sub else 0)


def call(reqs, n_rows=16, n_total=16, curve=0, k=None, null_reqs=False):
    from porla_amd import icc, lib
    arr = icc.mac_decode_requests(reqs)
    return lib.porla_icc_mac_decode_batch_device(None if null_reqs else arr, len(reqs) if k is None else k, n_rows, n_total, curve,
                                                 ctypes.c_void_p(0))


def refused(rc, *words):
    from porla_amd import lib
    assert rc == ERR_ARG
    msg = lib.porla_gpu_last_error().decode()
    assert msg and WHO in msg
    for w in words:
        assert w in msg, msg


def test_the_symbols_are_exported():
    from porla_amd import lib
    assert hasattr(lib, WHO) and hasattr(lib, "porla_icc_mac_decode_host")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_ICC_MAC_DECODE_REQ_BYTES, IccMacDecodeReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_ICC_MAC_DECODE_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(IccMacDecodeReq) == size == PORLA_ICC_MAC_DECODE_REQ_BYTES == 32
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert {f: getattr(IccMacDecodeReq, f).offset for f, _ in IccMacDecodeReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "icc_mac_decode.hip")).read()
    for f, off in offsets.items():
        assert "offsetof(porla_icc_mac_decode_req, %s) == %d" % (f, off) in src


def test_null_reqs_is_refused():
    refused(call([good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("field", ["d_macs", "d_out"])
def test_a_null_macs_or_out_pointer_is_refused(field):
    r = list(good(base=0x3000000))
    r[FIELDS.index(field)] = 0
    refused(call([good(), tuple(r)]), "NULL", "request 1")


@pytest.mark.parametrize("field,off,word", [("d_macs", 8, "16-byte"), ("d_out", 8, "16-byte"), ("d_sub", 8, "16-byte"),
                                            ("d_write_steps", 4, "8-byte")])
def test_a_misaligned_pointer_is_refused(field, off, word):
    r = list(good(steps=True, sub=True))
    r[FIELDS.index(field)] += off
    refused(call([tuple(r)]), word, "request 0")
    assert call([good(steps=True, sub=True)]) != ERR_ARG


@pytest.mark.parametrize("n_rows", [0, 1, 3, 12, 32, 1 << 17])
def test_a_bad_n_rows_is_refused(n_rows):
    refused(call([good()], n_rows=n_rows, n_total=16), "n_rows")


@pytest.mark.parametrize("n_total", [0, 1, 3, 1000, (1 << 16) + 1, 1 << 17])
def test_a_bad_n_total_is_refused(n_total):
    refused(call([good()], n_rows=2, n_total=n_total), "n_total")


def test_the_caps_pass_the_checks():
    assert call([(0x1000000, 0x80000000, 0, 0)], n_rows=1 << 16, n_total=1 << 16) != ERR_ARG
    assert call([good()], n_rows=2, n_total=1 << 16) != ERR_ARG


@pytest.mark.parametrize("curve", [-1, 2, 7])
def test_a_bad_curve_is_refused(curve):
    refused(call([good()], curve=curve), "curve")


def test_an_output_overlapping_anything_is_refused():
    n_rows = 16
    row_b = n_rows * 64
    a = good()
    # in place, the tail of the input, the head of the output
    refused(call([(a[0], a[0], 0, 0)]), "overlaps")
    refused(call([(a[0], a[0] + row_b - 16, 0, 0)]), "overlaps")
    refused(call([(a[0], a[0] - row_b + 16, 0, 0)]), "overlaps")
    assert call([(a[0], a[0] + row_b, 0, 0)]) != ERR_ARG           # back to back is fine
    assert call([(a[0], a[0] - row_b, 0, 0)]) != ERR_ARG
    # across requests: two outputs, an output on another request's input, on another request's sub
    b = good(base=0x5000000, sub=True)
    refused(call([a, (b[0], a[1] + 32, 0, 0)]), "overlaps")
    refused(call([a, (b[0], a[0] + 64, 0, 0)]), "overlaps")
    refused(call([(a[0], b[0] + 64, 0, 0), b]), "overlaps")
    refused(call([(a[0], b[3] + 64, 0, 0), b]), "overlaps")
    # the output over its own sub, over the write steps
    refused(call([(a[0], a[1], 0, a[1] + 16)]), "overlaps")
    refused(call([(a[0], a[1], a[1] + 8, 0)]), "overlaps")
    # two requests may read the same rows, the same steps and the same sub; the sub may be the rows themselves
    assert call([a, (a[0], b[1], 0, 0)]) != ERR_ARG
    assert call([good(steps=True, sub=True), (b[0], b[1], good(steps=True)[2], good(sub=True)[3])]) != ERR_ARG
    assert call([(a[0], a[1], 0, a[0])]) != ERR_ARG


def test_too_many_requests_are_refused():
    from porla_amd import lib
    from porla_amd.loader import IccMacDecodeReq
    k = 65536
    arr = (IccMacDecodeReq * k)()
    for i in range(k):
        arr[i] = IccMacDecodeReq(0x10000000 + 0x1000 * i, 0x40000000 + 0x1000 * i, None, None)
    refused(lib.porla_icc_mac_decode_batch_device(arr, k, 2, 2, 0, None), "65535")
    assert lib.porla_icc_mac_decode_batch_device(arr, k - 1, 2, 2, 0, None) != ERR_ARG


def test_a_byte_size_that_overflows_is_refused():
    """k <= 65535 requests of n_rows <= 2^16 rows always fit: what can overflow is a buffer that wraps around the address space"""
    top = (1 << 64) - (1 << 9)
    refused(call([(top, 0x1000, 0, 0)]), "overflow")
    refused(call([(0x1000, top, 0, 0)]), "overflow")
    refused(call([(0x1000, 0x100000, 0, top)]), "overflow")


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, null_reqs=True) == 0
    assert call([], k=0, null_reqs=True, curve=1) == 0


def test_the_host_form_refuses_before_the_device():
    from porla_amd import lib
    buf = bytes(2 * 64)
    out = ctypes.create_string_buffer(2 * 64)
    steps = (ctypes.c_ulonglong * 2)(1, 2)
    o = ctypes.cast(out, ctypes.c_void_p)

    def host(macs=buf, n_rows=2, n_total=2, curve=0, st=None, sub=None, out_p=o):
        return lib.porla_icc_mac_decode_host(macs, n_rows, n_total, curve, st, sub, out_p)

    for rc in (host(macs=None), host(out_p=None), host(n_rows=3), host(n_rows=4), host(n_total=3), host(curve=2)):
        assert rc == ERR_ARG
        assert "porla_icc_mac_decode_host" in lib.porla_gpu_last_error().decode()
    assert host() != ERR_ARG
    assert host(st=steps, sub=buf) != ERR_ARG


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both curves, with and without steps and sub, the host form) return
    PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, icc
def req(base, steps, sub):
    return (base, base + 0x400000, base + 0x800000 if steps else 0, base + 0xa00000 if sub else 0)
for curve in (0, 1):
    for n_total in (16, 32):
        reqs = [req(0x1000000, True, True), req(0x3000000, False, False), req(0x5000000, False, True)]
        print(lib.porla_icc_mac_decode_batch_device(icc.mac_decode_requests(reqs), 3, 16, n_total, curve, None))
out = ctypes.create_string_buffer(128)
print(lib.porla_icc_mac_decode_host(bytes(128), 2, 2, 0, None, None, ctypes.cast(out, ctypes.c_void_p)))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 5


def test_python_mirror_builds_requests():
    from porla_amd import icc
    arr = icc.mac_decode_requests([good(sub=True)])
    assert arr[0].d_macs == 0x1000000 and arr[0].d_out == 0x1400000 and arr[0].d_write_steps is None and arr[0].d_sub == 0x1a00000
    with pytest.raises(ValueError):
        icc.mac_decode_requests([good()[:3]])
    with pytest.raises(RuntimeError, match="n_rows"):
        icc.mac_decode_batch_device([good()], 3, 16, "bn254")
    with pytest.raises(KeyError):
        icc.mac_decode_batch_device([good()], 2, 16, "p256")

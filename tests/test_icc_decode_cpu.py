"""CPU: the ICC decode without a device.  The model the GPU tests compare against (tests/icc_decode_model.py) inverts the encode of
oracle/icc_py.py exactly -- on networks, on levels built with icc_py.mix, with the edge chunks -- and sees a tampered row; the facts
about the twiddles the kernels rest on hold at N = 2^16; the bound chain of the kernels closes (tools/check_fe30_bounds.py); and the C
ABI (include/porla_gpu.h: porla_icc_decode_batch_device / porla_icc_decode_host) exports its symbols, has the layout the library
static_asserts, refuses every bad argument with PORLA_ERR_ARG before the device is touched, returns 0 for k = 0 and
PORLA_ERR_NO_DEVICE for valid arguments without a device.  Nothing here computes on a device: the pointer values are never
dereferenced."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

import icc_py
from tests import common
from tests import icc_decode_model as model

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
WHO = "porla_icc_decode_batch_device"
CURVES = ("bn254", "secp256k1")
P = icc_py.P_ICC


def chunks_with_edges(n, ncols, curve, seed):
    """n rows of ncols random chunks, the edge chunks pinned to row 0, row n / 2 and the last row"""
    rng = random.Random(seed)
    rows = [[rng.getrandbits(256) for _ in range(ncols)] for _ in range(n)]
    edges = model.edge_chunks(curve)
    for r, shift in ((0, 0), (n // 2, 3), (n - 1, 5)):
        for c in range(ncols):
            rows[r][c] = edges[(c + shift) % len(edges)]
    return rows


# ---- the model against the encode
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [2, 4, 8, 32])
def test_model_round_trip(curve, n):
    rows = chunks_with_edges(n, 7, curve, 100 + n)
    X, _ = icc_py.crebuild(rows, curve)
    out, bad = model.decode_exact(X, curve)
    assert out == rows and bad == 0
    # the planes stay independent: inverting modulo LCM in one go gives the same values
    assert model.inverse_plane(X, icc_py.LCM[curve]) == rows
    assert model.decode_residue(X, n) == [[v % P for v in r] for r in rows]
    # ... and the byte forms
    data = model.rows_to_bytes(X, 64)
    assert model.decode_bytes("exact", data, n, 7, n, curve) == (model.rows_to_bytes(rows, 32), 0)
    assert model.decode_bytes("residue32", model.rows_to_bytes([[v % P for v in r] for r in X], 32), n, 7, n, curve)[0] == \
        model.rows_to_bytes([[v % P for v in r] for r in rows], 32)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("level,n_total", [(1, 8), (3, 8), (3, 16), (4, 16)])
def test_model_on_levels(curve, level, n_total):
    """a level as the update path builds it: the X half decodes to its blocks in write order, the Y half with the write steps to the
    chunks mod p_icc"""
    n = 1 << level
    blocks = chunks_with_edges(n, 5, curve, 7 * level + n_total)
    steps = [n_total + 3 + i for i in range(n)]
    X = model.level_x(blocks, n_total, curve)
    Y = model.level_y(blocks, steps, n_total, curve)
    assert len(X) == n and len(Y) == n
    assert model.decode_exact(X, curve) == (blocks, 0)
    want = [[v % P for v in r] for r in blocks]
    assert model.decode_residue(X, n_total) == want
    assert model.decode_residue(Y, n_total, steps) == want
    # without the unscale a Y half decodes to the rows HAdd stored: (chunk * wt_i) mod p_icc
    assert model.decode_residue(Y, n_total) == [icc_py.hadd(b, None, n_total, s, curve)[0] for b, s in zip(blocks, steps)]
    assert model.decode_exact(Y, curve)[0] == model.decode_residue(Y, n_total)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [2, 8, 64])
def test_model_sees_a_tampered_row(curve, n):
    rng = random.Random(n)
    ncols = 4
    rows = [[rng.getrandbits(256) for _ in range(ncols)] for _ in range(n)]
    X, _ = icc_py.crebuild(rows, curve)
    r, c = rng.randrange(n), 2
    X[r][c] = (X[r][c] + 1) % icc_py.LCM[curve]
    out, bad = model.decode_exact(X, curve)
    assert bad == n                                             # exactly that column's symbols
    for i in range(n):
        for j in range(ncols):
            if j != c:
                assert out[i][j] == rows[i][j]
            else:
                assert out[i][j] < P and out[i][j] != rows[i][j] % P


# ---- the twiddles
@pytest.mark.parametrize("curve", CURVES)
def test_twiddle_facts_at_2_16(curve):
    N, q = 1 << 16, icc_py.Q[curve]
    w = icc_py.root_w(N)
    assert pow(w, N, P) == 1 and pow(w, N // 2, P) != 1         # order exactly N: w^-e = w^(N - e)
    t = 1
    for _ in range(N):
        assert t % q != 0                                       # every (w^e mod p_icc) has an inverse modulo q
        t = t * w % P
    assert t == 1
    # the tables of every smaller n are subsets: root_w(n)^(n / m2) does not depend on n
    for n in (2, 8, 1 << 10):
        for m2 in (1, 2, n // 2):
            assert pow(icc_py.root_w(n), n // m2, P) == pow(w, N // m2, P)


def test_bound_chain():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import check_fe30_bounds as cb
    assert cb.check_icc_decode_chain()
    assert cb.ICC_DECODE_STAGES == 16
    assert cb.check_sub_tables()                                # K = 3 at b = 2 p - 1, the decode's difference


# ---- the C ABI
FIELDS = ("d_rows", "d_out", "d_write_steps", "d_bad")


def good(base=0x1000000, steps=False, bad=False):
    """one request as icc.decode_requests takes it: fake, far apart, aligned addresses"""
    return (base, base + 0x400000, base + 0x800000 if steps else 0, base + 0xa00000 if bad else 0)


def call(reqs, n_rows=16, n_cols=128, n_total=16, curve=0, form=0, k=None, null_reqs=False):
    from porla_amd import icc, lib
    arr = icc.decode_requests(reqs)
    return lib.porla_icc_decode_batch_device(None if null_reqs else arr, len(reqs) if k is None else k, n_rows, n_cols, n_total, curve,
                                             form, ctypes.c_void_p(0))


def refused(rc, *words):
    from porla_amd import lib
    assert rc == ERR_ARG
    msg = lib.porla_gpu_last_error().decode()
    assert msg and WHO in msg
    for w in words:
        assert w in msg, msg


def test_the_symbols_are_exported():
    from porla_amd import lib
    assert hasattr(lib, WHO) and hasattr(lib, "porla_icc_decode_host")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_ICC_DECODE_REQ_BYTES, IccDecodeReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_ICC_DECODE_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(IccDecodeReq) == size == PORLA_ICC_DECODE_REQ_BYTES == 32
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert {f: getattr(IccDecodeReq, f).offset for f, _ in IccDecodeReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "icc_decode.hip")).read()
    for f, off in offsets.items():
        assert "offsetof(porla_icc_decode_req, %s) == %d" % (f, off) in src
    for name, value in (("EXACT", 0), ("RESIDUE64", 1), ("RESIDUE32", 2)):
        assert int(re.search(r"#define PORLA_ICC_DECODE_%s\s+(\d+)" % name, header).group(1)) == value


def test_null_reqs_is_refused():
    refused(call([good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("field", ["d_rows", "d_out"])
def test_a_null_rows_or_out_pointer_is_refused(field):
    r = list(good(base=0x3000000))
    r[FIELDS.index(field)] = 0
    refused(call([good(), tuple(r)]), "NULL", "request 1")


@pytest.mark.parametrize("field,off,form,word", [("d_rows", 8, 0, "16-byte"), ("d_out", 8, 0, "16-byte"), ("d_write_steps", 4, 1, "8-byte"),
                                                 ("d_bad", 2, 0, "4-byte")])
def test_a_misaligned_pointer_is_refused(field, off, form, word):
    r = list(good(steps=form == 1, bad=form == 0))
    r[FIELDS.index(field)] += off
    refused(call([tuple(r)], form=form), word, "request 0")
    assert call([good(steps=form == 1, bad=form == 0)], form=form) != ERR_ARG


@pytest.mark.parametrize("n_rows", [0, 1, 3, 12, 32, 1 << 17])
def test_a_bad_n_rows_is_refused(n_rows):
    refused(call([good()], n_rows=n_rows, n_total=16), "n_rows")


@pytest.mark.parametrize("n_total", [0, 1, 3, 1000, (1 << 16) + 1, 1 << 17])
def test_a_bad_n_total_is_refused(n_total):
    refused(call([good()], n_rows=2, n_total=n_total), "n_total")


def test_the_caps_pass_the_checks():
    assert call([(0x1000000, 0x80000000, 0, 0)], n_rows=1 << 16, n_total=1 << 16, n_cols=1) != ERR_ARG
    assert call([good()], n_rows=2, n_total=1 << 16) != ERR_ARG


@pytest.mark.parametrize("n_cols", [0, 65536, 1 << 20])
def test_a_bad_n_cols_is_refused(n_cols):
    refused(call([(0x1000000, 0x4000000000, 0, 0)], n_cols=n_cols), "n_cols")


@pytest.mark.parametrize("curve", [-1, 2, 7])
def test_a_bad_curve_is_refused(curve):
    refused(call([good()], curve=curve), "curve")


@pytest.mark.parametrize("form", [-1, 3, 9])
def test_a_bad_form_is_refused(form):
    refused(call([good()], form=form), "form")


def test_write_steps_and_bad_go_with_their_forms_only():
    refused(call([good(steps=True)], form=0), "d_write_steps", "request 0")
    for form in (1, 2):
        refused(call([good(bad=True)], form=form), "d_bad", "request 0")
        assert call([good(steps=True)], form=form) != ERR_ARG
    assert call([good(bad=True)], form=0) != ERR_ARG


def test_an_output_overlapping_anything_is_refused():
    n_rows, n_cols = 16, 128
    in_b, out_b = n_rows * n_cols * 64, n_rows * n_cols * 32
    a = good()
    # in place, the tail of the input, the head of the output
    refused(call([(a[0], a[0], 0, 0)]), "overlaps")
    refused(call([(a[0], a[0] + in_b - 16, 0, 0)]), "overlaps")
    refused(call([(a[0], a[0] - out_b + 16, 0, 0)]), "overlaps")
    assert call([(a[0], a[0] + in_b, 0, 0)]) != ERR_ARG          # back to back is fine
    assert call([(a[0], a[0] - out_b, 0, 0)]) != ERR_ARG
    # across requests: two outputs, an output on another request's input
    b = good(base=0x5000000)
    refused(call([a, (b[0], a[1] + 32, 0, 0)]), "overlaps")
    refused(call([a, (b[0], a[0] + 64, 0, 0)]), "overlaps")
    refused(call([(a[0], b[0] + 64, 0, 0), b]), "overlaps")
    # the counter inside an input or an output; two requests sharing a counter
    refused(call([(a[0], a[1], 0, a[0] + 4)]), "overlaps")
    refused(call([(a[0], a[1], 0, a[1] + out_b - 4)]), "overlaps")
    refused(call([good(bad=True), (b[0], b[1], 0, good(bad=True)[3])]), "overlaps")
    # the output over the write steps
    refused(call([(a[0], a[1], a[1] + 8, 0)], form=1), "overlaps")
    # two requests may read the same rows and the same steps
    assert call([a, (a[0], b[1], 0, 0)]) != ERR_ARG
    assert call([good(steps=True), (b[0], b[1], good(steps=True)[2], 0)], form=1) != ERR_ARG
    # the 32-byte form's input is half as long
    assert call([(a[0], a[0] + out_b, 0, 0)], form=2) != ERR_ARG
    refused(call([(a[0], a[0] + out_b, 0, 0)], form=1), "overlaps")


def test_too_many_requests_are_refused():
    from porla_amd import lib
    from porla_amd.loader import IccDecodeReq
    k = 65536
    arr = (IccDecodeReq * k)()
    for i in range(k):
        arr[i] = IccDecodeReq(0x10000000 + 0x1000 * i, 0x40000000 + 0x1000 * i, None, None)
    refused(lib.porla_icc_decode_batch_device(arr, k, 2, 1, 2, 0, 0, None), "65535")
    assert lib.porla_icc_decode_batch_device(arr, k - 1, 2, 1, 2, 0, 0, None) != ERR_ARG


def test_a_byte_size_that_overflows_is_refused():
    refused(call([good()], n_rows=1 << 16, n_total=1 << 16, n_cols=1 << 60), "overflow")
    refused(call([good()], n_rows=1 << 16, n_total=1 << 16, n_cols=(1 << 41) + 1), "overflow")
    refused(call([((1 << 64) - (1 << 16), 0x1000, 0, 0)]), "overflow")           # the rows wrap around the address space


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, null_reqs=True) == 0
    assert call([], k=0, null_reqs=True, curve=1, form=2) == 0


def test_the_host_form_refuses_before_the_device():
    from porla_amd import lib
    buf = ctypes.create_string_buffer(2 * 64)
    out = ctypes.create_string_buffer(2 * 32)
    steps = (ctypes.c_ulonglong * 2)(1, 2)
    bad = ctypes.c_uint(0)
    o = ctypes.cast(out, ctypes.c_void_p)

    def host(rows=buf.raw, n_rows=2, n_cols=1, n_total=2, curve=0, form=0, st=None, out_p=o, bad_p=None):
        return lib.porla_icc_decode_host(rows, n_rows, n_cols, n_total, curve, form, st, out_p, bad_p)

    for rc in (host(rows=None), host(out_p=None), host(n_rows=3), host(n_rows=4), host(n_total=3), host(n_cols=0), host(curve=2),
               host(form=3), host(st=steps), host(form=1, bad_p=ctypes.byref(bad)), host(form=2, bad_p=ctypes.byref(bad))):
        assert rc == ERR_ARG
        assert "porla_icc_decode_host" in lib.porla_gpu_last_error().decode()
    assert host(bad_p=ctypes.byref(bad)) != ERR_ARG
    assert host(form=1, st=steps) != ERR_ARG


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both curves, the three forms, the host form) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, icc
def req(base, steps, bad):
    return (base, base + 0x400000, base + 0x800000 if steps else 0, base + 0xa00000 if bad else 0)
for curve in (0, 1):
    for form in (0, 1, 2):
        reqs = [req(0x1000000, form != 0, form == 0), req(0x3000000, False, False), req(0x5000000, form == 2, False)]
        print(lib.porla_icc_decode_batch_device(icc.decode_requests(reqs), 3, 16, 128, 32, curve, form, None))
out = ctypes.create_string_buffer(64)
print(lib.porla_icc_decode_host(bytes(128), 2, 1, 2, 0, 0, None, ctypes.cast(out, ctypes.c_void_p), None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 7


def test_python_mirror_builds_requests():
    from porla_amd import icc
    arr = icc.decode_requests([good(bad=True)])
    assert arr[0].d_rows == 0x1000000 and arr[0].d_out == 0x1400000 and arr[0].d_write_steps is None and arr[0].d_bad == 0x1a00000
    with pytest.raises(ValueError):
        icc.decode_requests([good()[:3]])
    with pytest.raises(RuntimeError, match="n_rows"):
        icc.decode_batch_device([good()], 3, 128, 16, "bn254", "exact")
    with pytest.raises(KeyError):
        icc.decode_batch_device([good()], 2, 128, 16, "bn254", "nearly")

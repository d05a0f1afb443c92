"""CPU: the verified retrieval without a device.  The relation the call rests on -- a coded MAC row of an exact half is
alpha Commit(row mod q) + s_j h with s the Z_q network of the blocks' hiding scalars -- holds on the oracle (icc_py.crebuild /
icc_py.mac_crebuild, both curves, both halves, with and without a write step); the model the GPU tests compare against
(tests/retrieve_model.py) calls a clean level clean and a tampered level by its row; and the C ABI (include/porla_gpu.h:
porla_{kzg,ipa}_retrieve_batch_device / porla_{kzg,ipa}_retrieve_host) exports its symbols, has the layout the library static_asserts,
refuses every bad argument with PORLA_ERR_ARG before the device is touched, returns 0 for k = 0 and PORLA_ERR_NO_DEVICE for valid
arguments without a device.  Nothing here computes on a device: the pointer values are never dereferenced."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
import icc_py
from tests import mac_decode_model as mdm
from tests import retrieve_model as model

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
KZG, IPA = "porla_kzg_retrieve_batch_device", "porla_ipa_retrieve_batch_device"
CURVES = ("bn254", "secp256k1")
NCOLS = 3


def key_of(curve):
    """a small key: KZG with a 61-bit tau and alpha; IPA with three alpha generators and a hiding point of unknown relation to them"""
    g = mdm.GEN[curve]
    if curve == "bn254":
        return {"curve": curve, "alpha": 0x1234567890abcdef, "tau": 0x0fedcba987654321, "h": icc_py.ec_mul(curve, g, 9)}
    return {"curve": curve, "alpha_generators": [icc_py.ec_mul(curve, g, 5 * (3 + i)) for i in range(NCOLS)], "h": icc_py.ec_mul(curve, g, 11)}


# ---- the relation on the oracle
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("write_step", ["0", "n + 3"])
def test_a_coded_mac_row_is_the_mac_of_its_coded_row(curve, n, write_step):
    """per-block MACs with arbitrary hiding scalars through icc_py.mac_crebuild, the blocks through icc_py.crebuild: X and Y row j of
    the MACs equal alpha Commit(row_j mod q) + s_j h, s = the Z_q network of the hiding scalars (times wt for Y)"""
    step = 0 if write_step == "0" else n + 3
    key, q = key_of(curve), icc_py.Q[curve]
    rng = random.Random(1000 * n + step)
    blocks = [[rng.getrandbits(256) for _ in range(NCOLS)] for _ in range(n)]
    u = [rng.getrandbits(256) for _ in range(n)]
    macs = [model.block_mac(b, ui, key) for b, ui in zip(blocks, u)]
    X, Y = icc_py.crebuild(blocks, curve, step)
    MX, MY = icc_py.mac_crebuild(macs, curve, step)
    wt = model.wt_of(n, step) % q
    for rows, mac_rows, s in ((X, MX, model.zq_network(u, curve)), (Y, MY, model.zq_network([wt * x for x in u], curve))):
        assert all(v < icc_py.LCM[curve] for row in rows for v in row)
        assert model.expected_macs(rows, s, key) == mac_rows
        assert model.expected_macs([[v % q for v in row] for row in rows], s, key) == mac_rows


@pytest.mark.parametrize("curve", CURVES)
def test_the_zq_network_inverts(curve):
    rng = random.Random(5)
    for n in (2, 4, 16):
        s = [rng.getrandbits(128) for _ in range(n)]
        assert model.zq_network(model.zq_network(s, curve, inverse=True), curve) == s


# ---- the model's verdicts
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("part,step", [(0, 0), (1, 11)])
def test_a_clean_level_is_clean_and_a_tampered_one_names_its_row(curve, part, step):
    n = 8
    key = key_of(curve)
    rng = random.Random(77 + part)
    blocks = [[rng.getrandbits(256) for _ in range(NCOLS)] for _ in range(n)]
    s = [rng.getrandbits(128) for _ in range(n)]
    rows, mac_rows, u = model.build_half(blocks, s, key, part, step)
    assert any(x >> 128 for x in u)                                        # (the blocks' own hiding scalars are no 128-bit values)
    macs = model.points_to_bytes(mac_rows)
    assert model.statuses(rows, macs, s, key) == bytes([1] * n)
    # one symbol: exactly its row
    bad_rows = [list(r) for r in rows]
    bad_rows[5][1] ^= 1
    assert model.statuses(bad_rows, macs, s, key) == bytes([1, 1, 1, 1, 1, 0, 1, 1])
    # one MAC row replaced by another valid point; one PRF value; infinity
    other = bytearray(macs)
    other[64 * 2:64 * 3] = macs[64 * 3:64 * 4]
    assert model.statuses(rows, bytes(other), s, key) == bytes([1, 1, 0, 1, 1, 1, 1, 1])
    assert model.statuses(rows, macs, s[:6] + [s[6] ^ 1] + s[7:], key) == bytes([1, 1, 1, 1, 1, 1, 0, 1])
    inf = bytearray(macs)
    inf[:64] = bytes(64)
    assert model.statuses(rows, bytes(inf), s, key) == bytes([0] + [1] * 7)
    # a stored coordinate >= p is not the canonical form
    p = icc_py.CURVE_P[curve]
    x0 = int.from_bytes(macs[:32], "big")
    if x0 + p < 1 << 256:
        nc = (x0 + p).to_bytes(32, "big") + macs[32:]
        assert mdm.bytes_to_points(nc[:64], curve) == mac_rows[:1] and model.statuses(rows, nc, s, key)[0] == 0
    # an all-zero row with PRF 0: the expected MAC is infinity
    assert model.statuses([[0] * NCOLS], bytes(64), [0], key) == bytes([1])


def test_prf_bytes_are_read_as_the_client_update_reads_them():
    from tests.client_update_model import prf_scalar
    raw = bytes(range(1, 17))
    for curve in CURVES:
        assert model.prf_scalar(curve, raw) == prf_scalar(curve, raw)
        assert model.prf_raw(curve, model.prf_scalar(curve, raw)) == raw


# ---- the C ABI
FIELDS = ("d_rows", "d_macs", "d_prf", "d_out", "d_status", "d_counts")
FAKE_FB = 0x7000000        # a base pointer the refusals never follow


def good(base=0x10000000, out=True, counts=True):
    """16 rows of 128 columns: rows 128 KiB, macs 1 KiB, prf 256 B, out 64 KiB, status 16 B, counts 8 B"""
    return (base, base + 0x100000, base + 0x200000, base + 0x300000 if out else 0, base + 0x400000, base + 0x500000 if counts else 0)


def call(reqs, n_rows=16, n_total=16, k=None, null_reqs=False, who=IPA, bases=(FAKE_FB, FAKE_FB + 0x1000)):
    from porla_amd import lib
    from porla_amd import multiexp as mx
    arr = mx.retrieve_requests(reqs)
    k = len(reqs) if k is None else k
    if who == KZG:
        return lib.porla_kzg_retrieve_batch_device(None if null_reqs else arr, k, n_rows, n_total, None)
    return lib.porla_ipa_retrieve_batch_device(bases[0] or None, bases[1] or None, None if null_reqs else arr, k, n_rows, n_total, None)


def refused(rc, who, *words):
    from porla_amd import lib
    assert rc == ERR_ARG
    msg = lib.porla_gpu_last_error().decode()
    assert msg and who in msg
    for w in words:
        assert w in msg, msg


BOTH = pytest.mark.parametrize("who", [KZG, IPA])


def test_the_symbols_are_exported():
    from porla_amd import lib
    for name in (KZG, IPA, "porla_kzg_retrieve_host", "porla_ipa_retrieve_host"):
        assert hasattr(lib, name)


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_RETRIEVE_REQ_BYTES, PORLA_RETRIEVE_ROW_OK, RetrieveReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_RETRIEVE_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(RetrieveReq) == size == PORLA_RETRIEVE_REQ_BYTES == 48
    assert int(re.search(r"#define PORLA_RETRIEVE_ROW_OK\s+(\d+)", header).group(1)) == PORLA_RETRIEVE_ROW_OK == model.ROW_OK
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert {f: getattr(RetrieveReq, f).offset for f, _ in RetrieveReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "retrieve_batch.hip")).read()
    for f, off in offsets.items():
        assert "offsetof(porla_retrieve_req, %s) == %d" % (f, off) in src
        assert re.search(r"\*%s;\s+/\* %d \*/" % (f, off), header), f


@BOTH
def test_null_reqs_is_refused(who):
    refused(call([good()], null_reqs=True, k=1, who=who), who, "NULL")


@BOTH
@pytest.mark.parametrize("field", ["d_rows", "d_macs", "d_prf", "d_status"])
def test_a_null_required_pointer_is_refused(who, field):
    r = list(good(base=0x30000000))
    r[FIELDS.index(field)] = 0
    refused(call([good(), tuple(r)], who=who), who, "NULL", "request 1")


@BOTH
@pytest.mark.parametrize("field,off,word", [("d_rows", 8, "16-byte"), ("d_macs", 8, "16-byte"), ("d_prf", 8, "16-byte"), ("d_out", 8, "16-byte"),
                                            ("d_counts", 2, "4-byte")])
def test_a_misaligned_pointer_is_refused(who, field, off, word):
    r = list(good())
    r[FIELDS.index(field)] += off
    refused(call([tuple(r)], who=who), who, word, "request 0")
    s = list(good())
    s[FIELDS.index("d_status")] += 1                                       # status bytes need no alignment; counters 4
    s[FIELDS.index("d_counts")] += 4
    assert call([tuple(s)], who=who) != ERR_ARG


@BOTH
@pytest.mark.parametrize("n_rows", [0, 1, 3, 12, 32, 1 << 17])
def test_a_bad_n_rows_is_refused(who, n_rows):
    refused(call([good()], n_rows=n_rows, n_total=16, who=who), who, "n_rows")


@BOTH
@pytest.mark.parametrize("n_total", [0, 1, 3, 1000, (1 << 16) + 1, 1 << 17])
def test_a_bad_n_total_is_refused(who, n_total):
    refused(call([good()], n_rows=2, n_total=n_total, who=who), who, "n_total")


@BOTH
def test_the_caps_and_the_optional_pointers_pass_the_checks(who):
    big = (0x100000000, 0x200000000, 0x300000000, 0x400000000, 0x500000000, 0x600000000)
    assert call([big], n_rows=1 << 16, n_total=1 << 16, who=who) != ERR_ARG
    assert call([good()], n_rows=2, n_total=1 << 16, who=who) != ERR_ARG
    assert call([good(out=False)], who=who) != ERR_ARG
    assert call([good(counts=False)], who=who) != ERR_ARG
    assert call([good(out=False, counts=False)], who=who) != ERR_ARG


@BOTH
def test_an_output_overlapping_anything_is_refused(who):
    a, b = good(), good(base=0x50000000)
    i = FIELDS.index

    def with_(r, **kw):
        r = list(r)
        for f, v in kw.items():
            r[i(f)] = v
        return tuple(r)

    # the status bytes on the MAC rows, on the PRF values, inside the data rows; the counters on the status bytes
    refused(call([with_(a, d_status=a[i("d_macs")])], who=who), who, "overlaps")
    refused(call([with_(a, d_status=a[i("d_prf")] + 15)], who=who), who, "overlaps")
    refused(call([with_(a, d_status=a[i("d_rows")] + 64)], who=who), who, "overlaps")
    refused(call([with_(a, d_counts=a[i("d_status")] + 12)], who=who), who, "overlaps")
    assert call([with_(a, d_counts=a[i("d_status")] + 16)], who=who) != ERR_ARG            # back to back is fine
    # the blocks on the MAC rows (d_out starts before them and runs into them), on the status bytes, in place
    refused(call([with_(a, d_out=a[i("d_macs")] - 32)], who=who), who, "overlaps")
    refused(call([with_(a, d_out=a[i("d_status")])], who=who), who, "overlaps")
    refused(call([with_(a, d_out=a[i("d_rows")])], who=who), who, "overlaps")
    # across requests: two status arrays, a status array on another request's rows, two counter pairs, counters on another's blocks
    refused(call([a, with_(b, d_status=a[i("d_status")] + 8)], who=who), who, "overlaps")
    refused(call([a, with_(b, d_status=a[i("d_rows")])], who=who), who, "overlaps")
    refused(call([a, with_(b, d_counts=a[i("d_counts")] + 4)], who=who), who, "overlaps")
    refused(call([a, with_(b, d_counts=a[i("d_out")] + 4)], who=who), who, "overlaps")
    # inputs may be shared: two requests over the same rows, MAC rows and PRF values
    assert call([a, with_(b, d_rows=a[i("d_rows")], d_macs=a[i("d_macs")], d_prf=a[i("d_prf")])], who=who) != ERR_ARG


@BOTH
def test_too_many_requests_are_refused(who):
    from porla_amd import lib
    from porla_amd.loader import RetrieveReq
    k = 65536
    arr = (RetrieveReq * k)()
    for j in range(k):
        b = 0x100000000 + 0x10000 * j
        arr[j] = RetrieveReq(b, b + 0x4000, b + 0x5000, None, b + 0x6000, None)
    if who == KZG:
        run = lambda kk: lib.porla_kzg_retrieve_batch_device(arr, kk, 2, 2, None)
    else:
        run = lambda kk: lib.porla_ipa_retrieve_batch_device(FAKE_FB, FAKE_FB + 0x1000, arr, kk, 2, 2, None)
    refused(run(k), who, "65535")
    assert run(k - 1) != ERR_ARG


@BOTH
def test_a_byte_size_that_overflows_is_refused(who):
    """k <= 65535 requests of n_rows <= 2^16 rows always fit: what can overflow is a buffer that wraps around the address space"""
    top = (1 << 64) - (1 << 9)
    a = list(good())
    for f in ("d_rows", "d_macs", "d_out"):
        r = list(a)
        r[FIELDS.index(f)] = top
        refused(call([tuple(r)], who=who), who, "overflow")
    # the short arrays wrap only from the very top: 16 PRF values, 16 status bytes, two counters
    for f, last in (("d_prf", 16 * 16), ("d_status", 16), ("d_counts", 8)):
        r = list(a)
        r[FIELDS.index(f)] = (1 << 64) - last + (16 if f == "d_prf" else 4)
        refused(call([tuple(r)], who=who), who, "overflow")
        r[FIELDS.index(f)] = (1 << 64) - last - 16
        assert call([tuple(r)], who=who) != ERR_ARG


def test_a_null_base_is_refused():
    refused(call([good()], bases=(0, FAKE_FB)), IPA, "NULL base")
    refused(call([good()], bases=(FAKE_FB, 0)), IPA, "NULL base")


@BOTH
def test_k_zero_returns_zero(who):
    assert call([], k=0, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who, bases=(0, 0)) == 0


def test_the_host_forms_refuse_before_the_device():
    from porla_amd import lib
    rows, macs, prf = bytes(2 * 128 * 64), bytes(2 * 64), bytes(2 * 16)
    status = ctypes.create_string_buffer(2)
    st = ctypes.cast(status, ctypes.c_void_p)

    def kzg(r=rows, m=macs, p=prf, n_rows=2, n_total=2, s=st):
        return lib.porla_kzg_retrieve_host(r, m, p, n_rows, n_total, None, s, None)

    def ipa(r=rows, m=macs, p=prf, n_rows=2, n_total=2, s=st, a=FAKE_FB, h=FAKE_FB):
        return lib.porla_ipa_retrieve_host(a, h, r, m, p, n_rows, n_total, None, s, None)

    for f, who in ((kzg, "porla_kzg_retrieve_host"), (ipa, "porla_ipa_retrieve_host")):
        for rc in (f(r=None), f(m=None), f(p=None), f(s=None), f(n_rows=3), f(n_rows=4), f(n_total=3)):
            assert rc == ERR_ARG
            assert who in lib.porla_gpu_last_error().decode()
        assert f() != ERR_ARG
    assert ipa(a=None) == ERR_ARG and ipa(h=None) == ERR_ARG


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both builds, with and without d_out and d_counts, the host forms) return
    PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib
from porla_amd import multiexp as mx
def req(base, out, counts):
    return (base, base + 0x100000, base + 0x200000, base + 0x300000 if out else 0, base + 0x400000, base + 0x500000 if counts else 0)
reqs = [req(0x10000000, True, True), req(0x30000000, False, False), req(0x50000000, True, False)]
for n_total in (16, 32):
    print(lib.porla_kzg_retrieve_batch_device(mx.retrieve_requests(reqs), 3, 16, n_total, None))
    print(lib.porla_ipa_retrieve_batch_device(0x7000000, 0x7001000, mx.retrieve_requests(reqs), 3, 16, n_total, None))
st = ctypes.create_string_buffer(2)
print(lib.porla_kzg_retrieve_host(bytes(2 * 128 * 64), bytes(128), bytes(32), 2, 2, None, ctypes.cast(st, ctypes.c_void_p), None))
print(lib.porla_ipa_retrieve_host(0x7000000, 0x7001000, bytes(2 * 128 * 64), bytes(128), bytes(32), 2, 2, None, ctypes.cast(st, ctypes.c_void_p), None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 6


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr = mx.retrieve_requests([good(out=False)])
    assert arr[0].d_rows == 0x10000000 and arr[0].d_macs == 0x10100000 and arr[0].d_prf == 0x10200000 and arr[0].d_out is None
    assert arr[0].d_status == 0x10400000 and arr[0].d_counts == 0x10500000
    with pytest.raises(ValueError):
        mx.retrieve_requests([good()[:5]])
    with pytest.raises(RuntimeError, match="n_rows"):
        mx.kzg_retrieve_batch_device([good()], 3, 16)
    # the host forms read exactly n_rows x 128 x 64, n_rows x 64 and n_rows x 16 bytes: other lengths never reach the library
    never = lambda *a: pytest.fail("the library was called")
    for rows, macs, prf in ((bytes(2 * 128 * 64 - 64), bytes(128), bytes(32)), (bytes(2 * 128 * 64), bytes(64), bytes(32)),
                            (bytes(2 * 128 * 64), bytes(128), bytes(31))):
        with pytest.raises(ValueError, match="the call reads"):
            mx._retrieve_host(never, rows, macs, prf, 2, 128, True)

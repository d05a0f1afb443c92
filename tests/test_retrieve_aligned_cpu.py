"""CPU: the aligned verified retrieval without a device.  The model the GPU tests compare against (tests/retrieve_aligned_model.py:
status_j = the stored MAC row is E_j - alpha A_j) calls every resident half of a file clean after each of seven ordinary writes and
after the aligned rebuild write, X and Y, both curves, with random complements added; without the alignment term every Y row with a
finite alignment fails; one altered symbol, MAC row or alignment row fails exactly its row.  And the C ABI (include/porla_gpu.h:
porla_{kzg,ipa}_retrieve_aligned_batch_device / porla_{kzg,ipa}_retrieve_aligned_host) exports its symbols, has the layout the library
static_asserts, refuses every bad argument with PORLA_ERR_ARG before the device is touched, returns 0 for k = 0 and
PORLA_ERR_NO_DEVICE for valid arguments without a device.  Nothing here computes on a device: the pointer values are never followed."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
import icc_py
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
KZG, IPA = "porla_kzg_retrieve_aligned_batch_device", "porla_ipa_retrieve_aligned_batch_device"
KZG_HOST, IPA_HOST = "porla_kzg_retrieve_aligned_host", "porla_ipa_retrieve_aligned_host"
CURVES = ("bn254", "secp256k1")
EXACT, RESIDUE64, RESIDUE32 = 0, 1, 2


# ---- the model
def check_half(rows, macs, align, key, rng, want_finite):
    """all rows OK with random 128-bit complements added; without the alignment term exactly the finite-alignment rows fail"""
    s = [rng.getrandbits(128) for _ in rows]
    stored = am.add_complements(macs, s, key)
    assert am.statuses_aligned(rows, stored, s, align, key) == bytes([1] * len(rows))
    finite = [a is not None for a in align]
    assert model.statuses(rows, stored, s, key) == bytes(0 if f else 1 for f in finite)
    if want_finite:
        assert any(finite)
    return s, stored


@pytest.mark.parametrize("curve", CURVES)
def test_every_resident_half_is_clean_after_each_of_seven_writes(curve):
    from tests.update_model import FileModel
    n_total, n_cols = 8, 4
    rng = random.Random(2200)
    key, base, g = am.known_key(curve, n_cols, rng)
    m = FileModel(n_total, n_cols, curve, base, fill=0xA5)
    halves = 0
    for _ in range(7):
        chunks = [rng.getrandbits(256) for _ in range(n_cols)]
        m.update(chunks, am.block_mac_known(chunks, key, g))
        for lv, is_empty in enumerate(m.empty):
            if is_empty:
                continue
            for part in "xy":
                rows, macs, align = am.half_of(m, lv, part)
                check_half(rows, macs, align, key, rng, want_finite=part == "y")
                halves += 1
    assert halves == 2 * (1 + 1 + 2 + 1 + 2 + 2 + 3)                           # the ruler sequence's non-empty levels


@pytest.mark.parametrize("curve", CURVES)
def test_the_aligned_top_level_is_clean_and_a_tampered_half_names_its_row(curve):
    from tests.server_rebuild_aligned_model import AlignedRebuildFileModel
    n_total, n_cols = 4, 3
    rng = random.Random(2201)
    key, base, g = am.known_key(curve, n_cols, rng)
    m = AlignedRebuildFileModel(n_total, n_cols, curve, base)
    blocks = [[rng.getrandbits(256) for _ in range(n_cols)] for _ in range(n_total)]
    for i in range(n_total - 1):
        m.store(i + 1, blocks[i], am.block_mac_known(blocks[i], key, g))
    top = m.height - 1
    m.update(blocks[-1], am.block_mac_known(blocks[-1], key, g), None, index=n_total, write_step=7)
    for part in "xy":
        rows, macs, align = am.half_of(m, top, part, "residue32")
        assert all(v < icc_py.P_ICC for row in rows for v in row)
        s, stored = check_half(rows, macs, align, key, rng, want_finite=True)
        only = lambda j: bytes(0 if i == j else 1 for i in range(n_total))
        bad_rows = [list(r) for r in rows]
        bad_rows[2][1] ^= 1
        assert am.statuses_aligned(bad_rows, stored, s, align, key) == only(2)
        bad_macs = bytearray(stored)
        bad_macs[64:128] = stored[:64]
        assert am.statuses_aligned(rows, bytes(bad_macs), s, align, key) == only(1)
        bad_align = list(align)
        bad_align[3] = icc_py.ec_add(curve, align[3], key["h"])
        assert am.statuses_aligned(rows, stored, s, bad_align, key) == only(3)


# ---- the C ABI
FIELDS = ("d_rows", "d_macs", "d_prf", "d_align", "d_write_steps", "d_out", "d_status", "d_counts")
FAKE_FB = 0x7000000        # a base pointer the refusals never follow
ALPHA_BE = (12345).to_bytes(32, "big")


def good(base=0x10000000, align=True, steps=False, out=True, counts=True):
    """16 rows of 128 columns: rows 128 KiB, macs 1 KiB, prf 256 B, align 1 KiB, steps 128 B, out 64 KiB, status 16 B, counts 8 B"""
    return (base, base + 0x100000, base + 0x200000, base + 0x280000 if align else 0, base + 0x2c0000 if steps else 0,
            base + 0x300000 if out else 0, base + 0x400000, base + 0x500000 if counts else 0)


def call(reqs, n_rows=16, n_total=16, form=EXACT, k=None, null_reqs=False, who=IPA, bases=(FAKE_FB, FAKE_FB + 0x1000), alpha=ALPHA_BE):
    from porla_amd import lib
    from porla_amd import multiexp as mx
    arr = mx.retrieve_aligned_requests(reqs)
    k = len(reqs) if k is None else k
    if who == KZG:
        return lib.porla_kzg_retrieve_aligned_batch_device(None if null_reqs else arr, k, n_rows, n_total, form, None)
    return lib.porla_ipa_retrieve_aligned_batch_device(bases[0] or None, bases[1] or None, alpha, None if null_reqs else arr, k, n_rows,
                                                       n_total, form, None)


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
    for name in (KZG, IPA, KZG_HOST, IPA_HOST):
        assert hasattr(lib, name)


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_RETRIEVE_ALIGNED_REQ_BYTES, RetrieveAlignedReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_RETRIEVE_ALIGNED_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(RetrieveAlignedReq) == size == PORLA_RETRIEVE_ALIGNED_REQ_BYTES == 64
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert {f: getattr(RetrieveAlignedReq, f).offset for f, _ in RetrieveAlignedReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "retrieve_batch.hip")).read()
    for f, off in offsets.items():
        assert "offsetof(porla_retrieve_aligned_req, %s) == %d" % (f, off) in src
        assert re.search(r"\*%s;\s+/\*\s+%d \*/" % (f, off), header), f


def test_the_forms_are_the_decode_s():
    from porla_amd import icc
    from porla_amd import multiexp as mx
    assert mx.RETRIEVE_FORM == icc.DECODE_FORM == {"exact": EXACT, "residue64": RESIDUE64, "residue32": RESIDUE32}
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    for name, v in (("EXACT", EXACT), ("RESIDUE64", RESIDUE64), ("RESIDUE32", RESIDUE32)):
        assert int(re.search(r"#define PORLA_ICC_DECODE_%s\s+(\d+)" % name, header).group(1)) == v


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
                                            ("d_align", 8, "16-byte"), ("d_write_steps", 4, "8-byte"), ("d_counts", 2, "4-byte")])
def test_a_misaligned_pointer_is_refused(who, field, off, word):
    r = list(good(steps=True))
    r[FIELDS.index(field)] += off
    refused(call([tuple(r)], form=RESIDUE64, who=who), who, word, "request 0")
    s = list(good(steps=True))
    s[FIELDS.index("d_status")] += 1                                       # status bytes need no alignment; counters 4, write steps 8
    s[FIELDS.index("d_counts")] += 4
    s[FIELDS.index("d_write_steps")] += 8
    assert call([tuple(s)], form=RESIDUE64, who=who) != ERR_ARG


@BOTH
@pytest.mark.parametrize("form", [-1, 3, 64])
def test_a_bad_form_is_refused(who, form):
    refused(call([good()], form=form, who=who), who, "form")


@BOTH
def test_write_steps_with_the_exact_form_are_refused(who):
    refused(call([good(), good(base=0x30000000, steps=True)], form=EXACT, who=who), who, "d_write_steps", "request 1")
    for form in (RESIDUE64, RESIDUE32):
        assert call([good(), good(base=0x30000000, steps=True)], form=form, who=who) != ERR_ARG


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
    big = (0x100000000, 0x200000000, 0x300000000, 0x380000000, 0x3c0000000, 0x400000000, 0x500000000, 0x600000000)
    for form in (RESIDUE64, RESIDUE32):
        assert call([big], n_rows=1 << 16, n_total=1 << 16, form=form, who=who) != ERR_ARG
    assert call([good()], n_rows=2, n_total=1 << 16, who=who) != ERR_ARG
    for kw in (dict(out=False), dict(counts=False), dict(align=False), dict(align=False, out=False, counts=False)):
        assert call([good(**kw)], who=who) != ERR_ARG


def with_(r, **kw):
    r = list(r)
    for f, v in kw.items():
        r[FIELDS.index(f)] = v
    return tuple(r)


@BOTH
def test_an_output_overlapping_anything_is_refused(who):
    a, b = good(steps=True), good(base=0x50000000, steps=True)
    i = FIELDS.index
    run = lambda reqs: call(reqs, form=RESIDUE64, who=who)
    # what the exact call refuses: the status bytes on the MAC rows, the PRF values, the data rows; the counters on the status bytes
    refused(run([with_(a, d_status=a[i("d_macs")])]), who, "overlaps")
    refused(run([with_(a, d_status=a[i("d_prf")] + 15)]), who, "overlaps")
    refused(run([with_(a, d_status=a[i("d_rows")] + 64)]), who, "overlaps")
    refused(run([with_(a, d_counts=a[i("d_status")] + 12)]), who, "overlaps")
    assert run([with_(a, d_counts=a[i("d_status")] + 16)]) != ERR_ARG                      # back to back is fine
    refused(run([with_(a, d_out=a[i("d_macs")] - 32)]), who, "overlaps")
    refused(run([with_(a, d_out=a[i("d_rows")])]), who, "overlaps")
    # the new inputs: an output on the alignment rows (first byte, last byte), on the write steps (last byte)
    refused(run([with_(a, d_status=a[i("d_align")])]), who, "overlaps")
    refused(run([with_(a, d_status=a[i("d_align")] + 16 * 64 - 1)]), who, "overlaps")
    assert run([with_(a, d_status=a[i("d_align")] + 16 * 64)]) != ERR_ARG
    refused(run([with_(a, d_counts=a[i("d_write_steps")] + 16 * 8 - 4)]), who, "overlaps")
    assert run([with_(a, d_counts=a[i("d_write_steps")] + 16 * 8)]) != ERR_ARG
    refused(run([with_(a, d_out=a[i("d_align")] - 32)]), who, "overlaps")
    # across requests
    refused(run([a, with_(b, d_status=a[i("d_status")] + 8)]), who, "overlaps")
    refused(run([a, with_(b, d_status=a[i("d_align")] + 64)]), who, "overlaps")
    refused(run([a, with_(b, d_counts=a[i("d_write_steps")])]), who, "overlaps")
    refused(run([a, with_(b, d_counts=a[i("d_out")] + 4)]), who, "overlaps")
    # inputs may be shared
    assert run([a, with_(b, d_rows=a[i("d_rows")], d_macs=a[i("d_macs")], d_prf=a[i("d_prf")], d_align=a[i("d_align")],
                         d_write_steps=a[i("d_write_steps")])]) != ERR_ARG


@BOTH
def test_the_byte_sizes_follow_the_form_s_row_width(who):
    """16 rows of 128 symbols (IPA; the KZG build sizes the rows by the SRS this process holds, by one column while there is none): 128 KiB
    of 64-byte symbols, 64 KiB of 32-byte ones -- a status array that far behind d_rows is inside the rows of the 64-byte forms and
    behind the rows of residue32"""
    from porla_amd import multiexp as mx
    a = good()
    half = 16 * (128 if who == IPA else max(mx.kzg_row_coefficients(), 1)) * 32
    r = with_(a, d_status=a[0] + half)
    for form in (EXACT, RESIDUE64):
        refused(call([r], form=form, who=who), who, "overlaps")
    assert call([r], form=RESIDUE32, who=who) != ERR_ARG
    refused(call([with_(a, d_status=a[0] + half - 1)], form=RESIDUE32, who=who), who, "overlaps")


@BOTH
def test_too_many_requests_are_refused(who):
    from porla_amd import lib
    from porla_amd.loader import RetrieveAlignedReq
    k = 65536
    arr = (RetrieveAlignedReq * k)()
    for j in range(k):
        b = 0x100000000 + 0x10000 * j
        arr[j] = RetrieveAlignedReq(b, b + 0x4000, b + 0x5000, b + 0x5800, None, None, b + 0x6000, None)
    if who == KZG:
        run = lambda kk: lib.porla_kzg_retrieve_aligned_batch_device(arr, kk, 2, 2, EXACT, None)
    else:
        run = lambda kk: lib.porla_ipa_retrieve_aligned_batch_device(FAKE_FB, FAKE_FB + 0x1000, ALPHA_BE, arr, kk, 2, 2, EXACT, None)
    refused(run(k), who, "65535")
    assert run(k - 1) != ERR_ARG


@BOTH
def test_a_byte_size_that_overflows_is_refused(who):
    top = (1 << 64) - (1 << 9)
    a = good(steps=True)
    for f in ("d_rows", "d_macs", "d_out", "d_align"):
        refused(call([with_(a, **{f: top})], form=RESIDUE64, who=who), who, "overflow")
    for f, last, step in (("d_prf", 16 * 16, 16), ("d_status", 16, 4), ("d_counts", 8, 4), ("d_write_steps", 16 * 8, 8)):
        refused(call([with_(a, **{f: (1 << 64) - last + step})], form=RESIDUE64, who=who), who, "overflow")
        assert call([with_(a, **{f: (1 << 64) - last - 16})], form=RESIDUE64, who=who) != ERR_ARG


def test_a_null_base_or_alpha_is_refused():
    refused(call([good()], bases=(0, FAKE_FB)), IPA, "NULL base")
    refused(call([good()], bases=(FAKE_FB, 0)), IPA, "NULL base")
    refused(call([good()], alpha=None), IPA, "alpha_be")


@BOTH
def test_k_zero_returns_zero(who):
    assert call([], k=0, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who, bases=(0, 0)) == 0


def test_the_host_forms_refuse_before_the_device():
    from porla_amd import lib
    rows, macs, prf, align = bytes(2 * 128 * 64), bytes(2 * 64), bytes(2 * 16), bytes(2 * 64)
    steps = (ctypes.c_ulonglong * 2)(1, 2)
    status = ctypes.create_string_buffer(2)
    st = ctypes.cast(status, ctypes.c_void_p)

    def kzg(r=rows, m=macs, p=prf, al=align, ws=None, n_rows=2, n_total=2, form=RESIDUE64, s=st):
        return lib.porla_kzg_retrieve_aligned_host(r, m, p, al, ws, n_rows, n_total, form, None, s, None)

    def ipa(r=rows, m=macs, p=prf, al=align, ws=None, n_rows=2, n_total=2, form=RESIDUE64, s=st, a=FAKE_FB, h=FAKE_FB, alpha=ALPHA_BE):
        return lib.porla_ipa_retrieve_aligned_host(a, h, alpha, r, m, p, al, ws, n_rows, n_total, form, None, s, None)

    for f, who in ((kzg, KZG_HOST), (ipa, IPA_HOST)):
        for rc in (f(r=None), f(m=None), f(p=None), f(s=None), f(n_rows=3), f(n_rows=4), f(n_total=3), f(form=3), f(form=-1),
                   f(ws=steps, form=EXACT)):
            assert rc == ERR_ARG
            assert who in lib.porla_gpu_last_error().decode()
        assert f() != ERR_ARG
        assert f(al=None) != ERR_ARG and f(ws=steps) != ERR_ARG and f(form=RESIDUE32) != ERR_ARG and f(form=EXACT) != ERR_ARG
    assert ipa(a=None) == ERR_ARG and ipa(h=None) == ERR_ARG and ipa(alpha=None) == ERR_ARG


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both builds, every form, with and without the optional pointers, the
    host forms) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib
from porla_amd import multiexp as mx
def req(base, align, steps, out, counts):
    return (base, base + 0x100000, base + 0x200000, base + 0x280000 if align else 0, base + 0x2c0000 if steps else 0,
            base + 0x300000 if out else 0, base + 0x400000, base + 0x500000 if counts else 0)
alpha = (7).to_bytes(32, "big")
for form in (0, 1, 2):
    reqs = [req(0x10000000, True, form != 0, True, True), req(0x30000000, False, False, False, False), req(0x50000000, True, False, True, False)]
    print(lib.porla_kzg_retrieve_aligned_batch_device(mx.retrieve_aligned_requests(reqs), 3, 16, 32, form, None))
    print(lib.porla_ipa_retrieve_aligned_batch_device(0x7000000, 0x7001000, alpha, mx.retrieve_aligned_requests(reqs), 3, 16, 32, form, None))
st = ctypes.create_string_buffer(2)
stp = ctypes.cast(st, ctypes.c_void_p)
print(lib.porla_kzg_retrieve_aligned_host(bytes(2 * 128 * 64), bytes(128), bytes(32), bytes(128), None, 2, 2, 1, None, stp, None))
print(lib.porla_ipa_retrieve_aligned_host(0x7000000, 0x7001000, alpha, bytes(2 * 128 * 32), bytes(128), bytes(32), None, None, 2, 2, 2, None, stp, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 8


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr = mx.retrieve_aligned_requests([good(out=False, steps=True)])
    assert arr[0].d_rows == 0x10000000 and arr[0].d_macs == 0x10100000 and arr[0].d_prf == 0x10200000 and arr[0].d_align == 0x10280000
    assert arr[0].d_write_steps == 0x102c0000 and arr[0].d_out is None and arr[0].d_status == 0x10400000 and arr[0].d_counts == 0x10500000
    with pytest.raises(ValueError):
        mx.retrieve_aligned_requests([good()[:6]])
    with pytest.raises(RuntimeError, match="n_rows"):
        mx.kzg_retrieve_aligned_batch_device([good()], 3, 16, "exact")
    with pytest.raises(KeyError):
        mx.kzg_retrieve_aligned_batch_device([good()], 16, 16, "residue16")
    assert mx._alpha_be(5) == (5).to_bytes(32, "big") and mx._alpha_be(None) is None
    assert callable(mx.FixedBase.ipa_retrieve_aligned_batch_device) and callable(mx.FixedBase.ipa_retrieve_aligned_host)
    # the host forms read exactly the form's sizes: other lengths never reach the library
    never = lambda *a: pytest.fail("the library was called")
    for form, rows, align in (("residue64", bytes(2 * 128 * 32), None), ("residue32", bytes(2 * 128 * 64), None),
                              ("residue32", bytes(2 * 128 * 32), bytes(64))):
        with pytest.raises(ValueError, match="the call reads"):
            mx._retrieve_aligned_host(never, rows, bytes(128), bytes(32), align, None, 2, 128, form, True)
    with pytest.raises(ValueError, match="write steps"):
        mx._retrieve_aligned_host(never, bytes(2 * 128 * 64), bytes(128), bytes(32), None, [1], 2, 128, "residue64", True)

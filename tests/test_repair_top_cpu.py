"""CPU: the top-level repair without a device.  The facts the call rests on, on stores made by tests/server_rebuild_model.py and
tests/server_rebuild_aligned_model.py and on icc_py.crebuild's own rows: wt times any X row is the Y row byte for byte, the forward
scale is the inverse of tests/extract_xyt_model.py:unscale_symbol, and the model the GPU tests compare against
(tests/repair_top_model.py) follows rules 2 to 8 of the header.  And the C ABI (include/porla_gpu.h:
porla_{kzg,ipa}_repair_top_batch_device): symbols, layout, every refusal, k = 0, PORLA_ERR_NO_DEVICE.  Nothing here computes on a
device: the pointer values are never followed."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
import icc_py
from tests import extract_xyt_model as tm
from tests import repair_top_model as rm
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model
from tests import test_extract_cpu as tc
from tests import test_extract_xyt_cpu as tx

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = tc.ERR_NO_DEVICE, tc.ERR_ARG
KZG, IPA = "porla_kzg_repair_top_batch_device", "porla_ipa_repair_top_batch_device"
CURVES = tc.CURVES
P = rm.P
N_COLS = tx.N_COLS
SHAPES = tx.SHAPES                                  # both curves x n in (2, 8) x step in (n: wt = 1, n + 3: a true twiddle) x both forms
DATA, MAC, LOST = rm.DATA, rm.MAC, rm.LOST


# ---- the model facts
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [8, 2])
@pytest.mark.parametrize("step_off", [3, 0])
def test_the_forward_scale_gives_crebuilds_own_y_rows(curve, n, step_off):
    """icc_py.crebuild(u, curve, step) -> (X rows, Y rows): wt X_j is Y_j symbol for symbol, below LCM and mod p_icc"""
    rnd = random.Random(8100 + n)
    step = n + step_off
    u = [[rnd.getrandbits(256) for _ in range(N_COLS)] for _ in range(n)]
    xs, ys = icc_py.crebuild(u, curve, step)[:2]
    e = rm.top_exponent(n, step)
    assert (e == 0) == (step_off == 0)
    for j in range(n):
        assert [rm.scale_symbol(v, e, n, curve, "exact") for v in xs[j]] == list(ys[j]), j
        assert [rm.scale_symbol(v % P, e, n, curve, "residue32") for v in xs[j]] == [v % P for v in ys[j]], j
    if e:
        assert xs != ys


@pytest.mark.parametrize("curve,n,step,form", SHAPES)
def test_the_forward_scale_gives_the_rebuild_models_y_half(curve, n, step, form):
    key, u, f, top_y = tx.rebuilt(curve, n, step, form)
    e = rm.top_exponent(n, step)
    rb = N_COLS * am.FORM_SYMBOL_BYTES[form]
    for j in range(n):
        assert rm.candidate_row(f.top[0][j * rb:(j + 1) * rb], True, e, n, curve, form) == top_y[0][j * rb:(j + 1) * rb], j
        assert rm.candidate_row(top_y[0][j * rb:(j + 1) * rb], False, e, n, curve, form) == f.top[0][j * rb:(j + 1) * rb], j


def test_the_forward_scale_is_the_inverse_of_unscale_symbol():
    rnd = random.Random(8200)
    for curve in CURVES:
        lcm = icc_py.LCM[curve]
        for n, e in ((8, 3), (8, 7), (2, 1), (64, 37)):
            for v in (0, 1, lcm - 1, rnd.randrange(lcm), rnd.randrange(lcm)):
                assert tm.unscale_symbol(rm.scale_symbol(v, e, n, curve, "exact"), e, n, curve, "exact") == v
                assert rm.scale_symbol(tm.unscale_symbol(v, e, n, curve, "exact"), e, n, curve, "exact") == v
            # any 64 bytes are defined: reduced as the decode's load reduces them
            for v in (lcm, lcm + 5, (1 << 512) - 1):
                r = rm.scale_symbol(v, e, n, curve, "exact")
                assert 0 <= r < lcm and r == rm.scale_symbol(v % lcm, e, n, curve, "exact")
            for v in (0, P - 1, rnd.randrange(P)):
                assert tm.unscale_symbol(rm.scale_symbol(v, e, n, curve, "residue32"), e, n, curve, "residue32") == v
            for v in (P, (1 << 256) - 1):
                assert rm.scale_symbol(v, e, n, curve, "residue32") == rm.scale_symbol(v % P, e, n, curve, "residue32") < P


def test_rule_2_on_hand_made_status_vectors():
    ax, ay = rm.actions_of(bytes([1, 0, 1, 0, 1]), bytes([1, 1, 0, 0, 1]))
    assert ax == [None, "repair", None, "lost", None] and ay == [None, None, "repair", "lost", None]


def halves_of(curve, n, step, form):
    key, u, f, top_y = tx.rebuilt(curve, n, step, form)
    return key, f.top, top_y


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


@pytest.mark.parametrize("curve,n,step,form", SHAPES)
def test_the_model_follows_rules_2_to_8(curve, n, step, form):
    key, x, y = halves_of(curve, n, step, form)
    w = am.FORM_SYMBOL_BYTES[form]
    rb = N_COLS * w
    run = lambda xx, yy, **kw: rm.repair_top(xx, yy, n, N_COLS, curve, form, step, key=key, **kw)
    clean = run(x, y)
    assert clean["status_x"] == clean["status_y"] == bytes([1] * n) and clean["counts"] == [0] * 8
    assert clean["action_x"] == clean["action_y"] == bytes(n)
    assert (clean["rows_x"], clean["macs_x"], clean["rows_y"], clean["macs_y"]) == (x[0], x[1], y[0], y[1])
    last = n - 1
    # a data row, in X and in Y: pristine again, exactly DATA, the other half untouched
    for h, half in ((0, x), (1, y)):
        bad = (flip(half[0], rb * last + w + 2, 0x10),) + half[1:]
        got = run(bad, y) if h == 0 else run(x, bad)
        st = bytes([1] * last + [0])
        assert got["status_" + "xy"[h]] == st and got["status_" + "yx"[h]] == bytes([1] * n)
        assert (got["rows_x"], got["macs_x"], got["rows_y"], got["macs_y"]) == (x[0], x[1], y[0], y[1])
        assert got["action_" + "xy"[h]] == bytes([0] * last + [DATA]) and got["action_" + "yx"[h]] == bytes(n)
        assert got["counts"] == [1 - h, h, 1 - h, 0, h, 0, 0, 0]
    # the MAC row alone; data and MAC
    bad = (x[0], flip(x[1], 64 * 0 + 33, 0x40)) + x[2:]
    got = run(bad, y)
    assert got["action_x"] == bytes([MAC] + [0] * last) and got["macs_x"] == x[1] and got["rows_x"] == x[0]
    assert got["counts"] == [1, 0, 0, 1, 0, 0, 0, 0]
    bad = (flip(y[0], 5), flip(y[1], 7)) + y[2:]
    got = run(x, bad)
    assert got["action_y"] == bytes([DATA | MAC] + [0] * last) and got["macs_y"] == y[1] and got["rows_y"] == y[0]
    assert got["counts"] == [0, 1, 0, 0, 1, 1, 0, 0]
    # a row index damaged in both halves: LOST, not one byte written; another row is repaired beside it
    bad_x = (flip(flip(x[0], rb * last + 1), 3),) + x[1:]
    bad_y = (flip(y[0], rb * last + 9, 2),) + y[1:]
    got = run(bad_x, bad_y)
    assert got["action_x"] == bytes([DATA] + [0] * (last - 1) + [LOST]) and got["action_y"] == bytes([0] * last + [LOST])
    assert got["rows_x"][rb * last:] == bad_x[0][rb * last:] and got["rows_y"] == bad_y[0] and got["rows_x"][:rb * last] == x[0][:rb * last]
    assert got["macs_x"] == x[1] and got["macs_y"] == y[1]
    assert got["counts"] == [2, 1, 1, 0, 0, 0, 1, 0]
    # rule 8: a second run on the repaired stores writes nothing
    again = run((got["rows_x"], got["macs_x"]) + x[2:], (got["rows_y"], got["macs_y"]) + y[2:])
    assert again["status_x"] == bytes([1] * last + [0]) and again["action_x"] == again["action_y"] == bytes([0] * last + [LOST])
    assert again["counts"] == [1, 1, 0, 0, 0, 0, 1, 0]
    # given statuses are taken as they are
    forced = run(x, y, status_x=bytes([0] + [1] * last), status_y=bytes([1] * n))
    assert forced["action_x"] == bytes(n) and forced["counts"] == [1, 0, 0, 0, 0, 0, 0, 0]      # intact bytes: nothing differs


@pytest.mark.parametrize("curve", CURVES)
def test_a_damaged_alignment_row_gets_the_mac_of_the_alignment_as_stored(curve):
    n, step, form = 8, 11, "residue32"
    key, x, y = halves_of(curve, n, step, form)
    finite = [j for j in range(n) if y[3][64 * j:64 * j + 64] != bytes(64)]
    assert finite
    j = finite[0]
    # another finite alignment row in place of row j's: a valid point, not the row's own
    other = next(i for i in finite[1:] + list(range(n)) if y[3][64 * i:64 * i + 64] not in (bytes(64), y[3][64 * j:64 * j + 64]))
    bad_align = y[3][:64 * j] + y[3][64 * other:64 * other + 64] + y[3][64 * (j + 1):]
    got = rm.repair_top(x, y[:3] + (bad_align,), n, N_COLS, curve, form, step, key=key)
    assert got["status_y"] == bytes(0 if i == j else 1 for i in range(n)) and got["rows_y"] == y[0]
    assert got["action_y"] == bytes(MAC if i == j else 0 for i in range(n)) and got["macs_y"] != y[1]
    assert got["counts"] == [0, 1, 0, 0, 0, 1, 0, 0]
    # and the half then passes the check with the alignment as stored
    assert rm.half_statuses((got["rows_y"], got["macs_y"], y[2], bad_align), N_COLS, form, key) == bytes([1] * n)


# ---- the C ABI
FIELDS = ("d_rows_x", "d_macs_x", "d_align_x", "d_prf_x", "d_rows_y", "d_macs_y", "d_align_y", "d_prf_y", "d_status_x", "d_status_y",
          "d_action_x", "d_action_y", "d_counts", "top_step", "reserved")
STORES = ("d_rows_x", "d_macs_x", "d_rows_y", "d_macs_y")
FAKE_FB, ALPHA_BE = tc.FAKE_FB, tc.ALPHA_BE
EXACT, RESIDUE64, RESIDUE32 = tc.EXACT, tc.RESIDUE64, tc.RESIDUE32


def good(base=0x10000000, top_step=19, align=True, counts=True, reserved=0):
    """n_total = 16, 128 columns: the halves 128 KiB each at base and base + 0x100000, MACs and alignments 1 KiB each, PRF values 256 B,
    statuses and actions 16 B each, counts 32 B -- one MiB-aligned slot per member"""
    at = lambda i: base + 0x100000 * i
    return (at(0), at(2), at(3) if align else 0, at(4), at(1), at(5), at(6) if align else 0, at(7), at(8), at(9), at(10), at(11),
            at(12) if counts else 0, top_step, reserved)


def with_(r, **kw):
    r = list(r)
    for f, v in kw.items():
        r[FIELDS.index(f)] = v
    return tuple(r)


def call(reqs, n_total=16, form=EXACT, k=None, null_reqs=False, who=IPA, bases=(FAKE_FB, FAKE_FB + 0x1000), alpha=ALPHA_BE):
    from porla_amd import lib
    from porla_amd import multiexp as mx
    arr = mx.repair_top_requests(reqs)
    k = len(reqs) if k is None else k
    if who == KZG:
        return lib.porla_kzg_repair_top_batch_device(None if null_reqs else arr, k, n_total, form, None)
    return lib.porla_ipa_repair_top_batch_device(bases[0] or None, bases[1] or None, alpha, None if null_reqs else arr, k, n_total, form, None)


refused = tc.refused
BOTH = pytest.mark.parametrize("who", [KZG, IPA])
I = FIELDS.index


def test_the_symbols_are_exported():
    from porla_amd import lib
    for name in (KZG, IPA):
        assert hasattr(lib, name)


def test_the_ctypes_struct_and_constants_match_the_library():
    from porla_amd import loader
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_REPAIR_TOP_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(loader.RepairTopReq) == size == loader.PORLA_REPAIR_TOP_REQ_BYTES == 120
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert {f: getattr(loader.RepairTopReq, f).offset for f, _ in loader.RepairTopReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "repair_batch.hip")).read()
    struct = header[header.index("typedef struct {", header.index("#define PORLA_REPAIR_TOP_REQ_BYTES")):header.index("} porla_repair_top_req;")]
    for f, off in offsets.items():
        assert "offsetof(porla_repair_top_req, %s) == %d" % (f, off) in src
        assert re.search(r"%s;\s+/\*\s+%d[: ]" % (f, off), struct), f
    assert "sizeof(porla_repair_top_req) == PORLA_REPAIR_TOP_REQ_BYTES" in src
    for name, v in (("DATA", 1), ("MAC", 2), ("LOST", 4)):
        assert int(re.search(r"#define PORLA_REPAIR_%s\s+(\d+)" % name, header).group(1)) == v == getattr(loader, "PORLA_REPAIR_" + name)
    assert (rm.DATA, rm.MAC, rm.LOST) == (1, 2, 4)
    # the existing structs keep their sizes
    assert ctypes.sizeof(loader.ExtractXytReq) == 224 and ctypes.sizeof(loader.RetrieveAlignedReq) == 64


@BOTH
def test_good_arguments_pass_the_refusals(who):
    for form in (EXACT, RESIDUE32):
        assert call([good(), good(base=0x30000000, top_step=16)], who=who, form=form) != ERR_ARG
        assert call([good(counts=False, align=False), good(base=0x30000000, top_step=(1 << 64) - 1)], who=who, form=form) != ERR_ARG
        assert call([with_(good(), d_align_x=0)], who=who, form=form) != ERR_ARG
    assert call([good()], n_total=2, who=who) != ERR_ARG
    if who == IPA:                                                        # (128 columns: 512 MiB per half at 2^16 rows)
        wide = tuple(0x100000000 + 0x40000000 * i for i in range(13)) + (19, 0)
        assert call([wide], n_total=1 << 16, who=who) not in (ERR_ARG, 0)


@BOTH
def test_null_reqs_is_refused(who):
    refused(call([good()], null_reqs=True, k=1, who=who), who, "reqs is NULL")


@BOTH
@pytest.mark.parametrize("field", STORES + ("d_prf_x", "d_prf_y", "d_status_x", "d_status_y", "d_action_x", "d_action_y"))
def test_a_null_pointer_is_refused(who, field):
    refused(call([good(), with_(good(base=0x30000000), **{field: 0})], who=who), who, "NULL", "request 1", field)


@BOTH
@pytest.mark.parametrize("field", STORES + ("d_align_x", "d_align_y", "d_prf_x", "d_prf_y"))
def test_a_misaligned_store_alignment_or_prf_pointer_is_refused(who, field):
    g = good()
    for off in (8, 1):
        refused(call([with_(g, **{field: g[I(field)] + off})], who=who), who, "16-byte", "request 0")


@BOTH
def test_the_other_refusals(who):
    g = good()
    refused(call([with_(g, d_counts=g[I("d_counts")] + 2)], who=who), who, "4-byte")
    for n in (0, 1, 3, 1000, 1 << 17):
        refused(call([g], n_total=n, who=who), who, "n_total")
    for form in (RESIDUE64, 3, -1):
        refused(call([g], form=form, who=who), who, "top_form")
    for v in (1, 1 << 63):
        refused(call([good(), good(base=0x30000000, reserved=v)], who=who), who, "reserved", "request 1")
    refused(call([good()] * 65536, who=who), who, "65535")


@BOTH
def test_a_byte_size_that_wraps_is_refused(who):
    g = good()
    for f in STORES + ("d_align_x", "d_align_y", "d_prf_x", "d_prf_y"):
        refused(call([with_(g, **{f: (1 << 64) - 64})], who=who), who, "overflow")
    for f in ("d_status_x", "d_status_y", "d_action_x", "d_action_y"):
        refused(call([with_(g, **{f: (1 << 64) - 16})], who=who), who, "overflow")
        assert call([with_(g, **{f: (1 << 64) - 32})], who=who) != ERR_ARG
    refused(call([with_(g, d_counts=(1 << 64) - 28)], who=who), who, "overflow")                       # eight words
    assert call([with_(g, d_counts=(1 << 64) - 48)], who=who) != ERR_ARG


@BOTH
def test_the_stores_are_outputs_in_the_overlap_walk(who):
    a, b = good(), good(base=0x50000000)
    run = lambda reqs, **kw: call(reqs, who=who, **kw)
    # a store against an input of the call, an output and another store
    refused(run([with_(a, d_prf_x=a[I("d_macs_x")] + 512)]), who, "overlaps")
    refused(run([with_(a, d_align_y=a[I("d_macs_y")])]), who, "overlaps")
    refused(run([with_(a, d_rows_y=a[I("d_rows_x")])]), who, "overlaps")
    refused(run([with_(a, d_macs_x=a[I("d_macs_y")] + 1008)]), who, "overlaps")
    refused(run([with_(a, d_status_x=a[I("d_macs_x")] + 1008)]), who, "overlaps")
    assert run([with_(a, d_status_x=a[I("d_macs_x")] + 1024)]) != ERR_ARG                            # back to back is fine
    refused(run([with_(a, d_action_y=a[I("d_status_y")])]), who, "overlaps")
    refused(run([with_(a, d_action_x=a[I("d_counts")] + 28)]), who, "overlaps")                      # the eight-word d_counts is 32 bytes
    assert run([with_(a, d_action_x=a[I("d_counts")] + 32)]) != ERR_ARG
    if who == IPA:                                                        # (the KZG build sizes the halves by its SRS: none here)
        refused(run([with_(a, d_prf_y=a[I("d_rows_y")] + 0x1fff0)]), who, "overlaps")
        assert run([with_(a, d_prf_y=a[I("d_rows_y")] + 0x1fff0)], form=RESIDUE32) != ERR_ARG          # 32-byte symbols: 64 KiB halves
        refused(run([with_(a, d_prf_y=a[I("d_rows_y")] + 0xfff0)], form=RESIDUE32), who, "overlaps")
    # across requests: unlike in the extraction no two requests may share a store
    for f in STORES:
        refused(run([a, with_(b, **{f: a[I(f)]})]), who, "overlaps")
    refused(run([a, with_(b, d_prf_x=a[I("d_macs_y")])]), who, "overlaps")
    refused(run([a, a]), who, "overlaps")
    # inputs may be shared
    shared = {f: a[I(f)] for f in ("d_align_x", "d_align_y", "d_prf_x", "d_prf_y")}
    assert run([a, with_(b, **shared)]) != ERR_ARG


def test_a_null_base_or_alpha_is_refused():
    refused(call([good()], bases=(0, FAKE_FB)), IPA, "NULL base")
    refused(call([good()], bases=(FAKE_FB, 0)), IPA, "NULL base")
    refused(call([good()], alpha=None), IPA, "alpha_be")


@BOTH
def test_k_zero_returns_zero(who):
    assert call([], k=0, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who, bases=(0, 0)) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both builds, both top forms) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import sys
sys.path.insert(0, %r)
from porla_amd import lib
from porla_amd import multiexp as mx
from tests.test_repair_top_cpu import good
alpha = (7).to_bytes(32, "big")
for form in (0, 2):
    reqs = [good(), good(base=0x30000000, top_step=16, align=False, counts=False)]
    arr = mx.repair_top_requests(reqs)
    print(lib.porla_kzg_repair_top_batch_device(arr, 2, 16, form, None))
    print(lib.porla_ipa_repair_top_batch_device(0x7000000, 0x7001000, alpha, arr, 2, 16, form, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 4


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr = mx.repair_top_requests([good(counts=False), good(align=False)[:14]])
    assert arr[0].d_rows_x == 0x10000000 and arr[0].d_rows_y == 0x10100000 and arr[0].d_macs_x == 0x10200000 and arr[0].d_counts is None
    assert arr[0].d_action_y == 0x10b00000 and arr[0].top_step == 19 and arr[0].reserved == 0
    assert arr[1].d_align_x is None and arr[1].d_align_y is None and arr[1].d_counts == 0x10c00000 and arr[1].reserved == 0
    with pytest.raises(ValueError):
        mx.repair_top_requests([good()[:12]])
    with pytest.raises(RuntimeError, match="n_total"):
        mx.kzg_repair_top_batch_device([good()], 3, "exact")
    assert callable(mx.FixedBase.ipa_repair_top_batch_device)

"""CPU: the file extraction with the top level's Y half without a device.  The facts the call rests on, on stores made by
tests/server_rebuild_model.py and tests/server_rebuild_aligned_model.py: every top-level Y row keeps the aligned relation with the
client's new-Y PRF values, and wt^-1 times any Y row is the X row byte for byte -- so the model the GPU tests compare against
(tests/extract_xyt_model.py) gives the clean extraction back from a top level with damaged X rows.  And the C ABI (include/porla_gpu.h:
porla_{kzg,ipa}_extract_xyt_batch_device): symbols, layout, every refusal, k = 0, PORLA_ERR_NO_DEVICE.  Nothing here computes on a
device: the pointer values are never followed."""
import ctypes
import functools
import itertools
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
import icc_py
from tests import extract_model as em
from tests import extract_xy_model as xm
from tests import extract_xyt_model as tm
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model
from tests import test_extract_cpu as tc
from tests import test_extract_xy_cpu as txy

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = tc.ERR_NO_DEVICE, tc.ERR_ARG
KZG, IPA = "porla_kzg_extract_xyt_batch_device", "porla_ipa_extract_xyt_batch_device"
CURVES = tc.CURVES
P = xm.P
N_COLS = 3
SHAPES = [(curve, n, step, form) for curve in CURVES for n in (2, 8) for step in (n, n + 3) for form in ("exact", "residue32")]


# ---- the model facts
@functools.lru_cache(maxsize=None)
def rebuilt(curve, n, step, form, seed=7100):
    """a top level written by the rebuild models at write step `step` over U (block b names index b + 1), complements on both halves:
    (key, U, the File of the top level alone, the top Y half as extract_xyt takes it)"""
    from tests.server_rebuild_aligned_model import AlignedRebuildFileModel
    from tests.server_rebuild_model import RebuildFileModel
    rng = random.Random(seed + n)
    key, base, g = am.known_key(curve, N_COLS, rng)
    m = (RebuildFileModel if form == "exact" else AlignedRebuildFileModel)(n, N_COLS, curve, base, fill=0xA5)
    u = [em.with_index(b + 1, [rng.getrandbits(256) for _ in range(N_COLS)]) for b in range(n)]
    for b in range(1, n):
        m.store(b + 1, u[b], am.block_mac_known(u[b], key, g))
    s = [rng.getrandbits(128) for _ in range(2 * n)]
    m.rebuild(u[0], am.block_mac_known(u[0], key, g), 1, [model.hiding(v, key) for v in s], write_step=step)
    top, w = m.height - 1, am.FORM_SYMBOL_BYTES[form]
    half = lambda part: (bytes(m.fam["data_" + part][top][:n * N_COLS * w]), bytes(m.fam["mac_" + part][top][:64 * n]))
    align = lambda part: bytes(m.fam["align_" + part][top][:64 * n]) if form != "exact" else None
    f = em.File(n, N_COLS, curve, 2 * n, {}, half("x") + (s[:n], align("x")), form)
    return key, u, f, half("y") + (s[n:], align("y"))


@pytest.mark.parametrize("curve,n,step,form", SHAPES)
def test_every_top_y_row_keeps_the_aligned_relation_with_the_new_y_prf_values(curve, n, step, form):
    key, u, f, top_y = rebuilt(curve, n, step, form)
    assert em.row_statuses(f, key) == bytes([1] * n)
    assert tm.statuses_top_y(f, top_y, key) == bytes([1] * n)
    if form == "residue32":
        assert any(top_y[3][64 * j:64 * j + 64] != bytes(64) for j in range(n))
    # a PRF value of the other half does not pass
    assert tm.statuses_top_y(f, top_y[:2] + (f.top[2], top_y[3]), key) == bytes(n)


@pytest.mark.parametrize("curve,n,step,form", SHAPES)
def test_patching_any_subset_of_x_rows_from_y_gives_the_x_half_back(curve, n, step, form):
    """Y_j = wt X_j row by row, mod LCM in the exact form and mod p_icc in the aligned one: wt = 1 at a step that is a multiple of
    n_total (the Y half IS the X half), a true twiddle otherwise"""
    key, u, f, top_y = rebuilt(curve, n, step, form)
    assert (tm.top_exponent(n, step) == 0) == (step % n == 0)
    assert (top_y[0] == f.top[0]) == (step % n == 0)
    subsets = itertools.chain.from_iterable(itertools.combinations(range(n), k) for k in range(n + 1))
    for rows in subsets:
        sources = ["y" if j in rows else "x" for j in range(n)]
        assert tm.patch(f.top[0], top_y[0], sources, n, N_COLS, curve, form, step) == f.top[0], rows
    # and the wrong step does not: the factor is the rebuild's own
    if n > 2:
        assert tm.patch(f.top[0], top_y[0], ["y"] * n, n, N_COLS, curve, form, step + 1) != f.top[0]


@pytest.mark.parametrize("curve,n,step,form", SHAPES)
def test_a_damaged_x_row_changes_nothing_but_from_y_and_the_new_counts(curve, n, step, form):
    key, u, f, top_y = rebuilt(curve, n, step, form)
    clean = tm.extract_xyt(f, {}, 0, top_y, step, 1, key=key)
    assert clean["counts"] == [0] * 8 and clean["row_status_top_y"] == bytes([1] * n) and clean["top_patch"] == f.top[0]
    assert clean["flags"] == bytes([xm.FOUND | (xm.RESIDUE if form == "residue32" else 0)] * n) and clean["steps"] == [0] * n
    assert clean["blocks"] == tc.chunk_bytes([c % P if form == "residue32" else c for blk in u for c in blk])
    same = xm.extract_xy(f, {}, 0, key=key)
    assert {k: clean[k] for k in same} == dict(same, counts=same["counts"] + [0, 0])
    w = am.FORM_SYMBOL_BYTES[form]
    ok_y = clean["row_status_top_y"]
    for row in sorted({0, n // 2, n - 1}):
        bad = bytearray(f.top[0])
        bad[w * (row * N_COLS + 1) + 2] ^= 0x10
        g = em.File(n, N_COLS, curve, f.write_step, {}, (bytes(bad),) + f.top[1:], form)
        st = bytes(0 if j == row else 1 for j in range(n))
        assert em.row_statuses(g, key) == st
        got = tm.extract_xyt(g, {}, 0, top_y, step, 1, statuses=st, status_top_y=ok_y)
        assert got["counts"] == [1, 0, 0, 0, 0, 0, 0, 1] and got["row_status"] == st and got["top_patch"] == f.top[0]
        assert got["flags"] == bytes(x | xm.FROM_Y for x in clean["flags"])
        for k in ("blocks", "steps", "row_status_y", "row_status_top_y"):
            assert got[k] == clean[k], (row, k)
        # not tried: the call without the top Y half, the top level failed
        lost = tm.extract_xyt(g, {}, 0, top_y, step, 0, statuses=st)
        want = xm.extract_xy(g, {}, 0, statuses=st)
        assert {k: lost[k] for k in want} == dict(want, counts=want["counts"] + [0, 0]) and lost["counts"][3] == n
        assert lost["row_status_top_y"] == bytes([xm.NOT_TRIED] * n)
    # the same row damaged in both halves: no source, the top level is failed
    bad_y = bytearray(top_y[0])
    bad_y[w * (1 * N_COLS + 2) + 5] ^= 1
    bad_x = bytearray(f.top[0])
    bad_x[w * (1 * N_COLS) + 1] ^= 2
    g = em.File(n, N_COLS, curve, f.write_step, {}, (bytes(bad_x),) + f.top[1:], form)
    got = tm.extract_xyt(g, {}, 0, (bytes(bad_y),) + top_y[1:], step, 1, key=key)
    assert got["counts"][0] == 1 and got["counts"][3] == n and got["counts"][6:] == [1, 0] and got["flags"] == bytes([xm.UNSURE] * n)
    # different rows: recovered
    bad_y = bytearray(top_y[0])
    bad_y[w * 2 + 5] ^= 1
    got = tm.extract_xyt(g, {}, 0, (bytes(bad_y),) + top_y[1:], step, 1, key=key)
    assert got["row_status_top_y"] == bytes([0] + [1] * (n - 1)) and got["row_status"] == bytes([1, 0] + [1] * (n - 2))
    assert got["counts"] == [1, 0, 0, 0, 0, 0, 1, 1] and got["blocks"] == clean["blocks"] and got["top_patch"] == f.top[0]


def test_any_bytes_of_a_y_symbol_are_defined():
    """the patch reduces as the decode's load does: a symbol at or above the modulus gives the product of its residue"""
    for curve in CURVES:
        lcm, q = icc_py.LCM[curve], icc_py.Q[curve]
        for v in (0, 1, lcm - 1, lcm, lcm + 5, (1 << 512) - 1):
            r = tm.unscale_symbol(v, 3, 8, curve, "exact")
            assert 0 <= r < lcm and r == tm.unscale_symbol(v % lcm, 3, 8, curve, "exact")
            wt = pow(icc_py.root_w(8), 3, P)
            assert r * wt % lcm == v % lcm
    for v in (0, P - 1, P, (1 << 256) - 1):
        r = tm.unscale_symbol(v, 5, 8, "bn254", "residue32")
        assert 0 <= r < P and r * pow(icc_py.root_w(8), 5, P) % P == v % P


# ---- the C ABI
NEW = ("d_top_rows_y", "d_top_macs_y", "d_top_align_y", "d_prf_top_y", "d_top_patch", "d_row_status_top_y", "top_step", "top_y")
FIELDS = txy.FIELDS + NEW
FAKE_FB, ALPHA_BE = tc.FAKE_FB, tc.ALPHA_BE
EXACT, RESIDUE64, RESIDUE32 = tc.EXACT, tc.RESIDUE64, tc.RESIDUE32


def good(base=0x10000000, write_step=7, top_y=1, top_step=16, null_top_y=False, **kw):
    """tests/test_extract_xy_cpu.py:good and the top level's Y half behind it (n_total = 16, 128 columns): rows 128 KiB at base +
    0x1100000, MACs and alignments 1 KiB each at + 0x1200000 / + 0x1210000, 16 PRF values at + 0x1220000, the patched half 128 KiB at
    + 0x1300000, 16 statuses at + 0x1400000; counts 32 B"""
    if null_top_y:
        return txy.good(base, write_step, **kw) + (0, 0, 0, 0, 0, 0, top_step, top_y)
    return txy.good(base, write_step, **kw) + (base + 0x1100000, base + 0x1200000, base + 0x1210000, base + 0x1220000, base + 0x1300000,
                                               base + 0x1400000, top_step, top_y)


def with_(r, **kw):
    r = list(r)
    for f, v in kw.items():
        r[FIELDS.index(f)] = v
    return tuple(r)


def call(reqs, n_total=16, form=EXACT, k=None, null_reqs=False, who=IPA, bases=(FAKE_FB, FAKE_FB + 0x1000), alpha=ALPHA_BE):
    from porla_amd import lib
    from porla_amd import multiexp as mx
    arr, keep = mx.extract_xyt_requests(reqs)
    k = len(reqs) if k is None else k
    if who == KZG:
        return lib.porla_kzg_extract_xyt_batch_device(None if null_reqs else arr, k, n_total, form, None)
    return lib.porla_ipa_extract_xyt_batch_device(bases[0] or None, bases[1] or None, alpha, None if null_reqs else arr, k, n_total, form, None)


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
    size = int(re.search(r"#define PORLA_EXTRACT_XYT_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(loader.ExtractXytReq) == size == loader.PORLA_EXTRACT_XYT_REQ_BYTES == 224
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert [offsets[f] for f in NEW] == [160, 168, 176, 184, 192, 200, 208, 216]
    assert {f: getattr(loader.ExtractXytReq, f).offset for f, _ in loader.ExtractXytReq._fields_} == offsets
    assert [f for f, _ in loader.ExtractXytReq._fields_[:20]] == [f for f, _ in loader.ExtractXyReq._fields_]
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "extract_batch.hip")).read()
    struct = header[header.index("typedef struct {", header.index("#define PORLA_EXTRACT_XYT_REQ_BYTES")):header.index("} porla_extract_xyt_req;")]
    for f, off in offsets.items():
        assert "offsetof(porla_extract_xyt_req, %s) == %d" % (f, off) in src
        assert re.search(r"%s;\s+/\*\s+%d[: ]" % (f, off), struct), f
    assert "sizeof(porla_extract_xyt_req) == PORLA_EXTRACT_XYT_REQ_BYTES" in src
    # the existing structs keep their sizes
    assert ctypes.sizeof(loader.ExtractXyReq) == 160 and ctypes.sizeof(loader.ExtractReq) == 104
    assert "RESIDUE is set too)" not in header                             # FROM_Y's comment: that holds for lower levels only


@BOTH
def test_good_arguments_pass_the_refusals(who):
    for form in (EXACT, RESIDUE32):
        assert call([good(), good(base=0x30000000, top_y=0)], who=who, form=form) != ERR_ARG
        assert call([good(counts=False), good(base=0x30000000, write_step=5, top=False)], who=who, form=form) != ERR_ARG
        assert call([good(top_step=19), good(base=0x30000000, write_step=32, top_step=(1 << 64) - 1)], who=who, form=form) != ERR_ARG


@BOTH
def test_everything_the_xy_call_refuses_is_refused(who):
    refused(call([good()], null_reqs=True, k=1, who=who), who, "NULL")
    for field in ("d_blocks", "d_steps", "d_flags", "d_prf", "d_row_status", "d_top_macs", "d_work", "data_x", "mac_x"):
        r = with_(good(base=0x30000000), **{field: None if field in ("data_x", "mac_x") else 0})
        refused(call([good(), r], who=who), who, "NULL", "request 1")
    for field in ("data_y", "mac_y", "align_y", "d_prf_y", "d_work_y", "d_row_status_y"):
        r = with_(good(base=0x30000000), **{field: None if field in ("data_y", "mac_y", "align_y") else 0})
        refused(call([good(), r], who=who), who, "NULL", "request 1", field)
    g = good()
    fam = list(g[1])
    fam[1] = 0
    refused(call([with_(g, data_x=fam)], who=who), who, "NULL", "level 1")
    fam = list(g[I("mac_y")])
    fam[2] = 0
    refused(call([with_(g, mac_y=fam)], who=who), who, "NULL", "level 2")
    refused(call([with_(g, d_blocks=g[I("d_blocks")] + 8)], who=who), who, "16-byte")
    refused(call([with_(g, d_work_y=g[I("d_work_y")] + 8)], who=who), who, "16-byte")
    refused(call([with_(g, d_counts=g[I("d_counts")] + 2)], who=who), who, "4-byte")
    refused(call([g], n_total=1000, who=who), who, "n_total")
    refused(call([g], form=RESIDUE64, who=who), who, "top_form")
    refused(call([with_(g, d_work=g[I("d_blocks")])], who=who), who, "overlaps")
    refused(call([with_(g, d_work_y=g[I("d_work")])], who=who), who, "overlaps")
    refused(call([with_(g, d_top_rows=(1 << 64) - 64)], who=who), who, "overflow")
    refused(call([with_(g, d_prf_y=(1 << 64) - 64)], who=who), who, "overflow")
    refused(call([good()] * 65536, who=who), who, "65535")


@BOTH
@pytest.mark.parametrize("field", ["d_top_rows_y", "d_top_macs_y", "d_prf_top_y", "d_top_patch", "d_row_status_top_y"])
def test_a_null_top_y_pointer_with_the_half_to_try_is_refused(who, field):
    r = with_(good(base=0x30000000), **{field: 0})
    refused(call([good(), r], who=who), who, "NULL", "request 1", field)
    assert call([good(), with_(r, top_y=0)], who=who) != ERR_ARG
    no_top = with_(good(base=0x30000000, top=False), **{field: 0})           # no top level: nothing to try
    assert call([good(), no_top], who=who) != ERR_ARG


@BOTH
def test_nothing_to_try_needs_no_top_y_pointer_and_the_alignment_store_may_be_null(who):
    assert call([good(null_top_y=True, top_y=0)], who=who) != ERR_ARG
    assert call([good(null_top_y=True, top_y=1, top=False)], who=who) != ERR_ARG
    assert call([good(null_top_y=True, top_y=0, null_y=True, y_levels=0)], who=who) != ERR_ARG
    refused(call([good(null_top_y=True)], who=who), who, "NULL")
    assert call([with_(good(), d_top_align_y=0)], who=who) != ERR_ARG


@BOTH
@pytest.mark.parametrize("top_y", [2, 3, 1 << 32, (1 << 64) - 1])
def test_a_top_y_above_one_is_refused(who, top_y):
    refused(call([good(), good(base=0x30000000, top_y=top_y)], who=who), who, "request 1", "top_y")
    refused(call([good(top_y=top_y, top=False, null_top_y=True)], who=who), who, "top_y")


@BOTH
@pytest.mark.parametrize("field", NEW[:6])
def test_a_misaligned_new_pointer_is_refused_wherever_given(who, field):
    g = good()
    for off in (8, 1):
        refused(call([with_(g, **{field: g[I(field)] + off})], who=who), who, "16-byte", "request 0", field)
        refused(call([with_(g, **{field: g[I(field)] + off}, top_y=0)], who=who), who, "16-byte", field)
    h = good(top=False)
    refused(call([with_(h, **{field: h[I(field)] + 8})], who=who), who, "16-byte", field)


@BOTH
def test_a_new_byte_size_that_wraps_is_refused(who):
    g = good()
    for f in ("d_top_rows_y", "d_top_macs_y", "d_top_align_y", "d_prf_top_y", "d_top_patch"):
        refused(call([with_(g, **{f: (1 << 64) - 64})], who=who), who, "overflow")
    refused(call([with_(g, d_row_status_top_y=(1 << 64) - 16)], who=who), who, "overflow")
    refused(call([with_(g, d_row_status_top_y=(1 << 64) - 16, top_y=0)], who=who), who, "overflow")     # filled with NOT_TRIED: written
    assert call([with_(g, d_row_status_top_y=(1 << 64) - 32)], who=who) != ERR_ARG
    refused(call([with_(g, d_counts=(1 << 64) - 28)], who=who), who, "overflow")                       # eight words
    assert call([with_(g, d_counts=(1 << 64) - 48)], who=who) != ERR_ARG


@BOTH
def test_the_new_outputs_count_in_the_overlap_walk(who):
    a, b = good(), good(base=0x50000000)
    run = lambda reqs, **kw: call(reqs, who=who, **kw)
    refused(run([with_(a, d_top_patch=a[I("d_top_rows")])]), who, "overlaps")
    if who == IPA:                                                        # (the KZG build sizes the halves by its SRS: none here)
        refused(run([with_(a, d_top_patch=a[I("d_top_rows_y")] + 0x10000)]), who, "overlaps")
        assert run([with_(a, d_top_patch=a[I("d_top_rows_y")] + 0x10000)], form=RESIDUE32) != ERR_ARG  # 32-byte symbols: 64 KiB halves
        refused(run([with_(a, d_top_patch=a[I("d_top_rows_y")] + 0x8000)], form=RESIDUE32), who, "overlaps")
    refused(run([with_(a, d_top_patch=a[I("d_top_rows_y")] + 0x100)]), who, "overlaps")
    refused(run([with_(a, d_top_patch=a[I("d_blocks")])]), who, "overlaps")
    refused(run([with_(a, d_row_status_top_y=a[I("d_prf_top_y")] + 16 * 16 - 16)]), who, "overlaps")
    assert run([with_(a, d_row_status_top_y=a[I("d_prf_top_y")] + 16 * 16)]) != ERR_ARG               # back to back is fine
    refused(run([with_(a, d_row_status_top_y=a[I("d_top_macs_y")] + 1008)]), who, "overlaps")
    refused(run([with_(a, d_row_status_top_y=a[I("d_top_align_y")] + 1008)]), who, "overlaps")
    refused(run([with_(a, d_row_status_top_y=a[I("d_row_status")] + 16)]), who, "overlaps")
    refused(run([with_(a, d_row_status_top_y=a[I("d_flags")], top_y=0)]), who, "overlaps")            # untried: still an output
    refused(run([with_(a, d_steps=a[I("d_counts")] + 28)]), who, "overlaps")                          # the eight-word d_counts is 32 bytes
    assert run([with_(a, d_steps=a[I("d_counts")] + 32)]) != ERR_ARG
    # across requests
    refused(run([a, with_(b, d_top_patch=a[I("d_top_patch")] + 64)]), who, "overlaps")
    refused(run([a, with_(b, d_row_status_top_y=a[I("d_row_status_top_y")])]), who, "overlaps")
    # the three Y inputs (and the alignment store) may be shared between requests
    shared = {f: a[I(f)] for f in ("d_top_rows_y", "d_top_macs_y", "d_top_align_y", "d_prf_top_y")}
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
    """in a child process that sees no device: valid arguments (both builds, both top forms, the top Y half tried and not) return
    PORLA_ERR_NO_DEVICE"""
    code = r"""
import sys
sys.path.insert(0, %r)
from porla_amd import lib
from porla_amd import multiexp as mx
from tests.test_extract_xyt_cpu import good
alpha = (7).to_bytes(32, "big")
for form in (0, 2):
    reqs = [good(), good(base=0x30000000, write_step=5, y_levels=4, align=False, counts=False, top_step=19),
            good(base=0x50000000, write_step=22, top=False, null_y=True, y_levels=0, null_top_y=True),
            good(base=0x70000000, null_y=True, y_levels=8, top_y=0, null_top_y=True)]
    arr, keep = mx.extract_xyt_requests(reqs)
    print(lib.porla_kzg_extract_xyt_batch_device(arr, 4, 16, form, None))
    print(lib.porla_ipa_extract_xyt_batch_device(0x7000000, 0x7001000, alpha, arr, 4, 16, form, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 4


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr, keep = mx.extract_xyt_requests([good(counts=False, top_step=19), good(null_y=True, y_levels=0, null_top_y=True, top_y=0)])
    assert arr[0].write_step == 7 and arr[0].d_blocks == 0x10900000 and arr[0].d_counts is None and arr[0].y_levels == 7
    fam = ctypes.cast(arr[0].data_y, ctypes.POINTER(ctypes.c_void_p))
    assert [fam[i] for i in range(4)] == [0x10b00000, 0x10c00000, 0x10d00000, None] and len(keep) == 7
    assert arr[0].d_top_rows_y == 0x11100000 and arr[0].d_top_macs_y == 0x11200000 and arr[0].d_top_align_y == 0x11210000
    assert arr[0].d_prf_top_y == 0x11220000 and arr[0].d_top_patch == 0x11300000 and arr[0].d_row_status_top_y == 0x11400000
    assert arr[0].top_step == 19 and arr[0].top_y == 1
    assert arr[1].data_y is None and arr[1].d_top_rows_y is None and arr[1].d_top_patch is None and arr[1].top_y == 0 and arr[1].top_step == 16
    with pytest.raises(ValueError):
        mx.extract_xyt_requests([good()[:20]])
    with pytest.raises(RuntimeError, match="n_total"):
        mx.kzg_extract_xyt_batch_device([good()], 3, "exact")
    assert callable(mx.FixedBase.ipa_extract_xyt_batch_device)

"""CPU: the file extraction with the Y halves without a device.  The model the GPU tests compare against
(tests/extract_xy_model.py) on tests/update_model.py:FileModel: a level whose X half fails comes back from its Y half mod p_icc when
its bit is set and is lost as before when it is not, both halves failed is the X-only result, and a Y block whose index is ambiguous mod
p_icc is never taken.  And the C ABI (include/porla_gpu.h: porla_{kzg,ipa}_extract_xy_batch_device): symbols, layout, constants, every
refusal, k = 0, PORLA_ERR_NO_DEVICE.  Nothing here computes on a device: the pointer values are never followed."""
import ctypes
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
from tests import icc_decode_model as dm
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model
from tests import test_extract_cpu as tc

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = tc.ERR_NO_DEVICE, tc.ERR_ARG
KZG, IPA = "porla_kzg_extract_xy_batch_device", "porla_ipa_extract_xy_batch_device"
CURVES = tc.CURVES
INDICES = tc.INDICES
P, D = xm.P, xm.D


def certain_block(rng, index, n_cols):
    return [xm.chunk0_certain(rng, index)] + [rng.getrandbits(256) for _ in range(n_cols - 1)]


class WrittenXY:
    """tests/test_extract_cpu.py:Written with chunk 0 of every block in [D, p_icc) and both halves kept: files[t] is the File after
    write t, ys[t] its resident Y halves, fresh complements on every resident row of both"""

    def __init__(self, curve, n_cols=3, seed=4100):
        from tests.update_model import FileModel
        self.curve, self.n, self.n_cols = curve, 8, n_cols
        self.rng = rng = random.Random(seed)
        self.key, base, self.g = am.known_key(curve, n_cols, rng)
        self.u = [certain_block(rng, b + 1, n_cols) for b in range(self.n)]
        rows = icc_py.crebuild(self.u, curve, 0)[0]
        prf = [rng.getrandbits(128) for _ in range(self.n)]
        self.top = (am.rows_bytes(rows, "exact"), model.points_to_bytes(model.expected_macs(rows, prf, self.key)), prf, None)
        self.m = FileModel(self.n, n_cols, curve, base, fill=0xA5)
        self.blocks, self.files, self.ys = {}, {0: em.File(self.n, n_cols, curve, 8, {}, self.top)}, {0: {}}
        for step, index in enumerate(INDICES, 1):
            chunks = certain_block(rng, index, n_cols)
            self.blocks[step] = chunks
            self.m.update(chunks, am.block_mac_known(chunks, self.key, self.g))
            lower, y = {}, {}
            for i, (rows_b, macs, _) in em.lower_from_model(self.m, lambda i: None).items():
                s = [rng.getrandbits(128) for _ in range(1 << i)]
                lower[i] = (rows_b, am.add_complements(macs, s, self.key), s)
            for i, (rows_b, macs, _, align) in xm.y_from_model(self.m, lambda i: None).items():
                s = [rng.getrandbits(128) for _ in range(1 << i)]
                y[i] = (rows_b, am.add_complements(macs, s, self.key), s, align)
            self.files[step] = em.File(self.n, n_cols, curve, 8 + step, lower, self.top)
            self.ys[step] = y


@pytest.fixture(scope="module", params=CURVES)
def written(request):
    return WrittenXY(request.param)


def blk(got, slot, n_cols):
    return got["blocks"][slot * 32 * n_cols:(slot + 1) * 32 * n_cols]


def test_every_resident_y_half_satisfies_the_aligned_relation_and_decodes_mod_p(written):
    W = written
    f, y = W.files[7], W.ys[7]
    assert xm.statuses_y(f, y, 7, W.key) == bytes([1] * 7)
    assert any(a != bytes(64) for i in y for a in [y[i][3][64 * j:64 * j + 64] for j in range(1 << i)])
    for i, lo, hi in em.resident_levels(7, 8):
        got = xm.decode_y(y[i][0], 1 << i, W.n_cols, 8, [8 + lo + p for p in range(1 << i)])
        assert got == [[c % P for c in W.blocks[s]] for s in range(lo, hi + 1)], "level %d" % i


def test_a_failed_x_half_comes_back_from_its_y_half(written):
    """every t, every resident level in turn with a failed X row: bit set -> the clean extraction except that the level's winners are
    chunk mod p_icc with FOUND | RESIDUE | FROM_Y; bit clear -> em.extract with the same statuses"""
    W = written
    for t in range(1, 8):
        f, y = W.files[t], W.ys[t]
        off, rows = em.row_offsets(t, 8, True)
        clean = em.extract(f, statuses=bytes([1] * rows))
        all_y = xm.statuses_y(f, y, t, W.key)
        assert all_y == bytes([1] * t), "t = %d" % t
        for i, lo, hi in em.resident_levels(t, 8):
            what = "t = %d level %d" % (t, i)
            st = bytearray([1] * rows)
            st[off[i] + (1 << i) - 1] = 0
            st = bytes(st)
            got = xm.extract_xy(f, y, 1 << i, statuses=st, status_y=all_y)
            assert got["steps"] == clean["steps"] and got["counts"] == [1, 0, 0, 0, 0, 0], what
            assert got["row_status_y"] == bytes(1 if off[i] <= r < off[i] + (1 << i) else xm.NOT_TRIED for r in range(t)), what
            won = 0
            for slot in range(8):
                if lo <= clean["steps"][slot] <= hi:
                    won += 1
                    chunks = W.blocks[clean["steps"][slot]]
                    assert blk(got, slot, W.n_cols) == tc.chunk_bytes([c % P for c in chunks]), what
                    assert got["flags"][slot] == xm.FOUND | xm.RESIDUE | xm.FROM_Y, what
                else:
                    assert blk(got, slot, W.n_cols) == blk(clean, slot, W.n_cols) and got["flags"][slot] == clean["flags"][slot], what
            assert won, what
            # the relation itself gives the same Y statuses
            assert xm.extract_xy(f, y, 1 << i, key=W.key, statuses=st) == got, what
            # the bit clear: the call without Y halves
            for mask in (0, 0xff & ~(1 << i)):
                none = xm.extract_xy(f, y, mask, statuses=st, status_y=all_y)
                want = em.extract(f, statuses=st)
                assert {k: none[k] for k in want} == dict(want, counts=want["counts"] + [0, 0]), what


def test_both_halves_failed_is_the_x_only_result(written):
    W = written
    f, y = W.files[7], W.ys[7]
    off, rows = em.row_offsets(7, 8, True)
    for i in (0, 1, 2):
        st = bytearray([1] * rows)
        st[off[i]] = 0
        sy = bytearray([1] * 7)
        sy[off[i] + (1 << i) - 1] = 0
        got = xm.extract_xy(f, y, 7, statuses=bytes(st), status_y=bytes(sy))
        want = em.extract(f, statuses=bytes(st))
        assert {k: got[k] for k in want} == dict(want, counts=want["counts"] + [1, 0]), "level %d" % i
        assert got["row_status_y"] == bytes(sy)
        # an altered Y MAC row fails exactly its row by the relation, with the same consequence
        rows_b, macs, prf, align = y[i]
        bad = bytearray(macs)
        bad[64 * ((1 << i) - 1) + 7] ^= 1
        g = xm.extract_xy(f, {**y, i: (rows_b, bytes(bad), prf, align)}, 7, key=W.key, statuses=bytes(st))
        assert g == got, "level %d" % i
    # a damaged Y half under a clean X half costs nothing but the count
    sy = bytes([1, 1, 0, 1, 1, 1, 1])
    got = xm.extract_xy(f, y, 7, statuses=bytes([1] * rows), status_y=sy)
    want = em.extract(f, statuses=bytes([1] * rows))
    assert {k: got[k] for k in want} == dict(want, counts=[0, 0, 0, 0, 1, 0])


# ---- the ambiguous index: n_total = 4, t = 3; level 1 holds the steps 1, 2 and is Y-sourced, level 0 (step 3) is clean
def ambiguity_case(shape, curve="bn254", n_cols=2, seed=4300):
    """(File, y, expected steps, expected flags, expected counts) of a shape: step 1 a certain block, step 2 the ambiguous one, step 3
    in level 0's clean X half.
      "wrap":     chunk 0 >= p_icc naming index 1: r0 has the candidates 0 and 1, only slot 0 is doubted; step 1 holds slot 0 (older)
      "last":     chunk 0 < D naming index 4 = n_total: the candidates 4 and 5, slot 3 is doubted; step 3 holds slot 3 (newer)
      "interior": chunk 0 < D naming index 2: the slots 1 and 2 are doubted; step 3 holds slot 1 (newer), step 1 slot 2 (older)"""
    n = 4
    rng = random.Random(seed)
    rest = lambda: [rng.getrandbits(256) for _ in range(n_cols - 1)]
    if shape == "wrap":
        amb = P + (rng.randrange(1, D >> 64) << 64)
        assert P <= amb < 1 << 256 and amb & xm.M64 == 1
        first, third = 1, 2
        steps, flags = [1, 3, em.NONE, em.NONE], [xm.FOUND | xm.RESIDUE | xm.FROM_Y | xm.UNSURE, xm.FOUND, 0, 0]
    elif shape == "last":
        amb = (rng.randrange(1, D >> 64) << 64) | n
        first, third = 3, 4
        steps, flags = [em.NONE, em.NONE, 1, 3], [0, 0, xm.FOUND | xm.RESIDUE | xm.FROM_Y, xm.FOUND]
    else:
        amb = (rng.randrange(1, D >> 64) << 64) | 2
        first, third = 3, 2
        steps, flags = [em.NONE, 3, 1, em.NONE], [0, xm.FOUND, xm.FOUND | xm.RESIDUE | xm.FROM_Y | xm.UNSURE, 0]
    assert amb % P < D
    blocks = [certain_block(rng, first, n_cols), [amb] + rest(), em.with_index(third, [rng.getrandbits(256)] + rest())]
    lower = {0: (am.rows_bytes([blocks[2]], "exact"), bytes(64), [0]),
             1: (am.rows_bytes(icc_py.mix([blocks[0]], [blocks[1]], n, curve), "exact"), bytes(128), [0, 0])}
    y = {0: (am.rows_bytes(dm.level_y(blocks[2:], [3], n, curve), "residue64"), bytes(64), [0], None),
         1: (am.rows_bytes(dm.level_y(blocks[:2], [1, 2], n, curve), "residue64"), bytes(128), [0, 0], None)}
    unsure = sum(1 for x in flags if x & xm.UNSURE)
    return em.File(n, n_cols, curve, 3, lower), y, blocks, steps, flags, [1, 0, 0, flags.count(0) + unsure, 0, 1]


@pytest.mark.parametrize("shape", ["wrap", "last", "interior"])
def test_an_ambiguous_block_is_set_aside_and_doubts_its_slots(shape):
    f, y, blocks, steps, flags, counts = ambiguity_case(shape)
    got = xm.extract_xy(f, y, 2, statuses=bytes([1, 0, 1]), status_y=bytes([1, 1, 1]))
    assert got["steps"] == steps and got["flags"] == bytes(flags) and got["counts"] == counts
    assert 2 not in got["steps"]                                          # the ambiguous block is never taken
    for slot, s in enumerate(steps):
        want = bytes(64) if s == em.NONE else tc.chunk_bytes(blocks[s - 1] if s == 3 else [c % P for c in blocks[s - 1]])
        assert blk(got, slot, 2) == want, "slot %d" % slot
    # with level 1's X half clean the block is exact and bids for its slot (only in "wrap" does no newer block hold it)
    clean = xm.extract_xy(f, y, 2, statuses=bytes([1, 1, 1]), status_y=bytes([1, 1, 1]))
    assert (2 in clean["steps"]) == (shape == "wrap") and clean["counts"] == [0, 0, 0, 2, 0, 0] and not any(x & xm.UNSURE for x in clean["flags"])


def test_candidates_of_a_residue():
    n = 4
    assert xm.candidates(D, n) == (True, []) and xm.candidates(D + 1, n) == (True, []) and xm.candidates(D + 4, n) == (True, [3])
    assert xm.candidates(0, n) == (False, [1]) and xm.candidates(n, n) == (False, [n]) and xm.candidates(2, n) == (False, [2, 3])
    assert xm.candidates(xm.M64, n) == (False, []) and xm.candidates(n + 1, n) == (False, [])
    assert xm.candidates(D - 1, n) == (False, []) and xm.candidates(P - 1, n) == (True, [])


# ---- the C ABI
FIELDS = tc.FIELDS + ("data_y", "mac_y", "align_y", "d_prf_y", "d_work_y", "d_row_status_y", "y_levels")
FAKE_FB, ALPHA_BE = tc.FAKE_FB, tc.ALPHA_BE
EXACT, RESIDUE64, RESIDUE32 = tc.EXACT, tc.RESIDUE64, tc.RESIDUE32


def good(base=0x10000000, write_step=7, y_levels=7, null_y=False, **kw):
    """tests/test_extract_cpu.py:good and the Y stores behind it: level i's Y data at base + 0xb00000 + (i MiB), its MACs at base +
    0xf00000 + 64 KiB * i, its alignments at base + 0xf40000 + 64 KiB * i, 7 PRF values, work 28 KiB, statuses 7 B; counts 24 B"""
    t = write_step % 16
    fam = lambda at, step: [base + at + step * i if t >> i & 1 else 0 for i in range(4)]
    if null_y:
        return tc.good(base, write_step, **kw) + (None, None, None, 0, 0, 0, y_levels)
    return tc.good(base, write_step, **kw) + (fam(0xb00000, 0x100000), fam(0xf00000, 0x10000), fam(0xf40000, 0x10000), base + 0xf80000,
                                              base + 0x1000000, base + 0x1010000, y_levels)


def with_(r, **kw):
    r = list(r)
    for f, v in kw.items():
        r[FIELDS.index(f)] = v
    return tuple(r)


def call(reqs, n_total=16, form=EXACT, k=None, null_reqs=False, who=IPA, bases=(FAKE_FB, FAKE_FB + 0x1000), alpha=ALPHA_BE):
    from porla_amd import lib
    from porla_amd import multiexp as mx
    arr, keep = mx.extract_xy_requests(reqs)
    k = len(reqs) if k is None else k
    if who == KZG:
        return lib.porla_kzg_extract_xy_batch_device(None if null_reqs else arr, k, n_total, form, None)
    return lib.porla_ipa_extract_xy_batch_device(bases[0] or None, bases[1] or None, alpha, None if null_reqs else arr, k, n_total, form, None)


refused = tc.refused
BOTH = pytest.mark.parametrize("who", [KZG, IPA])


def test_the_symbols_are_exported():
    from porla_amd import lib
    for name in (KZG, IPA):
        assert hasattr(lib, name)


def test_the_ctypes_struct_and_constants_match_the_library():
    from porla_amd import loader
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_EXTRACT_XY_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(loader.ExtractXyReq) == size == loader.PORLA_EXTRACT_XY_REQ_BYTES == 160
    assert int(re.search(r"#define PORLA_EXTRACT_FROM_Y\s+(\d+)", header).group(1)) == 8 == loader.PORLA_EXTRACT_FROM_Y == xm.FROM_Y
    assert int(re.search(r"#define PORLA_EXTRACT_ROW_NOT_TRIED\s+(\d+)", header).group(1)) == 2 == loader.PORLA_EXTRACT_ROW_NOT_TRIED == xm.NOT_TRIED
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert offsets["data_y"] == 104 and offsets["y_levels"] == 152
    assert {f: getattr(loader.ExtractXyReq, f).offset for f, _ in loader.ExtractXyReq._fields_} == offsets
    assert [f for f, _ in loader.ExtractXyReq._fields_[:13]] == [f for f, _ in loader.ExtractReq._fields_]
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "extract_batch.hip")).read()
    struct = header[header.index("typedef struct {", header.index("PORLA_EXTRACT_XY_REQ_BYTES")):header.index("} porla_extract_xy_req;")]
    for f, off in offsets.items():
        assert "offsetof(porla_extract_xy_req, %s) == %d" % (f, off) in src
        assert re.search(r"%s;\s+/\*\s+%d[: ]" % (f, off), struct), f
    assert "Not in this call: a level's Y half" not in header


@BOTH
def test_good_arguments_pass_the_refusals(who):
    assert call([good(), good(base=0x30000000, y_levels=2)], who=who) != ERR_ARG
    assert call([good(counts=False), good(base=0x30000000, write_step=5, top=False)], who=who) != ERR_ARG


@BOTH
def test_everything_the_existing_call_refuses_is_refused(who):
    refused(call([good()], null_reqs=True, k=1, who=who), who, "NULL")
    for field in ("d_blocks", "d_steps", "d_flags", "d_prf", "d_row_status", "d_top_macs", "d_work", "data_x", "mac_x"):
        r = with_(good(base=0x30000000), **{field: None if field in ("data_x", "mac_x") else 0})
        refused(call([good(), r], who=who), who, "NULL", "request 1")
    g = good()
    fam = list(g[1])
    fam[1] = 0
    refused(call([with_(g, data_x=fam)], who=who), who, "NULL", "level 1")
    refused(call([with_(g, d_blocks=g[FIELDS.index("d_blocks")] + 8)], who=who), who, "16-byte")
    refused(call([with_(g, d_counts=g[FIELDS.index("d_counts")] + 2)], who=who), who, "4-byte")
    refused(call([g], n_total=1000, who=who), who, "n_total")
    refused(call([g], form=RESIDUE64, who=who), who, "top_form")
    refused(call([with_(g, d_work=g[FIELDS.index("d_blocks")])], who=who), who, "overlaps")
    refused(call([with_(g, d_top_rows=(1 << 64) - 64)], who=who), who, "overflow")


@BOTH
@pytest.mark.parametrize("field", ["data_y", "mac_y", "align_y", "d_prf_y", "d_work_y", "d_row_status_y"])
def test_a_null_y_pointer_with_a_level_to_try_is_refused(who, field):
    r = with_(good(base=0x30000000), **{field: None if field in ("data_y", "mac_y", "align_y") else 0})
    refused(call([good(), r], who=who), who, "NULL", "request 1", field)
    assert call([good(), with_(r, y_levels=8)], who=who) != ERR_ARG           # (level 3 is not resident at t = 7: nothing to try)
    assert call([good(), with_(r, y_levels=0)], who=who) != ERR_ARG


@BOTH
def test_a_tried_level_with_a_null_entry_is_refused(who):
    g = good()
    for f in ("data_y", "mac_y"):
        for level in (0, 1, 2):
            fam = list(g[FIELDS.index(f)])
            fam[level] = 0
            refused(call([with_(g, **{f: fam})], who=who), who, "NULL", "level %d" % level)
            assert call([with_(g, **{f: fam}, y_levels=7 & ~(1 << level))], who=who) != ERR_ARG
    assert call([with_(g, align_y=[0, 0, 0, 0])], who=who) != ERR_ARG          # an alignment entry may be 0: all at infinity


@BOTH
def test_no_level_to_try_needs_no_y_pointer(who):
    assert call([good(null_y=True, y_levels=0)], who=who) != ERR_ARG
    assert call([good(null_y=True, y_levels=8)], who=who) != ERR_ARG           # y_levels & t == 0
    assert call([good(null_y=True, write_step=32, y_levels=(1 << 64) - 1)], who=who) != ERR_ARG
    refused(call([good(null_y=True, y_levels=1)], who=who), who, "NULL")


@BOTH
def test_a_misaligned_y_pointer_is_refused(who):
    g = good()
    i = FIELDS.index
    for f in ("d_prf_y", "d_work_y"):
        refused(call([with_(g, **{f: g[i(f)] + 8})], who=who), who, "16-byte", "request 0", f)
        refused(call([with_(g, **{f: g[i(f)] + 8}, y_levels=0)], who=who), who, "16-byte", f)      # whenever the pointer is given
    for f in ("data_y", "mac_y", "align_y"):
        fam = list(g[i(f)])
        fam[1] += 8
        refused(call([with_(g, **{f: fam})], who=who), who, "16-byte", "request 0", f)
    assert call([with_(g, d_row_status_y=g[i("d_row_status_y")] + 1)], who=who) != ERR_ARG


@BOTH
def test_a_y_byte_size_that_wraps_is_refused(who):
    g = good()
    for f in ("d_prf_y", "d_work_y"):
        refused(call([with_(g, **{f: (1 << 64) - 64})], who=who), who, "overflow")
    refused(call([with_(g, d_row_status_y=(1 << 64) - 3)], who=who), who, "overflow")
    assert call([with_(g, d_row_status_y=(1 << 64) - 23)], who=who) != ERR_ARG
    for f in ("data_y", "mac_y", "align_y"):
        fam = list(g[FIELDS.index(f)])
        fam[2] = (1 << 64) - 64
        refused(call([with_(g, **{f: fam})], who=who), who, "overflow")
    refused(call([with_(g, d_counts=(1 << 64) - 20)], who=who), who, "overflow")      # six words
    assert call([with_(g, d_counts=(1 << 64) - 40)], who=who) != ERR_ARG


@BOTH
def test_the_y_outputs_count_in_the_overlap_walk(who):
    a, b = good(), good(base=0x50000000)
    i = FIELDS.index
    run = lambda reqs: call(reqs, who=who)
    refused(run([with_(a, d_work_y=a[i("d_work")])]), who, "overlaps")
    refused(run([with_(a, d_work_y=a[i("data_y")][2])]), who, "overlaps")
    refused(run([with_(a, d_row_status_y=a[i("d_prf_y")] + 7 * 16 - 1)]), who, "overlaps")
    assert run([with_(a, d_row_status_y=a[i("d_prf_y")] + 7 * 16)]) != ERR_ARG                # back to back is fine
    refused(run([with_(a, d_row_status_y=a[i("mac_y")][2] + 255)]), who, "overlaps")
    refused(run([with_(a, d_row_status_y=a[i("align_y")][1] + 127)]), who, "overlaps")
    refused(run([with_(a, d_flags=a[i("align_y")][2])]), who, "overlaps")
    refused(run([with_(a, d_row_status_y=a[i("d_row_status")] + 22)]), who, "overlaps")
    refused(run([with_(a, d_steps=a[i("d_counts")] + 20)]), who, "overlaps")                 # the six-word d_counts is 24 bytes
    assert run([with_(a, d_steps=a[i("d_counts")] + 24)]) != ERR_ARG
    # across requests
    refused(run([a, with_(b, d_work_y=a[i("d_work_y")] + 32)]), who, "overlaps")
    refused(run([a, with_(b, d_row_status_y=a[i("d_row_status_y")] + 6)]), who, "overlaps")
    # the Y inputs may be shared
    assert run([a, with_(b, data_y=a[i("data_y")], mac_y=a[i("mac_y")], align_y=a[i("align_y")], d_prf_y=a[i("d_prf_y")])]) != ERR_ARG


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
    """in a child process that sees no device: valid arguments (both builds, both top forms, Y halves tried and not) return
    PORLA_ERR_NO_DEVICE"""
    code = r"""
import sys
sys.path.insert(0, %r)
from porla_amd import lib
from porla_amd import multiexp as mx
from tests.test_extract_xy_cpu import good
alpha = (7).to_bytes(32, "big")
for form in (0, 2):
    reqs = [good(), good(base=0x30000000, write_step=5, y_levels=4, align=False, counts=False),
            good(base=0x50000000, write_step=22, top=False, null_y=True, y_levels=0), good(base=0x70000000, null_y=True, y_levels=8)]
    arr, keep = mx.extract_xy_requests(reqs)
    print(lib.porla_kzg_extract_xy_batch_device(arr, 4, 16, form, None))
    print(lib.porla_ipa_extract_xy_batch_device(0x7000000, 0x7001000, alpha, arr, 4, 16, form, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 4


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr, keep = mx.extract_xy_requests([good(counts=False), good(null_y=True, y_levels=0)])
    assert arr[0].write_step == 7 and arr[0].d_blocks == 0x10900000 and arr[0].d_counts is None and arr[0].y_levels == 7
    fam = ctypes.cast(arr[0].data_y, ctypes.POINTER(ctypes.c_void_p))
    assert [fam[i] for i in range(4)] == [0x10b00000, 0x10c00000, 0x10d00000, None] and len(keep) == 7
    assert arr[0].d_prf_y == 0x10f80000 and arr[0].d_work_y == 0x11000000 and arr[0].d_row_status_y == 0x11010000
    assert arr[1].data_y is None and arr[1].align_y is None and arr[1].d_work_y is None and arr[1].y_levels == 0
    with pytest.raises(ValueError):
        mx.extract_xy_requests([good()[:13]])
    with pytest.raises(RuntimeError, match="n_total"):
        mx.kzg_extract_xy_batch_device([good()], 3, "exact")
    assert callable(mx.FixedBase.ipa_extract_xy_batch_device)

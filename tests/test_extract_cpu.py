"""CPU: the verified file extraction without a device.  The model the GPU tests compare against (tests/extract_model.py) returns
exactly the last written chunks per index after every write of a file that overwrites some indices several times and leaves others
in the top level only; its level occupancy and write-step ranges are those of tests/update_model.py:FileModel; a failed level gives
no block and marks the slots it could have held a newer copy of.  And the C ABI (include/porla_gpu.h: porla_{kzg,ipa}_extract_batch_device)
exports its symbols, has the layout the library static_asserts, refuses every bad argument with PORLA_ERR_ARG before the device is
touched, returns 0 for k = 0 and PORLA_ERR_NO_DEVICE for valid arguments without a device.  Nothing here computes on a device: the
pointer values are never followed."""
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
from tests import retrieve_aligned_model as am
from tests import retrieve_model as model

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
KZG, IPA = "porla_kzg_extract_batch_device", "porla_ipa_extract_batch_device"
CURVES = ("bn254", "secp256k1")
EXACT, RESIDUE64, RESIDUE32 = 0, 1, 2
INDICES = [3, 5, 3, 1, 5, 5, 3]           # writes 1 .. 7: 3 in levels 0, 1 and 2 at t = 7; 5 twice inside level 1 (steps 5, 6); 2, 4, 6, 7, 8 never


# ---- the model
def chunk_bytes(chunks):
    return b"".join(c.to_bytes(32, "little") for c in chunks)


class Written:
    """a file of n_total = 8 on the models: a top level holding U (block b names index b + 1), then the writes of INDICES through
    FileModel with known logarithms; after(t) is the File after write t with fresh complements on every resident row"""

    def __init__(self, curve, n_cols=3, seed=3100):
        from tests.update_model import FileModel
        self.curve, self.n, self.n_cols = curve, 8, n_cols
        self.rng = rng = random.Random(seed)
        self.key, base, self.g = am.known_key(curve, n_cols, rng)
        self.u = [em.with_index(b + 1, [rng.getrandbits(256) for _ in range(n_cols)]) for b in range(self.n)]
        rows = icc_py.crebuild(self.u, curve, 0)[0]
        prf = [rng.getrandbits(128) for _ in range(self.n)]
        self.top = (am.rows_bytes(rows, "exact"), model.points_to_bytes(model.expected_macs(rows, prf, self.key)), prf, None)
        self.m = FileModel(self.n, n_cols, curve, base, fill=0xA5)
        self.blocks, self.files = {}, {0: em.File(self.n, n_cols, curve, 8, {}, self.top)}
        for step, index in enumerate(INDICES, 1):
            chunks = em.with_index(index, [rng.getrandbits(256) for _ in range(n_cols)])
            self.blocks[step] = chunks
            self.m.update(chunks, am.block_mac_known(chunks, self.key, self.g))
            lower = {}
            for i, (rows_b, macs, _) in em.lower_from_model(self.m, lambda i: None).items():
                s = [rng.getrandbits(128) for _ in range(1 << i)]
                lower[i] = (rows_b, am.add_complements(macs, s, self.key), s)
            self.files[step] = em.File(self.n, n_cols, curve, step, lower, self.top)

    def want(self, t):
        """(chunks, rank) per slot: the last write of the index among the steps 1 .. t, else U"""
        out = [(self.u[b], 0) for b in range(self.n)]
        for step in range(1, t + 1):
            out[INDICES[step - 1] - 1] = (self.blocks[step], step)
        return out


@pytest.fixture(scope="module", params=CURVES)
def written(request):
    return Written(request.param)


def test_the_model_returns_the_last_written_chunks_for_every_t(written):
    W = written
    for t in range(8):
        f = W.files[t]
        got = em.extract(f, W.key)
        rows = t + 8
        assert got["row_status"] == bytes([1] * rows), "t = %d" % t
        assert got["blocks"] == b"".join(chunk_bytes(c) for c, _ in W.want(t)), "t = %d" % t
        assert got["steps"] == [r for _, r in W.want(t)]
        assert got["flags"] == bytes([em.FOUND] * 8) and got["counts"] == [0, 0, 0, 0]
        assert len(f.prf_values()) == rows


def test_without_a_top_level_the_unwritten_slots_are_empty(written):
    W = written
    f = W.files[7]
    got = em.extract(em.File(8, W.n_cols, W.curve, 7, f.lower, None), W.key)
    for slot, (chunks, rank) in enumerate(W.want(7)):
        blk = got["blocks"][slot * 32 * W.n_cols:(slot + 1) * 32 * W.n_cols]
        if rank:
            assert blk == chunk_bytes(chunks) and got["steps"][slot] == rank and got["flags"][slot] == em.FOUND
        else:
            assert blk == bytes(32 * W.n_cols) and got["steps"][slot] == em.NONE and got["flags"][slot] == 0
    assert got["counts"] == [0, 0, 0, 5]


def test_occupancy_and_write_step_ranges_are_the_file_model_s():
    """n_total = 16, every t: the resident levels are FileModel's non-empty ones, and the X half of level i decodes to the blocks of the
    steps hi_i - 2^i + 1 .. hi_i in write order -- the facts the call's rank rests on"""
    from tests.update_model import FileModel
    n, n_cols, curve = 16, 1, "bn254"
    rng = random.Random(3200)
    base = am.known_key(curve, n_cols, rng)[1]
    m = FileModel(n, n_cols, curve, base)
    blocks = {}
    assert em.resident_levels(0, n) == []
    for t in range(1, n):
        blocks[t] = [rng.getrandbits(256)]
        m.update(blocks[t], None)
        res = em.resident_levels(t, n)
        assert [i for i, _, _ in res] == [i for i, e in enumerate(m.empty) if not e]
        assert sorted(s for _, lo, hi in res for s in range(lo, hi + 1)) == list(range(1, t + 1))
        for i, lo, hi in res:
            assert hi - lo + 1 == 1 << i and hi == t >> i << i
            got, bad = em.decode_level(bytes(m.fam["data_x"][i][:(1 << i) * n_cols * 64]), 1 << i, n_cols, n, curve)
            assert got == [blocks[s] for s in range(lo, hi + 1)] and bad == 0
        off, rows = em.row_offsets(t, n, True)
        assert rows == t + n and off["top"] == t and all(off[i] == t & ((1 << i) - 1) for i, _, _ in res)


def test_a_failed_level_gives_no_block_and_marks_what_it_could_hold(written):
    """t = 7 with a top level, the statuses given: slot 3 - 1 is won by step 7 (level 0), 5 - 1 by step 6 (level 1), 1 - 1 by step 4 (level 2)"""
    W = written
    f = W.files[7]
    clean = em.extract(f, W.key)
    off, rows = em.row_offsets(7, 8, True)
    assert off == {0: 0, 1: 1, 2: 3, "top": 7} and rows == 15

    def run(bad_row):
        st = bytearray([1] * rows)
        st[bad_row] = 0
        return em.extract(f, statuses=bytes(st))

    blk = lambda got, slot: got["blocks"][slot * 32 * W.n_cols:(slot + 1) * 32 * W.n_cols]
    # level 0 fails (hi = 7): slot 2 falls back to step 3 (level 2); every slot is older than step 7 -> all UNSURE
    got = run(0)
    assert got["steps"] == [4, 0, 3, 0, 6, 0, 0, 0] and blk(got, 2) == chunk_bytes(W.blocks[3])
    assert got["flags"] == bytes([em.FOUND | em.UNSURE] * 8) and got["counts"] == [1, 0, 0, 8]
    # level 1 fails (hi = 6): slot 4 falls back to step 2; slot 2 (step 7) is newer than the failed level -> no UNSURE there
    got = run(2)
    assert got["steps"] == [4, 0, 7, 0, 2, 0, 0, 0] and blk(got, 4) == chunk_bytes(W.blocks[2])
    assert got["flags"] == bytes([em.FOUND | (0 if s == 2 else em.UNSURE) for s in range(8)]) and got["counts"] == [1, 0, 0, 7]
    # level 2 fails (hi = 4): slot 0 falls back to U; the winners of steps 7 and 6 carry no UNSURE
    got = run(5)
    assert got["steps"] == [0, 0, 7, 0, 6, 0, 0, 0] and blk(got, 0) == chunk_bytes(W.u[0])
    assert got["flags"] == bytes([em.FOUND | (0 if s in (2, 4) else em.UNSURE) for s in range(8)]) and got["counts"] == [1, 0, 0, 6]
    # the top level fails (highest step 0): only the slots without any winner are UNSURE, and they are zeroed
    got = run(9)
    assert got["steps"] == [4, em.NONE, 7, em.NONE, 6, em.NONE, em.NONE, em.NONE]
    assert got["flags"] == bytes([em.FOUND if s in (0, 2, 4) else em.UNSURE for s in range(8)]) and got["counts"] == [1, 0, 0, 5]
    assert blk(got, 1) == bytes(32 * W.n_cols) and blk(got, 0) == blk(clean, 0)
    # an altered symbol fails exactly its row by the relation itself, with the same consequence
    rows_b, macs, prf = f.lower[1]
    bad = bytearray(rows_b)
    bad[64 * W.n_cols + 5] ^= 1
    g = em.extract(em.File(8, W.n_cols, W.curve, 7, {**f.lower, 1: (bytes(bad), macs, prf)}, f.top), W.key)
    want = run(2)
    assert g["row_status"] == want["row_status"] and g["steps"] == want["steps"] and g["flags"] == want["flags"]


def test_indices_out_of_range_are_counted_and_dropped():
    """on the decode alone (statuses given): blocks naming 0 and n_total + 1 in level 1"""
    n, n_cols, curve = 4, 2, "bn254"
    rng = random.Random(3300)
    blocks = [em.with_index(i, [rng.getrandbits(256) for _ in range(n_cols)]) for i in (0, n + 1, 2)]
    lower = {0: (am.rows_bytes([blocks[2]], "exact"), bytes(64), [0]),
             1: (am.rows_bytes(icc_py.mix([blocks[0]], [blocks[1]], n, curve), "exact"), bytes(128), [0, 0])}
    got = em.extract(em.File(n, n_cols, curve, 3, lower), statuses=bytes([1, 1, 1]))
    assert got["counts"] == [0, 0, 2, 3] and got["steps"] == [em.NONE, 3, em.NONE, em.NONE]
    assert got["flags"] == bytes([0, em.FOUND, 0, 0]) and got["blocks"][64:128] == chunk_bytes(blocks[2])
    # level 0's decode is the low 32 bytes; a nonzero upper half is a bad symbol
    sym = bytearray(lower[0][0])
    sym[64 + 40] = 1
    got = em.extract(em.File(n, n_cols, curve, 3, {**lower, 0: (bytes(sym), bytes(64), [0])}), statuses=bytes([1, 1, 1]))
    assert got["counts"] == [0, 1, 2, 3] and got["blocks"][64:128] == chunk_bytes(blocks[2])


# ---- the C ABI
FIELDS = ("write_step", "data_x", "mac_x", "d_top_rows", "d_top_macs", "d_top_align", "d_prf", "d_work", "d_blocks", "d_steps", "d_flags",
          "d_row_status", "d_counts")
FAKE_FB = 0x7000000        # a base pointer the refusals never follow
ALPHA_BE = (12345).to_bytes(32, "big")


def good(base=0x10000000, write_step=7, top=True, align=True, counts=True, levels=None):
    """n_total = 16, t = 7, 128 columns: level i's data at base + (i + 1) MiB (8 KiB << i), its MACs at base + 5 MiB + 64 KiB * i; top rows
    128 KiB, top MACs and alignments 1 KiB each, 23 PRF values, work 28 KiB, blocks 64 KiB, steps 64 B, flags 16 B, statuses 23 B, counts 16 B"""
    t = write_step % 16
    data = [base + 0x100000 * (i + 1) if t >> i & 1 else 0 for i in range(4)]
    macs = [base + 0x500000 + 0x10000 * i if t >> i & 1 else 0 for i in range(4)]
    if levels is not None:
        data, macs = levels
    return (write_step, data, macs, base + 0x600000 if top else 0, base + 0x700000 if top else 0, base + 0x710000 if top and align else 0,
            base + 0x720000, base + 0x800000, base + 0x900000, base + 0xa00000, base + 0xa10000, base + 0xa20000,
            base + 0xa30000 if counts else 0)


def with_(r, **kw):
    r = list(r)
    for f, v in kw.items():
        r[FIELDS.index(f)] = v
    return tuple(r)


def call(reqs, n_total=16, form=EXACT, k=None, null_reqs=False, who=IPA, bases=(FAKE_FB, FAKE_FB + 0x1000), alpha=ALPHA_BE):
    from porla_amd import lib
    from porla_amd import multiexp as mx
    arr, keep = mx.extract_requests(reqs)
    k = len(reqs) if k is None else k
    if who == KZG:
        return lib.porla_kzg_extract_batch_device(None if null_reqs else arr, k, n_total, form, None)
    return lib.porla_ipa_extract_batch_device(bases[0] or None, bases[1] or None, alpha, None if null_reqs else arr, k, n_total, form, None)


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
    for name in (KZG, IPA):
        assert hasattr(lib, name)


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd import loader
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_EXTRACT_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(loader.ExtractReq) == size == loader.PORLA_EXTRACT_REQ_BYTES == 104
    for name, v in (("FOUND", em.FOUND), ("UNSURE", em.UNSURE), ("RESIDUE", em.RESIDUE)):
        assert int(re.search(r"#define PORLA_EXTRACT_%s\s+(\d+)" % name, header).group(1)) == v == getattr(loader, "PORLA_EXTRACT_" + name)
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert {f: getattr(loader.ExtractReq, f).offset for f, _ in loader.ExtractReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "extract_batch.hip")).read()
    for f, off in offsets.items():
        assert "offsetof(porla_extract_req, %s) == %d" % (f, off) in src
        assert re.search(r"%s;\s+/\*\s+%d[: ]" % (f, off), header), f


@BOTH
def test_null_reqs_is_refused(who):
    refused(call([good()], null_reqs=True, k=1, who=who), who, "NULL")


@BOTH
@pytest.mark.parametrize("field", ["d_blocks", "d_steps", "d_flags", "d_prf", "d_row_status", "d_top_macs", "d_work", "data_x", "mac_x"])
def test_a_null_required_pointer_is_refused(who, field):
    r = with_(good(base=0x30000000), **{field: None if field in ("data_x", "mac_x") else 0})
    refused(call([good(), r], who=who), who, "NULL", "request 1")


@BOTH
def test_a_resident_level_with_a_null_pointer_is_refused(who):
    g = good()
    for f in ("data_x", "mac_x"):
        for level in (0, 1, 2):
            fam = list(g[FIELDS.index(f)])
            fam[level] = 0
            refused(call([with_(g, **{f: fam})], who=who), who, "NULL", "level %d" % level)
    assert g[1][3] == 0 and call([g], who=who) != ERR_ARG                  # (level 3 is not resident at t = 7: its entries are ignored)


@BOTH
def test_t_zero_needs_no_lower_levels_and_no_work(who):
    r = with_(good(write_step=32), data_x=None, mac_x=None, d_work=0)
    assert call([r], who=who) != ERR_ARG
    # nothing resident at all: no rows, so no PRF values and no statuses either
    assert call([with_(good(write_step=16, top=False), data_x=None, mac_x=None, d_work=0, d_prf=0, d_row_status=0)], who=who) != ERR_ARG
    refused(call([with_(good(write_step=33), data_x=None)], who=who), who, "NULL")


@BOTH
@pytest.mark.parametrize("field,off,word", [("d_top_rows", 8, "16-byte"), ("d_top_macs", 8, "16-byte"), ("d_top_align", 8, "16-byte"),
                                            ("d_prf", 8, "16-byte"), ("d_work", 8, "16-byte"), ("d_blocks", 8, "16-byte"),
                                            ("d_steps", 2, "4-byte"), ("d_counts", 2, "4-byte")])
def test_a_misaligned_pointer_is_refused(who, field, off, word):
    g = good()
    refused(call([with_(g, **{field: g[FIELDS.index(field)] + off})], who=who), who, word, "request 0")
    for f in ("data_x", "mac_x"):
        fam = list(g[FIELDS.index(f)])
        fam[1] += 8
        refused(call([with_(g, **{f: fam})], who=who), who, "16-byte", "request 0")
    i = FIELDS.index
    assert call([with_(g, d_row_status=g[i("d_row_status")] + 1, d_flags=g[i("d_flags")] + 1, d_steps=g[i("d_steps")] + 4)], who=who) != ERR_ARG


@BOTH
@pytest.mark.parametrize("n_total", [0, 1, 3, 1000, (1 << 16) + 1, 1 << 17])
def test_a_bad_n_total_is_refused(who, n_total):
    refused(call([good()], n_total=n_total, who=who), who, "n_total")


@BOTH
@pytest.mark.parametrize("form", [-1, RESIDUE64, 3])
def test_a_bad_top_form_is_refused(who, form):
    refused(call([good()], form=form, who=who), who, "top_form")
    assert call([good()], form=RESIDUE32, who=who) != ERR_ARG


@BOTH
def test_an_output_overlapping_anything_is_refused(who):
    a, b = good(), good(base=0x50000000)
    i = FIELDS.index
    run = lambda reqs: call(reqs, who=who)
    refused(run([with_(a, d_row_status=a[i("d_top_macs")])]), who, "overlaps")
    refused(run([with_(a, d_row_status=a[i("d_prf")] + 23 * 16 - 1)]), who, "overlaps")
    assert run([with_(a, d_row_status=a[i("d_prf")] + 23 * 16)]) != ERR_ARG                  # back to back is fine
    refused(run([with_(a, d_flags=a[i("mac_x")][2] + 255)]), who, "overlaps")                # level 2: four MAC rows
    assert run([with_(a, d_flags=a[i("mac_x")][2] + 256)]) != ERR_ARG
    refused(run([with_(a, d_counts=a[i("d_top_align")] + 1020)]), who, "overlaps")
    refused(run([with_(a, d_counts=a[i("d_steps")] + 60)]), who, "overlaps")
    assert run([with_(a, d_counts=a[i("d_steps")] + 64)]) != ERR_ARG
    refused(run([with_(a, d_steps=a[i("d_flags")] + 12)]), who, "overlaps")
    refused(run([with_(a, d_blocks=a[i("data_x")][0])]), who, "overlaps")
    refused(run([with_(a, d_blocks=a[i("d_top_rows")])]), who, "overlaps")
    refused(run([with_(a, d_work=a[i("d_blocks")])]), who, "overlaps")                       # d_work counts as an output
    refused(run([with_(a, d_work=a[i("data_x")][2])]), who, "overlaps")
    # across requests
    refused(run([a, with_(b, d_flags=a[i("d_flags")] + 8)]), who, "overlaps")
    refused(run([a, with_(b, d_work=a[i("d_work")] + 32)]), who, "overlaps")
    refused(run([a, with_(b, d_counts=a[i("d_prf")])]), who, "overlaps")
    # inputs may be shared
    assert run([a, with_(b, data_x=a[i("data_x")], mac_x=a[i("mac_x")], d_top_rows=a[i("d_top_rows")], d_top_macs=a[i("d_top_macs")],
                         d_top_align=a[i("d_top_align")], d_prf=a[i("d_prf")])]) != ERR_ARG


@BOTH
def test_too_many_requests_are_refused(who):
    from porla_amd import lib
    from porla_amd.loader import ExtractReq
    k = 65536
    arr = (ExtractReq * k)()
    for j in range(k):
        b = 0x100000000 + 0x10000 * j                                     # n_total = 2, t = 0, a top level of two rows
        arr[j] = ExtractReq(0, None, None, b, b + 0x4000, None, b + 0x5000, None, b + 0x6000, b + 0xa000, b + 0xa100, b + 0xa200, None)
    if who == KZG:
        run = lambda kk: lib.porla_kzg_extract_batch_device(arr, kk, 2, EXACT, None)
    else:
        run = lambda kk: lib.porla_ipa_extract_batch_device(FAKE_FB, FAKE_FB + 0x1000, ALPHA_BE, arr, kk, 2, EXACT, None)
    refused(run(k), who, "65535")
    assert run(k - 1) != ERR_ARG


@BOTH
def test_a_byte_size_that_overflows_is_refused(who):
    high = (1 << 64) - 64                                                 # (the KZG build sizes the rows by its SRS, by one column without one)
    a = good()
    for f in ("d_top_rows", "d_top_macs", "d_top_align", "d_work", "d_blocks"):
        refused(call([with_(a, **{f: high})], who=who), who, "overflow")
    for f, last, step in (("d_prf", 23 * 16, 16), ("d_row_status", 23, 4), ("d_counts", 16, 4), ("d_steps", 64, 4), ("d_flags", 16, 4)):
        refused(call([with_(a, **{f: (1 << 64) - last + step})], who=who), who, "overflow")
        assert call([with_(a, **{f: (1 << 64) - last - 16})], who=who) != ERR_ARG
    fam = list(a[2])
    fam[2] = (1 << 64) - 64
    refused(call([with_(a, mac_x=fam)], who=who), who, "overflow")


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
    """in a child process that sees no device: valid arguments (both builds, both top forms, with and without a top level, an alignment
    store, counters and lower levels) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import sys
sys.path.insert(0, %r)
from porla_amd import lib
from porla_amd import multiexp as mx
from tests.test_extract_cpu import good, with_
alpha = (7).to_bytes(32, "big")
for form in (0, 2):
    reqs = [good(), good(base=0x30000000, write_step=5, align=False, counts=False), good(base=0x50000000, write_step=22, top=False),
            with_(good(base=0x70000000, write_step=16), data_x=None, mac_x=None, d_work=0)]
    arr, keep = mx.extract_requests(reqs)
    print(lib.porla_kzg_extract_batch_device(arr, 4, 16, form, None))
    print(lib.porla_ipa_extract_batch_device(0x7000000, 0x7001000, alpha, arr, 4, 16, form, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 4


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr, keep = mx.extract_requests([good(counts=False), with_(good(write_step=16), data_x=None, mac_x=None)])
    assert arr[0].write_step == 7 and arr[0].d_top_rows == 0x10600000 and arr[0].d_counts is None and arr[0].d_blocks == 0x10900000
    fam = ctypes.cast(arr[0].data_x, ctypes.POINTER(ctypes.c_void_p))
    assert [fam[i] for i in range(4)] == [0x10100000, 0x10200000, 0x10300000, None] and len(keep) == 2
    assert arr[1].data_x is None and arr[1].mac_x is None
    with pytest.raises(ValueError):
        mx.extract_requests([good()[:12]])
    with pytest.raises(RuntimeError, match="n_total"):
        mx.kzg_extract_batch_device([good()], 3, "exact")
    with pytest.raises(RuntimeError, match="top_form"):
        mx.kzg_extract_batch_device([good()], 16, "residue64")
    with pytest.raises(KeyError):
        mx.kzg_extract_batch_device([good()], 16, "residue16")
    assert callable(mx.FixedBase.ipa_extract_batch_device)

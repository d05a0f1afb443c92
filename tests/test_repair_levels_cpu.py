"""CPU: the lower-level repair without a device.  The two facts the call rests on, on stores made by tests/update_model.py (FileModel:
HAdd and the chain of HRebuild mixes), both curves, n_total 8 and 2, every t: every resident lower half equals the ONE-SHOT network
over its blocks (X) and over the rows y_p (Y), and every Y alignment row equals the commitment of the networked c_p row.  The model the
GPU tests lean on (tests/repair_levels_model.py) against rules 2 .. 7 of the header: a damaged store comes back as the pristine bytes;
the X_DAMAGED and the INCONSISTENT case.  And the C ABI (include/porla_gpu.h: porla_{kzg,ipa}_repair_levels_batch_device,
porla_repair_levels_work_bytes): symbols, layout, the work size against its documented formula, every refusal, k = 0,
PORLA_ERR_NO_DEVICE.  Nothing here computes on a device: the pointer values are never followed."""
import ctypes
import functools
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
import icc_py
from tests import mac_decode_model as mdm
from tests import repair_levels_model as rl
from tests import retrieve_aligned_model as am
from tests import test_extract_cpu as tc
from tests.update_model import FileModel, pt_tuple

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = tc.ERR_NO_DEVICE, tc.ERR_ARG
KZG, IPA = "porla_kzg_repair_levels_batch_device", "porla_ipa_repair_levels_batch_device"
CURVES = tc.CURVES
N_COLS = 3
DATA, MAC, ALIGN = rl.DATA, rl.MAC, rl.ALIGN
ALL = (1 << 64) - 1


# ---- the model facts
@functools.lru_cache(maxsize=None)
def written(curve, n):
    """a FileModel after each of the writes 1 .. n - 1 with known logarithms: (key, commit, blocks by step, {t: {level: the halves}})"""
    rnd = random.Random(9100 + n)
    key, base, g = am.known_key(curve, N_COLS, rnd)
    q, G = icc_py.Q[curve], mdm.GEN[curve]
    commit = lambda scalars: icc_py.ec_mul(curve, G, sum(c * x for c, x in zip(scalars, g)) % q)
    m = FileModel(n, N_COLS, curve, base)
    blocks, snaps = {}, {}
    for s in range(1, n):
        blocks[s] = [rnd.getrandbits(256) for _ in range(N_COLS)]
        m.update(blocks[s], am.block_mac_known(blocks[s], key, g))
        fam = m.family_bytes()
        snaps[s] = {i: {"x": (fam["data_x"][i][:(64 * N_COLS) << i], fam["mac_x"][i][:64 << i], [0] * (1 << i)),
                        "y": (fam["data_y"][i][:(64 * N_COLS) << i], fam["mac_y"][i][:64 << i], [0] * (1 << i), fam["align_y"][i][:64 << i])}
                    for i in range(n.bit_length() - 1) if s >> i & 1}
    return key, commit, blocks, snaps


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [8, 2])
def test_every_resident_half_is_the_one_shot_network(curve, n):
    """fact 1: the chain of mixes Server::HRebuild runs and the one-shot network agree symbol for symbol, below LCM"""
    key, commit, blocks, snaps = written(curve, n)
    for t in range(1, n):
        for i, lv in snaps[t].items():
            steps = rl.level_steps(t, n, i)
            chunks = [blocks[s] for s in steps]
            assert am.rows_of(lv["x"][0], N_COLS, "exact") == rl.network(chunks, curve), (t, i)
            assert am.rows_of(lv["y"][0], N_COLS, "exact") == rl.y_half(chunks, steps, n, curve), (t, i)
            assert rl.decode_x(am.rows_of(lv["x"][0], N_COLS, "exact"), curve) == (chunks, 0), (t, i)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [8, 2])
def test_every_y_alignment_row_is_the_commitment_of_the_networked_c_row(curve, n):
    """fact 2: the point network over Commit(c_p) is Commit of the data network's q plane over the rows c_p"""
    key, commit, blocks, snaps = written(curve, n)
    some = False
    for t in range(1, n):
        for i, lv in snaps[t].items():
            steps = rl.level_steps(t, n, i)
            rows = rl.align_scalars([blocks[s] for s in steps], steps, n, curve)
            for j, r in enumerate(rows):
                assert pt_tuple(lv["y"][3][64 * j:64 * j + 64]) == commit(r), (t, i, j)
                some = some or commit(r) is not None
    assert some


def test_the_level_steps_are_rule_3y():
    assert rl.level_steps(8 + 7, 8, 0) == [15] and rl.level_steps(8 + 7, 8, 1) == [13, 14] and rl.level_steps(8 + 7, 8, 2) == [9, 10, 11, 12]
    assert rl.level_steps(6, 8, 1) == [5, 6] and rl.level_steps(6, 8, 2) == [1, 2, 3, 4]


def flip(b, at, bit=1):
    b = bytearray(b)
    b[at] ^= bit
    return bytes(b)


def with_y(levels, i, data=None, macs=None, align=None, x_data=None):
    x, y = levels[i]["x"], levels[i]["y"]
    return {**levels, i: {"x": (x[0] if x_data is None else x_data, x[1], x[2]),
                          "y": (y[0] if data is None else data, y[1] if macs is None else macs, y[2], y[3] if align is None else align)}}


def pristine_y(levels):
    return {i: (lv["y"][0], lv["y"][1], lv["y"][3]) for i, lv in levels.items()}


@pytest.mark.parametrize("curve", CURVES)
def test_the_model_follows_rules_2_to_7(curve):
    n, t = 8, 7
    key, commit, blocks, snaps = written(curve, n)
    levels = snaps[t]
    run = lambda lv, mask=ALL: rl.repair_levels(lv, n, N_COLS, curve, t, mask, commit, key=key)
    got = run(levels)
    assert got["status_x"] == got["status_y"] == bytes([1] * 7) and got["action_y"] == bytes(7) and got["counts"] == [0] * 8
    assert got["level"] == bytes([rl.CLEAN] * 3 + [0] * 13) and got["y"] == pristine_y(levels)
    rb = 64 * N_COLS
    d, mc, _, al = levels[2]["y"]
    cases = [(dict(data=flip(d, rb + 70)), DATA), (dict(macs=flip(mc, 64 + 9)), MAC), (dict(align=flip(al, 64 + 40)), ALIGN),
             (dict(data=flip(d, rb + 1), macs=flip(mc, 64 + 63, 0x80), align=flip(al, 64)), DATA | MAC | ALIGN)]
    for change, bits in cases:
        got = run(with_y(levels, 2, **change))
        assert got["status_y"] == bytes([1, 1, 1, 1, 0, 1, 1]) and got["action_y"] == bytes([0, 0, 0, 0, bits, 0, 0]), sorted(change)
        assert got["level"] == bytes([rl.CLEAN, rl.CLEAN, rl.REPAIRED] + [0] * 13) and got["y"] == pristine_y(levels), sorted(change)
        assert got["counts"] == [0, 1, bits & 1, bits >> 3, (bits >> 1) & 1, 1, 0, 0], sorted(change)
    # no witness: every row of the half damaged
    bad = d
    for j in range(4):
        bad = flip(bad, j * rb + 5 * j)
    got = run(with_y(levels, 2, data=bad))
    assert got["y"] == pristine_y(levels) and got["counts"] == [0, 4, 4, 0, 0, 1, 0, 0]
    # level 0's one row, and an unnamed level
    got = run(with_y(levels, 0, data=flip(levels[0]["y"][0], 3)))
    assert got["y"] == pristine_y(levels) and got["action_y"] == bytes([DATA] + [0] * 6)
    damaged = with_y(levels, 1, data=flip(levels[1]["y"][0], 3))
    got = run(damaged, ALL & ~2)
    assert got["status_y"] == bytes([1, rl.NOT_TRIED, rl.NOT_TRIED, 1, 1, 1, 1]) and got["level"][1] == 0 and got["counts"] == [0] * 8
    assert 1 not in got["y"]


@pytest.mark.parametrize("curve", CURVES)
def test_x_damaged_and_inconsistent(curve):
    n = 8
    key, commit, blocks, snaps = written(curve, n)
    levels = snaps[7]
    run = lambda lv: rl.repair_levels(lv, n, N_COLS, curve, 7, ALL, commit, key=key)
    rb = 64 * N_COLS
    both = with_y(levels, 2, data=flip(levels[2]["y"][0], rb + 2), x_data=flip(levels[2]["x"][0], 2 * rb + 9))
    got = run(both)
    assert got["level"] == bytes([rl.CLEAN, rl.CLEAN, rl.X_DAMAGED] + [0] * 13) and got["action_y"] == bytes(7)
    assert got["counts"] == [1, 1, 0, 0, 0, 0, 1, 0] and got["y"] == pristine_y(both)
    # level 1's Y half of t = 3 (steps 1, 2) beside the X half of t = 7 (steps 5, 6): both pass their checks
    y3 = snaps[3][1]["y"]
    mixed = with_y(levels, 1, data=y3[0], macs=y3[1], align=y3[3])
    got = run(mixed)
    assert got["counts"] == [0] * 8 and got["level"][1] == rl.CLEAN
    got = run(with_y(mixed, 1, data=flip(y3[0], 7)))
    assert got["level"][1] == rl.INCONSISTENT and got["counts"] == [0, 1, 0, 0, 0, 0, 1, 1] and got["action_y"] == bytes(7)
    assert got["y"][1] == (flip(y3[0], 7), y3[1], y3[3])
    # a bad symbol in a row that still passes its check cannot be made here; the decode's count is the model's own
    assert rl.decode_x([[1 << 300, 5, 6]], curve) == ([[0, 5, 6]], 1)


# ---- the C ABI
FIELDS = ("write_step", "levels", "data_x", "mac_x", "d_prf_x", "d_prf_y", "data_y", "mac_y", "align_y", "d_work", "d_status_x", "d_status_y",
          "d_action_y", "d_level", "d_counts", "reserved")
FAMILIES = ("data_x", "mac_x", "data_y", "mac_y", "align_y")
FAKE_FB, ALPHA_BE = tc.FAKE_FB, tc.ALPHA_BE


def good(base=0x10000000, write_step=7, levels=ALL, counts=True, reserved=0):
    """n_total = 16, 128 columns: one MiB-aligned slot per level of every family and per other member (a data level of 4 rows is 32 KiB,
    the work area 200 * 128 * 7 bytes)"""
    at = lambda i: base + 0x100000 * i
    t = write_step % 16
    fam = lambda k: [at(4 * k + i) if t >> i & 1 else 0 for i in range(4)]
    return (write_step, levels, fam(0), fam(1), at(20), at(21), fam(2), fam(3), fam(4), at(22), at(23), at(24), at(25), at(26),
            at(27) if counts else 0, reserved)


def with_(r, **kw):
    r = list(r)
    for f, v in kw.items():
        r[FIELDS.index(f)] = v
    return tuple(r)


def with_level(r, family, i, v):
    fam = list(r[FIELDS.index(family)])
    fam[i] = v
    return with_(r, **{family: fam})


def call(reqs, n_total=16, k=None, null_reqs=False, who=IPA, bases=(FAKE_FB, FAKE_FB + 0x1000), alpha=ALPHA_BE):
    from porla_amd import lib
    from porla_amd import multiexp as mx
    arr, keep = mx.repair_levels_requests(reqs)
    k = len(reqs) if k is None else k
    if who == KZG:
        return lib.porla_kzg_repair_levels_batch_device(None if null_reqs else arr, k, n_total, None)
    return lib.porla_ipa_repair_levels_batch_device(bases[0] or None, bases[1] or None, alpha, None if null_reqs else arr, k, n_total, None)


refused = tc.refused
BOTH = pytest.mark.parametrize("who", [KZG, IPA])
I = FIELDS.index


def test_the_symbols_are_exported():
    from porla_amd import lib
    for name in (KZG, IPA, "porla_repair_levels_work_bytes"):
        assert hasattr(lib, name)


def test_the_ctypes_struct_and_constants_match_the_library():
    from porla_amd import loader
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_REPAIR_LEVELS_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(loader.RepairLevelsReq) == size == loader.PORLA_REPAIR_LEVELS_REQ_BYTES == 128
    offsets = {f: 8 * i for i, f in enumerate(FIELDS)}
    assert {f: getattr(loader.RepairLevelsReq, f).offset for f, _ in loader.RepairLevelsReq._fields_} == offsets
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "repair_levels_batch.hip")).read()
    struct = header[header.index("typedef struct {", header.index("#define PORLA_REPAIR_LEVELS_REQ_BYTES")):header.index("} porla_repair_levels_req;")]
    for f, off in offsets.items():
        assert "offsetof(porla_repair_levels_req, %s) == %d" % (f, off) in src
        assert re.search(r"%s;\s+/\*\s+%d[: ]" % (f, off), struct), f
    assert "sizeof(porla_repair_levels_req) == PORLA_REPAIR_LEVELS_REQ_BYTES" in src
    for name, v in (("DATA", 1), ("MAC", 2), ("ALIGN", 8), ("LEVEL_CLEAN", 1), ("LEVEL_X_DAMAGED", 2), ("LEVEL_INCONSISTENT", 3), ("LEVEL_REPAIRED", 4)):
        assert int(re.search(r"#define PORLA_REPAIR_%s\s+(\d+)" % name, header).group(1)) == v == getattr(loader, "PORLA_REPAIR_" + name)
    assert (rl.DATA, rl.MAC, rl.ALIGN, rl.CLEAN, rl.X_DAMAGED, rl.INCONSISTENT, rl.REPAIRED, rl.NOT_TRIED) == (1, 2, 8, 1, 2, 3, 4, 2)
    # the existing structs keep their sizes
    assert ctypes.sizeof(loader.RepairTopReq) == 120 and ctypes.sizeof(loader.ExtractXytReq) == 224


def test_the_work_size_is_the_documented_formula():
    from porla_amd import multiexp as mx
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    assert "200 * n_cols * m" in header and rl.WORK_PER_SYMBOL == 200
    for n, cols, step, mask in ((8, 128, 7, ALL), (8, 128, 15, 5), (16, 1024, 7, 2), (1 << 16, 128, (1 << 16) - 1, ALL), (2, 128, 1, 1),
                                (2048, 128, 1024, ALL), (8, 128, 8, ALL), (8, 128, 7, 8), (8, 0, 7, ALL)):
        want = 200 * cols * (mask & (step % n))
        assert mx.repair_levels_work_bytes(n, cols, step, mask) == want == rl.work_bytes(n, cols, step, mask), (n, cols, step, mask)
    for n in (0, 1, 3, 1 << 17):
        assert mx.repair_levels_work_bytes(n, 128, 7, ALL) == 0 == rl.work_bytes(n, 128, 7, ALL)
    assert mx.repair_levels_work_bytes(1 << 16, 1 << 62, (1 << 16) - 1, ALL) == 0                     # a size that overflows


@BOTH
def test_good_arguments_pass_the_refusals(who):
    assert call([good(), good(base=0x30000000, write_step=16 + 5)], who=who) != ERR_ARG
    assert call([good(counts=False), good(base=0x30000000, write_step=(1 << 64) - 1, levels=6)], who=who) != ERR_ARG
    assert call([good(write_step=1)], n_total=2, who=who) != ERR_ARG
    # nothing named: no family, PRF value or work area is needed; nothing resident: no status or action either
    bare = with_(good(levels=8), data_x=None, mac_x=None, data_y=None, mac_y=None, align_y=None, d_prf_x=0, d_prf_y=0, d_work=0)
    assert call([bare], who=who) != ERR_ARG
    assert call([with_(with_(good(write_step=16), d_status_x=0, d_status_y=0, d_action_y=0), data_x=None, mac_x=None, data_y=None, mac_y=None,
                       align_y=None, d_prf_x=0, d_prf_y=0, d_work=0)], who=who) != ERR_ARG
    # an unnamed level's entries are ignored
    assert call([with_level(with_level(good(levels=5), "align_y", 1, 0), "data_x", 1, 8)], who=who) != ERR_ARG


@BOTH
def test_null_reqs_is_refused(who):
    refused(call([good()], null_reqs=True, k=1, who=who), who, "reqs is NULL")


@BOTH
@pytest.mark.parametrize("field", FAMILIES + ("d_prf_x", "d_prf_y", "d_work", "d_status_x", "d_status_y", "d_action_y", "d_level"))
def test_a_null_pointer_is_refused(who, field):
    refused(call([good(), with_(good(base=0x30000000), **{field: None if field in FAMILIES else 0})], who=who), who, "NULL", "request 1", field)


@BOTH
@pytest.mark.parametrize("family", FAMILIES)
def test_a_named_level_with_a_null_entry_is_refused(who, family):
    refused(call([with_level(good(), family, 2, 0)], who=who), who, "NULL", "named level 2", family)
    assert call([with_level(good(levels=3), family, 2, 0)], who=who) != ERR_ARG


@BOTH
def test_misaligned_pointers_are_refused(who):
    g = good()
    for family in FAMILIES:
        for off in (8, 1):
            refused(call([with_level(g, family, 1, g[I(family)][1] + off)], who=who), who, "16-byte", "request 0")
    for field in ("d_prf_x", "d_prf_y", "d_work"):
        refused(call([with_(g, **{field: g[I(field)] + 8})], who=who), who, "16-byte", field)
    refused(call([with_(g, d_counts=g[I("d_counts")] + 2)], who=who), who, "4-byte")


@BOTH
def test_the_other_refusals(who):
    g = good()
    for n in (0, 1, 3, 1000, 1 << 17):
        refused(call([g], n_total=n, who=who), who, "n_total")
    for v in (1, 1 << 63):
        refused(call([good(), good(base=0x30000000, reserved=v)], who=who), who, "reserved", "request 1")
    refused(call([good()] * 65536, who=who), who, "65535")
    refused(call([with_level(g, "data_y", 2, (1 << 64) - 64)], who=who), who, "overflow")
    refused(call([with_(g, d_status_y=(1 << 64) - 4)], who=who), who, "overflow")
    if who == IPA:                                                        # five files of 2^16 - 1 named rows: above 2^18
        fam = lambda b, k:[b + 0x1000000000 * k + 0x40000000 * i for i in range(16)]
        req = lambda b: (65535, ALL, fam(b, 0), fam(b, 1), b + 0x5000000000, b + 0x5010000000, fam(b, 2), fam(b, 3), fam(b, 4), b + 0x6000000000,
                         b + 0x5020000000, b + 0x5030000000, b + 0x5040000000, b + 0x5050000000, b + 0x5060000000, 0)
        assert call([req(0x10000000000 * (a + 1)) for a in range(4)], n_total=1 << 16, who=who) not in (ERR_ARG, 0)
        refused(call([req(0x10000000000 * (a + 1)) for a in range(5)], n_total=1 << 16, who=who), who, "2^18")


@BOTH
def test_the_y_stores_are_outputs_in_the_overlap_walk(who):
    a, b = good(), good(base=0x50000000)
    run = lambda reqs: call(reqs, who=who)
    lv = lambda r, f, i: r[I(f)][i]
    refused(run([with_(a, d_prf_x=lv(a, "mac_y", 2) + 192)]), who, "overlaps")                        # a Y store against an input
    refused(run([with_level(a, "align_y", 2, lv(a, "mac_y", 2))]), who, "overlaps")                    # against another Y store
    refused(run([with_level(a, "data_y", 1, lv(a, "data_x", 1))]), who, "overlaps")                    # against the X store
    refused(run([with_(a, d_status_x=lv(a, "mac_y", 2) + 255)]), who, "overlaps")
    assert run([with_(a, d_status_x=lv(a, "mac_y", 2) + 256)]) != ERR_ARG                              # back to back is fine
    refused(run([with_(a, d_action_y=a[I("d_status_y")] + 6)]), who, "overlaps")
    assert run([with_(a, d_action_y=a[I("d_status_y")] + 7)]) != ERR_ARG
    refused(run([with_(a, d_level=a[I("d_counts")] + 28)]), who, "overlaps")                           # eight words of counts, 16 verdicts
    refused(run([with_(a, d_level=a[I("d_counts")] - 15)]), who, "overlaps")
    assert run([with_(a, d_level=a[I("d_counts")] + 32)]) != ERR_ARG
    refused(run([with_(a, d_work=lv(a, "mac_x", 0) - 16)]), who, "overlaps")                           # the work area is an output
    if who == IPA:                                                        # (the KZG build sizes rows and work by its SRS: none here)
        refused(run([with_(a, d_status_y=a[I("d_work")] + 200 * 128 * 7 - 1)]), who, "overlaps")
        assert run([with_(a, d_status_y=a[I("d_work")] + 200 * 128 * 7)]) != ERR_ARG
        refused(run([with_(a, d_prf_y=lv(a, "data_y", 2) + 0x7ff0)]), who, "overlaps")
    # across requests: no two requests may share a Y store; the X stores and PRF values may be shared
    for f in ("data_y", "mac_y", "align_y"):
        refused(run([a, with_level(b, f, 0, lv(a, f, 0))]), who, "overlaps")
    refused(run([a, a]), who, "overlaps")
    shared = {f: a[I(f)] for f in ("data_x", "mac_x", "d_prf_x", "d_prf_y")}
    assert run([a, with_(b, **shared)]) != ERR_ARG


def test_a_null_base_or_alpha_is_refused():
    refused(call([good()], bases=(0, FAKE_FB)), IPA, "NULL base")
    refused(call([good()], bases=(FAKE_FB, 0)), IPA, "NULL base")
    refused(call([good()], alpha=None), IPA, "alpha_be")
    q = icc_py.Q["secp256k1"]
    for zero in (bytes(32), q.to_bytes(32, "big")):
        refused(call([good()], alpha=zero), IPA, "alpha is 0")


@BOTH
def test_k_zero_returns_zero(who):
    assert call([], k=0, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who) == 0
    assert call([], k=0, null_reqs=True, who=who, bases=(0, 0)) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both builds) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import sys
sys.path.insert(0, %r)
from porla_amd import lib
from porla_amd import multiexp as mx
from tests.test_repair_levels_cpu import good
alpha = (7).to_bytes(32, "big")
reqs = [good(), good(base=0x30000000, write_step=21, counts=False, levels=4)]
arr, keep = mx.repair_levels_requests(reqs)
print(lib.porla_kzg_repair_levels_batch_device(arr, 2, 16, None))
print(lib.porla_ipa_repair_levels_batch_device(0x7000000, 0x7001000, alpha, arr, 2, 16, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr, keep = mx.repair_levels_requests([good(counts=False), good(levels=5)[:15]])
    assert arr[0].write_step == 7 and arr[0].levels == ALL and arr[0].d_prf_x == 0x10000000 + 20 * 0x100000 and arr[0].d_counts is None
    assert arr[0].d_work == 0x10000000 + 22 * 0x100000 and arr[0].d_level == 0x10000000 + 26 * 0x100000 and arr[0].reserved == 0
    assert arr[1].levels == 5 and arr[1].d_counts == 0x10000000 + 27 * 0x100000 and arr[1].reserved == 0
    data_y = ctypes.cast(arr[0].data_y, ctypes.POINTER(ctypes.c_void_p))
    assert [data_y[i] for i in range(4)] == [0x10000000 + (8 + i) * 0x100000 for i in range(3)] + [None]
    with pytest.raises(ValueError):
        mx.repair_levels_requests([good()[:12]])
    with pytest.raises(RuntimeError, match="n_total"):
        mx.kzg_repair_levels_batch_device([good()], 3)
    assert callable(mx.FixedBase.ipa_repair_levels_batch_device)

"""CPU: AES on the device, without a device.  The model (tests/challenge_model.py) reproduces the FIPS-197 / SP 800-38A vectors and
openssl; the host forms of the library (include/porla_gpu.h: porla_mac_prf_host, porla_client_prf_runs, porla_audit_challenge_host,
porla_diag_audit_walk(on_device = 0), porla_audit_complement_scalar_host) equal the model byte for byte; the C ABI exports its
symbols, has the layout the header states, refuses every bad argument with PORLA_ERR_ARG and its own name before a device is touched,
returns 0 for k = 0 and PORLA_ERR_NO_DEVICE for valid device-form arguments without a device; and the shared definitions
(porla_amd/csrc/challenge_host.hpp) run clean under the host compiler's address and undefined-behaviour sanitizers in a stand-alone
program (tools/challenge_selftest.cpp) whose digest equals the model's."""
import ctypes
import os
import random
import re
import shutil
import struct
import subprocess
import sys

import pytest

from tests import challenge_model as model
from tests import common

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
KEY = model.SECRET_KEY
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
VECTORS = [("000102030405060708090a0b0c0d0e0f", "00112233445566778899aabbccddeeff", "69c4e0d86a7b0430d8cdb78070b4c55a"),   # FIPS-197 C.1
           ("2b7e151628aed2a6abf7158809cf4f3c", "3243f6a8885a308d313198a2e0370734", "3925841d02dc09fbdc118597196a0b32"),   # FIPS-197 B
           ("2b7e151628aed2a6abf7158809cf4f3c", "6bc1bee22e409f96e93d7e117393172a", "3ad77bb40d7a3660a89ecaf32466ef97")]   # SP 800-38A F.1.1


def levels_for(num_blocks, mixed=False, split=False):
    """level descriptors (data_x, data_y, mac_x, mac_y, form): every half at its own base; mixed: levels <= 10 form 0, above form 1;
    split: the two halves far apart instead of back to back"""
    out, d, m = [], 7, 100000
    for i in range(num_blocks.bit_length()):
        l = 1 << i
        gap = 5 * l + 3 if split else l
        out.append((d, d + gap, m, m + gap, 1 if mixed and i > 10 else 0))
        d += gap + l + (11 if split else 0)
        m += gap + l + (13 if split else 0)
    return out


CHALLENGE_SHAPES = [(2, 1, {}), (2, 2, {}), (64, 63, {}), (64, 0, {}), (128, 127, {}), (128, 128, {}),
                    (256, 0, {}), (256, 1, {}), (256, 85, {}), (256, 255, {}), (256, 256 + 37, {}),
                    (1 << 15, (1 << 15) - 1, {}), (1 << 15, (1 << 15) - 1, dict(mixed=True)), (256, 85, dict(split=True)),
                    (1 << 15, 0x5a5a, dict(mixed=True, split=True))]


def seed_of(i):
    return bytes(random.Random(1000 + i).getrandbits(8) for _ in range(16))


# ---------------------------------------------------------------- the model's AES
@pytest.mark.parametrize("key,pt,ct", VECTORS)
def test_model_aes_reproduces_the_standard_vectors(key, pt, ct):
    assert model.aes128_encrypt(bytes.fromhex(key), bytes.fromhex(pt)).hex() == ct


def test_model_aes_equals_openssl_on_random_blocks():
    if not os.path.exists("/usr/bin/openssl"):
        pytest.skip("no /usr/bin/openssl")
    rnd = random.Random(77)
    key = bytes(rnd.getrandbits(8) for _ in range(16))
    pt = bytes(rnd.getrandbits(8) for _ in range(16 * 64))
    r = subprocess.run(["/usr/bin/openssl", "enc", "-aes-128-ecb", "-nopad", "-K", key.hex()], input=pt, capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rks = model.aes128_round_keys(key)
    assert b"".join(model.aes128_encrypt_rk(rks, pt[16 * i:16 * i + 16]) for i in range(64)) == r.stdout


# ---------------------------------------------------------------- the MAC PRF
@pytest.mark.parametrize("key,pt,ct", VECTORS)
def test_mac_prf_host_on_the_standard_vectors(key, pt, ct):
    """PRF input = the plaintext split into level / index / time"""
    from porla_amd import challenge as ch
    level, index, time = struct.unpack("<iiq", bytes.fromhex(pt))
    assert ch.mac_prf_host(bytes.fromhex(key), [(level, index, 1, time, 0)]).hex() == ct


def test_mac_prf_host_equals_the_model_on_random_runs():
    from porla_amd import challenge as ch
    rnd = random.Random(5)
    runs = [(0, 5, 1, 41, 0), (3, 0, 16, 1 << 40, 0), (0, 1, 8, (1 << 32) - 3, 1), (7, -4, 9, -2, 1), (2, INT32_MAX - 1, 4, 5, 0),
            (31, 100, 0, 0, 0), (4, 9, 7, 1000, 3), (1, 0, 5, (1 << 63) - 2, 1)]
    runs += [(rnd.randrange(25), rnd.randrange(-(1 << 31), 1 << 31), rnd.randrange(1, 40), rnd.randrange(-(1 << 62), 1 << 62), rnd.choice((0, 1)))
             for _ in range(12)]
    for key in (KEY, bytes(rnd.getrandbits(8) for _ in range(16))):
        want = b"".join(model.mac_prf(key, *t) for t in model.expand_runs(runs))
        assert ch.mac_prf_host(key, runs) == want
    assert ch.mac_prf_host(KEY, []) == b""


@pytest.mark.parametrize("n_total,W", [(8, 1), (8, 2), (8, 4), (16, 12), (1 << 15, 1 << 14)])
def test_update_runs_expand_to_the_model_triples(n_total, W):
    from porla_amd import challenge as ch
    L = model.lowest_set_bit(W)
    runs, n_values = ch.client_prf_runs("update", 5, W, n_total, level=L)
    want = model.update_triples(5, W, L)
    assert len(runs) == L + 2 and n_values == (1 << (L + 2)) - 1 == len(want)
    assert model.expand_runs(runs) == want
    assert sorted(want) == sorted(model.update_triples_reference_loop(5, W, L))     # t_i as the reference's loop accumulates it


@pytest.mark.parametrize("n_total,W", [(2, 2), (8, 8), (8, 24)])
def test_rebuild_runs_expand_to_the_model_triples(n_total, W):
    from porla_amd import challenge as ch
    runs, n_values = ch.client_prf_runs("rebuild", 3, W, n_total)
    want = model.rebuild_triples(3, W, n_total)
    assert len(runs) == 3 and n_values == 3 * n_total + 1 == len(want)
    assert model.expand_runs(runs) == want


# ---------------------------------------------------------------- the challenge
@pytest.mark.parametrize("case", range(len(CHALLENGE_SHAPES)))
def test_audit_challenge_host_equals_the_model(case):
    from porla_amd import challenge as ch
    num_blocks, write_step, kw = CHALLENGE_SHAPES[case]
    lv, seed = levels_for(num_blocks, **kw), seed_of(case)
    info, lists = ch.audit_challenge_host(seed, write_step, num_blocks, lv)
    want_info, want = model.challenge(model.PrgInts(seed), write_step, num_blocks, lv)
    assert info == want_info
    assert lists == want
    assert ch.audit_challenge_plan([(seed, write_step, num_blocks, lv)]) == [want_info]       # the plan-only form
    if kw.get("mixed"):
        assert info["n64"] and info["n32"]


def written_stream(num_blocks, write_step):
    """a stream with the magnitude cases at index and coefficient positions of every drawn level and at all-rows positions"""
    rnd = random.Random(num_blocks * 31 + write_step)
    ints = [rnd.randrange(INT32_MIN, INT32_MAX + 1) for _ in range(256 * 26)]
    height, ws, pos = num_blocks.bit_length(), write_step % num_blocks, 0
    edge = [INT32_MIN, -1, 0, INT32_MAX, 1, -INT32_MAX]
    for i in range(height):
        if not ((ws >> i) & 1 or i == height - 1):
            continue
        two_l = 2 << i
        if two_l > 128:
            vals = edge + [two_l - 1, two_l, -(two_l - 1), -two_l, two_l + 1]
            ints[pos:pos + len(vals)] = vals                        # indices
            ints[pos + 128:pos + 128 + len(edge)] = edge            # coefficients
            ints[pos + 127], ints[pos + 255] = INT32_MIN, INT32_MIN
            pos += 256
        else:
            for j in range(min(two_l, len(edge))):
                ints[pos + j] = edge[j]
            pos += two_l
    return ints


WALK_SHAPES = [(2, 1), (64, 63), (128, 127), (256, 85), (256, 255), (1 << 15, (1 << 15) - 1), (1 << 24, (1 << 24) - 1)]


@pytest.mark.parametrize("num_blocks,write_step", WALK_SHAPES)
def test_diag_walk_on_the_host_with_pinned_magnitudes(num_blocks, write_step):
    from porla_amd import challenge as ch
    lv = levels_for(num_blocks, mixed=True)
    ints = written_stream(num_blocks, write_step)
    info, lists = ch.diag_audit_walk(ints, write_step, num_blocks, lv, on_device=False)
    want_info, want = model.challenge(ints, write_step, num_blocks, lv)
    assert info == want_info and lists == want
    assert (1 << 31) in want["mac_coef"]                           # mag(INT32_MIN) is 2^31, on both sides


def test_the_tail_values_at_their_edges():
    from porla_amd import challenge as ch
    lv = levels_for(256)
    for a, z in ((INT32_MIN, -1), (-1, INT32_MIN), (0, 0), (INT32_MAX, INT32_MAX), (-INT32_MAX, 1)):
        ints = [3] * 430
        ints[298], ints[426] = a, z                                 # 256 blocks at 85: 298 points, 426 ints consumed
        info, _ = ch.diag_audit_walk(ints, 85, 256, lv)
        want_info, _ = model.challenge(ints, 85, 256, lv)
        assert info == want_info
        assert (info["a_raw"], info["random_point"], info["n_macs"]) == (a, z & ((1 << 64) - 1), 298)


@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
def test_complement_scalars_host_equal_the_model(curve):
    from porla_amd import challenge as ch
    reqs = [(seed_of(40), 1, 2), (seed_of(41), 85, 256), (seed_of(42), (5 << 32) + 255, 256), (seed_of(43), (1 << 15) - 1, 1 << 15)]
    got = ch.audit_complement_scalar_host(KEY, reqs, curve)
    assert got == [model.complement_scalar(KEY, s, w, n, curve) for s, w, n in reqs]
    assert all(0 < g < 1 << 172 for g in got)


# ---------------------------------------------------------------- the ABI
SYMBOLS = ("porla_mac_prf_batch_device", "porla_mac_prf_host", "porla_client_prf_runs", "porla_audit_challenge_batch_device",
           "porla_audit_challenge_host", "porla_audit_complement_scalar_batch_device", "porla_audit_complement_scalar_host",
           "porla_diag_audit_walk")


def test_the_symbols_are_exported():
    from porla_amd import lib
    for s in SYMBOLS:
        assert hasattr(lib, s), s


def test_the_ctypes_structs_match_the_header_and_the_library():
    from porla_amd import loader
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "challenge.hip")).read()
    for macro, cls, cname, size in (("PORLA_PRF_RUN_BYTES", loader.PrfRun, "porla_prf_run", 32),
                                    ("PORLA_AUDIT_LEVEL_BYTES", loader.AuditLevel, "porla_audit_level", 40),
                                    ("PORLA_AUDIT_CHALLENGE_REQ_BYTES", loader.AuditChallengeReq, "porla_audit_challenge_req", 88),
                                    ("PORLA_AUDIT_CHALLENGE_INFO_BYTES", loader.AuditChallengeInfo, "porla_audit_challenge_info", 72),
                                    ("PORLA_AUDIT_SCALAR_REQ_BYTES", loader.AuditScalarReq, "porla_audit_scalar_req", 32)):
        assert int(re.search(r"#define %s\s+(\d+)" % macro, header).group(1)) == size == ctypes.sizeof(cls) == getattr(loader, macro)
        assert "sizeof(%s) == %s" % (cname, macro) in src
        for f, _ in cls._fields_:
            assert "offsetof(%s, %s) == %d" % (cname, f, getattr(cls, f).offset) in src, (cname, f)
    assert int(re.search(r"#define PORLA_PRF_UPDATE\s+(\d+)", header).group(1)) == 0
    assert int(re.search(r"#define PORLA_PRF_REBUILD\s+(\d+)", header).group(1)) == 1


def refused(rc, who, *words):
    from porla_amd import lib
    assert rc == ERR_ARG
    msg = lib.porla_gpu_last_error().decode()
    assert msg and who in msg, msg
    for w in words:
        assert w in msg, msg


D = 0x10000000      # a pointer value that is never dereferenced: every call below is refused, or stops at the device check


def chal_call(device, num_blocks=256, levels=None, lists=(D, D + 0x10000, D + 0x20000, D + 0x30000, D + 0x40000, D + 0x50000), k=None,
              null_reqs=False, null_infos=False, null_levels=False):
    from porla_amd import challenge as ch, lib
    from porla_amd.loader import AuditChallengeInfo
    lv = levels if levels is not None else levels_for(1 << 15, mixed=True) + [(0, 0, 0, 0, 0)] * 16      # 32: any height in range
    arr = ch.challenge_requests([(seed_of(0), 85, num_blocks, lv, lists)])
    if null_levels:
        arr[0].levels = None
    infos = (AuditChallengeInfo * 1)()
    n = 1 if k is None else k
    if device:
        return lib.porla_audit_challenge_batch_device(None if null_reqs else arr, n, None if null_infos else infos, None)
    return lib.porla_audit_challenge_host(None if null_reqs else arr, n, None if null_infos else infos)


@pytest.mark.parametrize("device", [True, False])
def test_challenge_refusals(device):
    who = "porla_audit_challenge_batch_device" if device else "porla_audit_challenge_host"
    for nb in (0, 1, 3, 100, (1 << 24) + 1, 1 << 25):
        refused(chal_call(device, num_blocks=nb), who, "num_blocks", "request 0")
    lv = levels_for(256)
    bad = list(lv)
    bad[3] = lv[3][:4] + (2,)
    refused(chal_call(device, levels=bad), who, "form", "level 3")
    bad[3] = lv[3][:4] + (0, 1)
    refused(chal_call(device, levels=bad), who, "pad", "level 3")
    refused(chal_call(device, null_reqs=True), who, "reqs is NULL")
    refused(chal_call(device, null_infos=True), who, "infos_out is NULL")
    refused(chal_call(device, null_levels=True), who, "levels is NULL")
    full = [D, D + 0x10000, D + 0x20000, D + 0x30000, D + 0x40000, D + 0x50000]
    mixed = levels_for(1 << 15, mixed=True)
    for i in range(6):                                              # write_step 85 at 2^15 blocks, mixed forms: every list has entries
        lists = list(full)
        lists[i] = 0
        refused(chal_call(device, num_blocks=1 << 15, levels=mixed, lists=lists), who, "NULL list", "request 0")
    assert chal_call(device, k=0, null_reqs=True, null_infos=True) == 0


def test_challenge_device_form_alignment_and_count():
    who = "porla_audit_challenge_batch_device"
    full = [D, D + 0x10000, D + 0x20000, D + 0x30000, D + 0x40000, D + 0x50000]
    for i, off in ((0, 4), (1, 2), (2, 4), (3, 2), (4, 4), (5, 2)):
        lists = list(full)
        lists[i] += off
        refused(chal_call(True, lists=lists), who, "aligned", "request 0")
    refused(chal_call(True, k=65536), who, "65535")


def test_the_plan_only_form_touches_no_device():
    """all six lists NULL: the device form returns 0 with the infos filled, where a device exists or not"""
    from porla_amd import challenge as ch
    lv = levels_for(256)
    reqs = [(seed_of(i), 85 + i, 256, lv, None) for i in range(3)]
    assert ch.audit_challenge_batch_device(reqs) == ch.audit_challenge_plan(reqs)
    assert ch.audit_challenge_plan(reqs)[0] == model.challenge(model.PrgInts(seed_of(0)), 85, 256, lv)[0]


def test_prf_refusals():
    from porla_amd import challenge as ch, lib
    runs = ch.prf_runs([(0, 0, 4, 0, 0)])
    out = ctypes.create_string_buffer(64)
    for who, f, good in (("porla_mac_prf_batch_device", lambda *a: lib.porla_mac_prf_batch_device(*a, None), ctypes.c_void_p(D)),
                         ("porla_mac_prf_host", lib.porla_mac_prf_host, ctypes.cast(out, ctypes.c_void_p))):
        refused(f(None, runs, 1, good), who, "key16")
        refused(f(KEY, None, 1, good), who, "runs")
        refused(f(KEY, runs, 1, None), who, "out is NULL")
        refused(f(KEY, ch.prf_runs([(0, 0, (1 << 38) + 1, 0, 0)]), 1, good), who, "2^38")
        refused(f(KEY, ch.prf_runs([(0, 0, 1 << 38, 0, 0), (0, 0, 1, 0, 0)]), 2, good), who, "2^38")
        assert f(KEY, None, 0, None) == 0
        assert f(None, ch.prf_runs([(0, 0, 0, 0, 0)]), 1, None) == 0
    refused(lib.porla_mac_prf_batch_device(KEY, runs, 1, ctypes.c_void_p(D + 8), None), "porla_mac_prf_batch_device", "16-byte")


def test_client_prf_runs_refusals():
    from porla_amd import lib
    from porla_amd.loader import PrfRun
    who = "porla_client_prf_runs"
    arr, a, b = (PrfRun * 32)(), ctypes.c_size_t(), ctypes.c_size_t()

    def call(kind=0, W=4, level=2, n_total=8, runs=arr, max_runs=32, pa=ctypes.byref(a), pb=ctypes.byref(b)):
        return lib.porla_client_prf_runs(kind, 1, W, level, n_total, runs, max_runs, pa, pb)
    assert call() == 0 and call(kind=1, W=8) == 0
    refused(call(kind=2), who, "kind")
    refused(call(kind=-1), who, "kind")
    for n_total in (0, 1, 3, 12, 1 << 31):
        refused(call(n_total=n_total), who, "n_total")
        refused(call(kind=1, n_total=n_total), who, "n_total")
    refused(call(W=8), who, "write_step % n_total == 0")
    refused(call(W=0), who, "write_step % n_total == 0")
    refused(call(level=-1), who, "level")
    refused(call(level=3), who, "level")
    refused(call(max_runs=3), who, "max_runs")
    refused(call(kind=1, W=8, max_runs=2), who, "max_runs")
    refused(call(runs=None), who, "NULL")
    refused(call(pa=None), who, "NULL")
    refused(call(pb=None), who, "NULL")
    assert call(kind=1, W=5, level=-7) == 0                         # a rebuild takes any write_step and ignores level


def test_complement_scalar_refusals():
    from porla_amd import challenge as ch, lib
    out = ctypes.create_string_buffer(64)
    good = ch.scalar_requests([(seed_of(0), 85, 256)])
    for who, f, o in (("porla_audit_complement_scalar_batch_device", lambda *a: lib.porla_audit_complement_scalar_batch_device(*a, None), ctypes.c_void_p(D)),
                      ("porla_audit_complement_scalar_host", lib.porla_audit_complement_scalar_host, ctypes.cast(out, ctypes.c_void_p))):
        refused(f(None, good, 1, 0, o), who, "key16")
        refused(f(KEY, None, 1, 0, o), who, "reqs")
        refused(f(KEY, good, 1, 0, None), who, "scalars is NULL")
        for curve in (-1, 2):
            refused(f(KEY, good, 1, curve, o), who, "curve")
        for nb in (0, 1, 3, 1 << 25):
            refused(f(KEY, ch.scalar_requests([(seed_of(0), 85, 256), (seed_of(0), 85, nb)]), 2, 0, o), who, "num_blocks", "request 1")
        refused(f(KEY, good, 65536, 0, o), who, "65535")
        assert f(None, None, 0, 0, None) == 0


def test_diag_walk_refusals():
    from porla_amd import challenge as ch
    who = "porla_diag_audit_walk"
    lv = levels_for(256)
    with pytest.raises(RuntimeError, match=who + ".*n_ints"):
        ch.diag_audit_walk([1] * 300, 85, 256, lv)                  # the walk at 85 reads 2 + 8 + 32 + 128 + 256 ints and the tail
    with pytest.raises(RuntimeError, match=who + ".*num_blocks"):
        ch.diag_audit_walk([1] * 3000, 85, 100, lv)
    ch.diag_audit_walk([1] * 427, 85, 256, lv)


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid device-form arguments return PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, challenge as ch
from porla_amd.loader import AuditChallengeInfo
D = 0x10000000
KEY = bytes(range(16))
print(lib.porla_mac_prf_batch_device(KEY, ch.prf_runs([(0, 0, 300, 0, 1)]), 1, ctypes.c_void_p(D), None))
lv = [(0, 1 << i, 0, 1 << i, 0) for i in range(9)]
lists = [D + 0x10000 * i for i in range(6)]
infos = (AuditChallengeInfo * 2)()
arr = ch.challenge_requests([(KEY, 85, 256, lv, lists), (KEY, 3, 256, lv, None)])
print(lib.porla_audit_challenge_batch_device(arr, 2, infos, None))
print(infos[0].n_macs, infos[1].n_macs)
for curve in (0, 1):
    print(lib.porla_audit_complement_scalar_batch_device(KEY, ch.scalar_requests([(KEY, 85, 256)]), 1, curve, ctypes.c_void_p(D), None))
try:
    ch.diag_audit_walk([1] * 3000, 85, 256, lv, on_device=True)
    print("ran")
except RuntimeError as e:
    print("error -1" in str(e))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2 + ["298", "134"] + [str(ERR_NO_DEVICE)] * 2 + ["True"]


# ---------------------------------------------------------------- the shared definitions under the host sanitizers
def fnv1a(data, h=0xcbf29ce484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & ((1 << 64) - 1)
    return h


def selftest_digest():
    """what tools/challenge_selftest.cpp feeds its digest, from the model"""
    u32 = lambda v: struct.pack("<I", v & 0xffffffff)
    u64 = lambda v: struct.pack("<Q", v & ((1 << 64) - 1))
    data = b"".join(model.aes128_encrypt(bytes.fromhex(k), bytes.fromhex(p)) for k, p, _ in VECTORS)
    write_step, num_blocks = 255 + 3 * 256, 256
    ints = [model._wrap32(t * 2654435761 + 12345) for t in range(2048)]
    ints[0], ints[1] = INT32_MIN, -1
    ints[254 + 3], ints[254 + 4], ints[254 + 5] = INT32_MIN, 255, 256
    ints[254 + 128 + 5] = INT32_MIN
    ints[510 + 7] = INT32_MAX
    pts, pos = model.walk(ints, write_step, num_blocks)
    for level, index, coef in pts:
        data += u32(level) + u32(index) + u32(coef)
    a = ints[len(pts)]
    data += u64(ints[pos]) + u32(a) + (a % model.N_SECP256K1).to_bytes(32, "big")
    data += (INT32_MIN % model.N_SECP256K1).to_bytes(32, "big") + (-1 % model.N_SECP256K1).to_bytes(32, "big")
    for curve in ("bn254", "secp256k1"):
        s = sum(coef * model.prf_value(model.mac_prf(KEY, *t), curve) for coef, t in model.complement_triples(ints, write_step, num_blocks))
        data += s.to_bytes(32, "big")
    from porla_amd import challenge as ch
    runs = [(0, 5, 1, 11, 0), (0, 0, 2, 11, 0), (1, 0, 4, 10, 0), (2, 0, 8, 12, 0), (0, 3, 1, 23, 0), (0, 1, 8, 16, 1), (3, 0, 16, 24, 0)]
    assert model.expand_runs(runs) == model.update_triples(5, 12, 2) + model.rebuild_triples(3, 24, 8)
    assert runs == ch.client_prf_runs("update", 5, 12, 16, level=2)[0] + ch.client_prf_runs("rebuild", 3, 24, 8)[0]
    for r in runs:
        data += struct.pack("<iiQqq", *r)
        data += b"".join(model.mac_prf(KEY, *t) for t in model.expand_runs([r]))
    return fnv1a(data)


def test_sanitized_selftest_of_the_shared_definitions(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "challenge_selftest")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtime linked into the program where the compiler can (it then has no place in the order of shared libraries)
    for extra in (["-static-libasan"], []):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover"] + extra
        if (subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, timeout=300).returncode == 0
                and subprocess.run([str(tmp_path / "probe")], capture_output=True, timeout=300).returncode == 0):
            break
    else:
        pytest.skip("the host compiler has no usable sanitizer runtime")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall"] + san + [os.path.join(ROOT, "tools", "challenge_selftest.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "challenge_selftest digest=%016x" % selftest_digest()

"""CPU: the batched client update (include/porla_gpu.h: porla_kzg_client_update_batch_device / porla_ipa_client_update_batch_device).
1. The model the GPU tests compare against (tests/client_update_model.py) closes with the server's (tests/update_model.FileModel): fed
   the client's MAC and wire points, every resident MAC of the file is alpha * Commit(row) + s * h with s the PRF value the client drew
   for that slot -- what Client::audit relies on.  This pins the order of the PRF values and the direction of the subtraction without
   the engine.
2. The C ABI: the symbols, the struct layout, every refusal that needs no device, k = 0.  Nothing here computes on a device: the
   pointer values are never dereferenced."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
FAKE = 0x1000
OFFSETS = dict(d_block=0, d_prf=8, d_mac_out=16, d_complements_out=24, write_step=32, level=40, pad=44)


# ---- 1. closure of the two models
def test_the_client_model_closes_with_the_server_model_over_a_full_cycle():
    import icc_py
    from tests.client_update_model import client_update, n_prf
    from tests.update_model import FileModel, pt_tuple, row_vals
    curve, n_total, n_cols, alpha = "bn254", 16, 4, 5
    q = icc_py.Q[curve]
    o = common.oracle()
    tau, key_alpha = bytes.fromhex("ffeeddccbbaa99887766554433221100"), bytes.fromhex("00112233445566778899aabbccddeeff")
    o.oracle_kzg_init_key(tau, ctypes.c_size_t(len(tau)), key_alpha, ctypes.c_size_t(len(key_alpha)))
    o.oracle_kzg_init_srs(ctypes.c_size_t(n_cols), (1).to_bytes(32, "big"))
    raw = ctypes.create_string_buffer(64 * n_cols)
    o.oracle_kzg_srs_g1_raw(raw)
    m = FileModel(n_total, n_cols, curve, raw.raw, fill=0xA5)
    h = icc_py.ec_mul(curve, (1, 2), 9)                                     # a small hiding point
    rnd = random.Random(13)
    slots = {}                                                              # level -> (X scalars, Y scalars) the client drew for it
    levels = []
    for step in range(1, n_total):
        level = m.next_level()
        levels.append(level)
        prf = [rnd.getrandbits(128)]
        for i in range(level):
            prf += slots[i][0] + slots[i][1]                                # (the PRF reproduces what it gave when level i was written)
        new = [rnd.getrandbits(128) for _ in range(2 << level)]
        prf += new
        assert len(prf) == n_prf(level)
        chunks = [rnd.getrandbits(256) for _ in range(n_cols)]
        block_commit = icc_py.ec_mul(curve, m.commit([c % q for c in chunks]), alpha)
        mac, out = client_update(curve, n_total, step, level, prf, h, block_commit)
        assert m.update(chunks, mac, out) == (step, level)
        for i in range(level):
            del slots[i]
        slots[level] = (new[:1 << level], new[1 << level:])
        fams = m.family_bytes()
        assert sorted(slots) == [lv for lv in range(m.height) if not m.empty[lv]]
        for lv, (sx, sy) in slots.items():
            for part, s in (("x", sx), ("y", sy)):
                for r in range(1 << lv):
                    row = row_vals(fams["data_" + part][lv][r * 64 * n_cols:(r + 1) * 64 * n_cols])
                    mac_r = pt_tuple(fams["mac_" + part][lv][64 * r:64 * r + 64])
                    al_r = pt_tuple(fams["align_" + part][lv][64 * r:64 * r + 64])
                    lhs = icc_py.ec_add(curve, mac_r, icc_py.ec_mul(curve, al_r, alpha))
                    rhs = icc_py.ec_add(curve, icc_py.ec_mul(curve, m.commit([v % q for v in row]), alpha), icc_py.ec_mul(curve, h, s[r]))
                    assert lhs == rhs, (step, lv, part, r)
    assert levels == [0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0]


# ---- 2. the C ABI
def good(level=2, write_step=4, base=0x2000, **kw):
    r = dict(d_block=FAKE, d_prf=FAKE, d_mac_out=base, d_complements_out=base + 0x40, write_step=write_step, level=level)
    r.update(kw)
    return tuple(r[f] for f in OFFSETS if f != "pad")


def call(reqs, n_total=16, k=None, pad=None, null_reqs=False, ipa=None):
    from porla_amd import lib, multiexp as mx
    arr = mx.client_update_requests(reqs)
    if pad is not None:
        arr[0].pad = pad
    a = None if null_reqs else arr
    n = len(reqs) if k is None else k
    if ipa is not None:
        return lib.porla_ipa_client_update_batch_device(ctypes.c_void_p(ipa[0] or None), ctypes.c_void_p(ipa[1] or None), a, n, n_total,
                                                        ctypes.c_void_p(0))
    return lib.porla_kzg_client_update_batch_device(a, n, n_total, ctypes.c_void_p(0))


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def refused(rc, *words):
    assert rc == ERR_ARG
    msg = last_error()
    assert msg and ("porla_kzg_client_update_batch_device" in msg or "porla_ipa_client_update_batch_device" in msg)
    for w in words:
        assert w in msg, msg


def test_the_symbols_are_exported():
    from porla_amd import lib
    assert hasattr(lib, "porla_kzg_client_update_batch_device") and hasattr(lib, "porla_ipa_client_update_batch_device")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_CLIENT_UPDATE_REQ_BYTES, ClientUpdateReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_CLIENT_UPDATE_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(ClientUpdateReq) == size == PORLA_CLIENT_UPDATE_REQ_BYTES == 48
    assert {f: getattr(ClientUpdateReq, f).offset for f, _ in ClientUpdateReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "client_update_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_client_update_req, %s) == %d" % (f, off) in src


def test_null_reqs_is_refused():
    refused(call([good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("field", ["d_block", "d_prf", "d_mac_out", "d_complements_out"])
def test_a_null_pointer_is_refused(field):
    refused(call([good(), good(base=0x4000, **{field: 0})]), "NULL", "request 1")


@pytest.mark.parametrize("field", ["d_block", "d_prf", "d_mac_out", "d_complements_out"])
def test_a_misaligned_pointer_is_refused(field):
    refused(call([good(**{field: 0x8008})]), "aligned", "request 0")


@pytest.mark.parametrize("n_total", [0, 1, 3, 12, 1000, (1 << 20) + 1])
def test_n_total_not_a_power_of_two_or_below_two_is_refused(n_total):
    refused(call([good(level=0, write_step=1)], n_total=n_total), "n_total")


def test_a_bad_level_is_refused():
    refused(call([good(level=4, write_step=1)], n_total=16), "level")            # 2^4 > 16 / 2: the top level is CRebuild's
    assert call([good(level=3, write_step=8)], n_total=16) != ERR_ARG
    refused(call([good(level=1, write_step=1)], n_total=2), "level")
    assert call([good(level=0, write_step=1)], n_total=2) != ERR_ARG
    from porla_amd import lib, multiexp as mx
    arr = mx.client_update_requests([good()])
    arr[0].level = -1
    assert lib.porla_kzg_client_update_batch_device(arr, 1, 16, None) == ERR_ARG and "level" in last_error()


@pytest.mark.parametrize("write_step", [0, 16, 32, 16 << 20])
def test_crebuilds_step_is_refused(write_step):
    refused(call([good(write_step=write_step)], n_total=16), "CRebuild")


def test_a_nonzero_pad_is_refused():
    refused(call([good()], pad=1), "pad")


def test_two_requests_naming_one_output_pointer_are_refused():
    a = good(base=0x2000)
    refused(call([a, good(base=0x4000, d_mac_out=a[2])]), "output pointer", "request 1")
    refused(call([a, good(base=0x4000, d_complements_out=a[3])]), "output pointer", "request 1")
    refused(call([a, good(base=0x4000, d_complements_out=a[2])]), "output pointer", "request 1")
    refused(call([good(d_mac_out=0x2000, d_complements_out=0x2000)]), "output pointer", "request 0")
    # the same block or PRF buffer in two requests is the caller's business
    assert call([a, good(base=0x4000)]) != ERR_ARG


def test_ipa_null_bases_are_refused():
    refused(call([good()], ipa=(0, 0)), "NULL base")
    refused(call([good()], ipa=(FAKE, 0)), "NULL base")
    refused(call([good()], ipa=(0, FAKE)), "NULL base")
    # and the shared checks come first on this entry point too
    refused(call([good()], ipa=(0, 0), n_total=12), "n_total")


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, null_reqs=True) == 0
    assert call([], k=0, null_reqs=True, ipa=(0, 0)) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (levels 0 and 3) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import sys
sys.path.insert(0, %r)
from porla_amd import lib, multiexp as mx
F = 0x1000
reqs = [(F, F, 0x2000, 0x2040, 1, 0), (F, F, 0x4000, 0x4040, 8, 3)]
print(lib.porla_kzg_client_update_batch_device(mx.client_update_requests(reqs), 2, 16, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(ERR_NO_DEVICE)


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr = mx.client_update_requests([good(level=1, write_step=2)])
    assert arr[0].d_block == FAKE and arr[0].d_mac_out == 0x2000 and arr[0].write_step == 2 and arr[0].level == 1 and arr[0].pad == 0
    with pytest.raises(ValueError):
        mx.client_update_requests([good()[:5]])
    with pytest.raises(RuntimeError, match="CRebuild"):
        mx.kzg_client_update_batch_device([good(write_step=16)], 16)

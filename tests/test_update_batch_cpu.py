"""CPU: the batched server update's C ABI (include/porla_gpu.h: porla_kzg_update_batch_device / porla_ipa_update_batch_device) -- the
symbols are exported, the ctypes mirror of porla_update_req has the layout the library static_asserts, every bad argument is refused
with PORLA_ERR_ARG before the device is touched, k = 0 is a no-op, and valid arguments without a device give PORLA_ERR_NO_DEVICE.
Nothing here computes on a device: the pointer values are never dereferenced.  And the model the GPU tests compare against
(tests/update_model.py) is checked against the identity that ties the three stores of a level together."""
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
OFFSETS = dict(d_block=0, d_mac=8, d_complements=16, write_step=24, level=32, pad=36, data_x=40, data_y=48, mac_x=56, mac_y=64,
               align_x=72, align_y=80)


def good(level=2, write_step=4, base=FAKE, **kw):
    """one request as icc.update_requests takes it; every family gets its own fake level pointers"""
    r = dict(d_block=FAKE, d_mac=FAKE, d_complements=FAKE, write_step=write_step, level=level)
    for j, f in enumerate(("data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y")):
        r[f] = [base + 0x100 * j + 0x10 * (l + 1) for l in range(level + 1)]
    r.update(kw)
    return tuple(r[f] for f in OFFSETS if f != "pad")


def call(reqs, n_total=16, k=None, pad=None, null_reqs=False, ipa=None):
    from porla_amd import icc, lib
    arr = icc.update_requests(reqs)
    if pad is not None:
        arr[0].pad = pad
    a = None if null_reqs else arr
    n = len(reqs) if k is None else k
    if ipa is not None:
        return lib.porla_ipa_update_batch_device(ctypes.c_void_p(ipa or None), a, n, n_total, ctypes.c_void_p(0))
    return lib.porla_kzg_update_batch_device(a, n, n_total, ctypes.c_void_p(0))


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def test_the_symbols_are_exported():
    from porla_amd import lib
    assert hasattr(lib, "porla_kzg_update_batch_device") and hasattr(lib, "porla_ipa_update_batch_device")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_UPDATE_REQ_BYTES, UpdateReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_UPDATE_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(UpdateReq) == size == PORLA_UPDATE_REQ_BYTES == 88
    assert {f: getattr(UpdateReq, f).offset for f, _ in UpdateReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "update_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_update_req, %s) == %d" % (f, off) in src


def refused(rc, *words):
    assert rc == ERR_ARG
    msg = last_error()
    assert msg and ("porla_kzg_update_batch_device" in msg or "porla_ipa_update_batch_device" in msg)
    for w in words:
        assert w in msg, msg


def test_null_reqs_is_refused():
    refused(call([good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("field", ["d_block", "d_mac"])
def test_a_null_block_or_mac_is_refused(field):
    refused(call([good(base=0x2000), good(**{field: 0})]), "NULL", "request 1")


@pytest.mark.parametrize("field", ["data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y"])
def test_a_null_family_array_or_level_pointer_is_refused(field):
    refused(call([good(**{field: None})]), "NULL family")
    ptrs = list(good()[5 + ["data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y"].index(field)])
    ptrs[1] = 0
    refused(call([good(**{field: ptrs})]), "NULL level")


def test_null_complements_are_fine():
    # (passes the argument checks: the next refusal is the device's)
    assert call([good(d_complements=0)]) != ERR_ARG


@pytest.mark.parametrize("n_total", [0, 1, 3, 12, 1000, (1 << 20) + 1])
def test_n_total_not_a_power_of_two_or_below_two_is_refused(n_total):
    refused(call([good(level=0, write_step=1)], n_total=n_total), "n_total")


def test_a_bad_level_is_refused():
    refused(call([good(level=5, write_step=1)], n_total=16), "level")            # 2^5 > 16
    assert call([good(level=4, write_step=1)], n_total=16) != ERR_ARG            # 2^4 = n_total is the top level
    from porla_amd import icc, lib
    arr = icc.update_requests([good()])
    arr[0].level = -1
    assert lib.porla_kzg_update_batch_device(arr, 1, 16, None) == ERR_ARG and "level" in last_error()


@pytest.mark.parametrize("write_step", [0, 16, 32, 16 << 20])
def test_crebuilds_step_is_refused(write_step):
    refused(call([good(write_step=write_step)], n_total=16), "CRebuild")


def test_a_nonzero_pad_is_refused():
    refused(call([good()], pad=1), "pad")


@pytest.mark.parametrize("field", ["data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y"])
def test_two_requests_naming_one_level_0_pointer_are_refused(field):
    a, b = good(base=0x2000), good(base=0x4000)
    i = 5 + ["data_x", "data_y", "mac_x", "mac_y", "align_x", "align_y"].index(field)
    shared = list(b[i])
    shared[0] = a[i][0]
    b = b[:i] + (shared,) + b[i + 1:]
    refused(call([a, b]), "disjoint", "request 1")
    # the same level pointers ABOVE level 0 are not this check's business (a file's levels are its own)
    assert call([a, good(base=0x4000)]) != ERR_ARG


def test_ipa_null_base_is_refused():
    refused(call([good()], ipa=0), "generators_fb")
    # and the shared checks come first on this entry point too
    refused(call([good()], ipa=0, n_total=12), "n_total")


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, null_reqs=True) == 0
    assert call([], k=0, null_reqs=True, ipa=0) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (levels 0 and 3, with and without complements) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, icc
F = 0x1000
def req(base, level, ws, comp):
    return (F, F, comp, ws, level) + tuple([base + 0x100 * j + 0x10 * l for l in range(level + 1)] for j in range(6))
reqs = [req(0x10000, 0, 1, 0), req(0x20000, 3, 8, F), req(0x30000, 4, 17, F)]
print(lib.porla_kzg_update_batch_device(icc.update_requests(reqs), 3, 16, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(ERR_NO_DEVICE)


def test_python_mirror_builds_requests():
    from porla_amd import icc
    arr = icc.update_requests([good(level=1, write_step=2, d_complements=0)])
    assert arr[0].d_block == FAKE and arr[0].d_complements is None and arr[0].write_step == 2 and arr[0].level == 1 and arr[0].pad == 0
    assert arr[0].mac_y[1] == FAKE + 0x300 + 0x20
    with pytest.raises(ValueError):
        icc.update_requests([good()[:10]])
    with pytest.raises(RuntimeError, match="CRebuild"):
        icc.kzg_update_batch_device([good(write_step=16)], 16)


# ---- the model: MAC[r] + alpha * align[r] == alpha * Commit_srs(row[r] mod r) for every row of every non-empty level, X and Y.
# Derivation: at level 0 the X row is the block d with MAC X = alpha Commit(d) and align X = 0; the Y row is y = d wt mod p_icc with MAC Y
# = wt MAC X = alpha Commit(d wt) and align Y = Commit(c), c = (y - d wt) mod r, so MAC Y + alpha align Y = alpha Commit(y).  A mix
# forms a0 +- v^i a1 on the rows mod LCM = p_icc r (hence mod r) and the same combination, v^i taken mod r, on both point stores, so the
# identity is carried from the halves of level i to level i + 1.  Zero complements: they hide the MACs and are outside it.
def srs_and_alpha(n_cols):
    tau, alpha = bytes.fromhex("ffeeddccbbaa99887766554433221100"), bytes.fromhex("00112233445566778899aabbccddeeff")
    o = common.oracle()
    o.oracle_kzg_init_key(tau, ctypes.c_size_t(len(tau)), alpha, ctypes.c_size_t(len(alpha)))
    o.oracle_kzg_init_srs(ctypes.c_size_t(n_cols), (1).to_bytes(32, "big"))
    raw = ctypes.create_string_buffer(64 * n_cols)
    o.oracle_kzg_srs_g1_raw(raw)
    return raw.raw, int.from_bytes(alpha, "big")


def check_identity(fams, empty, n_cols, srs, alpha, commit):
    """fams: {family: [level bytes]}; every row of the resident half of every non-empty level"""
    import icc_py
    from tests.update_model import pt_tuple, row_vals
    q = icc_py.Q["bn254"]
    checked = 0
    for lv, is_empty in enumerate(empty):
        if is_empty:
            continue
        for part in ("x", "y"):
            for r in range(1 << lv):
                row = row_vals(fams["data_" + part][lv][r * 64 * n_cols:(r + 1) * 64 * n_cols])
                mac = pt_tuple(fams["mac_" + part][lv][64 * r:64 * r + 64])
                al = pt_tuple(fams["align_" + part][lv][64 * r:64 * r + 64])
                lhs = icc_py.ec_add("bn254", mac, icc_py.ec_mul("bn254", al, alpha))
                rhs = icc_py.ec_mul("bn254", commit([v % q for v in row]), alpha)
                assert lhs == rhs, (lv, part, r)
                checked += 1
    return checked


def test_the_model_keeps_the_mac_identity_through_seven_writes():
    import icc_py
    from tests.update_model import FileModel
    n_total, n_cols = 8, 4
    srs, alpha = srs_and_alpha(n_cols)
    m = FileModel(n_total, n_cols, "bn254", srs, fill=0xA5)
    rnd = random.Random(7)
    levels = []
    for _ in range(7):
        chunks = [rnd.getrandbits(256) for _ in range(n_cols)]
        mac = icc_py.ec_mul("bn254", m.commit([c % icc_py.Q["bn254"] for c in chunks]), alpha)   # compute_digest = alpha * Commit_srs
        _, level = m.update(chunks, mac)
        levels.append(level)
        assert check_identity(m.family_bytes(), m.empty, n_cols, srs, alpha, m.commit) > 0
    assert levels == [0, 1, 0, 2, 0, 1, 0]                                                        # the ruler sequence
    assert m.next_level() is None                                                                 # write 8 is CRebuild's

"""CPU: the batched server rebuild's C ABI (include/porla_gpu.h: porla_server_rebuild_batch_device) -- the symbol is exported, the ctypes
mirror of porla_server_rebuild_req has the layout the library static_asserts, every bad argument is refused with PORLA_ERR_ARG before
the device is touched, k = 0 is a no-op, and valid arguments without a device give PORLA_ERR_NO_DEVICE.  Nothing here computes on a
device: the pointer values are never dereferenced.  And the model the GPU tests compare against (tests/server_rebuild_model.py) is
checked against an independent statement of the two networks at n_total = 4 and 8."""
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
WHO = "porla_server_rebuild_batch_device"
POINTERS = ("d_block", "d_mac", "d_complements", "d_u_blocks", "d_u_macs", "d_data_x", "d_data_y", "d_mac_x", "d_mac_y", "d_align_x",
            "d_align_y")
OUTPUTS = POINTERS[3:]
OFFSETS = dict({f: 8 * i for i, f in enumerate(POINTERS)}, write_step=88, index=96)


def good(base=0x10000, **kw):
    """one request as icc.server_rebuild_requests takes it; every pointer its own fake 16-byte aligned address"""
    r = {f: base + 0x100 * (i + 1) for i, f in enumerate(POINTERS)}
    r.update(write_step=16, index=1)
    r.update(kw)
    return tuple(r[f] for f in OFFSETS)


def call(reqs, n_total=16, n_cols=128, curve=0, k=None, null_reqs=False):
    from porla_amd import icc, lib
    arr = icc.server_rebuild_requests(reqs)
    return lib.porla_server_rebuild_batch_device(None if null_reqs else arr, len(reqs) if k is None else k, n_total, n_cols, curve,
                                                 ctypes.c_void_p(0))


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def refused(rc, *words):
    assert rc == ERR_ARG
    msg = last_error()
    assert msg and WHO in msg
    for w in words:
        assert w in msg, msg


def test_the_symbol_is_exported():
    from porla_amd import lib
    assert hasattr(lib, WHO)


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import PORLA_SERVER_REBUILD_REQ_BYTES, ServerRebuildReq
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_SERVER_REBUILD_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(ServerRebuildReq) == size == PORLA_SERVER_REBUILD_REQ_BYTES == 104
    assert {f: getattr(ServerRebuildReq, f).offset for f, _ in ServerRebuildReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "server_rebuild_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_server_rebuild_req, %s) == %d" % (f, off) in src


def test_null_reqs_is_refused():
    refused(call([good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("field", [f for f in POINTERS if f != "d_complements"])
def test_a_null_pointer_is_refused(field):
    refused(call([good(), good(base=0x20000, **{field: 0})]), "NULL", "request 1")


def test_null_complements_are_fine():
    # (passes the argument checks: the next refusal is the device's)
    assert call([good(d_complements=0)]) != ERR_ARG


@pytest.mark.parametrize("field", POINTERS)
def test_a_misaligned_pointer_is_refused(field):
    refused(call([good(**{field: good()[POINTERS.index(field)] + 8})]), "16-byte aligned", "request 0")


@pytest.mark.parametrize("n_total", [0, 1, 3, 12, 1000, (1 << 16) + 1])
def test_n_total_not_a_power_of_two_or_below_two_is_refused(n_total):
    refused(call([good()], n_total=n_total), "n_total")


@pytest.mark.parametrize("n_total", [1 << 17, 1 << 20, 1 << 30])
def test_n_total_above_the_cap_is_refused_and_names_the_single_file_calls(n_total):
    refused(call([good()], n_total=n_total), "n_total", "2^16", "porla_icc_encode_xy_device", "porla_icc_mac_encode_xy_device")


def test_the_cap_itself_passes_the_checks():
    assert call([good(index=1 << 16)], n_total=1 << 16) != ERR_ARG


def test_zero_columns_are_refused():
    refused(call([good()], n_cols=0), "n_cols")


@pytest.mark.parametrize("curve", [-1, 2, 7])
def test_a_bad_curve_is_refused(curve):
    refused(call([good()], curve=curve), "curve")


@pytest.mark.parametrize("index", [0, 17, 1 << 40])
def test_an_index_outside_the_file_is_refused(index):
    refused(call([good(index=index)], n_total=16), "index", "request 0")
    assert call([good(index=16)], n_total=16) != ERR_ARG


@pytest.mark.parametrize("field", OUTPUTS)
def test_two_requests_sharing_an_output_or_store_pointer_are_refused(field):
    a, b = good(), good(base=0x20000)
    refused(call([a, good(base=0x20000, **{field: a[POINTERS.index(field)]})]), "disjoint", "request 1")
    # ... also across fields, and inside one request
    other = OUTPUTS[(OUTPUTS.index(field) + 1) % len(OUTPUTS)]
    refused(call([a, good(base=0x20000, **{field: a[POINTERS.index(other)]})]), "disjoint", "request 1")
    refused(call([good(**{field: a[POINTERS.index(other)]})]), "disjoint", "request 0")
    assert call([a, b]) != ERR_ARG
    # two requests may read the same block, MAC and complements
    assert call([a, good(base=0x20000, d_block=a[0], d_mac=a[1], d_complements=a[2])]) != ERR_ARG


def test_a_byte_size_that_overflows_is_refused():
    refused(call([good()], n_total=1 << 16, n_cols=1 << 60), "overflow")
    refused(call([good()], n_total=1 << 16, n_cols=(1 << 41) + 1), "overflow")       # n_total * n_cols * 128 wraps


def test_any_write_step_is_accepted():
    for ws in (0, 1, 16, 17, (1 << 64) - 1):
        assert call([good(write_step=ws)]) != ERR_ARG


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, null_reqs=True) == 0
    assert call([], k=0, null_reqs=True, curve=1) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both curves, with and without complements) return PORLA_ERR_NO_DEVICE"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, icc
def req(base, comp, ws, index):
    p = [base + 0x100 * (i + 1) for i in range(11)]
    p[2] = comp and p[2]
    return tuple(p) + (ws, index)
reqs = [req(0x10000, 1, 16, 1), req(0x20000, 0, 35, 16), req(0x30000, 1, 0, 7)]
for curve in (0, 1):
    print(lib.porla_server_rebuild_batch_device(icc.server_rebuild_requests(reqs), 3, 16, 128, curve, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2


def test_python_mirror_builds_requests():
    from porla_amd import icc
    arr = icc.server_rebuild_requests([good(d_complements=0, write_step=32, index=5)])
    assert arr[0].d_block == 0x10100 and arr[0].d_complements is None and arr[0].d_align_y == 0x10000 + 0x100 * 11
    assert arr[0].write_step == 32 and arr[0].index == 5
    with pytest.raises(ValueError):
        icc.server_rebuild_requests([good()[:12]])
    with pytest.raises(RuntimeError, match="index"):
        icc.server_rebuild_batch_device([good(index=0)], 16, 128, "bn254")


# ---- the model against an independent statement.  Data part: icc_py.linear_network_matrix (a recursive formulation) gives the X part
# mod p_icc, and the Y part is wt times it.  MAC part: MAC_U[i] = m_i * G for known scalars m_i, so the X part is (sum_i F[k][i] m_i) * G
# with F the same recursive network over Z_q -- its multipliers are the integers v^j mod p_icc, which the group reduces mod its order
# -- and the Y part wt times that.  Alignments: all infinity.  Complements: added on top.  The raw stores hold the write.
GENERATOR = {"bn254": (1, 2),
             "secp256k1": (0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
                           0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8)}


def network_mod_q(n, q):
    """linear_network_matrix's recursion with the multipliers (v^j mod p_icc) mod q"""
    import icc_py
    w = icc_py.root_w(n)

    def transform(vec):
        size = len(vec)
        if size == 1:
            return list(vec)
        half = size // 2
        lo, hi = transform(vec[:half]), transform(vec[half:])
        v = pow(w, n // half, icc_py.P_ICC)
        out = [0] * size
        for j in range(half):
            t = pow(v, j, icc_py.P_ICC) % q * hi[j] % q
            out[j], out[j + half] = (lo[j] + t) % q, (lo[j] - t) % q
        return out

    return transform


@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
@pytest.mark.parametrize("n_total,write_step", [(4, 8), (4, 7), (8, 16), (8, 21)])
def test_the_model_agrees_with_an_independent_statement(curve, n_total, write_step):
    import icc_py
    from tests.server_rebuild_model import RebuildFileModel
    from tests.update_model import pt_bytes, pt_tuple, row_vals
    n_cols, fill = 3, 0xA5
    rnd = random.Random(1000 * n_total + write_step)
    q, p_icc, G = icc_py.Q[curve], icc_py.P_ICC, GENERATOR[curve]
    m = RebuildFileModel(n_total, n_cols, curve, b"", fill=fill)
    rows = [[rnd.getrandbits(256) for _ in range(n_cols)] for _ in range(n_total)]
    ms = [rnd.randrange(q) for _ in range(n_total)]
    ms[1] = 0                                                                         # an infinity MAC in the store
    index = n_total - 1
    for i in range(n_total):
        if i + 1 != index:
            m.store(i + 1, rows[i], icc_py.ec_mul(curve, G, ms[i]))
    cs = [rnd.randrange(q) for _ in range(2 * n_total)]
    cs[0] = 0                                                                         # an infinity complement
    comps = [icc_py.ec_mul(curve, G, c) for c in cs]
    assert m.update(rows[index - 1], icc_py.ec_mul(curve, G, ms[index - 1]), comps, index=index, write_step=write_step) == \
        (write_step, m.height - 1)
    top = m.height - 1
    wt = pow(icc_py.root_w(n_total), icc_py.reverse_bits(write_step % n_total, top), p_icc)
    assert (wt == 1) == (write_step % n_total == 0)
    # the stores
    assert bytes(m.u_blocks) == b"".join(c.to_bytes(32, "little") for r in rows for c in r)
    assert bytes(m.u_macs) == b"".join(pt_bytes(icc_py.ec_mul(curve, G, s)) for s in ms)
    # data
    T = icc_py.linear_network_matrix(n_total)
    r = 64 * n_cols
    for c in range(n_cols):
        want = T([rows[i][c] % p_icc for i in range(n_total)])
        for k in range(n_total):
            x = row_vals(m.fam["data_x"][top][k * r:(k + 1) * r])[c]
            y = row_vals(m.fam["data_y"][top][k * r:(k + 1) * r])[c]
            assert x < icc_py.LCM[curve] and y < icc_py.LCM[curve]
            assert x % p_icc == want[k] and y % p_icc == wt * want[k] % p_icc
    # MACs with the complements on top, alignments
    F = network_mod_q(n_total, q)(ms)
    for k in range(n_total):
        assert pt_tuple(m.fam["mac_x"][top][64 * k:64 * k + 64]) == icc_py.ec_mul(curve, G, (F[k] + cs[k]) % q)
        assert pt_tuple(m.fam["mac_y"][top][64 * k:64 * k + 64]) == icc_py.ec_mul(curve, G, (wt % q * F[k] + cs[n_total + k]) % q)
    for f in ("align_x", "align_y"):
        assert bytes(m.fam[f][top][:64 * n_total]) == bytes(64 * n_total)
    # untouched: the incoming halves of the top level, every lower level
    for f in m.fam:
        row = r if f.startswith("data") else 64
        assert bytes(m.fam[f][top][n_total * row:]) == bytes([fill]) * (n_total * row)
        for lv in range(top):
            assert bytes(m.fam[f][lv]) == bytes([fill]) * len(m.fam[f][lv])
    assert m.empty == [True] * top + [False]


def test_the_model_runs_a_whole_cycle():
    """update() goes through the seven H writes of a file of eight blocks and then through CRebuild's step instead of asserting"""
    import icc_py
    from tests.server_rebuild_model import RebuildFileModel
    n_total, n_cols = 8, 2
    srs = b"".join(icc_py.ec_mul("bn254", (1, 2), 5 + i)[0].to_bytes(32, "big") + icc_py.ec_mul("bn254", (1, 2), 5 + i)[1].to_bytes(32, "big")
                   for i in range(n_cols))
    m = RebuildFileModel(n_total, n_cols, "bn254", srs, fill=0xA5)
    rnd = random.Random(5)
    for step in range(1, n_total + 1):
        chunks = [rnd.getrandbits(256) for _ in range(n_cols)]
        ws, level = m.update(chunks, icc_py.ec_mul("bn254", (1, 2), rnd.getrandbits(64)), index=step)
        assert ws == step and level == ((step & -step).bit_length() - 1)
    assert m.write_step == 8 and m.empty == [True, True, True, False]
    assert m.next_level() == 0                                                         # the next cycle starts at level 0

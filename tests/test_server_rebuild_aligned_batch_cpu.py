"""CPU: the C ABI of the server's rebuild write in the CRebuild_No_Cached form (include/porla_gpu.h:
porla_kzg_server_rebuild_aligned_batch_device / porla_ipa_server_rebuild_aligned_batch_device) -- the symbols are exported, every bad
argument is refused with PORLA_ERR_ARG and a message naming the entry point before the device is touched, k = 0 is a no-op, and valid
arguments without a device give PORLA_ERR_NO_DEVICE.  Nothing here computes on a device: the pointer values are never dereferenced
(the IPA base of the refusals is a fake handle the checks return in front of; calls that pass the checks run in a child process that
sees no device).  And the model the GPU tests compare against (tests/server_rebuild_aligned_model.py) is checked against the C oracle
at n_total = 8 and against the MAC relation the alignments exist for at n_total = 4."""
import ctypes
import os
import random
import subprocess
import sys

import pytest

from tests import common
from tests.test_server_rebuild_batch_cpu import GENERATOR, OUTPUTS, POINTERS, good, network_mod_q

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
WHO = {"kzg": "porla_kzg_server_rebuild_aligned_batch_device", "ipa": "porla_ipa_server_rebuild_aligned_batch_device"}
BUILDS = ["kzg", "ipa"]
FAKE_BASE = 0x7000                # a handle the checks never read: every call below is refused in front of it


def call(build, reqs, n_total=16, k=None, null_reqs=False, base=FAKE_BASE):
    from porla_amd import icc, lib
    arr = None if null_reqs else icc.server_rebuild_requests(reqs)
    k = len(reqs) if k is None else k
    if build == "kzg":
        return lib.porla_kzg_server_rebuild_aligned_batch_device(arr, k, n_total, ctypes.c_void_p(0))
    return lib.porla_ipa_server_rebuild_aligned_batch_device(ctypes.c_void_p(base), arr, k, n_total, ctypes.c_void_p(0))


def refused(build, rc, *words):
    from porla_amd import lib
    assert rc == ERR_ARG
    msg = lib.porla_gpu_last_error().decode()
    assert msg and WHO[build] in msg
    for w in words:
        assert w in msg, msg


@pytest.mark.parametrize("build", BUILDS)
def test_the_symbol_is_exported(build):
    from porla_amd import lib
    assert hasattr(lib, WHO[build])


@pytest.mark.parametrize("build", BUILDS)
def test_null_reqs_is_refused(build):
    refused(build, call(build, [good()], null_reqs=True, k=1), "NULL")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("field", [f for f in POINTERS if f != "d_complements"])
def test_a_null_pointer_is_refused(build, field):
    refused(build, call(build, [good(), good(base=0x20000, **{field: 0})]), "NULL", "request 1")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("field", POINTERS)
def test_a_misaligned_pointer_is_refused(build, field):
    refused(build, call(build, [good(**{field: good()[POINTERS.index(field)] + 8})]), "16-byte aligned", "request 0")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n_total", [0, 1, 3, 12, 1000, (1 << 16) + 1])
def test_n_total_not_a_power_of_two_or_below_two_is_refused(build, n_total):
    refused(build, call(build, [good()], n_total=n_total), "n_total")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n_total", [1 << 17, 1 << 20, 1 << 30])
def test_n_total_above_the_cap_is_refused(build, n_total):
    refused(build, call(build, [good()], n_total=n_total), "n_total", "2^16")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("index", [0, 17, 1 << 40])
def test_an_index_outside_the_file_is_refused(build, index):
    refused(build, call(build, [good(index=index)], n_total=16), "index", "request 0")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("field", OUTPUTS)
def test_two_requests_sharing_an_output_or_store_pointer_are_refused(build, field):
    a = good()
    refused(build, call(build, [a, good(base=0x20000, **{field: a[POINTERS.index(field)]})]), "disjoint", "request 1")
    other = OUTPUTS[(OUTPUTS.index(field) + 1) % len(OUTPUTS)]                         # ... also across fields, and inside one request
    refused(build, call(build, [a, good(base=0x20000, **{field: a[POINTERS.index(other)]})]), "disjoint", "request 1")
    refused(build, call(build, [good(**{field: a[POINTERS.index(other)]})]), "disjoint", "request 0")


@pytest.mark.parametrize("build", BUILDS)
def test_more_than_65535_requests_are_refused(build):
    from porla_amd import lib
    from porla_amd.loader import ServerRebuildReq
    arr = (ServerRebuildReq * 1)()
    if build == "kzg":
        rc = lib.porla_kzg_server_rebuild_aligned_batch_device(arr, 65536, 16, None)
    else:
        rc = lib.porla_ipa_server_rebuild_aligned_batch_device(ctypes.c_void_p(FAKE_BASE), arr, 65536, 16, None)
    refused(build, rc, "65535")


def test_a_null_base_is_refused():
    refused("ipa", call("ipa", [good()], base=0), "generators_fb", "NULL")


@pytest.mark.parametrize("build", BUILDS)
def test_k_zero_returns_zero(build):
    assert call(build, [], k=0) == 0
    assert call(build, [], k=0, null_reqs=True) == 0
    assert call(build, [], k=0, null_reqs=True, base=0) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (both builds, with and without complements, any write_step, the cap and
    the smallest file) return PORLA_ERR_NO_DEVICE.  No handle can exist there, so the IPA base is a fake one: it is not read in front
    of the device check."""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, icc
def req(base, comp, ws, index):
    p = [base + 0x100 * (i + 1) for i in range(11)]
    p[2] = comp and p[2]
    return tuple(p) + (ws, index)
reqs = [req(0x10000, 1, 16, 1), req(0x20000, 0, 35, 16), req(0x30000, 1, (1 << 64) - 1, 7)]
arr = icc.server_rebuild_requests(reqs)
one = icc.server_rebuild_requests([req(0x10000, 0, 0, 2)])
for n_total, a, k in ((16, arr, 3), (1 << 16, arr, 3), (2, one, 1)):
    print(lib.porla_kzg_server_rebuild_aligned_batch_device(a, k, n_total, None))
    print(lib.porla_ipa_server_rebuild_aligned_batch_device(ctypes.c_void_p(0x7000), a, k, n_total, None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 6


def test_python_mirrors_raise_on_a_refusal():
    from porla_amd import icc, multiexp as mx
    with pytest.raises(RuntimeError, match="index"):
        icc.kzg_server_rebuild_aligned_batch_device([good(index=0)], 16)
    with pytest.raises(ValueError):
        icc.kzg_server_rebuild_aligned_batch_device([good()[:12]], 16)
    assert callable(mx.FixedBase.ipa_server_rebuild_aligned_batch_device)


# ---- the model against the C oracle: oracle_icc_crebuild's `al` (rows mod p_icc) and `sc` (alignment scalars) outputs per part, and
# oracle_commit_batch on those scalars
def base_points(curve, n_cols):
    return (common.synth_points(n_cols) if curve == "bn254" else common.secp_bench_points(n_cols))[:64 * n_cols]


@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
@pytest.mark.parametrize("write_step", [16, 21])
def test_the_model_equals_the_c_oracle(curve, write_step):
    import icc_py
    from tests.server_rebuild_aligned_model import AlignedRebuildFileModel
    from tests.update_model import CURVE_ID
    n_total, n_cols, fill = 8, 5, 0xA5
    rnd = random.Random(300 + write_step)
    base = base_points(curve, n_cols)
    m = AlignedRebuildFileModel(n_total, n_cols, curve, base, fill=fill)
    rows = [[rnd.getrandbits(256) for _ in range(n_cols)] for _ in range(n_total)]
    rows[2] = [rnd.getrandbits(190) for _ in range(n_cols)]
    G = GENERATOR[curve]
    for i in range(n_total - 1):
        m.store(i + 1, rows[i], icc_py.ec_mul(curve, G, 3 + i))
    top = m.height - 1
    assert m.update(rows[-1], icc_py.ec_mul(curve, G, 99), None, index=n_total, write_step=write_step) == (write_step, top)
    L = common.oracle()
    raw = b"".join(c.to_bytes(32, "little") for r in rows for c in r)
    for part, fx, fa in ((0, "data_x", "align_x"), (1, "data_y", "align_y")):
        x = ctypes.create_string_buffer(64 * n_total * n_cols)
        al = ctypes.create_string_buffer(32 * n_total * n_cols)
        sc = ctypes.create_string_buffer(32 * n_total * n_cols)
        L.oracle_icc_crebuild(raw, ctypes.c_size_t(n_total), ctypes.c_size_t(n_cols), CURVE_ID[curve], part, ctypes.c_uint64(write_step), x, al,
                              sc, 2)
        half = 32 * n_total * n_cols
        assert len(m.fam[fx][top]) == 2 * half
        assert bytes(m.fam[fx][top][:half]) == al.raw
        assert bytes(m.fam[fx][top][half:]) == bytes([fill]) * half
        assert bytes(m.fam[fa][top][:64 * n_total]) == common.oracle_commit_batch(curve, sc.raw, n_total, n_cols, base)
        assert bytes(m.fam[fa][top][64 * n_total:]) == bytes([fill]) * (64 * n_total)
        assert any(bytes(m.fam[fa][top][64 * j:64 * j + 64]) != bytes(64) for j in range(n_total))


# ---- the relation the alignments exist for, at n_total = 4.  Every point is a known multiple of the generator: base point j = g_j G,
# h = eta G, MAC_i = alpha Commit(block_i) + s_i h.  The MAC network is linear with the data network's coefficients mod q, so the
# top-level MAC of row k is alpha Commit(A_k mod q) + s'_k h with s' = the network over the s_i; the stored row is A_k mod p_icc =
# A_k + c_k (mod q), and align_k = Commit(c_k).  Hence, for every resident row of either part,
#     mac + alpha * align == alpha * Commit(row mod q) + s' * h.
@pytest.mark.parametrize("curve", ["bn254", "secp256k1"])
@pytest.mark.parametrize("write_step", [4, 7])
def test_every_resident_row_satisfies_the_mac_relation(curve, write_step):
    import icc_py
    from tests.server_rebuild_aligned_model import AlignedRebuildFileModel, row32_vals
    from tests.update_model import pt_bytes, pt_tuple
    n_total, n_cols = 4, 3
    rnd = random.Random(900 + write_step)
    q, G = icc_py.Q[curve], GENERATOR[curve]
    alpha, eta = rnd.randrange(1, q), rnd.randrange(1, q)
    g = [rnd.randrange(1, q) for _ in range(n_cols)]
    base = b"".join(pt_bytes(icc_py.ec_mul(curve, G, x)) for x in g)
    rows = [[rnd.getrandbits(256) for _ in range(n_cols)] for _ in range(n_total)]
    s = [rnd.randrange(q) for _ in range(n_total)]
    macs = [icc_py.ec_mul(curve, G, (alpha * sum(c * x for c, x in zip(row, g)) + si * eta) % q) for row, si in zip(rows, s)]
    m = AlignedRebuildFileModel(n_total, n_cols, curve, base)
    for i in range(n_total - 1):
        m.store(i + 1, rows[i], macs[i])
    top = m.height - 1
    assert m.update(rows[-1], macs[-1], None, index=n_total, write_step=write_step) == (write_step, top)
    wt = pow(icc_py.root_w(n_total), icc_py.reverse_bits(write_step % n_total, top), icc_py.P_ICC)
    sx = network_mod_q(n_total, q)(s)
    nonzero = 0
    for part, scale in (("x", 1), ("y", wt % q)):
        for k in range(n_total):
            row = row32_vals(bytes(m.fam["data_" + part][top][32 * n_cols * k:32 * n_cols * (k + 1)]))
            assert all(v < icc_py.P_ICC for v in row)
            mac = pt_tuple(m.fam["mac_" + part][top][64 * k:64 * k + 64])
            align = pt_tuple(m.fam["align_" + part][top][64 * k:64 * k + 64])
            nonzero += align is not None
            lhs = icc_py.ec_add(curve, mac, icc_py.ec_mul(curve, align, alpha))
            rhs = icc_py.ec_mul(curve, G, (alpha * sum(v % q * x for v, x in zip(row, g)) + scale * sx[k] % q * eta) % q)
            assert lhs == rhs, "part %s, row %d" % (part, k)
    assert nonzero >= n_total                    # (the sums pass p_icc: the alignments are not all infinity)

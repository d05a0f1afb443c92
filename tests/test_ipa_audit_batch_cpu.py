"""CPU: the batched IPA audit's C ABI (include/porla_gpu.h: porla_ipa_audit_batch_device, porla_ipa_prove_batch_device) -- the symbols
are exported, the ctypes mirror of porla_ipa_audit_req has the layout the library static_asserts, every bad argument is refused with
PORLA_ERR_ARG before the device is touched, k = 0 is a no-op, and valid arguments without a device give PORLA_ERR_NO_DEVICE -- and
the feature's oracle on its own (tests/ipa_proof_py.py): the restated prover's proof passes the restated verifier and fails it after
one flipped bit, and the restated SHA-256 agrees with hashlib on the one hash that starts from the standard state.  Nothing here
computes on a device: the pointer values are never dereferenced."""
import ctypes
import hashlib
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
from tests import ipa_proof_py as ipa

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
FAKE = 0x1000
# the offsets porla_ipa_audit_batch_device static_asserts (porla_amd/csrc/ipa_audit_batch.hip)
OFFSETS = dict(d_rows64=0, d_idx64=8, d_coef64=16, n64=24, d_rows32=32, d_idx32=40, d_coef32=48, n32=56, d_mac_store=64,
               d_align_store=72, d_mac_idx=80, d_mac_coef=88, n_macs=96, a_value=104)


def good(**kw):
    a = dict(d_rows64=FAKE, d_idx64=FAKE, d_coef64=FAKE, n64=100, d_rows32=FAKE, d_idx32=FAKE, d_coef32=FAKE, n32=20,
             d_mac_store=FAKE, d_align_store=FAKE, d_mac_idx=FAKE, d_mac_coef=FAKE, n_macs=120, a_value=7)
    a.update(kw)
    return tuple(a[f] for f in OFFSETS)


def call(audits, k=None, out=FAKE, b=0, reqs=True, fb=FAKE):
    from porla_amd import lib, multiexp as mx
    arr = mx.ipa_audit_requests(audits) if reqs else None
    return lib.porla_ipa_audit_batch_device(ctypes.c_void_p(fb or None), arr, len(audits) if k is None else k, ctypes.c_void_p(out or None),
                                            ctypes.c_void_p(b or None), ctypes.c_void_p(0))


def prove_call(k, fb=FAKE, a=FAKE, b=FAKE, out=FAKE):
    from porla_amd import lib
    vp = ctypes.c_void_p
    return lib.porla_ipa_prove_batch_device(vp(fb or None), vp(a or None), vp(b or None), k, vp(out or None), vp(0))


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def test_the_symbols_are_exported():
    from porla_amd import lib
    assert hasattr(lib, "porla_ipa_audit_batch_device") and hasattr(lib, "porla_ipa_prove_batch_device")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import IpaAuditReq
    from porla_amd import multiexp as mx
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_IPA_AUDIT_REQ_BYTES\s+(\d+)", header).group(1))
    record = int(re.search(r"#define PORLA_IPA_AUDIT_RECORD_BYTES\s+(\d+)", header).group(1))
    proof = int(re.search(r"#define PORLA_IPA_PROOF_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(IpaAuditReq) == size == 136
    assert record == mx.IPA_AUDIT_RECORD_BYTES == 655 and proof == mx.IPA_PROOF_BYTES == ipa.PROOF_BYTES == 556
    assert {f: getattr(IpaAuditReq, f).offset for f, _ in IpaAuditReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "ipa_audit_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_ipa_audit_req, %s) == %d" % (f, off) in src


@pytest.mark.parametrize("field,counts", [
    ("d_rows64", "n64"), ("d_idx64", "n64"), ("d_coef64", "n64"),
    ("d_rows32", "n32"), ("d_idx32", "n32"), ("d_coef32", "n32"),
    ("d_mac_store", "n_macs"), ("d_align_store", "n_macs"), ("d_mac_idx", "n_macs"), ("d_mac_coef", "n_macs")])
def test_a_null_array_with_a_count_is_refused(field, counts):
    assert call([good(), good(**{field: 0})]) == ERR_ARG
    assert "NULL" in last_error() and "porla_ipa_audit_batch_device" in last_error()
    # with its count 0 the same NULL is fine (the call then fails on d_out)
    assert call([good(**{field: 0, counts: 0})], out=0) == ERR_ARG and "d_out" in last_error()


def test_more_than_32768_macs_is_refused():
    assert call([good(n_macs=32769)]) == ERR_ARG
    assert "32768" in last_error() and "porla_ipa_audit_device" in last_error()
    assert call([good(n_macs=32768)], out=0) == ERR_ARG and "d_out" in last_error()     # the limit itself passes the size check


def test_row_counts_at_or_above_2_to_32_are_refused():
    for n64, n32 in ((1 << 32, 0), (0, 1 << 32), ((1 << 31), (1 << 31)), ((1 << 32) - 1, 1), ((1 << 64) - 1, 2)):
        assert call([good(n64=n64, n32=n32)]) == ERR_ARG
        assert "2^32" in last_error()


def test_null_reqs_out_or_fixed_base_is_refused():
    assert call([good()], out=0) == ERR_ARG and "NULL" in last_error()
    assert call([good()], reqs=False, k=1) == ERR_ARG and "NULL" in last_error()
    assert call([good()], fb=0) == ERR_ARG and "gens_u_fb" in last_error()
    for kw in (dict(fb=0), dict(a=0), dict(b=0), dict(out=0)):
        assert prove_call(3, **kw) == ERR_ARG
        assert "NULL" in last_error() and "porla_ipa_prove_batch_device" in last_error()


def test_a_batch_whose_byte_size_overflows_is_refused():
    assert call([good()], k=(1 << 62), reqs=False) == ERR_ARG
    assert call([good()], k=(1 << 62)) == ERR_ARG and "overflow" in last_error()
    assert prove_call(1 << 62) == ERR_ARG and "overflow" in last_error()


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, out=0, reqs=False, fb=0) == 0
    assert prove_call(0) == 0 and prove_call(0, fb=0, a=0, b=0, out=0) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (empty challenges and no MACs included) return PORLA_ERR_NO_DEVICE.  A
    fixed base cannot exist without a device, so the handle is a stand-in that the library must not read before that check"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, multiexp as mx
F = 0x1000
audits = [(F, F, F, 3200, 0, 0, 0, 0, F, F, F, F, 3200, 5), (0, 0, 0, 0, F, F, F, 10, 0, 0, 0, 0, 0, 0),
          (0, 0, 0, 0, 0, 0, 0, 0, F, F, F, F, 32768, (1 << 256) - 1)]
vp = ctypes.c_void_p
print(lib.porla_ipa_audit_batch_device(vp(F), mx.ipa_audit_requests(audits), 3, vp(F), None, None))
print(lib.porla_ipa_prove_batch_device(vp(F), vp(F), vp(F), 64, vp(F), None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2


def test_python_mirror_builds_requests_and_splits_records():
    from porla_amd import multiexp as mx
    arr = mx.ipa_audit_requests([good(n64=5, a_value=(1 << 256) - 2), good(d_rows32=0, n32=0, a_value=b"\x01\x02")])
    assert arr[0].n64 == 5 and bytes(arr[0].a_value) == b"\xff" * 31 + b"\xfe" and arr[0].d_rows64 == FAKE
    assert arr[1].d_rows32 is None and arr[1].n32 == 0 and bytes(arr[1].a_value) == bytes(30) + b"\x01\x02"
    with pytest.raises(ValueError):
        mx.ipa_audit_requests([good()[:13]])
    with pytest.raises(ValueError):
        mx.ipa_audit_requests([good(a_value=bytes(33))])
    raw = b"".join(bytes([i + 1]) * 655 for i in range(3))
    recs = mx.split_ipa_records(raw, 3)
    assert [r["commitment"] for r in recs] == [bytes([i + 1]) * 33 for i in range(3)]
    assert recs[1]["combined_align"] == b"\x02" * 33 and len(recs[2]["proof"]) == 556 and len(recs[0]["rounds"]) == 6
    assert recs[2]["c"] == recs[2]["b1"] == int.from_bytes(b"\x03" * 32, "little") and recs[0]["rounds"][5] == (b"\x01" * 33,) * 2


# ---- the oracle on its own

def test_the_restated_sha256_agrees_with_hashlib_from_the_standard_state():
    """h0 = finalize(tag | c) is the only hash of the transcript that starts from the standard state"""
    for c in (bytes(32), bytes(range(32)), hashlib.sha256(b"c").digest()):
        t = ipa.Transcript()
        t.write(ipa.TAG)
        t.write(c)
        assert t.finalize() == hashlib.sha256(ipa.TAG + c).digest()
        assert t.s == [0] * 8 and t.bytes == 128 and t.buf == b""
        # ... and the next one is a single compression from the zero state over 33 bytes padded with the cumulative length
        t.write(b"\x02" + c)
        s = [0] * 8
        ipa.sha256_transform(s, b"\x02" + c + b"\x80" + bytes(22) + (8 * 161).to_bytes(8, "big"))
        assert t.finalize() == b"".join(v.to_bytes(4, "big") for v in s) and t.bytes == 192
    for n in (0, 1, 55, 56, 63, 64, 65, 200):
        t = ipa.Transcript()
        t.write(bytes(range(256))[:n])
        assert t.finalize() == hashlib.sha256(bytes(range(256))[:n]).digest()


def test_the_restated_prover_and_verifier_agree_and_one_flipped_bit_fails():
    rnd = random.Random(2279)
    pts = ipa.split_points(common.secp_bench_points(ipa.NUM_CHUNKS + 1), ipa.NUM_CHUNKS + 1)
    gens, u = pts[:ipa.NUM_CHUNKS], pts[ipa.NUM_CHUNKS]
    a = [rnd.randrange(ipa.N) for _ in range(ipa.NUM_CHUNKS)]
    b = ipa.audit_b(rnd.randrange(ipa.N))
    assert b[1] == b[0] * b[0] % ipa.N and b[2] == pow(b[0], 4, ipa.N)
    proof = ipa.prove(gens, u, a, b)
    commitment = ipa.msm(list(zip(a, gens)))
    assert ipa.verify(gens, u, commitment, proof)

    def flipped(at):
        p = bytearray(proof)
        p[at] ^= 1
        return bytes(p)
    assert not ipa.verify(gens, u, commitment, flipped(0))                   # c
    assert not ipa.verify(gens, u, commitment, flipped(32 + 66 * 2 + 5))     # an L (its X)
    assert not ipa.verify(gens, u, commitment, flipped(32 + 66 * 6))         # a0
    assert not ipa.verify(gens, u, ipa.msm([(2, commitment)]), proof)
    # compression round trip, infinity included
    assert ipa.decompress(ipa.compress(gens[5])) == gens[5] and ipa.decompress(ipa.compress(ipa.INF64)) == ipa.INF64

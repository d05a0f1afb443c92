"""CPU: the batched IPA verifier's C ABI (include/porla_gpu.h: porla_ipa_verify_batch_device) -- the symbol is exported, the ctypes
mirror of porla_ipa_verify_req has the layout the library static_asserts, every bad argument is refused with PORLA_ERR_ARG before
the device is touched, k = 0 is a no-op, and valid arguments without a device give PORLA_ERR_NO_DEVICE -- and the feature's oracle
on its own (tests/ipa_verify_py.py): the BVEC identity holds for the restated prover on the audit's b and fails on another b, the
closed form of x_values equals the replayed updates, and the restated parse rules accept what the prover writes and refuse a
prefix 4, X = p and an X off the curve.  Nothing here computes on a device: the pointer values are never dereferenced."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

from tests import common
from tests import ipa_proof_py as ipa
from tests import ipa_verify_py as ipv

ROOT = common.ROOT
ERR_NO_DEVICE, ERR_ARG = -1, -3
FAKE = 0x1000
# the offsets porla_ipa_verify_batch_device static_asserts (porla_amd/csrc/ipa_verify_batch.hip)
OFFSETS = dict(d_comp_store=0, d_idx=8, d_coef=16, n=24, alpha=32, a_value=64)


def good(**kw):
    a = dict(d_comp_store=FAKE, d_idx=FAKE, d_coef=FAKE, n=3200, alpha=b"\x11" * 16, a_value=7)
    a.update(kw)
    return tuple(a[f] for f in OFFSETS)


def call(verifs, k=None, records=FAKE, status=FAKE, reqs=True, fb=FAKE):
    from porla_amd import lib, multiexp as mx
    arr = mx.ipa_verify_requests(verifs) if reqs else None
    vp = ctypes.c_void_p
    return lib.porla_ipa_verify_batch_device(vp(fb or None), arr, len(verifs) if k is None else k, vp(records or None), vp(status or None),
                                             vp(0))


def last_error():
    from porla_amd import lib
    return lib.porla_gpu_last_error().decode()


def test_the_symbol_is_exported():
    from porla_amd import lib
    assert hasattr(lib, "porla_ipa_verify_batch_device")


def test_the_ctypes_struct_matches_the_library_layout():
    from porla_amd.loader import IpaVerifyReq
    from porla_amd import multiexp as mx
    header = open(os.path.join(ROOT, "include", "porla_gpu.h")).read()
    size = int(re.search(r"#define PORLA_IPA_VERIFY_REQ_BYTES\s+(\d+)", header).group(1))
    assert ctypes.sizeof(IpaVerifyReq) == size == 96
    assert {f: getattr(IpaVerifyReq, f).offset for f, _ in IpaVerifyReq._fields_} == OFFSETS
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "ipa_verify_batch.hip")).read()
    for f, off in OFFSETS.items():
        assert "offsetof(porla_ipa_verify_req, %s) == %d" % (f, off) in src
    for name, want in (("FULL", 1), ("PROOF", 2), ("MALFORMED", 4), ("BVEC", 8)):
        assert int(re.search(r"#define PORLA_IPA_VERIFY_%s\s+(\d+)" % name, header).group(1)) == want
        assert getattr(mx, "IPA_VERIFY_" + name) == getattr(ipv, name) == want
    assert mx.IPA_VERIFY_PASS == ipv.PASS == 3 and mx.IPA_VERIFY_PASS_BOUND == ipv.BOUND == 11


@pytest.mark.parametrize("field", ["d_comp_store", "d_idx", "d_coef"])
def test_a_null_array_with_a_count_is_refused(field):
    assert call([good(), good(**{field: 0})]) == ERR_ARG
    assert "NULL" in last_error() and "porla_ipa_verify_batch_device" in last_error()
    # with n = 0 the same NULL is fine (the call then fails on d_status)
    assert call([good(**{field: 0, "n": 0})], status=0) == ERR_ARG and "d_status" in last_error()


def test_more_than_32768_complements_is_refused():
    assert call([good(n=32769)]) == ERR_ARG
    assert "32768" in last_error()
    assert call([good(n=32768)], status=0) == ERR_ARG and "d_status" in last_error()     # the limit itself passes the size check


def test_null_reqs_records_status_or_fixed_base_is_refused():
    assert call([good()], records=0) == ERR_ARG and "NULL" in last_error()
    assert call([good()], status=0) == ERR_ARG and "NULL" in last_error()
    assert call([good()], reqs=False, k=1) == ERR_ARG and "NULL" in last_error()
    assert call([good()], fb=0) == ERR_ARG and "gens_u_fb" in last_error()


def test_a_batch_whose_byte_size_overflows_is_refused():
    assert call([good()], k=(1 << 62), reqs=False) == ERR_ARG
    assert call([good()], k=(1 << 62)) == ERR_ARG and "overflow" in last_error()


def test_k_zero_returns_zero():
    assert call([], k=0) == 0
    assert call([], k=0, records=0, status=0, reqs=False, fb=0) == 0


def test_valid_arguments_without_a_device_give_no_device():
    """in a child process that sees no device: valid arguments (an empty challenge included) return PORLA_ERR_NO_DEVICE.  A fixed
    base cannot exist without a device, so the handle is a stand-in that the library must not read before that check"""
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from porla_amd import lib, multiexp as mx
F = 0x1000
verifs = [(F, F, F, 3200, b"\x11" * 16, 5), (0, 0, 0, 0, 0, 0), (F, F, F, 32768, (1 << 256) - 1, (1 << 256) - 1)]
vp = ctypes.c_void_p
print(lib.porla_ipa_verify_batch_device(vp(F), mx.ipa_verify_requests(verifs), 3, vp(F), vp(F), None))
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)]


def test_python_mirror_builds_requests():
    from porla_amd import multiexp as mx
    arr = mx.ipa_verify_requests([good(n=5, alpha=b"\xaa" * 16, a_value=(1 << 256) - 2), good(d_comp_store=0, n=0, alpha=3, a_value=b"\x01\x02")])
    assert arr[0].n == 5 and arr[0].d_idx == FAKE and bytes(arr[0].alpha) == bytes(16) + b"\xaa" * 16
    assert bytes(arr[0].a_value) == b"\xff" * 31 + b"\xfe"
    assert arr[1].d_comp_store is None and arr[1].n == 0 and bytes(arr[1].alpha) == bytes(31) + b"\x03"
    assert bytes(arr[1].a_value) == bytes(30) + b"\x01\x02"
    with pytest.raises(ValueError):
        mx.ipa_verify_requests([good()[:5]])
    with pytest.raises(ValueError):
        mx.ipa_verify_requests([good(alpha=bytes(33))])
    with pytest.raises(ValueError):
        mx.ipa_verify_requests([good(a_value=bytes(33))])


# ---- the oracle on its own

def _setup():
    pts = ipa.split_points(common.secp_bench_points(ipa.NUM_CHUNKS + 1), ipa.NUM_CHUNKS + 1)
    return pts[:ipa.NUM_CHUNKS], pts[ipa.NUM_CHUNKS]


def test_the_closed_form_of_x_values_equals_the_replayed_updates():
    """x_values[j] = prod_r (bit 6 - r of j ? x_r : 1 / x_r): what a lane of k_ipa_verify_prep computes"""
    rnd = random.Random(11)
    for _ in range(3):
        xs = [rnd.randrange(1, ipa.N) for _ in range(6)]
        want = ipv.x_values(xs)
        inv = [ipa.inv(x) for x in xs]
        for j in range(ipa.NUM_CHUNKS):
            v = 1
            for r in range(6):
                v = v * (xs[r] if (j >> (6 - r)) & 1 else inv[r]) % ipa.N
            assert v == want[j], j


def test_the_folding_identity_on_random_inputs():
    """replaying the prover's fold of b on plain integers: its two survivors are the even / odd sums against x_values (20 trials)"""
    rnd = random.Random(12)
    for _ in range(20):
        xs = [rnd.randrange(1, ipa.N) for _ in range(6)]
        b = [rnd.randrange(ipa.N) for _ in range(ipa.NUM_CHUNKS)]
        xv = ipv.x_values(xs)
        cur, half = list(b), ipa.NUM_CHUNKS // 2
        for x in xs:
            ix = ipa.inv(x)
            cur = [(cur[i] * ix + cur[i + half] * x) % ipa.N for i in range(half)]
            half >>= 1
        assert len(cur) == 2
        for i in range(2):
            assert cur[i] == sum(b[j] * xv[j] for j in range(i, ipa.NUM_CHUNKS, 2)) % ipa.N


def test_bvec_holds_for_the_audits_b_and_fails_for_another_b():
    gens, u = _setup()
    rnd = random.Random(13)
    a = [rnd.randrange(ipa.N) for _ in range(ipa.NUM_CHUNKS)]
    v = rnd.randrange(ipa.N)
    commitment = ipa.msm(list(zip(a, gens)))
    honest = ipa.prove(gens, u, a, ipa.audit_b(v))
    assert ipa.verify(gens, u, commitment, honest) and ipv.bvec(honest, v)
    assert ipv.bvec(honest, v + ipa.N)                                   # a_value is taken mod n
    assert not ipv.bvec(honest, (v + 1) % ipa.N)                         # the wrong challenge value
    other = ipa.prove(gens, u, a, [rnd.randrange(ipa.N) for _ in range(ipa.NUM_CHUNKS)])
    assert ipa.verify(gens, u, commitment, other)                        # the reference's verifier takes b0, b1 on trust ...
    assert not ipv.bvec(other, v)                                        # ... this bit does not
    assert ipv.challenges(honest)[0] != ipv.challenges(other)[0]


def test_the_restated_parse_rules():
    gens, u = _setup()
    for pt in gens[:8] + [u, ipa.INF64]:
        c = ipa.compress(pt)
        assert ipv.parses(c) and ipa.decompress(c) == pt
    c = ipa.compress(gens[3])
    assert not ipv.parses(b"\x04" + c[1:])                               # an uncompressed-form prefix
    assert not ipv.parses(b"\x00" + c[1:]) and not ipv.parses(b"\x02" + bytes(32)[:31])
    assert not ipv.parses(b"\x02" + ipa.P.to_bytes(32, "big"))           # X = p
    assert not ipv.parses(b"\x03" + (2 ** 256 - 1).to_bytes(32, "big"))
    x = int.from_bytes(c[1:], "big")
    while pow((x ** 3 + 7) % ipa.P, (ipa.P - 1) // 2, ipa.P) == 1:
        x += 1
    off = b"\x02" + x.to_bytes(32, "big")
    assert not ipv.parses(off)                                           # X^3 + 7 is not a square
    with pytest.raises(ValueError):
        ipa.decompress(off)
    # the square root's addition chain as the kernel runs it: runs of ones of length 2, 3, 6, 9, 11, 22, 44, 88, 176, 220, 223
    e = 0
    for shift, add in ((223, 223), (23, 22), (6, 2), (2, 0)):
        e = (e << shift) | ((1 << add) - 1)
    assert e == (ipa.P + 1) // 4 == 2 ** 254 - 2 ** 30 - 244


def test_the_oracle_status_of_a_synthetic_reply():
    """one honest reply built on integers (no ICC level: A = O, M = alpha C + sum coef comp), then each bit switched off in turn"""
    gens, u = _setup()
    rnd = random.Random(14)
    a = [rnd.randrange(ipa.N) for _ in range(ipa.NUM_CHUNKS)]
    v, alpha = rnd.randrange(ipa.N), rnd.getrandbits(128)
    comp = [ipa.msm([(rnd.randrange(1, ipa.N), u)]) for _ in range(4)]
    idx, coef = [2, 0, 3], [rnd.getrandbits(31) for _ in range(3)]
    c_pt = ipa.msm(list(zip(a, gens)))
    m_pt = ipa.msm([(alpha, c_pt)] + [(cf, comp[i]) for i, cf in zip(idx, coef)])
    proof = ipa.prove(gens, u, a, ipa.audit_b(v))
    rec = ipa.compress(c_pt) + ipa.compress(m_pt) + ipa.INF33 + proof
    st = lambda r, al=alpha, av=v: ipv.status(gens, u, r, comp, idx, coef, al, av)
    assert st(rec) == ipv.BOUND
    assert st(rec, al=alpha + 1) == ipv.PROOF | ipv.BVEC
    assert st(rec, av=v + 1) == ipv.PASS
    flipped = bytearray(rec)
    flipped[99] ^= 1                                                     # c
    assert st(bytes(flipped)) == ipv.FULL
    assert st(b"\x04" + rec[1:]) == ipv.MALFORMED
    # L_0 = infinity: well-formed; L's hash leaves no trace in the transcript, so the challenges and BVEC stay, the proof fails
    assert st(rec[:99 + 32] + ipa.INF33 + rec[99 + 65:]) == ipv.FULL | ipv.BVEC

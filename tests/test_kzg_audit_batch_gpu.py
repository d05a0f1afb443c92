"""GPU: porla_kzg_audit_batch_device -- K complete KZG audits in one asynchronous call (include/porla_gpu.h).

Every record must be the reply Server::audit sends (Server.hpp:897-915), byte for byte what porla_kzg_audit_device gives for the
same audit with bn254_add(combined_align, align_value) as its last field; the proofs must verify; on a fresh level (alignment MACs at
infinity) the client's check commitment == combined_mac + combined_align must hold, and fail for a tampered row.  The stores come
from the protocol pipeline of test_audit_flow_gpu.py (encoded rows and encoded MACs of the same blocks)."""
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
P_ICC = 207 * 2 ** 248 + 1
NCOLS, NBLK = 128, 64
REC = 320


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _i64(v):
    import torch
    return torch.tensor(v, dtype=torch.int64).cuda()


def _u32(v):
    import numpy as np
    import torch
    return torch.tensor(np.array(v, dtype=np.uint32).view(np.int32)).cuda()


class Pipeline:
    """SRS of NCOLS, NBLK blocks encoded as the server keeps them (64-byte rows) with their encoded MACs, a second level of 32-byte
    rows < p_icc, and stores in separate allocations (a rotated MAC copy as the alignment store, a zero one for a fresh level)"""

    def __init__(self):
        import hashlib
        import torch
        from porla_amd import icc, multiexp as mx
        mx.init_key(TAU, ALPHA)
        mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))
        rows = b""
        for i in range(NBLK):
            rows += i.to_bytes(32, "little")
            rows += b"".join(hashlib.sha256(b"blk" + i.to_bytes(4, "little") + j.to_bytes(4, "little")).digest() for j in range(NCOLS - 1))
        rows_be = b"".join(rows[32 * k:32 * k + 32][::-1] for k in range(NBLK * NCOLS))
        macs_u = mx.kzg_commit_batch_host(rows_be, NBLK)
        self.x_rows = icc.crebuild_host(rows, NBLK, NCOLS, "bn254", 5, 0, want_aligned=False, want_scalars=False)[0]
        self.macs = icc.mac_crebuild_host(macs_u, NBLK, "bn254", 5, 0)
        rnd = random.Random(4242)
        self.rows32 = b"".join(rnd.randrange(P_ICC).to_bytes(32, "little") for _ in range(NBLK * NCOLS))
        self.d_rows64 = _dev(self.x_rows)
        self.d_rows32 = _dev(self.rows32)
        self.d_macs = _dev(self.macs)
        self.d_macs2 = _dev(self.macs)                             # the same MACs in another allocation
        self.d_align = _dev(self.macs[64 * 3:] + self.macs[:64 * 3])
        self.d_zero = torch.zeros(64 * NBLK, dtype=torch.uint8, device="cuda")
        self.keep = []
        torch.cuda.synchronize()

    def challenge(self, rnd, n):
        idx, coef = [rnd.randrange(NBLK) for _ in range(n)], [rnd.getrandbits(31) for _ in range(n)]
        t = (_i64(idx), _u32(coef)) if n else (None, None)
        self.keep.append(t)
        return t

    def audit(self, rnd, n64, n32, n_macs, z, mac_store=None, align_store=None, rows64=None, linked=False):
        """linked: the MACs of the challenged rows themselves (same indices and coefficients, as Server::audit draws them)"""
        i64, c64 = self.challenge(rnd, n64)
        i32, c32 = self.challenge(rnd, n32)
        im, cm = (i64, c64) if linked else self.challenge(rnd, n_macs)
        p = lambda t: t.data_ptr() if t is not None else 0
        ms = mac_store if mac_store is not None else self.d_macs
        al = align_store if align_store is not None else self.d_align
        r64 = rows64 if rows64 is not None else self.d_rows64
        return (p(r64) if n64 else 0, p(i64), p(c64), n64, self.d_rows32.data_ptr() if n32 else 0, p(i32), p(c32), n32,
                ms.data_ptr(), al.data_ptr(), p(im), p(cm), n_macs, z)


_PIPE = None


def pipe():
    global _PIPE
    if _PIPE is None:
        _PIPE = Pipeline()
    return _PIPE


def single_reply(a):
    """the record porla_kzg_audit_device gives for audit tuple a, and its B"""
    from porla_amd import multiexp as mx
    one = mx.kzg_audit_device(*a)
    rec = one["commitment"] + one["proof_h"] + one["point"] + one["claim"] + one["combined_mac"] + \
        mx.bn254_add(one["combined_align"], one["align_value"])
    return rec, one["b"]


def run_batch(audits, with_b=True, stream=None):
    import torch
    from porla_amd import multiexp as mx
    k = len(audits)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_out = torch.full((max(REC * k, 1),), 0xA5, dtype=torch.uint8, device="cuda")
        d_b = torch.full((max(32 * NCOLS * k, 1),), 0xA5, dtype=torch.uint8, device="cuda") if with_b else None
        mx.kzg_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr() if with_b else None, stream=s.cuda_stream)
    s.synchronize()
    return bytes(d_out.cpu().numpy()), bytes(d_b.cpu().numpy()) if with_b else None


def verify(rec):
    from porla_amd import multiexp as mx
    return mx.verify_proof(rec[0:64], rec[64:128], rec[128:160], rec[160:192])


def test_batch_records_equal_single_calls_and_verify():
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(11)
    audits = [
        P.audit(rnd, 3200, 0, 3200, rnd.getrandbits(64)),                            # the audit's size, 64-byte rows
        P.audit(rnd, 0, 700, 700, rnd.getrandbits(64)),                              # 32-byte rows only
        P.audit(rnd, 900, 300, 1200, rnd.getrandbits(64), mac_store=P.d_macs2),      # mixed, MACs in another allocation
        P.audit(rnd, 0, 0, 50, 12345),                                               # empty challenge
        P.audit(rnd, 400, 0, 0, 777),                                                # no MACs
        P.audit(rnd, 1000, 0, 32768, rnd.getrandbits(64)),                           # the entry limit
        P.audit(rnd, 64, 0, 64, 0),                                                  # z = 0
        P.audit(rnd, 128, 0, 128, (1 << 64) - 1),                                    # z = 2^64 - 1
        P.audit(rnd, 333, 0, 333, 99, align_store=P.d_zero, linked=True),            # a fresh level
    ]
    first = int(P.keep[-2][0][0].item())                                             # a block the fresh-level audit challenges
    audits += [P.audit(rnd, 1, 0, 1, 5, align_store=P.d_zero, linked=True),
               P.audit(rnd, 3200, 0, 3200, rnd.getrandbits(64), align_store=P.d_zero, linked=True)]
    # the tampered level: audit 8's challenge over rows with one flipped symbol in a challenged block
    tampered = bytearray(P.x_rows)
    tampered[64 * (first * NCOLS + 17)] ^= 1
    d_tampered = _dev(bytes(tampered))
    t = list(audits[8])
    t[0] = d_tampered.data_ptr()
    audits.append(tuple(t))
    got, got_b = run_batch(audits)
    recs = [got[REC * i:REC * (i + 1)] for i in range(len(audits))]
    for i, a in enumerate(audits):
        want, b = single_reply(a)
        assert recs[i] == want, "record %d differs from the single call" % i
        assert got_b[32 * NCOLS * i:32 * NCOLS * (i + 1)] == b
        assert verify(recs[i]), "proof of audit %d does not verify" % i
    assert int.from_bytes(recs[6][128:160], "big") == 0 and int.from_bytes(recs[7][128:160], "big") == (1 << 64) - 1
    assert recs[3][0:128] == bytes(128) and recs[3][160:192] == bytes(32)                 # empty challenge: B = 0
    assert recs[4][192:256] == bytes(64)                  # no MACs: combined_mac at infinity, combined_align = align_value
    # the client's check on a fresh level (Client.hpp:849-876 without alpha): commitment == combined_mac + combined_align
    for i in (8, 9, 10):
        assert recs[i][0:64] == mx.bn254_add(recs[i][192:256], recs[i][256:320])
    r = recs[11]
    assert r[0:64] != mx.bn254_add(r[192:256], r[256:320])


def _poly_store(polys, n):
    return b"".join(v.to_bytes(32, "little") for p in polys for v in p)


@pytest.mark.parametrize("n", [128, 100])
def test_device_opening_against_create_proof(n):
    """B = one 32-byte row with coefficient 1: the opening of chosen polynomials, r - 1 and 0 and values in [r, p_icc) included"""
    import torch
    from porla_amd import multiexp as mx
    mx.init_key(TAU, ALPHA)
    mx.init_SRS_from_data(n, mx.init_SRS(n))
    try:
        rnd = random.Random(n)
        polys = [[rnd.randrange(P_ICC) for _ in range(n)], [R - 1] * n, [0] * n, [rnd.randrange(R, P_ICC) for _ in range(n)],
                 [0] * (n - 1) + [R - 1], [R - 1] + [0] * (n - 1), [rnd.choice((0, R - 1, 1, R)) for _ in range(n)]]
        d_store = _dev(_poly_store(polys, n))
        one_idx, one_coef = [], []
        audits = []
        for j, _ in enumerate(polys):
            for z in (0, rnd.getrandbits(64), (1 << 64) - 1):
                d_i, d_c = _i64([j]), _u32([1])
                one_idx.append(d_i)
                one_coef.append(d_c)
                audits.append((0, 0, 0, 0, d_store.data_ptr(), d_i.data_ptr(), d_c.data_ptr(), 1, 0, 0, 0, 0, 0, z))
        torch.cuda.synchronize()
        k = len(audits)
        d_out = torch.zeros(REC * k, dtype=torch.uint8, device="cuda")
        d_b = torch.zeros(32 * n * k, dtype=torch.uint8, device="cuda")
        mx.kzg_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr())
        torch.cuda.synchronize()
        out, bb = bytes(d_out.cpu().numpy()), bytes(d_b.cpu().numpy())
        for i, a in enumerate(audits):
            p = polys[i // 3]
            b_be = b"".join(v.to_bytes(32, "big") for v in p)
            assert bb[32 * n * i:32 * n * (i + 1)] == b_be
            rec = out[REC * i:REC * (i + 1)]
            assert rec[0:192] == b"".join(mx.create_proof(a[13], b_be)), "opening %d (n=%d) differs from create_proof" % (i, n)
            assert verify(rec)
    finally:
        mx.init_SRS_from_data(NCOLS, mx.init_SRS(NCOLS))     # the same key: the same SRS as the pipeline's


def test_k_zero_one_and_three_hundred():
    import torch
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(300)
    canary = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    mx.kzg_audit_batch_device([], canary.data_ptr(), canary.data_ptr())
    torch.cuda.synchronize()
    assert bytes(canary.cpu().numpy()) == b"\x5a" * 4096
    a1 = [P.audit(rnd, 3200, 0, 3200, 31337)]
    got, _ = run_batch(a1, with_b=False)
    assert got == single_reply(a1[0])[0]
    many = [P.audit(rnd, 3200, 0, 3200, rnd.getrandbits(64)) for _ in range(300)]
    got, got_b = run_batch(many)
    for i in range(0, 300, 23):
        want, b = single_reply(many[i])
        assert got[REC * i:REC * (i + 1)] == want and got_b[32 * NCOLS * i:32 * NCOLS * (i + 1)] == b
    for i in (0, 150, 299):
        assert verify(got[REC * i:REC * (i + 1)])
    again, _ = run_batch(many, with_b=False)
    assert again == got


def test_stream_contract_async_upload():
    """the challenge uploaded asynchronously on a side stream behind a few ms of work, no host sync before the call"""
    import numpy as np
    import torch
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(5)
    specs = [(rnd.randrange(1, 3200), rnd.randrange(1, 3200), rnd.getrandbits(64)) for _ in range(6)]
    ref, late, keep = [], [], []
    for n_rows, n_macs, z in specs:
        idx, coef = [rnd.randrange(NBLK) for _ in range(n_rows)], [rnd.getrandbits(31) for _ in range(n_rows)]
        d_i, d_c = _i64(idx), _u32(coef)
        h_i = torch.tensor(idx, dtype=torch.int64).pin_memory()
        h_c = torch.tensor(np.array(coef, dtype=np.uint32).view(np.int32)).pin_memory()
        z_i = torch.zeros(n_rows, dtype=torch.int64, device="cuda")
        z_c = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
        keep += [d_i, d_c, h_i, h_c, z_i, z_c]
        m = min(n_macs, n_rows)
        ref.append((P.d_rows64.data_ptr(), d_i.data_ptr(), d_c.data_ptr(), n_rows, 0, 0, 0, 0, P.d_macs.data_ptr(), P.d_align.data_ptr(),
                    d_i.data_ptr(), d_c.data_ptr(), m, z))
        late.append((P.d_rows64.data_ptr(), z_i.data_ptr(), z_c.data_ptr(), n_rows, 0, 0, 0, 0, P.d_macs.data_ptr(), P.d_align.data_ptr(),
                     z_i.data_ptr(), z_c.data_ptr(), m, z))
    want, want_b = run_batch(ref)
    side = torch.cuda.Stream()
    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(REC * len(late), dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(32 * NCOLS * len(late), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big.normal_()
        for j in range(len(specs)):
            keep[6 * j + 4].copy_(keep[6 * j + 2], non_blocking=True)
            keep[6 * j + 5].copy_(keep[6 * j + 3], non_blocking=True)
        mx.kzg_audit_batch_device(late, d_out.data_ptr(), d_b.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert bytes(d_out.cpu().numpy()) == want and bytes(d_b.cpu().numpy()) == want_b


def test_two_threads_and_single_calls_interleaved():
    import torch
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(77)
    sets = [[P.audit(rnd, rnd.randrange(100, 3200), 0, rnd.randrange(0, 3200), rnd.getrandbits(64)) for _ in range(16)] for _ in range(2)]
    want = [run_batch(s)[0] for s in sets]
    singles = [single_reply(sets[0][i])[0] for i in range(4)]
    got = [[], []]
    sgot = []
    errs = []

    def batch_worker(t):
        try:
            s = torch.cuda.Stream()
            for _ in range(5):
                got[t].append(run_batch(sets[t], with_b=False, stream=s)[0])
        except Exception as e:                    # noqa: BLE001 -- reported below
            errs.append(e)

    def single_worker():
        try:
            for _ in range(5):
                sgot.append([single_reply(sets[0][i])[0] for i in range(4)])
        except Exception as e:                    # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=batch_worker, args=(t,)) for t in (0, 1)] + [threading.Thread(target=single_worker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for t in (0, 1):
        assert len(got[t]) == 5 and all(g == want[t] for g in got[t])
    assert all(s == singles for s in sgot)
    assert [want[0][REC * i:REC * (i + 1)] for i in range(4)] == singles

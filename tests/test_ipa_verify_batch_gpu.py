"""GPU: porla_ipa_verify_batch_device -- Client::audit's check (IPA build) of K replies in one asynchronous call (include/porla_gpu.h).

Every status byte must equal the oracle's (tests/ipa_verify_py.py: Python integers and the C secp256k1 oracle) AND the literal list
written beside it, so that a test whose construction is wrong fails instead of agreeing with itself.  The replies come from the
server batch (porla_ipa_audit_batch_device) over an honest level: rows -> their commitments on the generators -> the encoded MACs
M_i; complements comp_i = s_i h; the MAC store M'_i = alpha M_i + comp_i built with the batched MSM; a fresh level (alignment store
at infinity) and a linked challenge."""
import hashlib
import random
import threading

import pytest

from tests import common
from tests import ipa_proof_py as ipa
from tests import ipa_verify_py as ipv

pytestmark = pytest.mark.gpu

N = common.SECP_N
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")
NCOLS, NBLK = 128, 64
REC = 655
WINDOW = 11            # an explicit small table, as tests/test_ipa_audit_batch_gpu.py takes
FULL, PROOF, MALFORMED, BVEC = 1, 2, 4, 8
BOUND = FULL | PROOF | BVEC


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
    """NBLK blocks encoded as the server keeps them (64-byte rows) with their encoded MACs M_i = the ICC network over the rows'
    commitments on generators[0..127]; the client's complements comp_i = s_i h and the honest MAC store M'_i = alpha M_i + comp_i
    (the batched MSM over 2-pair entries); a zero alignment store (a fresh level)"""

    def __init__(self):
        import torch
        from porla_amd import icc, multiexp as mx
        pts = common.secp_bench_points(NCOLS + 2)
        self.gens_u = pts[:64 * (NCOLS + 1)]
        h = pts[64 * (NCOLS + 1):]
        self.points = ipa.split_points(self.gens_u, NCOLS + 1)
        self.gens, self.u = self.points[:NCOLS], self.points[NCOLS]
        self.fb = mx.FixedBase("secp256k1", self.gens_u, NCOLS + 1, WINDOW)
        rows = b""
        for i in range(NBLK):
            rows += i.to_bytes(32, "little")
            for j in range(NCOLS - 1):
                d = hashlib.sha256(b"blk" + i.to_bytes(4, "little") + j.to_bytes(4, "little")).digest()
                rows += d[:31] + bytes([d[31] & 0x7f])                       # a chunk below p_icc (little-endian: the top byte last)
        rows_be = b"".join(rows[32 * k:32 * k + 32][::-1] for k in range(NBLK * NCOLS))
        macs_u = self.fb.commit_host(rows_be, NBLK, NCOLS)
        self.x_rows = icc.crebuild_host(rows, NBLK, NCOLS, "secp256k1", 5, 0, want_aligned=False, want_scalars=False)[0]
        macs = icc.mac_crebuild_host(macs_u, NBLK, "secp256k1", 5, 0)
        rnd = random.Random(9191)
        self.comp_list = [ipa.msm([(rnd.randrange(1, N), h)]) for _ in range(NBLK)]
        self.comp = b"".join(self.comp_list)
        sc = (bytes(16) + ALPHA + (1).to_bytes(32, "big")) * NBLK
        pt = b"".join(macs[64 * i:64 * i + 64] + self.comp_list[i] for i in range(NBLK))
        self.macs_a = b"".join(mx.msm_batch_host("secp256k1", sc, pt, mx.batch_offsets([2] * NBLK)))
        self.d_rows64 = _dev(self.x_rows)
        self.d_macs_a = _dev(self.macs_a)
        self.d_comp = _dev(self.comp)
        self.d_zero = torch.zeros(64 * NBLK, dtype=torch.uint8, device="cuda")
        self.keep = []
        torch.cuda.synchronize()

    def reply(self, rnd, n, rows64=None, alpha=ALPHA, a_value=None):
        """(server audit tuple, client verify tuple, (idx, coef)) of a linked challenge of n rows on the fresh level"""
        idx, coef = [rnd.randrange(NBLK) for _ in range(n)], [rnd.getrandbits(31) for _ in range(n)]
        d_i, d_c = (_i64(idx), _u32(coef)) if n else (None, None)
        self.keep.append((d_i, d_c))
        p = lambda t: t.data_ptr() if t is not None else 0
        r64 = rows64 if rows64 is not None else self.d_rows64
        v = rnd.randrange(N) if a_value is None else a_value
        audit = (p(r64) if n else 0, p(d_i), p(d_c), n, 0, 0, 0, 0, self.d_macs_a.data_ptr(), self.d_zero.data_ptr(), p(d_i), p(d_c), n, v)
        return audit, (self.d_comp.data_ptr() if n else 0, p(d_i), p(d_c), n, alpha, v), (idx, coef)


_PIPE = None


def pipe():
    global _PIPE
    if _PIPE is None:
        _PIPE = Pipeline()
    return _PIPE


def server_records(audits, stream=None, want_b=False):
    """the server batch's records on the device (a tensor of 655 k bytes), complete when `stream` is"""
    import torch
    P = pipe()
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_out = torch.zeros(max(REC * len(audits), 1), dtype=torch.uint8, device="cuda")
        d_b = torch.zeros(max(32 * NCOLS * len(audits), 1), dtype=torch.uint8, device="cuda") if want_b else None
        P.fb.ipa_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr() if want_b else None, stream=s.cuda_stream)
    return (d_out, d_b) if want_b else d_out


def _records(d_out, k):
    import torch
    torch.cuda.synchronize()
    raw = bytes(d_out.cpu().numpy())
    return [raw[REC * i:REC * (i + 1)] for i in range(k)]


def oracle_status(rec, verif, challenge):
    P = pipe()
    alpha, a_value = verif[4], verif[5]
    alpha = int.from_bytes(alpha, "big") if not isinstance(alpha, int) else alpha
    return ipv.status(P.gens, P.u, rec, P.comp_list, challenge[0], challenge[1], alpha, a_value)


def verify_host_records(recs, verifs):
    import torch
    P = pipe()
    d = _dev(b"".join(recs)) if recs else torch.zeros(1, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return P.fb.ipa_verify_batch_device(verifs, d.data_ptr())


def _patched(rec, at, data):
    return rec[:at] + bytes(data) + rec[at + len(data):]


def _proof_scalar_plus(rec, at, delta):
    v = (int.from_bytes(rec[at:at + 32], "little") + delta) % N
    return _patched(rec, at, v.to_bytes(32, "little"))


A0_AT = 99 + 32 + 6 * 66


def point_at(r, right):
    """offset of L_r (right = 0) or R_r (right = 1) in a record"""
    return 99 + 32 + 66 * r + 33 * right


def test_mixed_batch_matches_the_oracle():
    import torch
    P = pipe()
    rnd = random.Random(1)
    items = [P.reply(rnd, n) for n in (1, 64, 3200, 32768, 0)]                    # 0..4 honest, and an empty challenge
    items += [P.reply(rnd, 3200), P.reply(rnd, 700), P.reply(rnd, 300), P.reply(rnd, 900)]   # 5..8: tampered with below
    t_item = P.reply(rnd, 500)
    first = t_item[2][0][0]
    tampered = bytearray(P.x_rows)
    tampered[64 * (first * NCOLS + 17)] ^= 1
    d_tampered = _dev(bytes(tampered))
    a = list(t_item[0])
    a[0] = d_tampered.data_ptr()
    items.append((tuple(a), t_item[1], t_item[2]))                                # 9: a tampered row (the MAC check fails, the proof holds)
    wa = P.reply(rnd, 900)
    items.append((wa[0], wa[1][:4] + (b"\x5a" * 16, wa[1][5]), wa[2]))           # 10: a wrong alpha
    items.append(P.reply(rnd, 400))                                               # 11: a proof for another b spliced in below
    wv = P.reply(rnd, 200)
    items.append((wv[0], wv[1][:5] + ((wv[1][5] + 1) % N,), wv[2]))              # 12: a wrong a_value in the request
    d_out, d_b = server_records([it[0] for it in items], want_b=True)
    recs = _records(d_out, len(items))
    assert recs[4][:99] == bytes(99)                                              # the empty challenge: C = M = A = O
    recs[5] = _patched(recs[5], 99, bytes([recs[5][99] ^ 1]))                     # 5: c with a flipped bit
    recs[6] = _patched(recs[6], point_at(3, 0), recs[6][point_at(3, 1):point_at(3, 1) + 33])    # 6: L_3 replaced by R_3
    recs[7] = _proof_scalar_plus(recs[7], A0_AT, 1)                               # 7: a0 + 1
    recs[8] = recs[1][:33] + recs[8][33:]                                         # 8: the commitment of another record
    # 11: the prover alone on a = B of that audit and a random b
    b_rand = b"".join(rnd.randrange(N).to_bytes(32, "big") for _ in range(NCOLS))
    d_brand = _dev(b_rand)
    d_proof = torch.zeros(556, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    P.fb.ipa_prove_batch_device(d_b.data_ptr() + 32 * NCOLS * 11, d_brand.data_ptr(), 1, d_proof.data_ptr())
    torch.cuda.synchronize()
    recs[11] = recs[11][:99] + bytes(d_proof.cpu().numpy())
    verifs = [it[1] for it in items]
    got = verify_host_records(recs, verifs)
    want = [oracle_status(recs[i], verifs[i], items[i][2]) for i in range(len(items))]
    print("status", got, "oracle", want)
    assert got == want
    assert want == [BOUND] * 5 + [FULL, FULL | BVEC, FULL | BVEC, BVEC, PROOF | BVEC, PROOF | BVEC, FULL | PROOF, FULL | PROOF]


def test_malformed_records_are_flagged_alone():
    P = pipe()
    rnd = random.Random(4)
    items = [P.reply(rnd, 64) for _ in range(6)]
    recs = _records(server_records([it[0] for it in items]), 6)
    verifs = [it[1] for it in items]
    assert verify_host_records(recs, verifs) == [BOUND] * 6
    bad = list(recs)
    bad[1] = b"\x04" + bad[1][1:]                                                 # prefix byte 4 on C
    bad[3] = _patched(bad[3], 34, ipa.P.to_bytes(32, "big"))                      # X = p on M
    x = int.from_bytes(bad[4][point_at(5, 1) + 1:point_at(5, 1) + 33], "big")
    while pow((x ** 3 + 7) % ipa.P, (ipa.P - 1) // 2, ipa.P) == 1:
        x += 1
    bad[4] = _patched(bad[4], point_at(5, 1) + 1, x.to_bytes(32, "big"))          # an X with no square root on R_5
    bad[5] = _patched(bad[5], point_at(1, 0), bytes(33))                          # L_1 = infinity: well-formed, no proof
    got = verify_host_records(bad, verifs)
    want = [oracle_status(bad[i], verifs[i], items[i][2]) for i in range(6)]
    print("status", got, "oracle", want)
    assert got == want
    assert want == [BOUND, MALFORMED, BOUND, MALFORMED, MALFORMED, FULL | BVEC]


def test_k_zero_one_three_and_three_hundred():
    import torch
    P = pipe()
    rnd = random.Random(5)
    fill = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert P.fb.ipa_verify_batch_device([], fill.data_ptr(), d_status=fill.data_ptr()) is None
    torch.cuda.synchronize()
    assert bytes(fill.cpu().numpy()) == b"\x5a" * 4096                            # k = 0 writes nothing
    assert P.fb.ipa_verify_batch_device([], 0) == []
    one = P.reply(rnd, 3200)
    recs = _records(server_records([one[0]]), 1)
    assert verify_host_records(recs, [one[1]]) == [BOUND]
    assert verify_host_records([_proof_scalar_plus(recs[0], A0_AT, 1)], [one[1]]) == [FULL | BVEC]
    three = [P.reply(rnd, n) for n in (5, 0, 70)]
    recs = _records(server_records([it[0] for it in three]), 3)
    recs[2] = _proof_scalar_plus(recs[2], A0_AT + 32, 1)                          # b0 + 1: neither the proof nor the binding holds
    got = verify_host_records(recs, [it[1] for it in three])
    assert got == [oracle_status(recs[i], three[i][1], three[i][2]) for i in range(3)] == [BOUND, BOUND, FULL]
    many = [P.reply(rnd, rnd.randrange(0, 3200)) for _ in range(300)]
    recs = _records(server_records([it[0] for it in many]), 300)
    for i in (17, 150, 299):
        recs[i] = _proof_scalar_plus(recs[i], A0_AT, i)
    got = verify_host_records(recs, [it[1] for it in many])
    for i in list(range(0, 300, 29)) + [17, 150, 299]:
        assert got[i] == oracle_status(recs[i], many[i][1], many[i][2]), i
    assert [i for i, s in enumerate(got) if s != BOUND] == [17, 150, 299]
    assert [got[i] for i in (17, 150, 299)] == [FULL | BVEC] * 3


def test_end_to_end_on_one_stream():
    """the server batch writes d_records and the verifier reads them on the same stream, no host copy or wait in between; the
    status bytes stay on the device until the stream is done"""
    import torch
    P = pipe()
    rnd = random.Random(2)
    items = [P.reply(rnd, rnd.choice((1, 64, 3200, 2000))) for _ in range(64)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    d_out = server_records([it[0] for it in items], stream=s)
    with torch.cuda.stream(s):
        d_status = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
        P.fb.ipa_verify_batch_device([it[1] for it in items], d_out.data_ptr(), d_status=d_status.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert list(bytes(d_status.cpu().numpy())) == [BOUND] * 64


def test_stream_contract_async_upload():
    """the records uploaded asynchronously on a side stream behind a few ms of work, no host sync before the call"""
    import torch
    P = pipe()
    rnd = random.Random(6)
    items = [P.reply(rnd, rnd.randrange(1, 3200)) for _ in range(6)]
    recs = _records(server_records([it[0] for it in items]), 6)
    recs[3] = _proof_scalar_plus(recs[3], A0_AT, 1)
    h_rec = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).pin_memory()
    late = torch.zeros(REC * 6, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        d_status = torch.zeros(6, dtype=torch.uint8, device="cuda")
        for _ in range(4):
            big.normal_()
        late.copy_(h_rec, non_blocking=True)
        P.fb.ipa_verify_batch_device([it[1] for it in items], late.data_ptr(), d_status=d_status.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert list(bytes(d_status.cpu().numpy())) == [BOUND] * 3 + [FULL | BVEC] + [BOUND] * 2


def test_two_threads_beside_the_server_batch_on_the_same_base():
    import torch
    P = pipe()
    rnd = random.Random(7)
    sets, d_recs = [], []
    for t in range(2):
        items = [P.reply(rnd, rnd.randrange(1, 3200)) for _ in range(16)]
        r = _records(server_records([it[0] for it in items]), 16)
        if t == 1:
            r[9] = _proof_scalar_plus(r[9], A0_AT, 5)
        sets.append(items)
        d_recs.append(_dev(b"".join(r)))
    want = [[BOUND] * 16, [BOUND] * 9 + [FULL | BVEC] + [BOUND] * 6]
    server_want = bytes(server_records([it[0] for it in sets[0]]).cpu().numpy())
    torch.cuda.synchronize()
    got = [[], []]
    sgot = []
    errs = []

    def verify_worker(t):
        try:
            s = torch.cuda.Stream()
            for _ in range(5):
                got[t].append(P.fb.ipa_verify_batch_device([it[1] for it in sets[t]], d_recs[t].data_ptr(), stream=s.cuda_stream))
        except Exception as e:                    # noqa: BLE001 -- reported below
            errs.append(e)

    def server_worker():
        try:
            s = torch.cuda.Stream()
            for _ in range(3):
                d = server_records([it[0] for it in sets[0]], stream=s)
                s.synchronize()
                sgot.append(bytes(d.cpu().numpy()))
        except Exception as e:                    # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=verify_worker, args=(t,)) for t in (0, 1)] + [threading.Thread(target=server_worker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for t in (0, 1):
        assert got[t] == [want[t]] * 5
    assert sgot == [server_want] * 3


def test_a_base_without_u_is_refused():
    from porla_amd import multiexp as mx
    P = pipe()
    short = mx.FixedBase("secp256k1", P.gens_u[:64 * NCOLS], NCOLS, WINDOW)
    it = P.reply(random.Random(8), 4)
    with pytest.raises(RuntimeError, match="129"):
        short.ipa_verify_batch_device([it[1]], P.d_comp.data_ptr(), d_status=P.d_zero.data_ptr())
    short.close()

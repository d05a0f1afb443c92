"""GPU: porla_kzg_verify_batch_device -- Client::audit's check of K replies in one call (include/porla_gpu.h).

Every status must be the verdict of the reference's own sequence for that reply (Client.hpp:685-869 through the 14 symbols:
compute_multi_exp over the challenged complements, mult_point by alpha twice, add_point twice, compare_commitment, verify_proof).
The replies come from the server batch (porla_kzg_audit_batch_device) over an honest level: complements comp_i = s_i h_MAC, the MAC
store M'_i = alpha M_i + comp_i built with the batched MSM, a fresh level (alignment store at infinity) and a linked challenge."""
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")
ALPHA32 = bytes(16) + ALPHA                     # bn254_scalar alpha: SECRET_KEY in bytes 16..31 (Client.hpp:851-853)
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
P_FIELD = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
NCOLS, NBLK = 128, 64
REC = 320
FULL, PROOF, MALFORMED = 1, 2, 4
PASS = FULL | PROOF


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
    """SRS of NCOLS, NBLK blocks encoded as the server keeps them (64-byte rows) with their encoded MACs M_i; the client's
    complements comp_i = s_i h_MAC (porla_kzg_complement_batch_host) and the honest MAC store M'_i = alpha M_i + comp_i (the batched
    MSM over 2-pair entries); a zero alignment store (a fresh level)"""

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
        macs = icc.mac_crebuild_host(macs_u, NBLK, "bn254", 5, 0)
        rnd = random.Random(9090)
        s = b"".join(rnd.randrange(1, R).to_bytes(32, "big") for _ in range(NBLK))
        self.comp = mx.kzg_complement_batch_host(s, NBLK)
        sc = (ALPHA32 + (1).to_bytes(32, "big")) * NBLK
        pt = b"".join(macs[64 * i:64 * i + 64] + self.comp[64 * i:64 * i + 64] for i in range(NBLK))
        self.macs_a = b"".join(mx.msm_batch_host("bn254", sc, pt, mx.batch_offsets([2] * NBLK)))
        self.d_rows64 = _dev(self.x_rows)
        self.d_macs_a = _dev(self.macs_a)
        self.d_comp = _dev(self.comp)
        self.d_zero = torch.zeros(64 * NBLK, dtype=torch.uint8, device="cuda")
        self.keep = []
        torch.cuda.synchronize()

    def reply(self, rnd, n, rows64=None, alpha=ALPHA):
        """(server audit tuple, client verify tuple, (idx, coef)) of a linked challenge of n rows on the fresh level"""
        idx, coef = [rnd.randrange(NBLK) for _ in range(n)], [rnd.getrandbits(31) for _ in range(n)]
        d_i, d_c = (_i64(idx), _u32(coef)) if n else (None, None)
        self.keep.append((d_i, d_c))
        p = lambda t: t.data_ptr() if t is not None else 0
        r64 = rows64 if rows64 is not None else self.d_rows64
        audit = (p(r64) if n else 0, p(d_i), p(d_c), n, 0, 0, 0, 0, self.d_macs_a.data_ptr(), self.d_zero.data_ptr(), p(d_i), p(d_c), n,
                 rnd.getrandbits(64))
        return audit, (self.d_comp.data_ptr(), p(d_i), p(d_c), n, alpha), (idx, coef)


_PIPE = None


def pipe():
    global _PIPE
    if _PIPE is None:
        _PIPE = Pipeline()
    return _PIPE


def server_records(audits, stream=None):
    """the server batch's records on the device (a tensor of 320 k bytes), complete when `stream` is"""
    import torch
    from porla_amd import multiexp as mx
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_out = torch.zeros(max(REC * len(audits), 1), dtype=torch.uint8, device="cuda")
        mx.kzg_audit_batch_device(audits, d_out.data_ptr(), stream=s.cuda_stream)
    return d_out


def reference_status(rec, challenge, alpha=ALPHA):
    """Client::audit's verdicts on one reply through the 14 symbols (Client.hpp:685-869)"""
    from porla_amd import multiexp as mx
    P = pipe()
    idx, coef = challenge
    if idx:
        pts = b"".join(P.comp[64 * i:64 * i + 64] for i in idx)
        comp = mx.bn254_multi_exp(pts, b"".join(mx.bn254_scalar_set_int(c) for c in coef), len(idx))
    else:
        comp = mx.bn254_set_infinity()
    a32 = bytes(32 - len(alpha)) + alpha
    commitment = mx.bn254_add(mx.bn254_mult(rec[0:64], a32), comp)
    combined_mac = mx.bn254_add(rec[192:256], mx.bn254_mult(rec[256:320], a32))
    full = mx.bn254_compare(commitment, combined_mac)
    proof = mx.verify_proof(rec[0:64], rec[64:128], rec[128:160], rec[160:192])
    return (FULL if full else 0) | (PROOF if proof else 0)


def verify_host_records(recs, verifs, weights=None):
    import torch
    from porla_amd import multiexp as mx
    d = _dev(b"".join(recs)) if recs else torch.zeros(1, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return mx.kzg_verify_batch_device(verifs, d.data_ptr(), weights=weights)


def _records(d_out, k):
    import torch
    torch.cuda.synchronize()
    raw = bytes(d_out.cpu().numpy())
    return [raw[REC * i:REC * (i + 1)] for i in range(k)]


def _with_claim(rec, delta):
    y = (int.from_bytes(rec[160:192], "big") + delta) % R
    return rec[:160] + y.to_bytes(32, "big") + rec[192:]


def test_mixed_batch_matches_the_reference_sequence():
    P = pipe()
    rnd = random.Random(1)
    items = [P.reply(rnd, n) for n in (1, 64, 3200, 32768, 0)]                   # honest, and an empty challenge
    items.append(P.reply(rnd, 3200))                                              # 5: claim flipped below
    items.append(P.reply(rnd, 700))                                               # 6: H swapped below
    t_item = P.reply(rnd, 500)
    first = t_item[2][0][0]
    tampered = bytearray(P.x_rows)
    tampered[64 * (first * NCOLS + 17)] ^= 1
    d_tampered = _dev(bytes(tampered))
    a = list(t_item[0])
    a[0] = d_tampered.data_ptr()
    items.append((tuple(a), t_item[1], t_item[2]))                                # 7: a tampered row (the MAC check fails)
    wa = P.reply(rnd, 900)
    items.append((wa[0], wa[1][:4] + (b"\x5a" * 16,), wa[2]))                    # 8: a wrong alpha
    recs = _records(server_records([it[0] for it in items]), len(items))
    assert recs[4][0:128] == bytes(128) and recs[4][160:192] == bytes(32)        # the empty challenge: C = H = O, claim 0
    recs[5] = _with_claim(recs[5], 1)
    recs[6] = recs[6][:64] + recs[1][64:128] + recs[6][128:]
    verifs = [it[1] for it in items]
    got = verify_host_records(recs, verifs)
    want = [reference_status(recs[i], items[i][2], verifs[i][4]) for i in range(len(items))]
    assert got == want
    assert want == [PASS] * 5 + [FULL, FULL, PROOF, PROOF]


def test_end_to_end_on_one_stream():
    """the server batch writes d_records and the verifier reads them on the same stream, no host copy or wait in between"""
    import torch
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(2)
    items = [P.reply(rnd, rnd.choice((1, 64, 3200, 2000))) for _ in range(64)]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    d_out = server_records([it[0] for it in items], stream=s)
    got = mx.kzg_verify_batch_device([it[1] for it in items], d_out.data_ptr(), stream=s.cuda_stream)
    assert got == [PASS] * 64


def test_cancelling_errors_are_caught_by_random_weights():
    """claims y1 + d and y2 - d cancel in the folded sum when the two weights are equal; drawn weights (per call) and random weights
    of the test's own catch both, and every other reply still passes"""
    P = pipe()
    rnd = random.Random(3)
    items = [P.reply(rnd, 3200) for _ in range(8)]
    recs = _records(server_records([it[0] for it in items]), 8)
    d = rnd.randrange(1, R)
    recs[2], recs[5] = _with_claim(recs[2], d), _with_claim(recs[5], -d)
    verifs = [it[1] for it in items]
    want = [reference_status(recs[i], items[i][2]) for i in range(8)]
    assert want == [PASS, PASS, FULL, PASS, PASS, FULL, PASS, PASS]
    assert verify_host_records(recs, verifs, weights=[12345] * 8) == [PASS] * 8     # the construction cancels
    for _ in range(2):
        assert verify_host_records(recs, verifs) == want
    assert verify_host_records(recs, verifs, weights=[rnd.getrandbits(128) | 1 for _ in range(8)]) == want


def test_malformed_records_are_flagged_alone():
    P = pipe()
    rnd = random.Random(4)
    items = [P.reply(rnd, 64) for _ in range(6)]
    recs = _records(server_records([it[0] for it in items]), 6)
    verifs = [it[1] for it in items]
    base = verify_host_records(recs, verifs)
    assert base == [PASS] * 6
    bad = list(recs)
    cy = (int.from_bytes(bad[1][32:64], "big") + 1) % P_FIELD
    bad[1] = bad[1][:32] + cy.to_bytes(32, "big") + bad[1][64:]                   # C off the curve
    bad[3] = bad[3][:192] + P_FIELD.to_bytes(32, "big") + bad[3][224:]           # a coordinate of M equal to p
    bad[4] = bad[4][:256] + b"\xff" * 32 + bad[4][288:]                          # a coordinate of A above 2^255
    got = verify_host_records(bad, verifs)
    assert got == [PASS, MALFORMED, PASS, MALFORMED, MALFORMED, PASS]
    bad[0] = _with_claim(bad[0], 7)                                              # with a failing opening beside them too
    got = verify_host_records(bad, verifs)
    assert got == [FULL, MALFORMED, PASS, MALFORMED, MALFORMED, PASS]


def test_k_zero_one_three_hundred_and_the_limit():
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(5)
    assert mx.kzg_verify_batch_device([], 0) == []
    one = P.reply(rnd, 3200)
    recs = _records(server_records([one[0]]), 1)
    assert verify_host_records(recs, [one[1]]) == [PASS]
    assert verify_host_records([_with_claim(recs[0], 1)], [one[1]]) == [FULL]
    many = [P.reply(rnd, rnd.randrange(0, 3200)) for _ in range(300)]
    recs = _records(server_records([it[0] for it in many]), 300)
    for i in (17, 150, 299):
        recs[i] = _with_claim(recs[i], i)
    got = verify_host_records(recs, [it[1] for it in many])
    for i in list(range(0, 300, 29)) + [17, 150, 299]:
        assert got[i] == reference_status(recs[i], many[i][2]), i
    assert [i for i, s in enumerate(got) if s != PASS] == [17, 150, 299]
    # the limit: 10 922 replies, P = one entry of 32 766 pairs; a few distinct replies tiled
    k = mx.KZG_VERIFY_MAX_K
    base = [P.reply(rnd, 64) for _ in range(6)]
    brecs = _records(server_records([it[0] for it in base]), 6)
    recs = [brecs[i % 6] for i in range(k)]
    recs[k - 1] = _with_claim(recs[k - 1], 3)
    got = verify_host_records(recs, [base[i % 6][1] for i in range(k)])
    assert got[:k - 1] == [PASS] * (k - 1) and got[k - 1] == FULL


def test_stream_contract_async_upload():
    """the challenge uploaded asynchronously on a side stream behind a few ms of work, no host sync before the call"""
    import numpy as np
    import torch
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(6)
    items = [P.reply(rnd, rnd.randrange(1, 3200)) for _ in range(6)]
    d_rec = server_records([it[0] for it in items])
    torch.cuda.synchronize()
    late, keep = [], []
    for _, v, (idx, coef) in items:
        h_i = torch.tensor(idx, dtype=torch.int64).pin_memory()
        h_c = torch.tensor(np.array(coef, dtype=np.uint32).view(np.int32)).pin_memory()
        z_i = torch.zeros(len(idx), dtype=torch.int64, device="cuda")
        z_c = torch.zeros(len(idx), dtype=torch.int32, device="cuda")
        keep.append((h_i, h_c, z_i, z_c))
        late.append((v[0], z_i.data_ptr(), z_c.data_ptr(), v[3], v[4]))
    side = torch.cuda.Stream()
    big = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            big.normal_()
        for h_i, h_c, z_i, z_c in keep:
            z_i.copy_(h_i, non_blocking=True)
            z_c.copy_(h_c, non_blocking=True)
        got = mx.kzg_verify_batch_device(late, d_rec.data_ptr(), stream=side.cuda_stream)
    assert got == [PASS] * 6


def test_two_threads_beside_single_verify_proof():
    import torch
    from porla_amd import multiexp as mx
    P = pipe()
    rnd = random.Random(7)
    sets, recs = [], []
    for t in range(2):
        items = [P.reply(rnd, rnd.randrange(1, 3200)) for _ in range(16)]
        r = _records(server_records([it[0] for it in items]), 16)
        if t == 1:
            r[9] = _with_claim(r[9], 5)
        sets.append([it[1] for it in items])
        recs.append(r)
    want = [[PASS] * 16, [PASS] * 9 + [FULL] + [PASS] * 6]
    d_recs = [_dev(b"".join(r)) for r in recs]
    torch.cuda.synchronize()
    got = [[], []]
    singles = []
    errs = []

    def batch_worker(t):
        try:
            s = torch.cuda.Stream()
            for _ in range(5):
                got[t].append(mx.kzg_verify_batch_device(sets[t], d_recs[t].data_ptr(), stream=s.cuda_stream))
        except Exception as e:                    # noqa: BLE001 -- reported below
            errs.append(e)

    def single_worker():
        try:
            for _ in range(5):
                singles.append([mx.verify_proof(r[0:64], r[64:128], r[128:160], r[160:192]) for r in recs[1][8:11]])
        except Exception as e:                    # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=batch_worker, args=(t,)) for t in (0, 1)] + [threading.Thread(target=single_worker)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for t in (0, 1):
        assert got[t] == [want[t]] * 5
    assert singles == [[True, False, True]] * 5

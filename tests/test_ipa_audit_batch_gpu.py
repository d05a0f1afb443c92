"""GPU: porla_ipa_audit_batch_device and porla_ipa_prove_batch_device -- K complete IPA audits, inner-product proofs included, in one
asynchronous call (include/porla_gpu.h).

Every proof must be byte-identical to the Python restatement of Server::inner_product_prove (tests/ipa_proof_py.py, the oracle of this
feature) and pass the restated Client::inner_product_verify; the record's points and B must be what porla_ipa_audit_device gives for
the same audit (compressed), with secp256k1 add(combined_align, align_value) as combined_align.  The stores are synthetic: code
symbols below LCM = p_icc * n (64-byte rows) and below p_icc (32-byte rows), MAC stores of secp256k1 points."""
import random
import threading

import pytest

from tests import common
from tests import ipa_proof_py as ipa

pytestmark = pytest.mark.gpu

P_ICC = 207 * 2 ** 248 + 1
N = common.SECP_N
NCOLS, NBLK = 128, 64
REC, PROOF = 655, 556
WINDOW = 11            # an explicit small table (129 points x 24 windows x 1 024 multiples: 203 MB), not a share of the HBM


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
    def __init__(self):
        import torch
        from porla_amd import multiexp as mx
        pts = common.secp_bench_points(NCOLS + 1 + NBLK)
        self.gens_u = pts[:64 * (NCOLS + 1)]
        self.points = ipa.split_points(self.gens_u, NCOLS + 1)
        self.gens, self.u = self.points[:NCOLS], self.points[NCOLS]
        self.fb = mx.FixedBase("secp256k1", self.gens_u, NCOLS + 1, WINDOW)
        macs = pts[64 * (NCOLS + 1):]
        rnd = random.Random(4242)
        self.rows64 = b"".join(rnd.randrange(P_ICC * N).to_bytes(64, "little") for _ in range(NBLK * NCOLS))
        self.rows32 = b"".join(rnd.randrange(P_ICC).to_bytes(32, "little") for _ in range(NBLK * NCOLS))
        self.d_rows64, self.d_rows32 = _dev(self.rows64), _dev(self.rows32)
        self.d_macs = _dev(macs)
        self.d_align = _dev(macs[64 * 3:] + macs[:64 * 3])
        self.keep = []
        torch.cuda.synchronize()

    def challenge(self, rnd, n):
        idx, coef = [rnd.randrange(NBLK) for _ in range(n)], [rnd.getrandbits(31) for _ in range(n)]
        t = (_i64(idx), _u32(coef)) if n else (None, None)
        self.keep.append(t)
        return t

    def audit(self, rnd, n64, n32, n_macs, a_value):
        i64, c64 = self.challenge(rnd, n64)
        i32, c32 = self.challenge(rnd, n32)
        im, cm = self.challenge(rnd, n_macs)
        p = lambda t: t.data_ptr() if t is not None else 0
        return (self.d_rows64.data_ptr() if n64 else 0, p(i64), p(c64), n64, self.d_rows32.data_ptr() if n32 else 0, p(i32), p(c32), n32,
                self.d_macs.data_ptr(), self.d_align.data_ptr(), p(im), p(cm), n_macs, a_value)


_PIPE = None


def pipe():
    global _PIPE
    if _PIPE is None:
        _PIPE = Pipeline()
    return _PIPE


def single_reply(a):
    """commitment | combined_mac | combined_align after align_MAC (compressed) of porla_ipa_audit_device for audit tuple a, and its B"""
    P = pipe()
    one = P.fb.ipa_audit_device(*a[:8], NCOLS, *a[8:13])
    align = ipa.msm([(1, one["combined_align"]), (1, one["align_value"])])
    return ipa.compress(one["commitment"]) + ipa.compress(one["combined_mac"]) + ipa.compress(align), one["b"]


def run_batch(audits, with_b=True, stream=None):
    import torch
    P = pipe()
    k = len(audits)
    s = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(s):
        d_out = torch.full((max(REC * k, 1),), 0xA5, dtype=torch.uint8, device="cuda")
        d_b = torch.full((max(32 * NCOLS * k, 1),), 0xA5, dtype=torch.uint8, device="cuda") if with_b else None
        P.fb.ipa_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr() if with_b else None, stream=s.cuda_stream)
    s.synchronize()
    return bytes(d_out.cpu().numpy()), bytes(d_b.cpu().numpy()) if with_b else None


def ints_be(raw):
    return [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(len(raw) // 32)]


def check_records(audits, got, got_b, proofs_of=None):
    """every record against the single call and the Python prover / verifier (proofs_of: the audits whose proof is restated; all)"""
    P = pipe()
    for i, a in enumerate(audits):
        rec = got[REC * i:REC * (i + 1)]
        want, b = single_reply(a)
        assert rec[:99] == want, "points of record %d differ from the single call" % i
        assert got_b[32 * NCOLS * i:32 * NCOLS * (i + 1)] == b, "B of audit %d" % i
        if proofs_of is not None and i not in proofs_of:
            continue
        assert rec[99:] == ipa.prove(P.gens, P.u, ints_be(b), ipa.audit_b(a[13])), "proof %d differs from the Python prover" % i
        assert ipa.verify(P.gens, P.u, ipa.decompress(rec[0:33]), rec[99:]), "proof %d does not verify" % i


@pytest.mark.parametrize("k", [1, 3, 64])
def test_prover_is_byte_identical_to_the_python_prover(k):
    import torch
    P = pipe()
    rnd = random.Random(100 + k)
    a = [[rnd.randrange(N) for _ in range(NCOLS)] for _ in range(k)]
    b = [[rnd.randrange(N) for _ in range(NCOLS)] for _ in range(k)]
    if k >= 3:
        a[0] = [0] * NCOLS                                                   # L = R = cL u = infinity in every round
        b[1] = ipa.audit_b(0)                                                # a_value = 0
        a[2] = [rnd.choice((N, N + 1, 2 ** 256 - 1, rnd.randrange(N, 2 ** 256))) for _ in range(NCOLS)]   # inputs >= n: reduced
        b[2] = [2 ** 256 - 1 - j for j in range(NCOLS)]
    if k == 64:
        b[3] = ipa.audit_b(rnd.randrange(N))
    be = lambda rows: b"".join(v.to_bytes(32, "big") for r in rows for v in r)
    d_a, d_b = _dev(be(a)), _dev(be(b))
    d_p = torch.full((PROOF * k,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    P.fb.ipa_prove_batch_device(d_a.data_ptr(), d_b.data_ptr(), k, d_p.data_ptr())
    torch.cuda.synchronize()
    got = bytes(d_p.cpu().numpy())
    for i in range(k):
        want = ipa.prove(P.gens, P.u, a[i], b[i])
        assert got[PROOF * i:PROOF * (i + 1)] == want, "proof %d of %d" % (i, k)
        assert ipa.verify(P.gens, P.u, ipa.msm(list(zip(a[i], P.gens))), want)
    if k >= 3:
        p0 = got[:PROOF]
        assert p0[:32 + 6 * 66] == bytes(32 + 6 * 66) and p0[32 + 6 * 66:32 + 6 * 66 + 32] == bytes(32)   # c = 0, 33-zero-byte points, a0 = 0


def test_k_zero_writes_nothing():
    import torch
    P = pipe()
    canary = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    P.fb.ipa_audit_batch_device([], canary.data_ptr(), canary.data_ptr())
    P.fb.ipa_prove_batch_device(canary.data_ptr(), canary.data_ptr(), 0, canary.data_ptr())
    torch.cuda.synchronize()
    assert bytes(canary.cpu().numpy()) == b"\x5a" * 4096


def test_a_base_without_u_or_on_bn254_is_refused():
    from porla_amd import multiexp as mx
    P = pipe()
    short = mx.FixedBase("secp256k1", P.gens_u[:64 * NCOLS], NCOLS, WINDOW)
    with pytest.raises(RuntimeError, match="129"):
        short.ipa_prove_batch_device(P.d_macs.data_ptr(), P.d_macs.data_ptr(), 1, P.d_macs.data_ptr())
    with pytest.raises(RuntimeError, match="129"):
        short.ipa_audit_batch_device([P.audit(random.Random(1), 4, 0, 4, 5)], P.d_macs.data_ptr())
    short.close()


def test_one_audit():
    P = pipe()
    rnd = random.Random(1)
    audits = [P.audit(rnd, 3200, 0, 3200, rnd.randrange(N))]
    got, got_b = run_batch(audits)
    check_records(audits, got, got_b)


def test_five_audits_of_mixed_shapes():
    P = pipe()
    rnd = random.Random(5)
    audits = [
        P.audit(rnd, 0, 700, 1, rnd.randrange(N)),                  # 32-byte rows only, one MAC
        P.audit(rnd, 3200, 0, 64, rnd.randrange(2 ** 256)),         # 64-byte rows only, a_value taken mod n
        P.audit(rnd, 900, 300, 65, 0),                              # both, a_value = 0
        P.audit(rnd, 0, 0, 3200, rnd.randrange(N)),                 # empty challenge: B = 0
        P.audit(rnd, 3200, 0, 3200, rnd.randrange(N)),              # the audit's size
    ]
    got, got_b = run_batch(audits)
    check_records(audits, got, got_b)
    assert got[REC * 3:REC * 3 + 33] == bytes(33) and got_b[32 * NCOLS * 3:32 * NCOLS * 4] == bytes(32 * NCOLS)
    again, _ = run_batch(audits, with_b=False)
    assert again == got


def test_sixty_four_audits_of_3200_rows():
    P = pipe()
    rnd = random.Random(64)
    audits = [P.audit(rnd, 3200, 0, 3200, rnd.randrange(N)) for _ in range(64)]
    got, got_b = run_batch(audits)
    check_records(audits, got, got_b)


def test_stream_contract_async_upload():
    """the challenge uploaded asynchronously on a side stream behind a few ms of work, no host sync before the call"""
    import numpy as np
    import torch
    P = pipe()
    rnd = random.Random(55)
    specs = [(rnd.randrange(1, 3200), rnd.randrange(1, 3200), rnd.randrange(N)) for _ in range(6)]
    ref, late, keep = [], [], []
    for n_rows, n_macs, v in specs:
        idx, coef = [rnd.randrange(NBLK) for _ in range(n_rows)], [rnd.getrandbits(31) for _ in range(n_rows)]
        d_i, d_c = _i64(idx), _u32(coef)
        h_i = torch.tensor(idx, dtype=torch.int64).pin_memory()
        h_c = torch.tensor(np.array(coef, dtype=np.uint32).view(np.int32)).pin_memory()
        z_i = torch.zeros(n_rows, dtype=torch.int64, device="cuda")
        z_c = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
        keep += [d_i, d_c, h_i, h_c, z_i, z_c]
        m = min(n_macs, n_rows)
        ref.append((P.d_rows64.data_ptr(), d_i.data_ptr(), d_c.data_ptr(), n_rows, 0, 0, 0, 0, P.d_macs.data_ptr(), P.d_align.data_ptr(),
                    d_i.data_ptr(), d_c.data_ptr(), m, v))
        late.append((P.d_rows64.data_ptr(), z_i.data_ptr(), z_c.data_ptr(), n_rows, 0, 0, 0, 0, P.d_macs.data_ptr(), P.d_align.data_ptr(),
                     z_i.data_ptr(), z_c.data_ptr(), m, v))
    want, want_b = run_batch(ref)
    check_records(ref, want, want_b, proofs_of=(0,))
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
        P.fb.ipa_audit_batch_device(late, d_out.data_ptr(), d_b.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    assert bytes(d_out.cpu().numpy()) == want and bytes(d_b.cpu().numpy()) == want_b


def test_two_threads_and_single_calls_interleaved():
    import torch
    P = pipe()
    rnd = random.Random(77)
    sets = [[P.audit(rnd, rnd.randrange(100, 3200), 0, rnd.randrange(1, 3200), rnd.randrange(N)) for _ in range(16)] for _ in range(2)]
    want = [run_batch(s)[0] for s in sets]          # one after the other
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
    assert [want[0][REC * i:REC * i + 99] for i in range(4)] == singles

"""GPU: the host scaffold the batched entry points share (porla_amd/csrc/batch_host.hpp, PinnedList) on the path none of their own
tests drives: call A with K = 2 on one stream, held in flight behind a few milliseconds of other work, then, with no host
synchronisation in between, call B with K = 5 on another stream.  B's work list and buffers are larger than A's, so the device
buffers regrow behind the fence and the staged work list is too small or still queued.  Both calls' outputs must be byte-equal to what
the entry point's own test module expects (single calls, the Python models and oracles), never to a batched call's.

Shapes: entries of 3 pairs (k_batch_tiny) and of 70 pairs (k_batch_bucket), n64 = 5 and n32 = 3 challenged rows, update levels 0 and
2 of n_total = 8.  The KZG verify batch blocks by design, so there A and B come from two threads."""
import random
import threading

import pytest

pytestmark = pytest.mark.gpu

KA, KB = 2, 5


def _pairs(k, seed):
    """k entry sizes, both MSM paths in every call: A = 70, 3 and B = 3, 70, 3, 70, 3"""
    return ([3, 70] * k)[seed % 2:seed % 2 + k]


class Call:
    """issue(stream): the batched call on `stream`, nothing waited for; check(): the outputs against the expected values (after a
    device synchronisation)"""

    def __init__(self, issue, check):
        self.issue, self.check = issue, check


def msm_call(k, seed):
    import torch
    from porla_amd import multiexp as mx
    from tests import test_msm_batch_gpu as t
    rnd = random.Random(seed)
    sizes = _pairs(k, seed)
    offsets = mx.batch_offsets(sizes)
    n = offsets[-1]
    sc = b"".join(t.be(rnd.getrandbits(256)) for _ in range(n))
    pts = t.points_for("bn254", n)
    d_sc, d_pt = t.dev(sc), t.dev(pts)
    d_out = torch.full((64 * k,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ones = t.singles(mx, "bn254", d_sc, d_pt, offsets)
    want = [t.oracle("bn254", sc[32 * offsets[i]:32 * offsets[i + 1]], pts[64 * offsets[i]:64 * offsets[i + 1]], sizes[i]) for i in range(k)]
    assert ones == want

    def check():
        assert mx.split_outputs(bytes(d_out.cpu().numpy()), k) == want
    return Call(lambda s: mx.msm_batch_device("bn254", d_sc.data_ptr(), d_pt.data_ptr(), offsets, d_out.data_ptr(), s.cuda_stream), check)


def kzg_audit_call(k, seed):
    import torch
    from porla_amd import multiexp as mx
    from tests import test_kzg_audit_batch_gpu as t
    P = t.pipe()
    rnd = random.Random(seed)
    audits = [P.audit(rnd, 5, 3, m, rnd.getrandbits(64)) for m in _pairs(k, seed)]
    d_out = torch.full((t.REC * k,), 0xA5, dtype=torch.uint8, device="cuda")
    d_b = torch.full((32 * t.NCOLS * k,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    want = [t.single_reply(a) for a in audits]

    def check():
        assert bytes(d_out.cpu().numpy()) == b"".join(w[0] for w in want)
        assert bytes(d_b.cpu().numpy()) == b"".join(w[1] for w in want)
    return Call(lambda s: mx.kzg_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr(), stream=s.cuda_stream), check)


def ipa_audit_call(k, seed):
    import torch
    from tests import test_ipa_audit_batch_gpu as t
    P = t.pipe()
    rnd = random.Random(seed)
    audits = [P.audit(rnd, 5, 3, m, rnd.randrange(t.N)) for m in _pairs(k, seed)]
    d_out = torch.full((t.REC * k,), 0xA5, dtype=torch.uint8, device="cuda")
    d_b = torch.full((32 * t.NCOLS * k,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def check():                                    # the single call's points and B, the Python prover's proof, byte for byte
        t.check_records(audits, bytes(d_out.cpu().numpy()), bytes(d_b.cpu().numpy()))
    return Call(lambda s: P.fb.ipa_audit_batch_device(audits, d_out.data_ptr(), d_b.data_ptr(), stream=s.cuda_stream), check)


def ipa_verify_call(k, seed):
    import torch
    from tests import test_ipa_verify_batch_gpu as t
    P = t.pipe()
    rnd = random.Random(seed)
    items = [P.reply(rnd, n) for n in _pairs(k, seed)]
    recs = t._records(t.server_records([it[0] for it in items]), k)
    recs[1] = t._patched(recs[1], 99, bytes([recs[1][99] ^ 1]))                  # c with a flipped bit: the proof fails
    verifs = [it[1] for it in items]
    want = [t.oracle_status(recs[i], verifs[i], items[i][2]) for i in range(k)]
    assert want == [t.BOUND, t.FULL] + [t.BOUND] * (k - 2)
    d_recs = t._dev(b"".join(recs))
    d_status = torch.full((k,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def check():
        assert list(bytes(d_status.cpu().numpy())) == want
    return Call(lambda s: P.fb.ipa_verify_batch_device(verifs, d_recs.data_ptr(), d_status.data_ptr(), stream=s.cuda_stream), check)


def kzg_update_call(k, seed):
    import torch
    from tests import test_update_batch_gpu as t
    S = t.setup_of("bn254")
    rnd = random.Random(seed)
    n_total = 8
    files = [(2, 4), (0, 3), (2, 12), (0, 5), (0, 7)][:k]                         # (level, write_step)
    models = [t.prepared_file(rnd, S, n_total, level, ws) for level, ws in files]
    devs = [t.DevFile(m) for m in models]
    writes = [t.random_write(rnd, S, level, a != 1) for a, (level, ws) in enumerate(files)]
    reqs = [d.req(*w, ws, level) for d, w, (level, ws) in zip(devs, writes, files)]
    torch.cuda.synchronize()

    def check():
        for a, (m, d, w, (level, ws)) in enumerate(zip(models, devs, writes, files)):
            assert m.update(*w) == (ws, level)
            t.assert_families_equal(d.bytes(), m.family_bytes(), "file %d of %d:" % (a, k))
    return Call(lambda s: S.call(reqs, n_total, s.cuda_stream), check)


def kzg_verify_call(k, seed):
    import torch
    from porla_amd import multiexp as mx
    from tests import test_kzg_verify_batch_gpu as t
    P = t.pipe()
    rnd = random.Random(seed)
    items = [P.reply(rnd, n) for n in _pairs(k, seed)]
    recs = t._records(t.server_records([it[0] for it in items]), k)
    recs[1] = t._with_claim(recs[1], 1)                                           # a wrong claim: the proof fails
    verifs = [it[1] for it in items]
    want = [t.reference_status(recs[i], items[i][2]) for i in range(k)]
    assert want == [t.PASS, t.FULL] + [t.PASS] * (k - 2)
    d_recs = t._dev(b"".join(recs))
    torch.cuda.synchronize()
    got = []

    def check():
        assert got == [want]
    return Call(lambda s: got.append(mx.kzg_verify_batch_device(verifs, d_recs.data_ptr(), stream=s.cuda_stream)), check)


CALLS = {"msm_bn254": msm_call, "kzg_audit": kzg_audit_call, "ipa_audit": ipa_audit_call, "ipa_verify": ipa_verify_call,
         "kzg_update": kzg_update_call, "kzg_verify": kzg_verify_call}


@pytest.mark.parametrize("name", list(CALLS))
def test_a_larger_call_on_another_stream_while_the_first_is_in_flight(name):
    import torch
    make = CALLS[name]
    a, b = make(KA, 1), make(KB, 2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ballast = torch.empty(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        for _ in range(4):
            ballast.normal_()                       # a few milliseconds ahead of A on its stream: A is in flight when B comes
    if name == "kzg_verify":                        # blocking: each call from a thread of its own
        errs = []

        def worker(call, s):
            try:
                call.issue(s)
            except Exception as e:                  # noqa: BLE001 -- reported below
                errs.append(e)
        ts = [threading.Thread(target=worker, args=(a, s1)), threading.Thread(target=worker, args=(b, s2))]
        for th in ts:
            th.start()
        for th in ts:
            th.join()
        assert not errs, errs
    else:
        a.issue(s1)
        b.issue(s2)
    torch.cuda.synchronize()
    a.check()
    b.check()

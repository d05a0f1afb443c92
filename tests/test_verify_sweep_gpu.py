"""GPU: every field of an audit reply swept through both batched verifiers (porla_ipa_verify_batch_device,
porla_kzg_verify_batch_device), entry by entry of tests/reply_mutations.py.

A verifier that ignores part of a reply passes every honest reply, so no comparison of honest outputs can see it.  Here one honest
reply of an 8-row challenge is mutated in every way the catalogue lists; a group of mutations goes through ONE verify call with the
honest record first and last, and for EVERY entry, none sampled:
    the mutated bytes differ from the honest ones,
    the status equals the oracle's (tests/ipa_verify_py.status; for KZG the reference's own sequence, reference_status of
    tests/test_kzg_verify_batch_gpu.py, behind the header's well-formedness rule restated on Python integers), and
    the status equals the literal the catalogue wrote beside the mutation, where it gives one.
tests/test_reply_mutations_cpu.py checks the same literals against the oracles on a synthetic reply without a device, and the same
entry counts (reply_mutations.COUNTS).  The pipelines, the server batches and the oracles are those of the two verifiers' own test
modules, imported."""
import random

import pytest

from tests import ipa_proof_py as ipa
from tests import ipa_verify_py as ipv
from tests import reply_mutations as rm
from tests import test_ipa_verify_batch_gpu as iv
from tests import test_kzg_verify_batch_gpu as kv

pytestmark = pytest.mark.gpu

ROWS = 8                       # rows per challenge: the verifier's work per reply does not depend on it beyond the complement entry
ZERO_AT = 11                   # the block whose complement is infinity in the zero-complement stores
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _be32(v):
    return v if isinstance(v, bytes) else int(v).to_bytes(32, "big")


# ================================================================ IPA
def ipa_honest():
    """(audit tuple, verify tuple, (idx, coef)) of one 8-row challenge, and the server batch's record for it"""
    def make():
        P = iv.pipe()
        item = P.reply(random.Random(2101), ROWS)
        rec = iv._records(iv.server_records([item[0]]), 1)[0]
        return item, rec
    return _once("ipa_honest", make)


def ipa_catalogue():
    return _once("ipa_catalogue", lambda: rm.ipa_mutations(ipa_honest()[1]))


def ipa_oracle(rec, verif, challenge, comp_list=None):
    """ipa_verify_py.status, once per distinct (record, request)"""
    P = iv.pipe()
    alpha = int.from_bytes(verif[4], "big") if not isinstance(verif[4], int) else verif[4]
    key = ("ipa", rec, alpha, verif[5], tuple(challenge[0]), tuple(challenge[1]), comp_list is None)
    return _once(key, lambda: ipv.status(P.gens, P.u, rec, comp_list or P.comp_list, challenge[0], challenge[1], alpha, verif[5]))


def test_the_ipa_catalogue_is_whole():
    """the counts the CPU check prints, on the device's own honest record; every name once"""
    cat = ipa_catalogue()
    tally = rm.tally("ipa", cat)
    print("catalogue", tally)
    assert tally == {k: v for k, v in rm.COUNTS.items() if k.startswith("ipa:") and k != "ipa:request"}
    assert len({e[1] for e in cat}) == len(cat)


@pytest.mark.parametrize("group", ["cma", "l", "r", "rounds", "scalars"])
def test_ipa_record_mutations(group):
    (_, verif, chal), rec = ipa_honest()
    entries = [e for e in ipa_catalogue() if e[0] == group]
    assert len(entries) == rm.COUNTS["ipa:" + group]
    recs = [rec] + [e[2] for e in entries] + [rec]
    got = iv.verify_host_records(recs, [verif] * len(recs))
    assert got[0] == got[-1] == ipa_oracle(rec, verif, chal) == iv.BOUND
    asserted = 0
    for (_, name, mutated, expected), status in zip(entries, got[1:-1]):
        want = ipa_oracle(mutated, verif, chal)
        print("%-18s status %2d oracle %2d literal %s" % (name, status, want, expected))
        assert len(mutated) == iv.REC and mutated != rec, name
        assert status == want, name
        if expected is not None:
            assert status == expected, name
        else:
            assert status & (iv.FULL | iv.MALFORMED) == iv.FULL, name            # a proof scalar is no part of the MAC equation
        asserted += 1
    print("asserted", asserted, "entries of ipa:" + group)
    assert asserted == rm.COUNTS["ipa:" + group]


def test_ipa_request_mutations():
    (_, verif, chal), rec = ipa_honest()
    entries = rm.ipa_request_mutations(verif[5])
    fields = dict(alpha=4, a_value=5)
    verifs = [verif]
    for _, override, _ in entries:
        v = list(verif)
        for f, value in override.items():
            v[fields[f]] = value
        assert tuple(v) != verif
        verifs.append(tuple(v))
    verifs.append(verif)
    got = iv.verify_host_records([rec] * len(verifs), verifs)
    assert got[0] == got[-1] == ipa_oracle(rec, verif, chal) == iv.BOUND
    for (name, _, expected), v, status in zip(entries, verifs[1:-1], got[1:-1]):
        want = ipa_oracle(rec, v, chal)
        print("%-14s status %2d oracle %2d literal %2d" % (name, status, want, expected))
        assert status == want == expected, name
    print("asserted", len(entries), "entries of ipa:request")
    assert len(entries) == rm.COUNTS["ipa:request"]


def test_ipa_challenge_shapes():
    """the server batch and the verifier on the same challenge: a zero coefficient, the largest one, one index eight times, a row
    whose complement is infinity (stores of their own: comp[ZERO_AT] = O and M'[ZERO_AT] = alpha M, i.e. the honest entry minus the
    complement) and the empty challenge.  Nothing is mutated: every status is BOUND"""
    import torch
    P = iv.pipe()
    (_, verif, chal), rec = ipa_honest()
    z = ZERO_AT
    comp_list = list(P.comp_list)
    comp_list[z] = ipa.INF64
    mac_z = ipa.msm([(1, P.macs_a[64 * z:64 * z + 64]), (iv.N - 1, P.comp_list[z])])
    d_comp = iv._dev(b"".join(comp_list))
    d_macs = iv._dev(P.macs_a[:64 * z] + mac_z + P.macs_a[64 * z + 64:])
    shapes = rm.challenge_shapes(iv.NBLK, z)
    rnd = random.Random(2102)
    keep, audits, verifs, chals = [], [], [], []
    for name, idx, coef in shapes:
        n = len(idx)
        d_i, d_c = (iv._i64(idx), iv._u32(coef)) if n else (None, None)
        keep.append((d_i, d_c))
        p = lambda t: t.data_ptr() if t is not None else 0
        own = name == "zero_complement"
        v = rnd.randrange(iv.N)
        audits.append((P.d_rows64.data_ptr() if n else 0, p(d_i), p(d_c), n, 0, 0, 0, 0, (d_macs if own else P.d_macs_a).data_ptr(),
                       P.d_zero.data_ptr(), p(d_i), p(d_c), n, v))
        verifs.append(((d_comp if own else P.d_comp).data_ptr() if n else 0, p(d_i), p(d_c), n, iv.ALPHA, v))
        chals.append((idx, coef))
    assert z in chals[3][0] and len(set(chals[2][0])) == 1
    torch.cuda.synchronize()
    recs = iv._records(iv.server_records(audits), len(shapes))
    got = iv.verify_host_records([rec] + recs + [rec], [verif] + verifs + [verif])
    assert got[0] == got[-1] == iv.BOUND
    for (name, _, _), r, v, ch, status in zip(shapes, recs, verifs, chals, got[1:-1]):
        want = ipa_oracle(r, v, ch, comp_list if name == "zero_complement" else None)
        print("%-16s status %2d oracle %2d" % (name, status, want))
        assert status == want == iv.BOUND, name
    print("asserted", len(shapes), "entries of shapes")
    assert len(shapes) == rm.COUNTS["shapes"]


# ================================================================ KZG
def kzg_honest():
    """two replies of 8-row challenges: the one that is mutated, and another whose points replace the first's role by role"""
    def make():
        P = kv.pipe()
        rnd = random.Random(2201)
        items = [P.reply(rnd, ROWS) for _ in range(2)]
        recs = kv._records(kv.server_records([it[0] for it in items]), 2)
        return items[0], recs[0], recs[1]
    return _once("kzg_honest", make)


def kzg_catalogue():
    return _once("kzg_catalogue", lambda: rm.kzg_mutations(*kzg_honest()[1:]))


def g1_well_formed(b):
    """the header's rule on Python integers: both coordinates below p, and on y^2 = x^3 + 3 or 64 zero bytes"""
    x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
    if x >= kv.P_FIELD or y >= kv.P_FIELD:
        return False
    return (x == 0 and y == 0) or (y * y - x * x * x - 3) % kv.P_FIELD == 0


def kzg_oracle(rec, challenge, alpha=kv.ALPHA, comp=None):
    """MALFORMED by the rule above; otherwise the reference's sequence (reference_status; restated here only where the complement
    store is not the pipeline's), once per distinct (record, request)"""
    def make():
        if not all(g1_well_formed(rec[at:at + 64]) for _, at in rm.KZG_POINTS):
            return kv.MALFORMED
        if comp is None:
            return kv.reference_status(rec, challenge, alpha)
        from porla_amd import multiexp as mx
        idx, coef = challenge
        pts = b"".join(comp[64 * i:64 * i + 64] for i in idx)
        csum = mx.bn254_multi_exp(pts, b"".join(mx.bn254_scalar_set_int(c) for c in coef), len(idx))
        a32 = bytes(32 - len(alpha)) + alpha
        left = mx.bn254_add(mx.bn254_mult(rec[0:64], a32), csum)
        right = mx.bn254_add(rec[192:256], mx.bn254_mult(rec[256:320], a32))
        proof = mx.verify_proof(rec[0:64], rec[64:128], rec[128:160], rec[160:192])
        return (kv.FULL if mx.bn254_compare(left, right) else 0) | (kv.PROOF if proof else 0)
    return _once(("kzg", rec, bytes(alpha), tuple(challenge[0]), tuple(challenge[1]), comp is None), make)


def test_the_kzg_catalogue_is_whole():
    cat = kzg_catalogue()
    tally = rm.tally("kzg", cat)
    print("catalogue", tally)
    assert tally == {k: v for k, v in rm.COUNTS.items() if k.startswith("kzg:") and k != "kzg:request"}
    assert len({e[1] for e in cat}) == len(cat)


@pytest.mark.parametrize("group", ["points", "scalars"])
def test_kzg_record_mutations(group):
    (_, verif, chal), rec, _ = kzg_honest()
    entries = [e for e in kzg_catalogue() if e[0] == group]
    assert len(entries) == rm.COUNTS["kzg:" + group]
    recs = [rec] + [e[2] for e in entries] + [rec]
    got = kv.verify_host_records(recs, [verif] * len(recs))
    assert got[0] == got[-1] == kzg_oracle(rec, chal) == kv.PASS
    asserted = 0
    for (_, name, mutated, expected), status in zip(entries, got[1:-1]):
        want = kzg_oracle(mutated, chal)
        print("%-18s status %d oracle %d literal %s" % (name, status, want, expected))
        assert len(mutated) == kv.REC and mutated != rec, name
        assert status == want, name
        if expected is not None:
            assert status == expected, name
        else:
            assert status & (kv.FULL | kv.MALFORMED) == kv.FULL, name            # z and y are no part of the MAC equation
        asserted += 1
    print("asserted", asserted, "entries of kzg:" + group)
    assert asserted == rm.COUNTS["kzg:" + group]
    # the encodings v + r and v + 2 r alone, where the folded check must hold and no fall-back runs
    same = [e for e in entries if e[3] == kv.PASS]
    if group == "scalars":
        assert len(same) == 4
        assert kv.verify_host_records([e[2] for e in same], [verif] * 4) == [kv.PASS] * 4


def test_kzg_request_mutations():
    (_, verif, chal), rec, _ = kzg_honest()
    entries = rm.kzg_request_mutations()
    verifs = [verif] + [verif[:4] + (_be32(o["alpha"]),) for _, o, _ in entries] + [verif]
    got = kv.verify_host_records([rec] * len(verifs), verifs)
    assert got[0] == got[-1] == kzg_oracle(rec, chal) == kv.PASS
    for (name, _, expected), v, status in zip(entries, verifs[1:-1], got[1:-1]):
        want = kzg_oracle(rec, chal, alpha=v[4])
        print("%-10s status %d oracle %d literal %d" % (name, status, want, expected))
        assert bytes(32 - len(verif[4])) + verif[4] != v[4], name
        assert status == want == expected, name
    print("asserted", len(entries), "entries of kzg:request")
    assert len(entries) == rm.COUNTS["kzg:request"]


def test_kzg_challenge_shapes():
    """as test_ipa_challenge_shapes: every status is PASS"""
    import torch
    from porla_amd import multiexp as mx
    P = kv.pipe()
    (_, verif, chal), rec, _ = kzg_honest()
    z = ZERO_AT
    minus_one = (kv.R - 1).to_bytes(32, "big")
    mac_z = mx.bn254_add(P.macs_a[64 * z:64 * z + 64], mx.bn254_mult(P.comp[64 * z:64 * z + 64], minus_one))
    comp = P.comp[:64 * z] + bytes(64) + P.comp[64 * z + 64:]
    d_comp = kv._dev(comp)
    d_macs = kv._dev(P.macs_a[:64 * z] + mac_z + P.macs_a[64 * z + 64:])
    shapes = rm.challenge_shapes(kv.NBLK, z)
    keep, audits, verifs, chals = [], [], [], []
    for k, (name, idx, coef) in enumerate(shapes):
        n = len(idx)
        d_i, d_c = (kv._i64(idx), kv._u32(coef)) if n else (None, None)
        keep.append((d_i, d_c))
        p = lambda t: t.data_ptr() if t is not None else 0
        own = name == "zero_complement"
        audits.append((P.d_rows64.data_ptr() if n else 0, p(d_i), p(d_c), n, 0, 0, 0, 0, (d_macs if own else P.d_macs_a).data_ptr(),
                       P.d_zero.data_ptr(), p(d_i), p(d_c), n, 0x1234567 + k))
        verifs.append(((d_comp if own else P.d_comp).data_ptr(), p(d_i), p(d_c), n, kv.ALPHA))
        chals.append((idx, coef))
    assert z in chals[3][0] and len(set(chals[2][0])) == 1
    torch.cuda.synchronize()
    recs = kv._records(kv.server_records(audits), len(shapes))
    got = kv.verify_host_records([rec] + recs + [rec], [verif] + verifs + [verif])
    assert got[0] == got[-1] == kv.PASS
    for (name, _, _), r, ch, status in zip(shapes, recs, chals, got[1:-1]):
        want = kzg_oracle(r, ch, comp=comp if name == "zero_complement" else None)
        print("%-16s status %d oracle %d" % (name, status, want))
        assert status == want == kv.PASS, name
    print("asserted", len(shapes), "entries of shapes")
    assert len(shapes) == rm.COUNTS["shapes"]


def _z_plus(rec, delta):
    z = (int.from_bytes(rec[rm.KZG_Z_AT:rm.KZG_Z_AT + 32], "big") + delta) % kv.R
    return rec[:rm.KZG_Z_AT] + z.to_bytes(32, "big") + rec[rm.KZG_Z_AT + 32:]


def kzg_sixteen():
    def make():
        P = kv.pipe()
        rnd = random.Random(2202)
        items = [P.reply(rnd, ROWS) for _ in range(16)]
        return items, kv._records(kv.server_records([it[0] for it in items]), 16)
    return _once("kzg_sixteen", make)


@pytest.mark.parametrize("where", [(0,), (15,), (0, 15), tuple(range(16))], ids=["first", "last", "first_and_last", "all"])
def test_the_fallback_wherever_the_bad_opening_stands(where):
    """the per-reply fall-back behind a failed folded check, with z + 1 in the first reply, the last, both, and all sixteen"""
    items, honest = kzg_sixteen()
    recs = [_z_plus(r, 1) if i in where else r for i, r in enumerate(honest)]
    got = kv.verify_host_records(recs, [it[1] for it in items])
    want = [kzg_oracle(recs[i], items[i][2]) for i in range(16)]
    assert got == want
    assert want == [kv.FULL if i in where else kv.PASS for i in range(16)]


def test_the_fallback_on_a_batch_of_one():
    items, honest = kzg_sixteen()
    bad = _z_plus(honest[5], 1)
    assert kv.verify_host_records([honest[5]], [items[5][1]]) == [kzg_oracle(honest[5], items[5][2])] == [kv.PASS]
    assert kv.verify_host_records([bad], [items[5][1]]) == [kzg_oracle(bad, items[5][2])] == [kv.FULL]


def test_cancelling_errors_on_z_are_caught_by_random_weights():
    """one honest record twice, so both replies carry the same H, with z + d and z - d: under equal weights w the folded
    P = sum w (C - y G + z_k H) is 2 w (C - y G) + w (z + d + z - d) H, the honest reply's twice over, and Q is untouched, so the
    construction cancels; drawn weights (per call) and random weights of the test's own catch both"""
    items, honest = kzg_sixteen()
    rnd = random.Random(2203)
    d = rnd.randrange(1, kv.R)
    recs = [_z_plus(honest[3], d), _z_plus(honest[3], -d)]
    verifs = [items[3][1]] * 2
    want = [kzg_oracle(r, items[3][2]) for r in recs]
    assert want == [kv.FULL, kv.FULL]
    assert kv.verify_host_records(recs, verifs, weights=[12345] * 2) == [kv.PASS] * 2     # the construction cancels
    for _ in range(2):
        assert kv.verify_host_records(recs, verifs) == want
    assert kv.verify_host_records(recs, verifs, weights=[rnd.getrandbits(128) | 1 for _ in range(2)]) == want

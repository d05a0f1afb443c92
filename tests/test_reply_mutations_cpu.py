"""CPU: the catalogue of reply mutations (tests/reply_mutations.py) against the oracles, on synthetic honest replies built without a
device -- what keeps the device sweep (tests/test_verify_sweep_gpu.py) from being vacuous: every mutation changes the bytes, every
literal status is what the oracle computes, no two names collide, and the entry counts are reply_mutations.COUNTS, which the sweep
asserts again (run with -s to see them).

IPA: the reply of tests/test_ipa_verify_batch_cpu.py's synthetic test, with a finite A (M = alpha C + sum coef comp - alpha A), and
ipa_verify_py.status.  KZG: an opening from oracle/bn254_py.KZG over an SRS of 4; FULL on bn254_py's point arithmetic, PROOF on the
Python pairing (oracle/bn254_pairing_py), MALFORMED by the header's rule on integers."""
import random
import time

from tests import common
from tests import ipa_proof_py as ipa
from tests import ipa_verify_py as ipv
from tests import reply_mutations as rm

import bn254_py as bn


def test_the_literals_are_the_headers_and_the_oracles():
    import os
    import re
    header = open(os.path.join(common.ROOT, "include", "porla_gpu.h")).read()
    for name in ("FULL", "PROOF", "MALFORMED", "BVEC"):
        assert int(re.search(r"#define PORLA_IPA_VERIFY_%s\s+(\d+)" % name, header).group(1)) == getattr(rm, "IPA_" + name) == getattr(ipv, name)
    for name in ("FULL", "PROOF", "MALFORMED"):
        assert int(re.search(r"#define PORLA_KZG_VERIFY_%s\s+(\d+)" % name, header).group(1)) == getattr(rm, "KZG_" + name)
    assert (rm.SECP_P, rm.SECP_N, rm.BN_P, rm.BN_R) == (ipa.P, ipa.N, bn.P, bn.R)
    assert rm.IPA_REC == ipv.REC and rm.IPA_BOUND == ipv.BOUND
    assert [rec_at for _, rec_at in rm.ipa_point_offsets()] == [33 * i for i in range(3)] + [99 + 32 + 33 * i for i in range(12)]
    # the generators and their small multiples are on their curves
    for m in range(1, 20):
        x, y = rm.small_multiple(rm.SECP_P, rm.SECP_G, m)
        assert (y * y - x ** 3 - 7) % rm.SECP_P == 0 and ipv.parses(rm.secp_compressed((x, y)))
        assert bn.is_on_curve(rm.small_multiple(rm.BN_P, rm.BN_G, m)) and rm.small_multiple(rm.BN_P, rm.BN_G, m) == bn.g1_mul(bn.G1, m)


# ================================================================ IPA
class IpaReply:
    """one honest reply on integers: C = Commit(a), a finite A, M = alpha C + sum coef comp[idx] - alpha A, the restated prover"""

    def __init__(self):
        pts = ipa.split_points(common.secp_bench_points(ipa.NUM_CHUNKS + 1), ipa.NUM_CHUNKS + 1)
        self.gens, self.u = pts[:ipa.NUM_CHUNKS], pts[ipa.NUM_CHUNKS]
        rnd = random.Random(3101)
        self.a = [rnd.randrange(ipa.N) for _ in range(ipa.NUM_CHUNKS)]
        self.v, self.alpha = rnd.randrange(1, ipa.N - 1), rnd.getrandbits(128)
        self.comp = [ipa.msm([(rnd.randrange(1, ipa.N), self.u)]) for _ in range(16)]
        self.c_pt = ipa.msm(list(zip(self.a, self.gens)))
        self.a_pt = ipa.msm([(rnd.randrange(1, ipa.N), self.u)])
        self.proof = ipa.prove(self.gens, self.u, self.a, ipa.audit_b(self.v))
        self.idx, self.coef = [rnd.randrange(16) for _ in range(8)], [rnd.getrandbits(31) for _ in range(8)]
        self.rec = self.record(self.idx, self.coef, self.comp)

    def record(self, idx, coef, comp):
        m_pt = ipa.msm([(self.alpha, self.c_pt), (ipa.N - self.alpha, self.a_pt)] + [(cf, comp[i]) for i, cf in zip(idx, coef)])
        return ipa.compress(self.c_pt) + ipa.compress(m_pt) + ipa.compress(self.a_pt) + self.proof

    def status(self, rec, alpha=None, a_value=None, idx=None, coef=None, comp=None):
        return ipv.status(self.gens, self.u, rec, comp or self.comp, self.idx if idx is None else idx, self.coef if coef is None else coef,
                          self.alpha if alpha is None else alpha, self.v if a_value is None else a_value)


_IPA = None


def ipa_reply():
    global _IPA
    if _IPA is None:
        _IPA = IpaReply()
    return _IPA


def test_the_whole_ipa_catalogue_against_the_oracle():
    """all 169 record mutations: the bytes change, the names are distinct, ipa_verify_py.status gives the literal; where the
    catalogue leaves the literal open (a proof scalar set to 0, n, n + 1, 2^256 - 1) the status keeps FULL and is not MALFORMED"""
    R = ipa_reply()
    assert R.status(R.rec) == ipv.BOUND
    cat = rm.ipa_mutations(R.rec)
    tally = rm.tally("ipa", cat)
    print("catalogue", tally)
    assert tally == {k: v for k, v in rm.COUNTS.items() if k.startswith("ipa:") and k != "ipa:request"}
    assert len({name for _, name, _, _ in cat}) == len(cat) == 169
    assert len({mutated for _, _, mutated, _ in cat}) == len(cat)
    open_literals = 0
    for _, name, mutated, expected in cat:
        assert len(mutated) == ipv.REC and mutated != R.rec, name
        got = R.status(mutated)
        if expected is None:
            open_literals += 1
            assert got & (ipv.FULL | ipv.MALFORMED) == ipv.FULL, name
        else:
            assert got == expected, (name, got, expected)
    assert open_literals == 20
    # the reduced encodings are the same residue to the oracle: n is 0 and n + 1 is 1
    by_name = {name: mutated for _, name, mutated, _ in cat}
    for s in ("c", "a0", "b0", "a1", "b1"):
        if s != "c":                         # c is hashed as bytes, so its encodings give different challenges
            assert R.status(by_name[s + ":n"]) == R.status(by_name[s + ":0"])


def test_the_ipa_request_mutations_against_the_oracle():
    R = ipa_reply()
    entries = rm.ipa_request_mutations(R.v)
    print("catalogue", {"ipa:request": len(entries)})
    assert len(entries) == rm.COUNTS["ipa:request"] and len({e[0] for e in entries}) == len(entries)
    for name, override, expected in entries:
        assert override.get("alpha", R.alpha) % ipa.N != R.alpha or override.get("a_value", R.v) % ipa.N != R.v, name
        assert R.status(R.rec, **override) == expected, name


def test_the_challenge_shapes_leave_an_honest_ipa_reply_honest():
    R = ipa_reply()
    shapes = rm.challenge_shapes(16, 5)
    print("catalogue", {"shapes": len(shapes)})
    assert len(shapes) == rm.COUNTS["shapes"] and len({s[0] for s in shapes}) == len(shapes)
    comp0 = list(R.comp)
    comp0[5] = ipa.INF64
    for name, idx, coef in shapes:
        comp = comp0 if name == "zero_complement" else R.comp
        assert len(idx) == len(coef) and all(0 <= i < 16 for i in idx) and all(0 <= c < 2 ** 31 for c in coef), name
        rec = R.record(idx, coef, comp)
        assert R.status(rec, idx=idx, coef=coef, comp=comp) == ipv.BOUND, name
    d = {s[0]: s for s in shapes}
    assert d["n1_coef0"][2] == [0] and d["n1_coef_max"][2] == [2 ** 31 - 1] and d["n0"][1] == []
    assert len(set(d["all_idx_equal"][1])) == 1 and len(d["all_idx_equal"][1]) == 8
    assert 5 in d["zero_complement"][1] and len(d["zero_complement"][1]) == 8


# ================================================================ KZG
TAU = bytes.fromhex("ffeeddccbbaa99887766554433221100")
ALPHA = bytes.fromhex("00112233445566778899aabbccddeeff")


class KzgReply:
    """two honest replies over an SRS of 4 (C, H, z, y from create_proof), finite A = t G, M = alpha C + sum coef comp - alpha A"""

    def __init__(self):
        self.kzg = bn.KZG()
        self.kzg.init_key(TAU, ALPHA)
        self.kzg.init_srs(4, h_scalar=0x5eed)
        rnd = random.Random(3201)
        self.alpha = int.from_bytes(ALPHA, "big")
        self.comp = [bn.g1_mul(self.kzg.h_mac, rnd.randrange(1, bn.R)) for _ in range(16)]
        self.idx, self.coef = [rnd.randrange(16) for _ in range(8)], [rnd.getrandbits(31) for _ in range(8)]
        self.recs = [self.record(rnd) for _ in range(2)]
        self.pairings, self.seconds = {}, 0.0

    def record(self, rnd):
        data = b"".join(rnd.randrange(bn.R).to_bytes(32, "big") for _ in range(4))
        c, h, z, y = self.kzg.create_proof(rnd.getrandbits(64), data)
        a_pt = bn.g1_mul(bn.G1, rnd.randrange(1, bn.R))
        m_pt = bn.g1_add(bn.g1_mul(bn.g1_unmarshal(c), self.alpha), bn.g1_neg(bn.g1_mul(a_pt, self.alpha)))
        for i, cf in zip(self.idx, self.coef):
            m_pt = bn.g1_add(m_pt, bn.g1_mul(self.comp[i], cf))
        return c + h + z + y + bn.g1_marshal(m_pt) + bn.g1_marshal(a_pt)

    @staticmethod
    def well_formed(b):
        x, y = int.from_bytes(b[:32], "big"), int.from_bytes(b[32:], "big")
        return x < bn.P and y < bn.P and ((x == 0 and y == 0) or bn.is_on_curve((x, y)))

    def proof(self, rec):
        """kzg.Verify on the Python pairing, once per distinct (C, H, z, y)"""
        key = rec[:192]
        if key not in self.pairings:
            t = time.time()
            self.pairings[key] = self.kzg.verify_proof_with_pairing(rec[0:64], rec[64:128], rec[128:160], rec[160:192])
            self.seconds += time.time() - t
        return self.pairings[key]

    def status(self, rec, alpha=None):
        if not all(self.well_formed(rec[at:at + 64]) for _, at in rm.KZG_POINTS):
            return rm.KZG_MALFORMED
        alpha = self.alpha if alpha is None else alpha % bn.R
        c, m, a = (bn.g1_unmarshal(rec[at:at + 64]) for at in (0, 192, 256))
        left = bn.g1_mul(c, alpha)
        for i, cf in zip(self.idx, self.coef):
            left = bn.g1_add(left, bn.g1_mul(self.comp[i], cf))
        full = left == bn.g1_add(m, bn.g1_mul(a, alpha))
        return (rm.KZG_FULL if full else 0) | (rm.KZG_PROOF if self.proof(rec) else 0)


def test_the_whole_kzg_catalogue_against_the_pairing_oracle():
    """all 41 record mutations and the 4 of alpha.  One Python pairing check takes 0.65 s here; the catalogue has 17 entries with
    a well-formed (C, H, z, y) of their own (3 each for C and H, 11 for z and y: the malformed ones, and M and A, need none), so with
    the honest record the whole catalogue costs 18 pairing checks, about 12 s, below the 17 s of this suite's slowest test
    (test_ecmult_chain_expected_point): ALL of it runs here, nothing is left to the device sweep alone.  The MAC side (M, A, alpha)
    is bn254_py point arithmetic alone"""
    K = KzgReply()
    rec, other = K.recs
    assert K.status(rec) == rm.KZG_PASS
    for r in (rec, other):
        assert K.kzg.verify_proof_with_tau(r[0:64], r[64:128], r[128:160], r[160:192])
    cat = rm.kzg_mutations(rec, other)
    tally = rm.tally("kzg", cat)
    tally["kzg:request"] = len(rm.kzg_request_mutations())
    print("catalogue", tally)
    assert tally == {k: v for k, v in rm.COUNTS.items() if k.startswith("kzg:")}
    assert len({name for _, name, _, _ in cat}) == len(cat) == 41
    assert len({mutated for _, _, mutated, _ in cat}) == len(cat)
    open_literals = 0
    for _, name, mutated, expected in cat:
        assert len(mutated) == rm.KZG_REC and mutated != rec, name
        got = K.status(mutated)
        if expected is None:
            open_literals += 1
            assert got & (rm.KZG_FULL | rm.KZG_MALFORMED) == rm.KZG_FULL, name
        else:
            assert got == expected, (name, got, expected)
    assert open_literals == 2
    print("pairing checks", len(K.pairings), "in %.1f s" % K.seconds)
    assert len(K.pairings) == 18            # the honest record and 17 mutations
    for name, override, expected in rm.kzg_request_mutations():
        assert override["alpha"] % bn.R != K.alpha, name
        assert K.status(rec, alpha=override["alpha"]) == expected, name

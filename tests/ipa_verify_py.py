"""The oracle of the batched IPA verifier (porla_ipa_verify_batch_device) on Python integers: the four status bits of one reply.

  PROOF      tests/ipa_proof_py.verify, the restated Client::inner_product_verify (Client.hpp:1465-1633)
  FULL       alpha C + sum_j coef_j comp[idx_j] == M + alpha A as two MSMs through the C oracle (Client.hpp:801-829)
  BVEC       b_i == sum_(j = i mod 2) v^(2^j) x_values[j] (mod n), i = 0, 1, with x_values replayed as the verifier updates them
  MALFORMED  secp256k1_eckey_pubkey_parse's rules on the record's 3 + 12 compressed points (33 zero bytes = infinity is well-formed)

A record is 655 bytes: commitment(33) | combined_MAC(33) | combined_align(33) | proof(556)."""
from tests import ipa_proof_py as ipa

N, P = ipa.N, ipa.P
FULL, PROOF, MALFORMED, BVEC = 1, 2, 4, 8
PASS = FULL | PROOF
BOUND = PASS | BVEC
REC = 99 + ipa.PROOF_BYTES


def parses(c):
    """secp256k1_eckey_pubkey_parse on 33 bytes: first byte 2 or 3, X < p, X^3 + 7 a square; or this library's infinity"""
    c = bytes(c)
    if len(c) != 33:
        return False
    if c == ipa.INF33:
        return True
    if c[0] not in (2, 3):
        return False
    x = int.from_bytes(c[1:], "big")
    if x >= P:
        return False
    rhs = (x * x * x + 7) % P
    return pow(rhs, (P - 1) // 2, P) == 1 or rhs == 0


def record_points(rec):
    """the fifteen compressed points of a record: C, M, A, then L_0, R_0, ..., L_5, R_5"""
    return [rec[33 * i:33 * i + 33] for i in range(3)] + [rec[99 + 32 + 33 * i:99 + 32 + 33 * i + 33] for i in range(12)]


def challenges(proof):
    """x_0 .. x_5 of the transcript over the proof's own bytes"""
    sha = ipa.Transcript()
    sha.write(ipa.TAG)
    sha.write(proof[:32])
    h = sha.finalize()
    out = []
    for r in range(6):
        out.append(ipa.challenge(h))
        sha.write(proof[32 + 66 * r:65 + 66 * r])
        sha.finalize()
        sha.write(proof[65 + 66 * r:98 + 66 * r])
        h = sha.finalize()
    return out


def x_values(xs):
    """the verifier's array after the six rounds, updated block by block as Client::inner_product_verify does"""
    xv = [1] * ipa.NUM_CHUNKS
    half, k = ipa.NUM_CHUNKS // 2, 1
    for x in xs:
        inv_x = ipa.inv(x)
        for i in range(k):
            p = (i << 1) + 1
            for j in range(p * half, (p + 1) * half):
                xv[j] = xv[j] * x % N
        for i in range(k):
            p = i << 1
            for j in range(p * half, (p + 1) * half):
                xv[j] = xv[j] * inv_x % N
        half >>= 1
        k <<= 1
    return xv


def bvec(proof, a_value):
    """the proof's b0, b1 are the fold of b = audit_b(a_value)"""
    xv = x_values(challenges(proof))
    b = ipa.audit_b(int(a_value) % N)
    tail = proof[32 + 6 * 66:]
    b0 = int.from_bytes(tail[32:64], "little") % N
    b1 = int.from_bytes(tail[96:128], "little") % N
    return (b0 == sum(b[j] * xv[j] for j in range(0, ipa.NUM_CHUNKS, 2)) % N and
            b1 == sum(b[j] * xv[j] for j in range(1, ipa.NUM_CHUNKS, 2)) % N)


def full(rec, comp, idx, coef, alpha):
    """comp: the complement store as a list of 64-byte points; idx, coef: the challenge"""
    c, m, a = (ipa.decompress(rec[33 * i:33 * i + 33]) for i in range(3))
    alpha = int(alpha) % N
    left = ipa.msm([(alpha, c)] + [(cf, comp[i]) for i, cf in zip(idx, coef)])
    right = ipa.msm([(1, m), (alpha, a)])
    return left == right


def status(gens, u, rec, comp, idx, coef, alpha, a_value):
    """the status byte porla_ipa_verify_batch_device must write for this reply"""
    rec = bytes(rec)
    assert len(rec) == REC
    if not all(parses(c) for c in record_points(rec)):
        return MALFORMED
    s = 0
    if full(rec, comp, idx, coef, alpha):
        s |= FULL
    if ipa.verify(gens, u, ipa.decompress(rec[:33]), rec[99:]):
        s |= PROOF
    if bvec(rec[99:], a_value):
        s |= BVEC
    return s

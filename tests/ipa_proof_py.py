"""The IPA build's inner-product proof restated on Python integers, loop for loop from the reference's text: the oracle of the batched
IPA audit (porla_ipa_audit_batch_device, porla_ipa_prove_batch_device).

  Transcript      the reference's one secp256k1_sha256 object (porla/Utils/secp256k1_lib/hash_impl.h:37-165), written to again after
                  every finalize: finalize pads, emits the state and ZEROES the eight state words while the byte counter runs on.
                  hashlib cannot express that, hence the compression function below with a settable state and length.
  prove           Server::inner_product_prove, porla/Server/Server.hpp:2279-2452
  verify          Client::inner_product_verify, porla/Client/Client.hpp:1465-1633
  audit_b         the b vector of Server::audit, Server.hpp:859-867: repeated squaring of audit_values[n_points]

Points are 64 bytes X || Y big-endian (64 zero bytes = infinity); curve sums go through the C oracle's secp256k1 MSM
(tests/common.py:oracle_secp_msm).  Infinity, which the reference cannot serialise, is 33 zero bytes in a proof -- the engine's
documented form -- and is hashed as those 33 bytes."""
from tests import common

N = common.SECP_N
P = 2 ** 256 - 2 ** 32 - 977
NUM_CHUNKS = 128
TAG = b"hash of P, c, etc. all that jazz"
PROOF_BYTES = 32 + 6 * 66 + 128
INF64, INF33 = bytes(64), bytes(33)

_K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_M = 0xffffffff


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & _M


def sha256_transform(s, chunk):
    """secp256k1_sha256_transform: one compression of the 64-byte chunk into the state s (list of eight words), in place"""
    w = [int.from_bytes(chunk[4 * i:4 * i + 4], "big") for i in range(16)]
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & _M)
    a, b, c, d, e, f, g, h = s
    for t in range(64):
        t1 = (h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & _M & g)) + _K[t] + w[t]) & _M
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & _M
        a, b, c, d, e, f, g, h = (t1 + t2) & _M, a, b, c, (d + t1) & _M, e, f, g
    for i, v in enumerate((a, b, c, d, e, f, g, h)):
        s[i] = (s[i] + v) & _M


class Transcript:
    """secp256k1_sha256 with the reference's initialize / write / finalize (hash_impl.h:37-47, :132-165)"""

    def __init__(self):
        self.s = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
        self.buf = b""
        self.bytes = 0

    def write(self, data):
        self.bytes += len(data)
        self.buf += bytes(data)
        while len(self.buf) >= 64:
            sha256_transform(self.s, self.buf[:64])
            self.buf = self.buf[64:]

    def finalize(self):
        sizedesc = (self.bytes << 3).to_bytes(8, "big")
        self.write(b"\x80" + bytes((119 - (self.bytes % 64)) % 64))
        self.write(sizedesc)
        out = b"".join(v.to_bytes(4, "big") for v in self.s)
        self.s = [0] * 8                      # hash_impl.h:162 -- the object is used again afterwards
        return out


def le32(v):
    """convert_ZZ_to_arr (utils.h:353-364): eight little-endian 32-bit words from the low word up"""
    return int(v).to_bytes(32, "little")


def challenge(h):
    """convert_arr_to_ZZ_p (utils.h:384-393): the hash as eight little-endian words, low word first, mod n"""
    return int.from_bytes(h, "little") % N


def inv(x):
    return pow(x, N - 2, N)                   # (NTL::inv raises on 0; probability 2^-256)


def compress(pt):
    """secp256k1_eckey_pubkey_serialize, compressed; infinity as 33 zero bytes"""
    if pt == INF64:
        return INF33
    return bytes([2 | (pt[63] & 1)]) + pt[:32]


def decompress(c):
    if c == INF33:
        return INF64
    if len(c) != 33 or c[0] not in (2, 3):
        raise ValueError("not a compressed point")
    x = int.from_bytes(c[1:], "big")
    y = pow((x * x * x + 7) % P, (P + 1) // 4, P)
    if x >= P or (y * y - x * x * x - 7) % P:
        raise ValueError("not on the curve")
    if (y & 1) != (c[0] & 1):
        y = P - y
    return c[1:] + y.to_bytes(32, "big")


def msm(terms):
    """sum of scalar * point over (scalar, 64-byte point) pairs; zero scalars and infinities dropped"""
    terms = [(s % N, p) for s, p in terms if s % N and p != INF64]
    if not terms:
        return INF64
    return common.oracle_secp_msm(b"".join(s.to_bytes(32, "big") for s, _ in terms), b"".join(p for _, p in terms), len(terms))


def audit_b(a_value):
    """Server.hpp:859-867: A[i] = A_value; A_value = A_value^2 mod n"""
    out, v = [], a_value % N
    for _ in range(NUM_CHUNKS):
        out.append(v)
        v = v * v % N
    return out


def prove(gens, u, a, b):
    """Server::inner_product_prove: gens = 128 points of 64 bytes, u one; a, b lists of 128 integers -> the 556-byte proof"""
    a, b = [v % N for v in a], [v % N for v in b]
    inner = sum(x * y for x, y in zip(a, b)) % N
    proof = le32(inner)
    x_values = [1] * NUM_CHUNKS
    sha = Transcript()
    sha.write(TAG)
    sha.write(proof[:32])
    random_str = sha.finalize()
    half, k = NUM_CHUNKS // 2, 1
    while half > 1:
        x = challenge(random_str)
        inv_x = inv(x)
        cl = sum(a[i] * b[half + i] for i in range(half)) % N
        cr = sum(a[half + i] * b[i] for i in range(half)) % N
        terms = []
        for i in range(k):
            pos = (i << 1) + 1
            for q, j in enumerate(range(pos * half, (pos + 1) * half)):
                terms.append((a[q] * x_values[j] % N, gens[j]))
                x_values[j] = x_values[j] * x % N
        ser = compress(msm(terms + [(cl, u)]))
        proof += ser
        sha.write(ser)
        random_str = sha.finalize()
        terms = []
        for i in range(k):
            pos = i << 1
            for q, j in enumerate(range(pos * half, (pos + 1) * half)):
                terms.append((a[half + q] * x_values[j] % N, gens[j]))
                x_values[j] = x_values[j] * inv_x % N
        ser = compress(msm(terms + [(cr, u)]))
        proof += ser
        sha.write(ser)
        random_str = sha.finalize()
        a = [(a[i] * x + a[i + half] * inv_x) % N for i in range(half)]
        b = [(b[i] * inv_x + b[i + half] * x) % N for i in range(half)]
        half >>= 1
        k <<= 1
    for i in range(2):
        proof += le32(a[i]) + le32(b[i])
    assert len(proof) == PROOF_BYTES
    return proof


def verify(gens, u, commitment, proof):
    """Client::inner_product_verify: commitment = the 64-byte Commit(a) -> True where the reference's ge_equals_ge holds"""
    if len(proof) != PROOF_BYTES:
        return False
    c = int.from_bytes(proof[:32], "little")
    left = [(1, commitment), (c, u)]
    pos = 32
    x_values = [1] * NUM_CHUNKS
    sha = Transcript()
    sha.write(TAG)
    sha.write(proof[:32])
    random_str = sha.finalize()
    half, k = NUM_CHUNKS // 2, 1
    while half > 1:
        x = challenge(random_str)
        inv_x = inv(x)
        for i in range(k):
            p = (i << 1) + 1
            for j in range(p * half, (p + 1) * half):
                x_values[j] = x_values[j] * x % N
        for i in range(k):
            p = i << 1
            for j in range(p * half, (p + 1) * half):
                x_values[j] = x_values[j] * inv_x % N
        x2 = x * x % N
        inv_x2 = inv(x2)
        try:
            big_l = decompress(proof[pos:pos + 33])
            big_r = decompress(proof[pos + 33:pos + 66])
        except ValueError:
            return False
        sha.write(proof[pos:pos + 33])
        random_str = sha.finalize()
        sha.write(proof[pos + 33:pos + 66])
        random_str = sha.finalize()
        pos += 66
        left += [(x2, big_l), (inv_x2, big_r)]
        half >>= 1
        k <<= 1
    ab, a2, b2 = 0, [], []
    for i in range(2):
        a2.append(int.from_bytes(proof[pos:pos + 32], "little"))
        b2.append(int.from_bytes(proof[pos + 32:pos + 64], "little"))
        ab += a2[i] * b2[i]
        pos += 64
    right = [(ab % N, u)]
    for i in range(NUM_CHUNKS >> 1):
        right.append((a2[0] * x_values[i << 1] % N, gens[i << 1]))
    for i in range(NUM_CHUNKS >> 1):
        right.append((a2[1] * x_values[(i << 1) + 1] % N, gens[(i << 1) + 1]))
    return msm(left) == msm(right)


def split_points(raw, n):
    return [raw[64 * i:64 * i + 64] for i in range(n)]

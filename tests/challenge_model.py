"""Pure-Python model of the seed-in entry points (include/porla_gpu.h: porla_mac_prf_*, porla_client_prf_runs,
porla_audit_challenge_*, porla_audit_complement_scalar_*), written from FIPS-197 and the reference's lines, independently of the C++:
AES-128 on byte lists, the PRG's int stream (porla/Utils/prg.h:44-50, 84-97), the MAC PRF (Client.hpp:423-443), the audit walk
(Server.hpp:604-732, Client.hpp:687-744), the d_prf orders of the client writes (Client.hpp:467-534, 585-588), the complement scalar."""
import struct

SECRET_KEY = bytes.fromhex("00112233445566778899aabbccddeeff")   # config.hpp:38
N_SECP256K1 = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
NUM_CHECK_AUDIT = 128


# ---- AES-128, FIPS-197, bytes in the order of the standard (state column c = bytes 4c .. 4c+3)
def _xtime(a):
    a <<= 1
    return (a ^ 0x11b) & 0xff if a & 0x100 else a


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = _xtime(a)
        b >>= 1
    return r


def _make_sbox():
    box = []
    for x in range(256):
        inv = 0
        if x:
            inv = next(y for y in range(1, 256) if _gmul(x, y) == 1)
        s = inv
        for i in range(1, 5):
            s ^= ((inv << i) | (inv >> (8 - i))) & 0xff
        box.append(s ^ 0x63)
    return box


SBOX = _make_sbox()


def aes128_round_keys(key):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = t[1:] + t[:1]
            t = [SBOX[b] for b in t]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]


def aes128_encrypt_rk(rks, block):
    s = [b ^ k for b, k in zip(block, rks[0])]
    for r in range(1, 11):
        s = [SBOX[b] for b in s]
        s = [s[4 * ((c + row) % 4) + row] for c in range(4) for row in range(4)]      # ShiftRows
        if r < 10:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_xtime(a[0]) ^ _xtime(a[1]) ^ a[1] ^ a[2] ^ a[3],
                      a[0] ^ _xtime(a[1]) ^ _xtime(a[2]) ^ a[2] ^ a[3],
                      a[0] ^ a[1] ^ _xtime(a[2]) ^ _xtime(a[3]) ^ a[3],
                      _xtime(a[0]) ^ a[0] ^ a[1] ^ a[2] ^ _xtime(a[3])]
            s = m
        s = [b ^ k for b, k in zip(s, rks[r])]
    return bytes(s)


def aes128_encrypt(key, block):
    return aes128_encrypt_rk(aes128_round_keys(bytes(key)), bytes(block))


# ---- the PRG's int stream and the MAC PRF
class PrgInts:
    """int t of PRG::reseed(seed, 0): the little-endian int32 at byte 4t of the blocks AES(seed, counter as u64 LE | 0)"""

    def __init__(self, seed):
        self.rks = aes128_round_keys(bytes(seed))
        self.blocks = {}

    def __getitem__(self, t):
        c = t // 4
        if c not in self.blocks:
            self.blocks[c] = aes128_encrypt_rk(self.rks, struct.pack("<QQ", c, 0))
        return struct.unpack_from("<i", self.blocks[c], 4 * (t % 4))[0]


def _wrap32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def _wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


_PRF_RKS = {}


def mac_prf(key, level, index, time):
    key = bytes(key)
    if key not in _PRF_RKS:
        _PRF_RKS[key] = aes128_round_keys(key)
    return aes128_encrypt_rk(_PRF_RKS[key], struct.pack("<iiq", _wrap32(level), _wrap32(index), _wrap64(time)))


def expand_runs(runs):
    """the triples (level, index, time) of a run list"""
    return [(level, _wrap32(index0 + t), _wrap64(time0 + t * stride)) for level, index0, count, time0, stride in runs for t in range(count)]


def mag(v):
    """|v| as a uint32, mag(INT32_MIN) = 2^31"""
    return -v if v < 0 else v


# ---- the walk
def walk(s, write_step, num_blocks):
    """points (level, index, coef) in order and the position behind the last int consumed"""
    height = num_blocks.bit_length()
    ws = write_step % num_blocks
    pos, pts = 0, []
    for i in range(height):
        l = 1 << i
        if not ((ws >> i) & 1 or i == height - 1):
            continue
        if 2 * l > NUM_CHECK_AUDIT:
            for j in range(NUM_CHECK_AUDIT):
                pts.append((i, mag(s[pos + j]) % (2 * l), mag(s[pos + NUM_CHECK_AUDIT + j])))
            pos += 2 * NUM_CHECK_AUDIT
        else:
            for j in range(2 * l):
                pts.append((i, j, mag(s[pos + j])))
            pos += 2 * l
    return pts, pos


def challenge(s, write_step, num_blocks, levels):
    """(info, lists) of a challenge over the int stream s; levels: tuples (data_x, data_y, mac_x, mac_y, form)"""
    pts, pos = walk(s, write_step, num_blocks)
    L = dict(idx64=[], coef64=[], idx32=[], coef32=[], mac_idx=[], mac_coef=[])
    for i, index, coef in pts:
        dx, dy, mx, my, form = levels[i][:5]
        l = 1 << i
        y, row = index >= l, index - l if index >= l else index
        L["mac_idx"].append((my if y else mx) + row)
        L["mac_coef"].append(coef)
        L["idx32" if form else "idx64"].append((dy if y else dx) + row)
        L["coef32" if form else "coef64"].append(coef)
    a = s[len(pts)]
    info = dict(n64=len(L["idx64"]), n32=len(L["idx32"]), n_macs=len(pts), random_point=s[pos] & ((1 << 64) - 1), a_raw=a,
                a_value=(a % N_SECP256K1).to_bytes(32, "big"))
    return info, L


def complement_triples(s, write_step, num_blocks):
    """(coef, (level, index, time)) of the client's complements of a challenge: the FULL write_step, low i bits cleared"""
    pts, _ = walk(s, write_step, num_blocks)
    return [(coef, (i, index, write_step & ~((1 << i) - 1))) for i, index, coef in pts]


def prf_value(raw, curve):
    """a PRF output as the write batches read it: KZG a big-endian 128-bit integer, IPA r.d[0], r.d[1]: a little-endian one"""
    return int.from_bytes(raw, "big" if curve == "bn254" else "little")


def complement_scalar(key, seed, write_step, num_blocks, curve):
    return sum(coef * prf_value(mac_prf(key, *t), curve) for coef, t in complement_triples(PrgInts(seed), write_step, num_blocks))


# ---- d_prf orders of the client writes
def update_triples(block_id, W, L):
    """Client.hpp:467, 505-534, 585-588; W = write_step after the ++ of :480, L = the level the write lands on"""
    out = [(0, block_id, W - 1)]
    for i in range(L):
        t = (W & ~(1 << L)) | ((1 << L) - (1 << i))
        out += [(i, j, t) for j in range(1 << i)]
        out += [(i, j + (1 << i), t) for j in range(1 << i)]
    out += [(L, j, W) for j in range(2 << L)]
    return out


def update_triples_reference_loop(block_id, W, L):
    """the same set in the order the reference's loops visit it (Client.hpp:512-534): used to check t_i, not the order"""
    out = [(0, block_id, W - 1)]
    t = W & ~(1 << L)
    for i in range(L - 1, -1, -1):
        t |= 1 << i
        for j in range(1 << i):
            out += [(i, j, t), (i, j + (1 << i), t)]
    out += [(L, j, W) for j in range(2 << L)]
    return out


def rebuild_triples(block_id, W, N):
    """Client.hpp:467, 488-497, 585-588"""
    out = [(0, block_id, W - 1)]
    out += [(0, i + 1, W - N + i) for i in range(N)]
    out += [(N.bit_length() - 1, j, W) for j in range(2 * N)]
    return out


def lowest_set_bit(W):
    return (W & -W).bit_length() - 1

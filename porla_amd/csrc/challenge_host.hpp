// The definitions behind the seed-in entry points (include/porla_gpu.h: porla_mac_prf_*, porla_client_prf_runs,
// porla_audit_challenge_*, porla_audit_complement_scalar_*, porla_diag_audit_walk), written once: AES-128, the reference's AES-CTR PRG
// stream (porla/Utils/prg.h:44-50, 84-97), the MAC PRF (Client.hpp:423-443), the audit walk (Server.hpp:604-732, Client.hpp:687-744),
// the d_prf orders of the two client write batches (Client.hpp:467-534, 585-588) and the client's complement scalar.
// Plain C++17 with no HIP types: challenge.hip compiles this text for the device, tools/challenge_selftest.cpp for the host alone.
#pragma once
#include <cstddef>
#include <cstdint>

#if !defined(PORLA_HD)             // (fe.hip.h has its own, with an inline in it)
#if defined(__HIPCC__)
#define PORLA_HD __host__ __device__
#else
#define PORLA_HD
#endif
#endif

namespace porla {
namespace chal {

// ---------------------------------------------------------------- AES-128 (FIPS-197)
// State and round keys are four words, word c = bytes 4c .. 4c+3 little-endian (byte 4c in the low bits): the bytes of a block are
// never swapped.  ONE table of 256 words: te0[x] = 2S | S << 8 | S << 16 | 3S << 24 with S = sbox[x], the column MixColumns makes of
// a row-0 byte; rows 1, 2, 3 are its left rotations by 8, 16, 24, and S itself is its byte 1 (the last round, the key schedule).
struct AesTe0 { uint32_t v[256]; };
struct AesRk { uint32_t w[44]; };

constexpr uint8_t aes_xtime(uint8_t x) { return (uint8_t)((x << 1) ^ ((x & 0x80) ? 0x1b : 0)); }
constexpr uint32_t aes_te0_word(uint8_t s) {
    const uint8_t s2 = aes_xtime(s);
    return (uint32_t)s2 | (uint32_t)s << 8 | (uint32_t)s << 16 | (uint32_t)(uint8_t)(s2 ^ s) << 24;
}
// the S-box from its definition: p runs through the powers of the generator 3, q through their inverses (q = p^-1), S = affine(q)
constexpr AesTe0 aes_make_te0() {
    AesTe0 t{};
    uint8_t p = 1, q = 1;
    do {
        p = (uint8_t)(p ^ aes_xtime(p));                             // p *= 3
        q = (uint8_t)(q ^ (q << 1));                                 // q /= 3
        q = (uint8_t)(q ^ (q << 2));
        q = (uint8_t)(q ^ (q << 4));
        if (q & 0x80) q ^= 0x09;
        uint8_t s = q;
        for (int i = 1; i <= 4; i++) s ^= (uint8_t)((q << i) | (q >> (8 - i)));
        t.v[p] = aes_te0_word((uint8_t)(s ^ 0x63));
    } while (p != 1);
    t.v[0] = aes_te0_word(0x63);
    return t;
}

PORLA_HD static uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
PORLA_HD static uint32_t aes_sub(const uint32_t* te0, uint32_t x) { return (te0[x & 0xff] >> 8) & 0xff; }
PORLA_HD static uint32_t load_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
PORLA_HD static void store_le32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// the 11 round keys of a 16-byte key
PORLA_HD static void aes128_expand(const uint32_t* te0, const uint8_t key[16], AesRk* rk) {
    for (int c = 0; c < 4; c++) rk->w[c] = load_le32(key + 4 * c);
    uint32_t rcon = 1;
    for (int i = 4; i < 44; i++) {
        uint32_t t = rk->w[i - 1];
        if ((i & 3) == 0) {
            t = (t >> 8) | (t << 24);                                  // RotWord: (a0, a1, a2, a3) -> (a1, a2, a3, a0)
            t = aes_sub(te0, t) | aes_sub(te0, t >> 8) << 8 | aes_sub(te0, t >> 16) << 16 | aes_sub(te0, t >> 24) << 24;
            t ^= rcon;
            rcon = (rcon << 1) ^ ((rcon & 0x80) ? 0x11b : 0);
        }
        rk->w[i] = rk->w[i - 4] ^ t;
    }
}

// one block: in / out as four little-endian words
PORLA_HD static void aes128_encrypt(const uint32_t* te0, const AesRk& rk, const uint32_t in[4], uint32_t out[4]) {
    uint32_t s0 = in[0] ^ rk.w[0], s1 = in[1] ^ rk.w[1], s2 = in[2] ^ rk.w[2], s3 = in[3] ^ rk.w[3];
#define PORLA_AES_COL(a, b, c, d)                                                                                                   \
    (te0[(a) & 0xff] ^ rotl32(te0[((b) >> 8) & 0xff], 8) ^ rotl32(te0[((c) >> 16) & 0xff], 16) ^ rotl32(te0[(d) >> 24], 24))
    for (int r = 1; r < 10; r++) {
        const uint32_t t0 = PORLA_AES_COL(s0, s1, s2, s3) ^ rk.w[4 * r + 0];
        const uint32_t t1 = PORLA_AES_COL(s1, s2, s3, s0) ^ rk.w[4 * r + 1];
        const uint32_t t2 = PORLA_AES_COL(s2, s3, s0, s1) ^ rk.w[4 * r + 2];
        const uint32_t t3 = PORLA_AES_COL(s3, s0, s1, s2) ^ rk.w[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
#undef PORLA_AES_COL
#define PORLA_AES_LAST(a, b, c, d)                                                                                                  \
    (aes_sub(te0, (a)) | aes_sub(te0, (b) >> 8) << 8 | aes_sub(te0, (c) >> 16) << 16 | aes_sub(te0, (d) >> 24) << 24)
    out[0] = PORLA_AES_LAST(s0, s1, s2, s3) ^ rk.w[40];
    out[1] = PORLA_AES_LAST(s1, s2, s3, s0) ^ rk.w[41];
    out[2] = PORLA_AES_LAST(s2, s3, s0, s1) ^ rk.w[42];
    out[3] = PORLA_AES_LAST(s3, s0, s1, s2) ^ rk.w[43];
#undef PORLA_AES_LAST
}

// ---------------------------------------------------------------- the PRG stream and the MAC PRF
// int t of the stream of PRG::reseed(seed, 0): the little-endian int32 at byte 4t, block t / 4 = AES(seed, counter t / 4 as a
// little-endian u64 in bytes 0 .. 7, zeros behind it)
struct PrgStream {
    const uint32_t* te0;
    const AesRk* rk;
    PORLA_HD int32_t operator()(uint32_t t) const {
        const uint32_t in[4] = {t >> 2, 0, 0, 0};
        uint32_t o[4];
        aes128_encrypt(te0, *rk, in, o);
        return (int32_t)o[t & 3];
    }
};
// ... and a stream the caller wrote (porla_diag_audit_walk)
struct IntStream {
    const int32_t* s;
    PORLA_HD int32_t operator()(uint32_t t) const { return s[t]; }
};

// AES(SECRET_KEY, level | index | time): level and index int32, time int64, all little-endian (Client.hpp:172-174, 426-429)
PORLA_HD static void mac_prf(const uint32_t* te0, const AesRk& rk, int32_t level, int32_t index, int64_t time, uint32_t out[4]) {
    const uint32_t in[4] = {(uint32_t)level, (uint32_t)index, (uint32_t)(uint64_t)time, (uint32_t)((uint64_t)time >> 32)};
    aes128_encrypt(te0, rk, in, out);
}

// |v| as a uint32 with mag(INT32_MIN) = 2^31.  The one deliberate definition: the reference calls abs(), undefined there; its index
// abs(v) % (2l) is 0 in practice and so is 2^31 mod 2l, its coefficient is whatever set_int makes of a negative int, ours is 2^31.
PORLA_HD static uint32_t mag(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

// ---------------------------------------------------------------- the audit walk
constexpr uint32_t AUDIT_CHECKS = 128;        // NUM_CHECK_AUDIT
constexpr int AUDIT_MAX_LEVELS = 25;          // num_blocks <= 2^24
// the largest point count the sums below are sized for: every level challenged at num_blocks = 2^24
constexpr uint32_t AUDIT_MAX_POINTS = 254 + 128 * 18;

// one challenged level: points [first_point, first_point + n) of the audit, ints from `pos` of the stream
struct WalkLevel {
    uint32_t level, n, first_point, pos, drawn, pad;
};
struct WalkPlan {
    uint32_t n_levels, n_points, pos_end, height;
    WalkLevel lv[AUDIT_MAX_LEVELS];
};

// num_blocks: a power of two, 2 .. 2^24
PORLA_HD static void walk_plan(uint64_t write_step, uint64_t num_blocks, WalkPlan* P) {
    uint32_t height = 1;
    while (((uint64_t)1 << (height - 1)) < num_blocks) height++;
    const uint64_t ws = write_step % num_blocks;
    uint32_t pos = 0, pts = 0, nl = 0;
    for (uint32_t i = 0; i < height; i++) {
        if (!(((ws >> i) & 1) || i == height - 1)) continue;
        const uint32_t two_l = 2u << i;
        WalkLevel& L = P->lv[nl++];
        L.level = i;
        L.drawn = two_l > AUDIT_CHECKS ? 1 : 0;
        L.n = L.drawn ? AUDIT_CHECKS : two_l;
        L.first_point = pts;
        L.pos = pos;
        L.pad = 0;
        pts += L.n;
        pos += L.drawn ? 2 * AUDIT_CHECKS : two_l;
    }
    P->n_levels = nl;
    P->n_points = pts;
    P->pos_end = pos;
    P->height = height;
}

// point j of a level: index in 0 .. 2l - 1 (>= l: the Y half, row index - l) and coefficient
template <class S>
PORLA_HD static void walk_point(const WalkLevel& L, uint32_t j, const S& s, uint32_t* index, uint32_t* coef) {
    if (L.drawn) {
        *index = mag(s(L.pos + j)) % (2u << L.level);
        *coef = mag(s(L.pos + AUDIT_CHECKS + j));
    } else {
        *index = j;
        *coef = mag(s(L.pos + j));
    }
}

// the level of point p
PORLA_HD static uint32_t walk_level_of(const WalkPlan& P, uint32_t p) {
    uint32_t a = 0;
    while (a + 1 < P.n_levels && p >= P.lv[a + 1].first_point) a++;
    return a;
}

// the order n of secp256k1, big-endian
PORLA_HD static void ipa_a_value(int32_t a, uint8_t out[32]) {
    const uint8_t n_be[32] = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xfe,
                              0xba, 0xae, 0xdc, 0xe6, 0xaf, 0x48, 0xa0, 0x3b, 0xbf, 0xd2, 0x5e, 0x8c, 0xd0, 0x36, 0x41, 0x41};
    const uint32_t m = mag(a);
    if (a >= 0) {
        for (int i = 0; i < 28; i++) out[i] = 0;
        out[28] = (uint8_t)(m >> 24); out[29] = (uint8_t)(m >> 16); out[30] = (uint8_t)(m >> 8); out[31] = (uint8_t)m;
        return;
    }
    uint32_t borrow = 0;                      // n - |a|
    for (int i = 31; i >= 0; i--) {
        const uint32_t sub = (i >= 28 ? (m >> (8 * (31 - i))) & 0xff : 0) + borrow;
        const uint32_t v = n_be[i];
        out[i] = (uint8_t)(v - sub);
        borrow = v < sub ? 1 : 0;
    }
}

// the tail values: KZG's random_point = (uint64)(int64) s[pos_end] (Server.hpp:907), IPA's a = s[n_points] (Server.hpp:861)
template <class S>
PORLA_HD static void walk_tail(const WalkPlan& P, const S& s, uint64_t* random_point, int32_t* a_raw, uint8_t a_value[32]) {
    *random_point = (uint64_t)(int64_t)s(P.pos_end);
    *a_raw = s(P.n_points);
    ipa_a_value(*a_raw, a_value);
}

// the time of the client's complement at level i (Client.hpp:646-650): the FULL write_step with its low i bits cleared
PORLA_HD static int64_t complement_time(uint64_t write_step, uint32_t level) {
    return (int64_t)(write_step & ~(((uint64_t)1 << level) - 1));
}

// ---------------------------------------------------------------- the complement scalar: sum_p coef_p * val_p, exact
// Each term is < 2^32 * 2^128 and an audit has at most AUDIT_MAX_POINTS < 2^12 points, so the sum is < 2^172: below the order of
// either group (both > 2^253), no reduction, six 32-bit limbs.
struct Acc192 { uint32_t v[6]; };

// the PRF output as the write batches read it: curve 0 (KZG) a big-endian 128-bit integer, curve 1 (IPA) r.d[0], r.d[1], a
// little-endian one; limbs little-endian
PORLA_HD static void prf_value_limbs(const uint32_t o[4], int curve, uint32_t val[4]) {
    if (curve == 1) {
        for (int k = 0; k < 4; k++) val[k] = o[k];
    } else {
        for (int k = 0; k < 4; k++) {
            const uint32_t w = o[3 - k];
            val[k] = (w >> 24) | ((w >> 8) & 0xff00) | ((w << 8) & 0xff0000) | (w << 24);
        }
    }
}
PORLA_HD static void acc_add_mul(Acc192* A, uint32_t coef, const uint32_t val[4]) {
    uint64_t carry = 0;
    for (int k = 0; k < 6; k++) {
        const uint64_t t = (uint64_t)A->v[k] + (k < 4 ? (uint64_t)coef * val[k] : 0) + carry;   // < 2^32 + (2^32-1)^2 + 2^32 < 2^64
        A->v[k] = (uint32_t)t;
        carry = t >> 32;
    }
}
PORLA_HD static void acc_store_be(const Acc192& A, uint8_t out[32]) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    for (int k = 0; k < 6; k++) {
        const uint32_t w = A.v[5 - k];
        out[8 + 4 * k] = (uint8_t)(w >> 24); out[9 + 4 * k] = (uint8_t)(w >> 16); out[10 + 4 * k] = (uint8_t)(w >> 8); out[11 + 4 * k] = (uint8_t)w;
    }
}
// one point's term: stream ints -> (index, coef), the PRF of (level, index, complement_time)
template <class S>
PORLA_HD static void complement_term(const uint32_t* te0, const AesRk& prf_rk, const WalkLevel& L, uint32_t j, const S& s,
                                            uint64_t write_step, int curve, Acc192* A) {
    uint32_t index, coef, o[4], val[4];
    walk_point(L, j, s, &index, &coef);
    mac_prf(te0, prf_rk, (int32_t)L.level, (int32_t)index, complement_time(write_step, L.level), o);
    prf_value_limbs(o, curve, val);
    acc_add_mul(A, coef, val);
}

// ---------------------------------------------------------------- d_prf orders of the client write batches
// slot t of a run is the triple (level, index0 + t, time0 + t * time_stride); layout of porla_prf_run
struct PrfRun {
    int32_t level, index0;
    uint64_t count;
    int64_t time0, time_stride;
};
PORLA_HD static void prf_run_slot(const uint32_t* te0, const AesRk& rk, const PrfRun& R, uint64_t t, uint32_t out[4]) {
    mac_prf(te0, rk, R.level, (int32_t)((uint32_t)R.index0 + (uint32_t)t), (int64_t)((uint64_t)R.time0 + t * (uint64_t)R.time_stride), out);
}

// Update write (Client.hpp:467, 505-534, 585-588), W = the write_step after the ++ of :480, L = the level: level + 2 runs,
// 2^(L+2) - 1 values.  The X part (i, j) and the Y part (i, j + 2^i) of a level are one run of 2^(i+1) indices.
static inline size_t prf_runs_update(int32_t block_id, uint64_t W, int L, PrfRun* out) {
    size_t n = 0;
    out[n++] = PrfRun{0, block_id, 1, (int64_t)(W - 1), 0};
    for (int i = 0; i < L; i++) {
        const uint64_t t_i = (W & ~((uint64_t)1 << L)) | (((uint64_t)1 << L) - ((uint64_t)1 << i));
        out[n++] = PrfRun{i, 0, (uint64_t)2 << i, (int64_t)t_i, 0};
    }
    out[n++] = PrfRun{L, 0, (uint64_t)2 << L, (int64_t)W, 0};
    return n;
}
// Rebuild write (Client.hpp:467, 488-497, 585-588), N = num_blocks: 3 runs, 3 N + 1 values
static inline size_t prf_runs_rebuild(int32_t block_id, uint64_t W, uint64_t N, PrfRun* out) {
    int top = 0;
    while (((uint64_t)1 << top) < N) top++;                           // height - 1
    out[0] = PrfRun{0, block_id, 1, (int64_t)(W - 1), 0};
    out[1] = PrfRun{0, 1, N, (int64_t)(W - N), 1};
    out[2] = PrfRun{top, 0, 2 * N, (int64_t)W, 0};
    return 3;
}

}  // namespace chal
}  // namespace porla

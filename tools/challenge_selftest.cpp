// Stand-alone host check of porla_amd/csrc/challenge_host.hpp, the text challenge.hip compiles for the device: the FIPS-197 /
// SP 800-38A vectors, a walk over a written stream with INT32_MIN at an index, a coefficient and an all-rows position, the run lists
// of an update and a rebuild write with their PRF values, and the complement scalars of that walk.  Everything computed is fed to
// one FNV-1a digest, printed as the single output line; tests/test_challenge_cpu.py builds this file with the host compiler's address
// and undefined-behaviour sanitizers and compares the digest with its Python model's.
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover tools/challenge_selftest.cpp -o challenge_selftest
#include "../porla_amd/csrc/challenge_host.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace porla::chal;

static uint64_t g_h = 0xcbf29ce484222325ull;
static void feed(const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; i++) { g_h ^= b[i]; g_h *= 0x100000001b3ull; }
}
static void feed32(uint32_t v) { uint8_t b[4]; store_le32(b, v); feed(b, 4); }
static void feed64(uint64_t v) { feed32((uint32_t)v); feed32((uint32_t)(v >> 32)); }

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
static void unhex(const char* s, uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = (uint8_t)(hexval(s[2 * i]) << 4 | hexval(s[2 * i + 1]));
}

static const AesTe0 te0 = aes_make_te0();

static void encrypt_bytes(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
    AesRk rk;
    aes128_expand(te0.v, key, &rk);
    uint32_t i4[4], o4[4];
    for (int c = 0; c < 4; c++) i4[c] = load_le32(in + 4 * c);
    aes128_encrypt(te0.v, rk, i4, o4);
    for (int c = 0; c < 4; c++) store_le32(out + 4 * c, o4[c]);
}

int main() {
    // ---- FIPS-197 C.1, FIPS-197 B, SP 800-38A F.1.1 block 1
    static const char* const vec[3][3] = {
        {"000102030405060708090a0b0c0d0e0f", "00112233445566778899aabbccddeeff", "69c4e0d86a7b0430d8cdb78070b4c55a"},
        {"2b7e151628aed2a6abf7158809cf4f3c", "3243f6a8885a308d313198a2e0370734", "3925841d02dc09fbdc118597196a0b32"},
        {"2b7e151628aed2a6abf7158809cf4f3c", "6bc1bee22e409f96e93d7e117393172a", "3ad77bb40d7a3660a89ecaf32466ef97"}};
    for (int v = 0; v < 3; v++) {
        uint8_t key[16], in[16], want[16], got[16];
        unhex(vec[v][0], key, 16); unhex(vec[v][1], in, 16); unhex(vec[v][2], want, 16);
        encrypt_bytes(key, in, got);
        if (memcmp(got, want, 16) != 0) { printf("challenge_selftest FAILED: AES vector %d\n", v); return 1; }
        feed(got, 16);
    }

    // ---- a walk over a written stream: num_blocks = 256, write_step % num_blocks = 255 (every level challenged; the ints of level 7,
    // the first drawn one, begin at 254, those of the top level 8 at 510)
    const uint64_t write_step = 255 + 3 * 256, num_blocks = 256;
    std::vector<int32_t> ints(2048);
    for (size_t t = 0; t < ints.size(); t++) ints[t] = (int32_t)((uint32_t)t * 2654435761u + 12345u);
    ints[0] = INT32_MIN;            // a coefficient of an all-rows level
    ints[1] = -1;
    ints[254 + 3] = INT32_MIN;      // an index of level 7
    ints[254 + 4] = 255;            // 2l - 1
    ints[254 + 5] = 256;            // 2l
    ints[254 + 128 + 5] = INT32_MIN;   // a coefficient of level 7
    ints[510 + 7] = INT32_MAX;
    const IntStream s{ints.data()};
    WalkPlan P;
    walk_plan(write_step, num_blocks, &P);
    Acc192 acc[2] = {{{0, 0, 0, 0, 0, 0}}, {{0, 0, 0, 0, 0, 0}}};
    const uint8_t secret[16] = {0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77, 0x88, 0x99, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0xff};
    AesRk prf_rk;
    aes128_expand(te0.v, secret, &prf_rk);
    for (uint32_t p = 0; p < P.n_points; p++) {
        const WalkLevel& L = P.lv[walk_level_of(P, p)];
        uint32_t index, coef;
        walk_point(L, p - L.first_point, s, &index, &coef);
        feed32(L.level); feed32(index); feed32(coef);
        for (int curve = 0; curve < 2; curve++) complement_term(te0.v, prf_rk, L, p - L.first_point, s, write_step, curve, &acc[curve]);
    }
    uint64_t z; int32_t a; uint8_t a_value[32];
    walk_tail(P, s, &z, &a, a_value);
    feed64(z); feed32((uint32_t)a); feed(a_value, 32);
    ipa_a_value(INT32_MIN, a_value); feed(a_value, 32);
    ipa_a_value(-1, a_value); feed(a_value, 32);
    for (int curve = 0; curve < 2; curve++) { uint8_t be[32]; acc_store_be(acc[curve], be); feed(be, 32); }

    // ---- the run lists of an update write (block 5, W = 12, level 2) and a rebuild write (block 3, W = 24, N = 8), and their values
    PrfRun runs[40];
    size_t n = prf_runs_update(5, 12, 2, runs);
    n += prf_runs_rebuild(3, 24, 8, runs + n);
    for (size_t r = 0; r < n; r++) {
        feed32((uint32_t)runs[r].level); feed32((uint32_t)runs[r].index0); feed64(runs[r].count);
        feed64((uint64_t)runs[r].time0); feed64((uint64_t)runs[r].time_stride);
        for (uint64_t t = 0; t < runs[r].count; t++) {
            uint32_t o[4];
            prf_run_slot(te0.v, prf_rk, runs[r], t, o);
            for (int c = 0; c < 4; c++) feed32(o[c]);
        }
    }
    printf("challenge_selftest digest=%016llx\n", (unsigned long long)g_h);
    return 0;
}

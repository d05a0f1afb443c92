// Pieces the batched IPA audit (ipa_audit_batch.hip) and the batched IPA verifier (ipa_verify_batch.hip) share: the record's layout,
// the transcript's compression function, the arithmetic mod n of a block of 128 lanes, and the check of the generators' fixed base
// (the host scaffold of the calls is batch_host.hpp's).
#pragma once
#include "engine.hpp"
#include "icc.hip.h"
#include "kzg_batch.hip.h"
#include "../../include/porla_gpu.h"

#include <cstddef>
#include <mutex>
#include <string>

namespace porla {

constexpr size_t IPA_RECORD = PORLA_IPA_AUDIT_RECORD_BYTES;
constexpr size_t IPA_PROOF = PORLA_IPA_PROOF_BYTES;
constexpr uint32_t IPA_N = 128;                    // NUM_CHUNKS: the prover's index pattern is written for it
constexpr uint32_t IPA_ROUNDS = 6;                 // half_width = 64 .. 2
constexpr uint32_t IPA_ROW_COEFFS = IPA_N + 1;     // the generators' coefficients, then u's
static_assert(IPA_PROOF == 32 + IPA_ROUNDS * 66 + 128 && IPA_RECORD == 99 + IPA_PROOF, "the reply of Server.hpp:856, :880-892");

using Fn = IccSecp256k1Fn;

struct Sha256K {
    static constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    // the transcript's tag, "hash of P, c, etc. all that jazz" (Server.hpp:2284), as big-endian words
    static constexpr uint32_t TAG[8] = {0x68617368u, 0x206f6620u, 0x502c2063u, 0x2c206574u, 0x632e2061u, 0x6c6c2074u, 0x68617420u, 0x6a617a7au};
    static constexpr uint32_t IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
};

__device__ __forceinline__ uint32_t rotr32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
// one SHA-256 compression of the 16 big-endian words w (destroyed) into the state s; fully unrolled, so that the message schedule
// stays in registers
__device__ __forceinline__ void sha256_compress(uint32_t (&s)[8], uint32_t (&w)[16]) {
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = s[i];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            w[t & 15] += (rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3)) + w[(t + 9) & 15] + (rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t e = v[4], a = v[0];
        const uint32_t t1 = v[7] + (rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25)) + ((e & v[5]) ^ (~e & v[6])) + Sha256K::K[t] + w[t & 15];
        const uint32_t t2 = (rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22)) + ((a & v[1]) ^ (a & v[2]) ^ (v[1] & v[2]));
        v[7] = v[6]; v[6] = v[5]; v[5] = v[4]; v[4] = v[3] + t1; v[3] = v[2]; v[2] = v[1]; v[1] = v[0]; v[0] = t1 + t2;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] += v[i];
}

// the sum of the 128 lanes' values mod n, to every lane (red: 128 x 8 words of LDS, free again on return)
__device__ __forceinline__ Fe<Fn> block_sum(Fe<Fn> v, uint32_t (*red)[8]) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int w = 0; w < 8; w++) red[t][w] = v.v[w];
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = IPA_N / 2; s >= 1; s >>= 1) {
        if (t < s) {
            Fe<Fn> o;
#pragma unroll
            for (int w = 0; w < 8; w++) o.v[w] = red[t + s][w];
            v = fe_add<Fn>(v, o);
#pragma unroll
            for (int w = 0; w < 8; w++) red[t][w] = v.v[w];
        }
        __syncthreads();
    }
    Fe<Fn> r;
#pragma unroll
    for (int w = 0; w < 8; w++) r.v[w] = red[0][w];
    __syncthreads();
    return r;
}

// 32 big-endian bytes taken mod n, in the Montgomery form
__device__ __forceinline__ Fe<Fn> load_scalar_mont(const uint8_t* src) {
    Fe<Fn> f;
    load_be256(f.v, src);
    fe_reduce_plain<Fn>(f.v, Fn::MAX_Q_IN);
    return fe_to_mont<Fn>(f);
}

// the fixed base of an IPA batch call: secp256k1, the 128 generators and u.  (A handle exists only where a device does, so this comes
// after ensure_device: without a device every non-NULL handle is refused as PORLA_ERR_NO_DEVICE before it is read.)
static inline int ipa_check_base(const porla_fixed_base* fb, const char* who) {
    if (fb->curve != 1 || fb->secp.n_points < IPA_ROW_COEFFS) {
        set_last_error(std::string(who) + ": gens_u_fb must be a secp256k1 fixed base over generators[0..127] || u (129 points)");
        return PORLA_ERR_ARG;
    }
    return PORLA_OK;
}

}  // namespace porla

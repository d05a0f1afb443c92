// Device pieces the KZG row evaluations share (kzg_client_batch.hip: k_kzg_eval_rows30 / k_kzg_eval_rows_lazy on 32-byte coefficients;
// retrieve_batch.hip.h: the same two forms on 64-byte code symbols): the constants of the Horner form, the end of an evaluation, and
// the 29-bit limbs and 64-bit columns of the dot-product form.
#pragma once
#include "msm.hip.h"
#include "icc30.hip.h"

namespace porla {

// compute_digest hoisted over rows (main.go:70-89): out[r] = big-endian bytes of alpha * f_r(tau) mod r, f_r given by n
// coefficients of 32 big-endian bytes (fr.SetBytes: reduced mod r).
// The evaluation with EIGHT lanes per row in the reduced-radix plain stream (rows longer than KZG_LAZY_MAX_COEFFS) of icc30.hip.h (modulus r = IccBn254Fr's q):
//   f(tau) = sum_{j<8} tau^j g_j(tau^8),   g_j(x) = sum_k c_{8k+j} x^k
// lane j runs Horner over its 16 coefficients with tau^8 in the 2^270 form -- acc * (tau^8 2^270) / 2^270 + c: the stream stays plain,
// a raw 256-bit coefficient is added unreduced (SetBytes' reduction happens in the last step), ONE product per coefficient where
// k_kzg_eval_rows spends two and a reduction -- then times tau^j, a butterfly sum over the eight lanes, and lane 0 multiplies by
// alpha and reduces once.  The 8 lanes of a row read 8 consecutive coefficients (256 B) per step, a wave 8 such runs; a row is 16
// dependent products deep instead of 128.  Bounds: acc < p + 2^248 + 2^256 < 2^258 at every step, the lane sum < 2^261.
struct KzgEvalConsts {
    uint32_t tj[8][8];   // tau^j * 2^270 mod r, canonical words, j < 8
    uint32_t t8[8];      // tau^8 * 2^270 mod r
    uint32_t alpha[8];   // alpha * 2^270 mod r
};
// The end the evaluation kernels share: the butterfly sum over a row's eight lanes (wave-wide, so idle lanes come this far), the
// MAC batch's second scalar copied beside the result by lane 1 (out_stride = 64), and lane 0's product with alpha in the 2^270
// form, the one reduction and the store.  Nothing follows it in any kernel: its returns are the Horner kernels' returns and the
// dot-product kernels' continues.  PRF16: `second` holds 16 raw bytes per row, a big-endian 128-bit integer (the MAC PRF as
// compute_digest_complement reads it), which lane 1 writes left-padded to the 32 bytes of the scalar; otherwise 32 bytes per row.
template <class Q, bool PRF16 = false>
__device__ __forceinline__ void kzg_eval_finish(F30<Q> acc, bool live, uint32_t j, size_t r, const uint32_t (&alpha270)[8],
                                                uint8_t* __restrict__ out, uint32_t out_stride, const uint8_t* __restrict__ second) {
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        F30<Q> o;
#pragma unroll
        for (int l = 0; l < 9; l++) o.v[l] = (uint32_t)__shfl_xor((int)acc.v[l], m);
        acc = icc30_add<Q>(acc, o);
    }
    if (!live) return;
    if (j == 1 && second) {
        uint4* dst = (uint4*)(out + r * out_stride + 32);
        if constexpr (PRF16) {
            dst[0] = make_uint4(0, 0, 0, 0);
            dst[1] = *(const uint4*)second;                    // (the caller's pointer is the row's own value)
        } else {
            const uint4* src = (const uint4*)(second + r * 32);
            dst[0] = src[0]; dst[1] = src[1];
        }
    }
    if (j != 0) return;
    const Fe<Q> res = icc30_canonical<Q>(icc30_reduce_top<Q>(icc30_mul<Q>(acc, f30_unpack<Q>(alpha270))));
    store_be256(out + r * out_stride, res.v);
}

// The evaluation as a DOT PRODUCT with the reduction left to the end: f(tau) = sum_i c_i tau^i with the powers of tau in a table
// (9 limbs of 29 bits each, staged in LDS), lane j of a row's eight taking i = 8k + j.  A coefficient times a power is 81
// multiply-adds into 17 64-bit columns and nothing else -- no reduction, no carries: limbs below 2^29 make a column's nine
// products of one coefficient < 2^61.2, so SIX coefficients accumulate before the columns are rippled (6 * 9 * 2^58 + 2^29 <
// 2^64) -- where the Horner form above pays a full modular product (81 + 90 multiply-adds and the carries) per coefficient.
// The lane's sum (< steps * 2^510) is then three 256-bit pieces hi, mid, lo joined by two products with 2^256 in the 2^270 form,
// and from there the lanes are summed, multiplied by alpha and reduced exactly as in the Horner form.
constexpr int KZG_LAZY_ENTRY_WORDS = 12;      // 9 limbs + 3 words of padding: three 16-byte LDS reads per power
constexpr uint32_t KZG_LAZY_MAX_COEFFS = 1024;
constexpr uint32_t KZG_M29 = (1u << 29) - 1u;
constexpr int KZG_LAZY_GROUP = 6;              // coefficients accumulated between two ripples of the columns
// (reading all six coefficients of a group ahead of their products: 142 registers, 0.51 ms against 0.46 at 2^19 rows; one step
// ahead, as in k_kzg_eval_rows_lazy: 0.44)
// a 256-bit value as 9 limbs of 29 bits (the kernel's coefficients; on the host, the table's powers of tau)
__host__ __device__ __forceinline__ void kzg_unpack29(const uint32_t w[8], uint32_t out[9]) {
#pragma unroll
    for (int l = 0; l < 9; l++) {
        const int bit = 29 * l, i = bit >> 5, sft = bit & 31;
        const uint64_t two = (uint64_t)w[i] | (i + 1 < 8 ? (uint64_t)w[i + 1] << 32 : 0ull);
        out[l] = (uint32_t)(two >> sft) & KZG_M29;
    }
}
__device__ __forceinline__ void kzg_ripple29(uint64_t (&col)[19]) {
    uint64_t carry = 0;
#pragma unroll
    for (int k = 0; k < 19; k++) {
        const uint64_t t = col[k] + carry;
        col[k] = t & KZG_M29;
        carry = t >> 29;
    }
}
// the rippled columns (a sum below 2^544) -> the lane's value in the plain stream: 19 limbs of 29 bits -> 17 words of 32, lo = words
// 0..7, mid = 8..15, hi = word 16, joined by two products with 2^256 in the 2^270 form
template <class Q>
__device__ __forceinline__ F30<Q> kzg_columns_join(const uint64_t (&col)[19]) {
    uint32_t W[17];
#pragma unroll
    for (int w = 0; w < 17; w++) {
        const int bit = 32 * w, l = bit / 29, sft = bit % 29;
        uint64_t v = col[l] >> sft;
        if (l + 1 < 19) v |= col[l + 1] << (29 - sft);
        if (l + 2 < 19 && 58 - sft < 32) v |= col[l + 2] << (58 - sft);
        W[w] = (uint32_t)v;
    }
    uint32_t hi[8];
#pragma unroll
    for (int w = 0; w < 8; w++) hi[w] = w == 0 ? W[16] : 0u;
    const F30<Q> C526 = f30_const<Q>(Icc30Const<Q>::C526);
    F30<Q> acc = icc30_add<Q>(icc30_mul<Q>(f30_unpack<Q>(hi), C526), f30_unpack<Q>(W + 8));
    return icc30_add<Q>(icc30_mul<Q>(acc, C526), f30_unpack<Q>(W));
}
struct KzgAlpha270 { uint32_t w[8]; };       // alpha * 2^270 mod r

}  // namespace porla

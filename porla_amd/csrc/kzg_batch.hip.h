// Device pieces the batched audits (kzg_audit_batch.hip, ipa_audit_batch.hip) and the batched verifier (kzg_verify_batch.hip) share: the gather of
// challenged store entries into batched-MSM pairs, and the conversion of a lane's projective points to affine with one inversion.
#pragma once
#include "fixed_base.hip.h"

namespace porla {

constexpr uint32_t KZG_GATHER_PAIRS = 64;          // pairs per block of a gather kernel (four lanes per pair)

// The pairs (coef_i, store_a[idx_i]) at pair0 + i and, when TWO, (coef_i, store_b[idx_i]) at pair0 + n + i, for the pairs
// i = 64 blk + threadIdx.x / 4 < n of the calling block; four lanes per pair as k_audit_gather (msm_impl.hip.h), the scalar a 32-byte
// big-endian integer (bn254_scalar_set_int).
template <bool TWO>
__device__ __forceinline__ void kzg_gather_pairs(const uint8_t* store_a, const uint8_t* store_b, const uint64_t* idx, const uint32_t* coef,
                                                 uint32_t n, uint64_t pair0, uint32_t blk, uint8_t* scalars, uint8_t* points) {
    const uint32_t i = blk * KZG_GATHER_PAIRS + (threadIdx.x >> 2), q = threadIdx.x & 3u;
    if (i >= n) return;
    const uint64_t src = idx[i];
    const size_t pa = pair0 + i, pb = pair0 + n + i;
    reinterpret_cast<uint4*>(points + 64 * pa)[q] = reinterpret_cast<const uint4*>(store_a + 64 * src)[q];
    if (TWO) reinterpret_cast<uint4*>(points + 64 * pb)[q] = reinterpret_cast<const uint4*>(store_b + 64 * src)[q];
    if (q < 2) {
        uint4 z = make_uint4(0, 0, 0, 0);
        if (q == 1) z.w = __builtin_bswap32(coef[i]);         // bytes 28..31 of the big-endian scalar
        reinterpret_cast<uint4*>(scalars + 32 * pa)[q] = z;
        if (TWO) reinterpret_cast<uint4*>(scalars + 32 * pb)[q] = z;
    }
}

// N projective points to affine with ONE inversion: Montgomery's trick over their ZZZ, as k_fb_finish does for a lane's rows.
// emit(j, live, x, y) for j = N - 1 .. 0: the plain (non-Montgomery) coordinates of point j, or live = false for infinity
template <class C, int N, class Emit>
__device__ __forceinline__ void xyzz_each_affine_one_inv(const XYZZ<typename C::Fp> (&p)[N], Emit emit) {
    using M = typename C::Fp;
    Fe<M> zzz[N], pre[N];
    bool live[N];
    Fe<M> acc = fe_one<M>();
#pragma unroll
    for (int j = 0; j < N; j++) {
        live[j] = !fe_is_zero<M>(p[j].zzz);
        zzz[j] = live[j] ? p[j].zzz : fe_one<M>();
        pre[j] = acc;
        acc = fe_mul_call<M>(acc, zzz[j]);
    }
    Fe<M> inv;
    if constexpr (C::F30_BUCKETS) inv = fe_inv_safegcd<M>(acc);
    else inv = fe_inv_dev<M>(acc);
    Fe<M> one = fe_zero<M>();
    one.v[0] = 1;
#pragma unroll
    for (int j = N - 1; j >= 0; j--) {
        const Fe<M> inv_j = fe_mul_call<M>(inv, pre[j]);
        inv = fe_mul_call<M>(inv, zzz[j]);
        if (!live[j]) {
            emit(j, false, one, one);
            continue;
        }
        const Affine<M> af = xyzz_to_affine_with_inv<M>(p[j], inv_j);
        const Fe<M> x = fe_mul_call<M>(af.x, one), y = fe_mul_call<M>(af.y, one);   // out of Montgomery form
        emit(j, true, x, y);
    }
}

// ... to 64-byte big-endian affine at base + at[j] (64 zero bytes = infinity)
template <class C, int N>
__device__ __forceinline__ void xyzz_to_be_one_inv(const XYZZ<typename C::Fp> (&p)[N], uint8_t* base, const uint32_t (&at)[N]) {
    using M = typename C::Fp;
    xyzz_each_affine_one_inv<C, N>(p, [&](int j, bool live, const Fe<M>& x, const Fe<M>& y) {
        uint8_t* dst = base + at[j];
        if (!live) {
            const uint4 z = make_uint4(0, 0, 0, 0);
            uint4* q = reinterpret_cast<uint4*>(dst);
            q[0] = z; q[1] = z; q[2] = z; q[3] = z;
            return;
        }
        store_be256(dst, x.v);
        store_be256(dst + 32, y.v);
    });
}

}  // namespace porla

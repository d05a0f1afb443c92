// The passes the client's batches share (client_update_batch.hip, client_rebuild_batch.hip).  The block pass: step 1 of both is
// MAC = Commit_alpha(block) + comp0 (porla/Client/Client.hpp:467-471), and Commit_alpha(block) of K blocks is one commitment pass over K
// big-endian coefficient rows -- KZG: the digest row of porla_kzg_digest_batch_device (k_kzg_eval_rows_lazy and the one-point table of
// G1[0]); IPA: alpha_generators_fb over the 128 coefficients of a row.  The h pass: scalars against the hiding base's one-point table.
// Here: the lane that turns a raw chunk into its coefficient (either batch's expand kernel), the two passes, the KZG build's precheck.
#pragma once
#include "kzg_state.hpp"
#include "../../include/porla_gpu.h"

namespace porla {

// chunk t of `block` (32 bytes little-endian, any 256-bit value) -> the big-endian coefficient at `coeff`; the pass reduces mod the
// group order itself
__device__ __forceinline__ void cu_chunk_to_coeff(const uint8_t* __restrict__ block, uint32_t t, uint8_t* __restrict__ coeff) {
    const uint4* s4 = reinterpret_cast<const uint4*>(block + 32 * (size_t)t);
    const uint4 lo = s4[0], hi = s4[1];
    uint4* d4 = reinterpret_cast<uint4*>(coeff);
    d4[0] = make_uint4(__builtin_bswap32(hi.w), __builtin_bswap32(hi.z), __builtin_bswap32(hi.y), __builtin_bswap32(hi.x));
    d4[1] = make_uint4(__builtin_bswap32(lo.w), __builtin_bswap32(lo.z), __builtin_bswap32(lo.y), __builtin_bswap32(lo.x));
}

// K rows of ncols coefficients at d_rows -> K affine points at d_blk.  fb_alpha == nullptr: the KZG build (the resident key and SRS).
template <class C>
static int client_block_pass(FixedBase<C>* fb_alpha, const uint8_t* d_rows, size_t k, size_t ncols, uint8_t* d_blk, hipStream_t stream) {
    if constexpr (std::is_same<C, Bn254G1>::value) {
        return porla_kzg_digest_batch_device(d_rows, k, d_blk, stream);
    } else {
        std::lock_guard<std::mutex> lk(fb_alpha->mu);
        return fb_alpha->commit_device(d_rows, k, ncols, 32 * ncols, d_blk, stream);
    }
}

// the h pass: n_rows 32-byte scalars at d_scal times the hiding base (fb_h == nullptr: KZG's resident one) -> affine points at d_hpts
template <class C>
static int client_h_pass(FixedBase<C>* fb_h, const uint8_t* d_scal, size_t n_rows, uint8_t* d_hpts, hipStream_t stream) {
    if constexpr (std::is_same<C, Bn254G1>::value) {
        return porla_kzg_complement_batch_device(d_scal, n_rows, d_hpts, stream);
    } else {
        std::lock_guard<std::mutex> lk(fb_h->mu);
        return fb_h->commit_device(d_scal, n_rows, 1, 32, d_hpts, stream);
    }
}

// the KZG build before any device work: the key and the SRS (an empty digest batch makes exactly that check), then the row width
static inline int client_kzg_row_width(size_t* ncols) {
    if (int rc = porla_kzg_digest_batch_device(nullptr, 0, nullptr, nullptr)) return rc;
    return kzg_row_width(ncols);
}

}  // namespace porla

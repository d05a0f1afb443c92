// Kernels of the server's rebuild write for K independent files (server_rebuild_batch.hip: porla_server_rebuild_batch_device): the step
// of Server::update that calls CRebuild_Cached instead of HAdd (porla/Server/Server.hpp:413-469, :1487-1833).  The arithmetic is that
// of the single-file encodes -- the data network of icc30_split.hip.h (icc30_plane / icc30_round, the finish step in its XY form), the
// MAC network of mac_fft.hip.h (maco_butterfly, macq_ladder + macq_butterfly_out, mac30_scalar_mul) -- whose device functions these
// kernels call; what is new is the addressing.  A kernel that needs a request's pointers is indexed blockIdx.y = request and reads
// them from the uploaded descriptors; the stages of the MAC network run on ONE work array of K * n_total points (request r at
// r * n_total), where butterfly t of a stage finds its pair from t alone because n_total is a multiple of every stage's block.
#pragma once
#include "icc.hip.h"
#include "icc30.hip.h"
#include "icc30_split.hip.h"
#include "mac_fft.hip.h"

namespace porla {

// One request as the kernels see it.  wt = w^reverse_bits(write_step % N, height - 1): the Montgomery residue pair the data side
// multiplies by, and the plain integer reduced mod the group order (little-endian words) the MAC side multiplies by.
struct SrDesc {
    const uint8_t* block;
    const uint8_t* mac;
    const uint8_t* comp;          // 2 * n_total points (X, then Y), or nullptr
    uint8_t* u_blocks;
    uint8_t* u_macs;
    uint8_t* data_x; uint8_t* data_y;
    uint8_t* mac_x; uint8_t* mac_y;
    uint8_t* align_x; uint8_t* align_y;
    uint32_t wt_p[8], wt_q[8], wt_sc[8];
    uint32_t row, pad;            // row = index - 1: the row of U the block lands on
};
static_assert(sizeof(SrDesc) == 192, "SrDesc: 88 bytes of pointers, 96 of wt, the row");

// ---- the store: U[index - 1] = block, MAC_U[index - 1] = mac (Server.hpp:413-427), 16 bytes per lane and turn
// (static: no template, and two translation units include this file)
static __global__ void __launch_bounds__(256)
k_sr_store(const SrDesc* __restrict__ desc, uint32_t ncols) {
    const SrDesc& D = desc[blockIdx.y];
    const size_t bu = (size_t)ncols * 2;                                   // 16-byte units of a block; the MAC is four more
    const uint4* sb = reinterpret_cast<const uint4*>(D.block);
    const uint4* sm = reinterpret_cast<const uint4*>(D.mac);
    uint4* ub = reinterpret_cast<uint4*>(D.u_blocks + (size_t)D.row * ncols * 32);
    uint4* um = reinterpret_cast<uint4*>(D.u_macs + (size_t)D.row * 64);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < bu + 4; u += stride) {
        if (u < bu) ub[u] = sb[u];
        else um[u - bu] = sm[u - bu];
    }
}

// ---- one pass of the data network of request blockIdx.y: k_icc_split30's tiles, planes and rounds (icc30_split.hip.h) on the
// request's own store.  FIRST reads the raw chunks of U (the X part's network: no init scaling), a pass that is not LAST leaves the
// two residue planes in the request's slice of `work` (plane_words words per plane), LAST writes both parts: X from the registers of
// the last round, Y_k = wt X_k mod LCM from one more product per plane (the XY form).  A mod p_icc of either part waits for the q
// plane in the first 32 bytes of the symbol's own 64-byte output slot, which the same lane then overwrites with the value mod LCM.
template <class Q, bool FIRST, bool LAST>
__global__ void __launch_bounds__(ICC30_SPLIT_THREADS) __attribute__((amdgpu_waves_per_eu(LAST ? 3 : 4, 4)))
k_sr_data(const SrDesc* __restrict__ desc, uint32_t* __restrict__ work, size_t plane_words, const uint32_t* __restrict__ twp,
          const uint32_t* __restrict__ twq, uint32_t n, uint32_t ncols, int s0, int ns, int cc_log) {
    __shared__ uint2 lds2[ICC_TILE_ELEMS * ICC30_PSLOT_WORDS / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(lds2);
    const SrDesc& D = desc[blockIdx.y];
    const uint8_t* raw = D.u_blocks;
    uint32_t* work_p = work + (size_t)blockIdx.y * 2 * plane_words;
    uint32_t* work_q = work_p + plane_words;
    IccTile T;
    T.n = n; T.ncols = ncols; T.s0 = s0; T.ns = ns; T.cc_log = (uint32_t)cc_log;
    T.elems = (1u << ns) << cc_log;
    T.raw = FIRST;
    T.lo_bits = (uint32_t)(s0 - 1);
    const uint32_t Cc = 1u << cc_log;
    const uint32_t col_tiles = (ncols + Cc - 1) >> cc_log;
    uint32_t tile = blockIdx.x;                                            // (an XCD owns a contiguous range of tiles, as k_icc_split30)
    if ((gridDim.x & 7u) == 0) tile = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const uint32_t ct = tile % col_tiles;
    tile /= col_tiles;
    T.lo = tile & ((1u << T.lo_bits) - 1u);
    const uint32_t hi = tile >> T.lo_bits;
    T.row_base = (hi << (T.lo_bits + ns)) + T.lo;
    T.c0 = ct << cc_log;
    const IccOut ox{D.data_x, nullptr, nullptr, nullptr, 0}, oy{D.data_y, nullptr, nullptr, nullptr, 0};
    uint32_t slot[4];
    {
        F30<IccFp> rp[4];
        icc30_plane<IccFp, FIRST>(lds, T, raw, F30<IccFp>{}, work_p, twp, rp, slot);
        F30<IccFp> Ky = F30<IccFp>{};
        if (LAST) {                                                       // wt in the 2^270 form
            Fe<IccFp> w;
#pragma unroll
            for (int j = 0; j < 8; j++) w.v[j] = D.wt_p[j];
            Ky = icc30_mul<IccFp>(f30_unpack<IccFp>(w.v), f30_const<IccFp>(Icc30Const<IccFp>::C284));
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const uint32_t mid = slot[i] >> cc_log, col = slot[i] & (Cc - 1);
                const size_t gi = (size_t)(T.row_base + (mid << T.lo_bits)) * ncols + T.c0 + col;
                if (LAST) {
                    st_fe<IccFp>(reinterpret_cast<uint32_t*>(ox.x + 64 * gi), icc30_finish_p(rp[i]));
                    st_fe<IccFp>(reinterpret_cast<uint32_t*>(oy.x + 64 * gi), icc30_finish_p(icc30_mul<IccFp>(rp[i], Ky)));
                } else {
                    icc30_st_work<IccFp>(work_p + gi * ICC30_PLANE_WORDS, rp[i]);
                }
            }
        }
        __syncthreads();                                 // every lane has read its last round's symbols: the region is free
    }
    {
        F30<Q> rq[4];
        icc30_plane<Q, FIRST>(lds, T, raw, F30<Q>{}, work_q, twq, rq, slot);
        F30<Q> Ky = F30<Q>{};
        if (LAST) {
            Fe<Q> w;
#pragma unroll
            for (int j = 0; j < 8; j++) w.v[j] = D.wt_q[j];
            Ky = icc30_mul<Q>(f30_unpack<Q>(w.v), f30_const<Q>(Icc30Const<Q>::C284));
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (slot[i] != 0xffffffffu) {
                const uint32_t mid = slot[i] >> cc_log, col = slot[i] & (Cc - 1);
                const size_t gi = (size_t)(T.row_base + (mid << T.lo_bits)) * ncols + T.c0 + col;
                if (LAST) {
                    Fe<IccFp> P;                                           // what this lane stored after the p_icc plane
                    const uint32_t* sx = reinterpret_cast<const uint32_t*>(ox.x + 64 * gi);
#pragma unroll
                    for (int k = 0; k < 8; k++) P.v[k] = sx[k];
                    icc30_finish_q<Q>(P, rq[i], gi, ox);
                    const uint32_t* sy = reinterpret_cast<const uint32_t*>(oy.x + 64 * gi);
#pragma unroll
                    for (int k = 0; k < 8; k++) P.v[k] = sy[k];
                    icc30_finish_q<Q>(P, icc30_mul<Q>(rq[i], Ky), gi, oy);  // (wt X) mod q
                } else {
                    icc30_st_work<Q>(work_q + gi * ICC30_PLANE_WORDS, rq[i]);
                }
            }
        }
    }
}

// ---- MAC_U of request blockIdx.y -> its n points of the work array (the lazy memory form): a lane per point
template <class C>
__global__ void __launch_bounds__(64)
k_sr_mac_load(const SrDesc* __restrict__ desc, uint32_t n, XYZZ<typename C::Fp>* __restrict__ work) {
    using M = typename C::Fp;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_xyzz<M>(work + (size_t)blockIdx.y * n + i, load_affine_be_lazy<M>(desc[blockIdx.y].u_macs + (size_t)i * 64));
}

// ---- stage s of the MAC network over the whole work array: butterfly t < total = K n / 2 is pair (k, k + 2^(s-1)) with
// k = (t >> (s-1)) 2^s + j, j = t mod 2^(s-1) -- inside one request, because n is a multiple of 2^s -- and its twiddle is entry
// j * (n >> (s-1)) of the table of n_total, never of the work array's length.  The three forms of k_mac_stage30_oct / _quad / k_mac_stage30
// with per-butterfly scalars (stage 1, every twiddle 1: k_mac_stage1_quad itself on K n points, or the lane form's s == 1 branch).
__device__ __forceinline__ void sr_stage_index(uint32_t t, uint32_t n, int s, uint32_t& k, uint32_t& m2, uint32_t (&sc)[8],
                                               const uint32_t* __restrict__ tws) {
    m2 = 1u << (s - 1);
    const uint32_t j = t & (m2 - 1);
    k = ((t >> (s - 1)) << s) + j;
    const uint32_t e = j * (n >> (s - 1));
    const uint4* w4 = reinterpret_cast<const uint4*>(tws + (size_t)e * 8);
    const uint4 a = w4[0], b = w4[1];
    sc[0] = a.x; sc[1] = a.y; sc[2] = a.z; sc[3] = a.w; sc[4] = b.x; sc[5] = b.y; sc[6] = b.z; sc[7] = b.w;
}
template <class C>
__global__ void __launch_bounds__(8 * MACO_BF) MACO_ATTR
k_sr_mac_stage_oct(XYZZ<typename C::Fp>* __restrict__ work, const uint32_t* __restrict__ tws, uint32_t n, uint32_t total, int s) {
    using M = typename C::Fp;
    MACO_LDS(L);
    __builtin_amdgcn_s_setprio(3);                                         // (as k_mac_stage30_oct: a latency-bound wave must win the issue arbitration)
    const uint32_t o = threadIdx.x >> 3, half = (threadIdx.x >> 2) & 1u, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t t = blockIdx.x * MACO_BF + o;
    const bool valid = t < total;
    if (!valid) t = 0;                                                     // padding octets compute butterfly 0 and store nothing
    uint32_t k, m2, sc[8];
    sr_stage_index(t, n, s, k, m2, sc, tws);
    if (half) macq_copy_coord<M>(&L.um[o], work + k, r);
    else macq_copy_coord<M>(&L.qd[o].tbl[0], work + k + m2, r);
    macq_sync();
    maco_butterfly<C>(L, o, half, r, lane, sc, work + k, work + k + m2, valid);
}
template <class C>
__global__ void __launch_bounds__(4 * MACQ_BF) MACQ_GUEST_ATTR
k_sr_mac_stage_quad(XYZZ<typename C::Fp>* __restrict__ work, const uint32_t* __restrict__ tws, uint32_t n, uint32_t total, int s) {
    using M = typename C::Fp;
    MACQ_LDS(L);
    __builtin_amdgcn_s_setprio(3);
    const uint32_t q = threadIdx.x >> 2, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t t = blockIdx.x * MACQ_BF + q;
    const bool valid = t < total;
    if (!valid) t = 0;
    uint32_t k, m2, sc[8];
    sr_stage_index(t, n, s, k, m2, sc, tws);
    macq_copy_coord<M>(&L.qd[q].tbl[0], work + k + m2, r);
    macq_copy_coord<M>(&L.um[q], work + k, r);
    macq_sync();
    F30<M> c;
    bool inf;
    macq_ladder<C>(L.qd[q], &L.acc[q], &L.tmp[q], r, lane, sc, c, inf);
    macq_butterfly_out<M>(&L.um[q], &L.acc[q], &L.tmp[q], c, inf, work + k, work + k + m2, valid, r, lane);
}
template <class C>
__global__ void __launch_bounds__(256)
k_sr_mac_stage_lane(XYZZ<typename C::Fp>* __restrict__ work, const uint32_t* __restrict__ tws, uint32_t n, uint32_t total, int s) {
    using M = typename C::Fp;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    uint32_t k, m2, sc[8];
    sr_stage_index(t, n, s, k, m2, sc, tws);
    XYZZ<M> hi = load_xyzz<M>(work + k + m2);
    XYZZ<M> tm;
    if (s == 1) tm = hi;                                                   // stage 1: every twiddle is w^0 = 1 (uniform over the launch)
    else mac30_scalar_mul<C>(&tm, &hi, sc);
    XYZZ<M> sum = load_xyzz<M>(work + k);
    XYZZ<M> dif = sum;
    xyzz30_add_mem<M>(&sum, &tm, 0, 0, nullptr);
    xyzz30_add_mem<M>(&dif, &tm, 1, 0, nullptr);
    store_xyzz<M>(work + k, sum);
    store_xyzz<M>(work + k + m2, dif);
}

// ---- the Y part: work_y[i] = wt * work[i] for the n points of request blockIdx.y (Y_k = wt X_k, mac_fft.hip:mac_encode_core).  A
// block belongs to one request, so every wave multiplies by one scalar: the wave-uniform ladders of k_mac_load30_quad / k_mac_scale30.
template <class C>
__global__ void __launch_bounds__(4 * MACQ_BF) MACQ_GUEST_ATTR
k_sr_mac_scale_quad(const SrDesc* __restrict__ desc, uint32_t n, const XYZZ<typename C::Fp>* __restrict__ work,
                    XYZZ<typename C::Fp>* __restrict__ work_y) {
    using M = typename C::Fp;
    MACQ_LDS(L);
    __builtin_amdgcn_s_setprio(3);
    const uint32_t q = threadIdx.x >> 2, r = threadIdx.x & 3u, lane = threadIdx.x & 63u;
    uint32_t i = blockIdx.x * MACQ_BF + q;
    const bool valid = i < n;
    if (!valid) i = 0;                                                     // padding quads compute point 0 and store nothing
    uint32_t sc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) sc[j] = desc[blockIdx.y].wt_sc[j];
    const size_t at = (size_t)blockIdx.y * n + i;
    macq_copy_coord<M>(&L.qd[q].tbl[0], work + at, r);
    macq_sync();
    F30<M> c;
    bool inf;
    macq_ladder_uniform<C>(L, q, r, lane, threadIdx.x >> 6, sc, c, inf);
    if (valid) macq_store_point<M>(work_y + at, c, inf, r);
}
template <class C>
__global__ void __launch_bounds__(64)
k_sr_mac_scale_lane(const SrDesc* __restrict__ desc, uint32_t n, const XYZZ<typename C::Fp>* __restrict__ work,
                    XYZZ<typename C::Fp>* __restrict__ work_y) {
    using M = typename C::Fp;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t at = (size_t)blockIdx.y * n + i;
    XYZZ<M> p = load_xyzz<M>(work + at);
    uint32_t k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = desc[blockIdx.y].wt_sc[j];
    XYZZ<M> rr;
    __shared__ __align__(8) uint16_t wdig[MACQ_CODES_STRIDE];              // (64 lanes = one wave per block; one scalar for every MAC)
    mac30_scalar_mul_uniform<C>(&rr, &p, k, wdig);
    store_xyzz<M>(work_y + at, rr);
}

// ---- the close of request blockIdx.y: a lane per output point g < 2 n (X part, then Y).  The MAC network's result (work / work_y,
// projective) plus the request's complement (Server.hpp:449-469 with updated_level = height - 1) as one general addition, to affine
// with one inversion per lane -- the network's finish folded in; without complements the result alone -- into the resident half of
// MAC X / MAC Y, and 64 zero bytes (infinity, Server.hpp:1527-1535) into the same place of the resident half of align X / align Y.
template <class C>
__global__ void __launch_bounds__(256)
k_sr_close(const SrDesc* __restrict__ desc, uint32_t n, const XYZZ<typename C::Fp>* __restrict__ work,
           const XYZZ<typename C::Fp>* __restrict__ work_y) {
    using M = typename C::Fp;
    const SrDesc& D = desc[blockIdx.y];
    const size_t base = (size_t)blockIdx.y * n;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < 2 * (size_t)n; g += stride) {
        const bool y = g >= n;
        const size_t j = y ? g - n : g;
        XYZZ<M> a = load_xyzz<M>((y ? work_y : work) + base + j);
        if (D.comp) {
            const XYZZ<M> b = load_affine_be_lazy<M>(D.comp + 64 * g);
            xyzz30_add_mem<M>(&a, &b, 0, 0, nullptr);
        }
        store_affine_be<M>((y ? D.mac_y : D.mac_x) + 64 * j, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
        uint4* al = reinterpret_cast<uint4*>((y ? D.align_y : D.align_x) + 64 * j);
        al[0] = zero; al[1] = zero; al[2] = zero; al[3] = zero;
    }
}

}  // namespace porla

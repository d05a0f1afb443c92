// Kernels of the client's rebuild write (client_rebuild_batch.hip: porla_kzg_client_rebuild_batch_device /
// porla_ipa_client_rebuild_batch_device): Client::CRebuild (porla/Client/Client.hpp:483-502, :1040-1453, the wire loop :584-614) for K
// independent writes, computed in the SCALAR domain.  On the client every point of that step is a known scalar times the one hiding
// point h: complements_U[i] = s_i h, the network's multipliers are the integers v^j mod p_icc reduced mod the group order q by the group
// itself, the new complements are s'_j h.  The network is linear over Z_q, so
//
//     out[j]     = (s'_j     -      T_j) h,      T = the butterfly network of oracle mac_crebuild applied to (s_i) in Z_q,
//     out[N + j] = (s'_{N+j} - wt * T_j) h       (the Y part is the X part's network on inputs scaled by wt: mac_fft.hip),
//
// N/2 log2 N products mod q and ONE fixed-base pass over one-coefficient rows where the point domain spends as many scalar
// multiplications on the curve.  The affine points, hence the bytes, are the same.
//
// The symbols are canonical plain residues mod q (8 x 32-bit words, fe.hip.h); the twiddles are the plain table the MAC side keeps per
// (n_total, curve) (mac_fft.hip: tws[e] = (w^e mod p_icc) mod q), taken into the Montgomery form on the way in so that the product with
// a plain symbol is plain again: two field products per butterfly, none where the twiddle is w^0 by construction (stage 1).
#pragma once
#include "client_block_pass.hip.h"
#include "mac_fft.hip.h"

namespace porla {

// T: the stages with m <= T touch only aligned runs of T consecutive symbols and run inside one block on an LDS tile (32 KiB); every
// later stage is one element-wise launch over all requests.  Mirrored as porla_amd.multiexp.CLIENT_REBUILD_TILE.
constexpr uint32_t CR_TILE_LOG = 10, CR_TILE = 1u << CR_TILE_LOG, CR_THREADS = 256;
static_assert(CR_TILE <= 4096, "a tile of T <= 4096 symbols");

// One request as the kernels see it; wt_sc: wt mod q, plain (UpdDesc's).
struct CrDesc {
    const uint8_t* block;
    const uint8_t* prf;
    uint8_t* mac_out;
    uint8_t* comp_out;
    uint32_t wt_sc[8];
};
static_assert(sizeof(CrDesc) == 64, "CrDesc: 32 bytes of pointers, 32 of wt");

// rows of the h pass per request: the 2 N differences, then comp0
__host__ __device__ __forceinline__ size_t cr_rows(uint32_t n) { return 2 * (size_t)n + 1; }

// PRF value i (16 raw bytes) as a plain residue: LE_PRF false (KZG): a big-endian 128-bit integer (compute_digest_complement); true
// (IPA): r.d[0], r.d[1] as little-endian 64-bit words (Client.hpp:435-436).  Below 2^128, hence below either group order.
template <class Q, bool LE_PRF>
__device__ __forceinline__ Fe<Q> cr_prf(const uint8_t* __restrict__ prf, size_t i) {
    const uint4 v = reinterpret_cast<const uint4*>(prf)[i];
    Fe<Q> r = fe_zero<Q>();
    if (LE_PRF) { r.v[0] = v.x; r.v[1] = v.y; r.v[2] = v.z; r.v[3] = v.w; }
    else { r.v[0] = __builtin_bswap32(v.w); r.v[1] = __builtin_bswap32(v.z); r.v[2] = __builtin_bswap32(v.y); r.v[3] = __builtin_bswap32(v.x); }
    return r;
}
// a plain residue as the big-endian scalar of a row of the h pass (both curves' one-point tables read big-endian rows)
template <class Q>
__device__ __forceinline__ void cr_store_row(uint8_t* __restrict__ row, const Fe<Q>& c) {
    uint4* q4 = reinterpret_cast<uint4*>(row);
    q4[0] = make_uint4(__builtin_bswap32(c.v[7]), __builtin_bswap32(c.v[6]), __builtin_bswap32(c.v[5]), __builtin_bswap32(c.v[4]));
    q4[1] = make_uint4(__builtin_bswap32(c.v[3]), __builtin_bswap32(c.v[2]), __builtin_bswap32(c.v[1]), __builtin_bswap32(c.v[0]));
}
// plain residue (a table twiddle, wt) times a plain symbol -> plain
template <class Q>
__device__ __forceinline__ Fe<Q> cr_mul_plain(const Fe<Q>& sym, const Fe<Q>& plain) {
    return fe_mul<Q>(sym, fe_to_mont<Q>(plain));
}

// ---- expand: blockIdx.y = the request; a lane per chunk (the coefficient row of the block pass, as k_cu_expand), then a lane per PRF
// value that enters the network: complements_U[i] = prf[1 + i] into the request's work array, and prf[0] (the block's own complement)
// as row 2 N of the request's rows of the h pass.  The 2 N new values are read by the close.
template <class Q, bool LE_PRF>
__global__ void __launch_bounds__(256)
k_cr_expand(const CrDesc* __restrict__ desc, uint32_t ncols, uint32_t n, uint8_t* __restrict__ rows, uint32_t* __restrict__ work,
            uint8_t* __restrict__ scalars) {
    const uint32_t q = blockIdx.y;
    const CrDesc& D = desc[q];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ncols) {
        cu_chunk_to_coeff(D.block, t, rows + 32 * ((size_t)q * ncols + t));
    } else if (t - ncols < n) {
        const uint32_t i = t - ncols;
        st_fe<Q>(work + 8 * ((size_t)q * n + i), cr_prf<Q, LE_PRF>(D.prf, (size_t)i + 1));
    } else if (t - ncols == n) {
        cr_store_row<Q>(scalars + 32 * ((size_t)q * cr_rows(n) + 2 * (size_t)n), cr_prf<Q, LE_PRF>(D.prf, 0));
    }
}

// butterfly (k, k + m2) of stage s on the array x (LDS tile or the work array; j = k mod m2 is the same in either):
// t = (v^j mod p_icc) x[k + m2]; x[k] = u + t; x[k + m2] = u - t, v^j = w^(j N / m2) (Client.hpp:1083-1450, oracle mac_crebuild)
template <class Q>
__device__ __forceinline__ void cr_butterfly(uint32_t* x, uint32_t b, uint32_t s, uint32_t n, const uint32_t* __restrict__ tws) {
    const uint32_t m2 = 1u << (s - 1), j = b & (m2 - 1u);
    const size_t k = ((size_t)(b >> (s - 1)) << s) + j;
    const Fe<Q> u = ld_fe<Q>(x + 8 * k);
    Fe<Q> t = ld_fe<Q>(x + 8 * (k + m2));
    if (s > 1) t = cr_mul_plain<Q>(t, ld_fe<Q>(tws + 8 * ((size_t)j * (n >> (s - 1)))));      // stage 1: every twiddle is w^0 = 1
    st_fe<Q>(x + 8 * k, fe_add<Q>(u, t));
    st_fe<Q>(x + 8 * (k + m2), fe_sub<Q>(u, t));
}

// ---- the network, stages 1 .. tile_log (2^tile_log = min(N, T)): block (x, y) carries symbols [x 2^tile_log, (x + 1) 2^tile_log) of
// request y through them on an LDS tile
template <class Q>
__global__ void __launch_bounds__(CR_THREADS)
k_cr_network(uint32_t* __restrict__ work, uint32_t n, uint32_t tile_log, const uint32_t* __restrict__ tws) {
    __shared__ __attribute__((aligned(16))) uint32_t L[8 * CR_TILE];
    const uint32_t tile = 1u << tile_log;
    uint32_t* base = work + 8 * ((size_t)blockIdx.y * n + (size_t)blockIdx.x * tile);
    for (uint32_t i = threadIdx.x; i < tile; i += CR_THREADS) st_fe<Q>(L + 8 * i, ld_fe<Q>(base + 8 * (size_t)i));
    __syncthreads();
    for (uint32_t s = 1; s <= tile_log; s++) {
        for (uint32_t b = threadIdx.x; b < tile / 2; b += CR_THREADS) cr_butterfly<Q>(L, b, s, n, tws);
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < tile; i += CR_THREADS) st_fe<Q>(base + 8 * (size_t)i, ld_fe<Q>(L + 8 * i));
}
// ---- one later stage s (m = 2^s > T), element-wise: blockIdx.y = the request, a lane per butterfly
template <class Q>
__global__ void __launch_bounds__(CR_THREADS)
k_cr_network_stage(uint32_t* __restrict__ work, uint32_t n, uint32_t s, const uint32_t* __restrict__ tws) {
    const uint32_t b = blockIdx.x * CR_THREADS + threadIdx.x;
    if (b >= n / 2) return;
    cr_butterfly<Q>(work + 8 * (size_t)blockIdx.y * n, b, s, n, tws);
}

// ---- close: blockIdx.y = the request, a lane per output g < 2 N: the scalar of out[g] as row g of the request's rows of the h pass:
// (s'_j - X_j) mod q for g = j < N, (s'_{N+j} - wt X_j) mod q for g = N + j; s' = prf[N + 1 + g] (the new ones of :586-588, X then Y)
template <class Q, bool LE_PRF>
__global__ void __launch_bounds__(256)
k_cr_close(const CrDesc* __restrict__ desc, uint32_t n, const uint32_t* __restrict__ work, uint8_t* __restrict__ scalars) {
    const uint32_t q = blockIdx.y;
    const CrDesc& D = desc[q];
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 2 * n) return;
    Fe<Q> x = ld_fe<Q>(work + 8 * ((size_t)q * n + (g & (n - 1u))));
    if (g >= n) {
        Fe<Q> wt;
#pragma unroll
        for (int i = 0; i < 8; i++) wt.v[i] = D.wt_sc[i];
        x = cr_mul_plain<Q>(x, wt);
    }
    cr_store_row<Q>(scalars + 32 * ((size_t)q * cr_rows(n) + g), fe_sub<Q>(cr_prf<Q, LE_PRF>(D.prf, (size_t)n + 1 + g), x));
}

// ---- place: blockIdx.y = the request; the 2 N affine points of the h pass to d_complements_out, 16 bytes per lane and turn, and on
// one lane MAC = block commitment (row y of the block pass) + comp0 (row 2 N), k_cu_place's addition
template <class C>
__global__ void __launch_bounds__(256)
k_cr_place(const CrDesc* __restrict__ desc, uint32_t n, const uint8_t* __restrict__ blk, const uint8_t* __restrict__ hpts) {
    using M = typename C::Fp;
    const uint32_t q = blockIdx.y;
    const CrDesc& D = desc[q];
    const uint8_t* mine = hpts + 64 * ((size_t)q * cr_rows(n));
    const uint4* src = reinterpret_cast<const uint4*>(mine);
    uint4* dst = reinterpret_cast<uint4*>(D.comp_out);
    const size_t units = 8 * (size_t)n;                                    // 2 N points of four units
    for (size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (size_t)gridDim.x * blockDim.x) dst[u] = src[u];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        XYZZ<M> a = load_affine_be_lazy<M>(blk + 64 * (size_t)q);
        const XYZZ<M> b = load_affine_be_lazy<M>(mine + 128 * (size_t)n);
        xyzz30_add_mem<M>(&a, &b, 0, 0, nullptr);
        store_affine_be<M>(D.mac_out, xyzz30_to_xyzz<M>(xyzz30_load_lazy<M>(&a)));
    }
}

}  // namespace porla

// Batched MSM: K independent MSMs of 0 .. SMALL_MAX_N pairs each over one concatenated scalar / point array, in a fixed number
// of launches per launch round, with the fold and the affine conversion on the device (porla_*_msm_batch_device, include/porla_gpu.h).
//
// One call of porla_*_msm_device costs ~0.1 ms whatever its size below a few thousand pairs: one launch, a chain of ~15 dependent
// additions, a host fold.  K of them cost K times that while the chip idles.  Here the host turns the offsets into a work list and
// every entry takes the form that suits its size:
//
//   tiny entries (<= BATCH_TINY_MAX = 64 pairs, empty ones included): k_batch_tiny -- one QUAD per pair (64 per block): the endomorphism
//       split, 33 signed 4-bit windows over a table of the multiples 1 .. 8 of the point (the ladder of mac_fft.hip.h:macq_ladder,
//       accumulator in the quad's registers, ec30.hip.h:xyzz30_dbl_quadreg / xyzz30_add_quadreg); the entry's quads then add their
//       products as a tree (log2 n levels) and its first quad writes the entry's sum.  A 1-pair entry is ~130 doublings + ~70
//       additions on four lanes.
//   larger entries: k_batch_bucket -- the blocks of k_small_msm (msm_small.hip.h) with a work list instead of gridDim: block
//       (entry, window, slice), digits and endomorphism split by small_cfg, LDS counting sort by bucket, lane sums, the bit-sliced
//       tree on quads (small_quad_adds), the last block of a window folds the slices' sums into the entry's window sums (HBM).
//       An entry gets fewer blocks than a lone k_small_msm (ceil(n / 64), at least the windows' count): a lone MSM buys latency with
//       idle lanes, a batch fills the chip with other entries instead.  When the round's entries would occupy no more than two
//       blocks per compute unit even with the lone MSM's allotment (192, 256 above 4 096 pairs), they get that.
//   k_batch_fold -- one quad per bucket entry: the Horner fold over the W x c single-bit window sums (the fold host_fold64.hpp:
//       h_fold_tree64 runs on the host for a lone MSM), accumulator in registers.  The GLV recombination needs no step of its own:
//       the second sub-scalar's points enter the buckets as phi(P) (msm_small.hip.h).
//   k_fb_finish (fixed_base.hip.h) -- XYZZ -> affine, one division-step inversion per four entries (Montgomery's trick), big-endian
//       X || Y straight into the caller's output (64 zero bytes = infinity).
//
// Same group law and the same input handling (scalars reduced mod the group order, coordinates reduced mod p as SetBytes does),
// so each output is the same group element as porla_*_msm_device's and its 64 bytes are identical.
#pragma once
#include "msm_small.hip.h"
#include "fixed_base.hip.h"
#include "quad30.hip.h"

namespace porla {

constexpr int BATCH_QUADS = 64;                     // quads per block of k_batch_tiny / k_batch_fold (256 lanes)
constexpr uint32_t BATCH_TINY_MAX = BATCH_QUADS;    // entries of up to this many pairs: k_batch_tiny (one block holds them; crossover: DESIGN.md §4)
constexpr size_t BATCH_ROUND_ENTRIES = 1u << 18;    // per launch round: entries (the round's sums: 32 MiB) ...
constexpr size_t BATCH_ROUND_PAIRS = 1u << 24;      // ... pairs (32-bit offsets inside a round) ...
constexpr uint32_t BATCH_ROUND_BLOCKS = 1u << 15;   // ... bucket blocks (their partial sums and window sums: 2 x 32 MiB) ...
constexpr uint32_t BATCH_ROUND_QUADS = 1u << 20;    // ... and quads of k_batch_tiny
constexpr uint32_t BATCH_IDLE = 0xffffffffu;        // a quad of k_batch_tiny without a pair (padding: an entry's quads share a block)

// one entry of a round's work list: its pairs [off, off + n) relative to the round's first pair; bucket entries own the bucket
// blocks [base, base + blocks) of the round (their slots of the partial sums, the window sums and the arrival counters)
struct BatchEntry {
    uint32_t off, n, base, blocks;
};

// the quad's register-form point (lane r: coordinate r) into memory form at dst; infinity = zero words.  final: the 2^256 form
template <class M>
__device__ __forceinline__ void batch_store_point(XYZZ<M>* dst, const F30<M>& c, bool inf, uint32_t r, bool final) {
    if (inf) {
        uint4* d = reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(dst) + 8 * r);
        d[0] = make_uint4(0, 0, 0, 0); d[1] = d[0];
    } else {
        xyzz30_store_coord<M>(dst, (int)r, c, final);
    }
}
// quad30.hip.h:macq_add for an operand e that may be infinity (zero words: skipped).  All four lanes together.
template <class M>
__device__ __forceinline__ void batch_add_maybe_inf(F30<M>& c, bool& inf, const XYZZ<M>* e, XYZZ<M>* slot_a, XYZZ<M>* slot_b, uint32_t r,
                                                    uint32_t lane) {
    bool z;
    (void)xyzz30_load_coord<M>(e, 2, &z);
    if (macq_quad_any(z, lane)) return;
    macq_add<M>(c, inf, e, reinterpret_cast<const uint32_t*>(e), false, slot_a, slot_b, r, lane);
}

// ---------------------------------------------------------------- tiny entries: one quad per pair
template <class M>
struct BatchTinyLds {
    struct Quad {
        XYZZ<M> tbl[8];            // (i + 1) P
        uint32_t bx[8][8];         // beta X of tbl[i]: the endomorphism's half reads its X here
    };
    Quad qd[BATCH_QUADS];
    XYZZ<M> res[BATCH_QUADS], sa[BATCH_QUADS], sb[BATCH_QUADS];
};

// tq[quad] = entry | pair << 20 (BATCH_IDLE: padding); an entry's quads are consecutive and in one block, its first (pair 0) writes
// sums[entry] in the 2^256 form.  An empty entry has one quad, which writes infinity.
template <class C>
__global__ void __launch_bounds__(4 * BATCH_QUADS)
k_batch_tiny(const uint8_t* __restrict__ scalars, const uint8_t* __restrict__ points, const BatchEntry* __restrict__ ents,
             const uint32_t* __restrict__ tq, uint32_t nq, XYZZ<typename C::Fp>* __restrict__ sums) {
    using M = typename C::Fp;
    using G = typename C::Glv;
    __shared__ BatchTinyLds<M> L;
    const uint32_t tid = threadIdx.x, q = tid >> 2, r = tid & 3u, lane = tid & 63u;
    const uint32_t gq = blockIdx.x * BATCH_QUADS + q;
    const uint32_t code = gq < nq ? tq[gq] : BATCH_IDLE;
    const bool idle = code == BATCH_IDLE;
    const uint32_t e = code & 0xfffffu, j = code >> 20;
    BatchEntry E = {0, 0, 0, 0};
    if (!idle) E = ents[e];
    typename BatchTinyLds<M>::Quad& Q = L.qd[q];
    F30<M> c;
    bool inf = true;
    if (!idle && j < E.n) {
        const size_t p = (size_t)E.off + j;
        Affine<M> a;
        load_be256(a.x.v, points + p * 64);
        load_be256(a.y.v, points + p * 64 + 32);
        fe_reduce_plain<M>(a.x.v, 6);                      // G1Affine.Unmarshal: SetBytes reduces
        fe_reduce_plain<M>(a.y.v, 6);
        uint32_t k[8];
        load_be256(k, scalars + p * 32);
        for (int t = 0; t < C::MAX_Q; t++) {               // fr.SetBytes: reduced mod the group order
            uint32_t d[8];
            uint32_t br = 0;
#pragma unroll
            for (int t2 = 0; t2 < 8; t2++) d[t2] = sbb32(k[t2], C::ORDER[t2], br);
            if (br) break;
#pragma unroll
            for (int t2 = 0; t2 < 8; t2++) k[t2] = d[t2];
        }
        if (!aff_is_inf<M>(a)) {
            // P in the register form with ZZ = ZZZ = 1 (the 2^270 form for the Montgomery field; plain residues otherwise)
            Fe<M> one = fe_zero<M>();
            one.v[0] = 1;
            F30<M> v = f30_from_fe<M>(r == 0u ? a.x : (r == 1u ? a.y : one));
            if constexpr (!M::PSEUDO_MERSENNE) v = f30_mul<M>(v, f30_const<M>(M::RR_30));
            batch_store_point<M>(&Q.tbl[0], v, false, r, false);
            macq_sync();                                   // the additions below read tbl[0]'s other coordinates
            c = v;
            // tbl[i] = (i + 1) P: one doubling, six additions of P
            xyzz30_dbl_quadreg<M>(c, r);
            batch_store_point<M>(&Q.tbl[1], c, false, r, false);
            macq_sync();
            bool tinf = false;
#pragma unroll 1
            for (int i = 2; i < 8; i++) {
                macq_add<M>(c, tinf, &Q.tbl[0], reinterpret_cast<const uint32_t*>(&Q.tbl[0]), false, &L.sa[q], &L.sb[q], r, lane);
                batch_store_point<M>(&Q.tbl[i], c, tinf, r, false);
            }
            macq_sync();
            {
                const F30<M> beta30 = f30_const<M>(G::BETA_30);
#pragma unroll 1
                for (int t = 0; t < 2; t++) {
                    const uint32_t i = r + 4u * (uint32_t)t;
                    bool z;
                    const F30<M> x = xyzz30_load_coord<M>(&Q.tbl[i], 0, &z);
                    batch_store_point<M>(reinterpret_cast<XYZZ<M>*>(&Q.bx[i][0]), f30_mul<M>(x, beta30), false, 0, false);
                }
            }
            macq_sync();
            uint32_t m0[4], m1[4];
            bool ng0, ng1;
            glv_split<G>(k, m0, ng0, m1, ng1);
#pragma unroll 1
            for (int i = 32; i >= 0; i--) {
                if (!inf) {
#pragma unroll 1
                    for (int d = 0; d < 4; d++) xyzz30_dbl_quadreg<M>(c, r);
                }
#pragma unroll 1
                for (int h = 0; h < 2; h++) {
                    const int dg = mac_signed_digit(h ? m1 : m0, i);
                    if (dg == 0) continue;
                    const uint32_t mag = (uint32_t)(dg < 0 ? -dg : dg) - 1u;
                    const XYZZ<M>* te = &Q.tbl[mag];
                    macq_add<M>(c, inf, te, h ? &Q.bx[mag][0] : reinterpret_cast<const uint32_t*>(te), (dg < 0) != (h ? ng1 : ng0),
                                &L.sa[q], &L.sb[q], r, lane);
                }
            }
        }
    }
    // the entry's sum as a tree over its quads (pairs 0 .. n - 1 sit on consecutive quads of this block): at level h the quads of
    // pair j = 0 mod 2h add the partial sum h quads further on -- log2(n) dependent additions instead of n - 1
    batch_store_point<M>(&L.res[q], c, inf, r, false);
    const uint32_t cnt = idle ? 0u : E.n;
#pragma unroll 1
    for (uint32_t h = 1; h < (uint32_t)BATCH_QUADS; h <<= 1) {
        __syncthreads();                                   // (every lane of the block passes every level's barrier)
        if (!idle && (j & (2 * h - 1)) == 0 && j + h < cnt) {
            batch_add_maybe_inf<M>(c, inf, &L.res[q + h], &L.sa[q], &L.sb[q], r, lane);
            batch_store_point<M>(&L.res[q], c, inf, r, false);
        }
    }
    if (idle || j != 0) return;
    batch_store_point<M>(sums + e, c, inf, r, true);
}

// ---------------------------------------------------------------- larger entries: the blocks of k_small_msm from a work list
// blk[block] = entry.  Block b - base of entry e is block (w, s) of e's shape (small_cfg over e's own allotment of blocks); the last
// block of window w to arrive writes its c sums (S, M_0 .. M_(c-2), memory form) to fin[base * SMALL_MAX_C + w * c + k].  Block 0 of
// the entry writes the shape (W | c << 8) to shape[e].  counters[base .. base + W) start at zero (the host clears them per round).
template <class C>
__global__ void __launch_bounds__(SMALL_THREADS) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_batch_bucket(const uint8_t* __restrict__ scalars_r, const uint8_t* __restrict__ points_r, const BatchEntry* __restrict__ ents,
               const uint32_t* __restrict__ blk, int c_flags, XYZZ<typename C::Fp>* __restrict__ part, uint32_t* __restrict__ counters,
               XYZZ<typename C::Fp>* __restrict__ fin, uint32_t* __restrict__ shape) {
    using M = typename C::Fp;
    __shared__ uint32_t ent[SMALL_MAX_SUB];                    // sorted entries: sub-scalar index | sign << 31
    __shared__ XYZZ<M> pts[SMALL_THREADS];                     // first the unsorted digits (uint32 view), then the lane sums
    __shared__ XYZZ<M> bk[SMALL_MAX_B];                        // bucket sums
    __shared__ XYZZ<M> slev[SMALL_MAX_B];                      // S levels of the tree: B/2 + B/4 + ... + 1
    __shared__ XYZZ<M> mlev[SMALL_MAX_B / 2 + 2];              // M slots, two ping-pong halves
    __shared__ uint32_t hist[SMALL_MAX_B], cursor[SMALL_MAX_B];
    __shared__ uint32_t orw[8], pat[8];
    __shared__ uint32_t last_flag;
    const uint32_t tid = threadIdx.x;
    uint32_t* raw = reinterpret_cast<uint32_t*>(pts);
    const uint32_t eidx = blk[blockIdx.x];
    const BatchEntry E = ents[eidx];
    const uint32_t bx = blockIdx.x - E.base, n = E.n;
    const uint8_t* __restrict__ scalars = scalars_r + (size_t)E.off * 32;
    const uint8_t* __restrict__ points = points_r + (size_t)E.off * 64;

    // ---- 0. bit length of the entry's scalars (every block for itself)
    if (tid < 8) orw[tid] = 0;
    if (tid < SMALL_MAX_B) hist[tid] = 0;
    __syncthreads();
    {
        uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t i = tid; i < n; i += 4 * SMALL_THREADS) {
            uint32_t t[4][8];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t j = i + (uint32_t)u * SMALL_THREADS;
                load_be256(t[u], scalars + (size_t)(j < n ? j : i) * 32);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int k = 0; k < 8; k++) acc[k] |= t[u][k];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint32_t v = acc[k];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v |= __shfl_xor(v, m, 64);
            if ((tid & 63) == 0 && v) atomicOr(&orw[k], v);
        }
    }
    __syncthreads();
    int used = 0;
#pragma unroll
    for (int k = 7; k >= 0; k--)
        if (used == 0 && orw[k]) used = 32 * k + (32 - __clz(orw[k]));
    const SmallCfg g = small_cfg<C>(n, used, c_flags, (int)E.blocks);
    // (the host sizes every allotment so that neither bound is ever met: W <= blocks, a slice fits the LDS)
    if (g.W > (int)E.blocks || (g.n_sub + (uint32_t)g.S - 1) / (uint32_t)g.S > SMALL_MAX_SUB) return;
    if (bx == 0 && tid == 0) shape[eidx] = (uint32_t)g.W | ((uint32_t)g.c << 8);
    if (bx >= (uint32_t)(g.W * g.S)) return;
    const uint32_t w = bx / g.S, s = bx % g.S;
    const int c = g.c;
    const uint32_t mask = (1u << c) - 1;
    const uint32_t Bfull = 1u << (c - 1);
    const int cw = (w + 1 == (uint32_t)g.W) ? g.L + 1 - c * (g.W - 1) : c;      // 1 .. c
    const uint32_t B = 1u << (cw - 1);
    const bool reduce = used >= 250;
    const uint32_t SUBS = g.glv ? 2u : 1u;
    const uint32_t i0 = (uint32_t)((uint64_t)s * n / g.S), i1 = (uint32_t)((uint64_t)(s + 1) * n / g.S);

    const uint32_t wc = w * (uint32_t)c;
    if (tid < 8) {
        uint32_t v = 0;
        for (uint32_t b = (uint32_t)c - 1 - (32 * tid) % (uint32_t)c; b < 32; b += (uint32_t)c) v |= 1u << b;
        pat[tid] = v;
    }
    __syncthreads();
    // ---- 1. digits of window w for the slice, unsorted into raw[], histogram by bucket (as k_small_msm)
    for (uint32_t i = i0 + tid; i < i1; i += SMALL_THREADS) {
        uint32_t k[8];
        load_be256(k, scalars + (size_t)i * 32);
        if (reduce) {
            for (int q = 0; q < C::MAX_Q; q++) {
                uint32_t d[8];
                uint32_t br = 0;
#pragma unroll
                for (int q2 = 0; q2 < 8; q2++) d[q2] = sbb32(k[q2], C::ORDER[q2], br);
                if (br) break;
#pragma unroll
                for (int q2 = 0; q2 < 8; q2++) k[q2] = d[q2];
            }
        }
        uint32_t sub[2][8];
        uint32_t sneg[2] = {0, 0};
        if (g.glv) {
            uint32_t m1[4], m2[4];
            bool n1, n2;
            glv_split<typename C::Glv>(k, m1, n1, m2, n2);
#pragma unroll
            for (int q = 0; q < 4; q++) { sub[0][q] = m1[q]; sub[1][q] = m2[q]; sub[0][4 + q] = 0; sub[1][4 + q] = 0; }
            sneg[0] = n1 ? 1u : 0u; sneg[1] = n2 ? 1u : 0u;
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) { sub[0][q] = k[q]; sub[1][q] = 0; }
        }
#pragma unroll
        for (uint32_t e = 0; e < 2; e++) {
            if (e >= SUBS) break;
            bool gt = false, eq = true;
#pragma unroll
            for (int q = 7; q >= 0; q--) {
                const uint32_t below = wc > 32u * q ? wc - 32u * q : 0u;
                const uint32_t m = below >= 32u ? 0xffffffffu : ((1u << below) - 1u);
                const uint32_t a = sub[e][q] & m, b = pat[q] & m;
                gt = eq ? (a > b) : gt;
                eq = eq && (a == b);
            }
            uint32_t rawd = gt ? 1u : 0u;
            if (wc < 256u) {
                const uint32_t limb = wc >> 5, sh = wc & 31u;
                uint32_t a = 0, b = 0;
#pragma unroll
                for (uint32_t q = 0; q < 8; q++) {
                    a = (q == limb) ? sub[e][q] : a;
                    b = (q == limb + 1) ? sub[e][q] : b;
                }
                rawd += (uint32_t)((((uint64_t)b << 32) | a) >> sh) & mask;
            }
            uint32_t mag = rawd, dneg = 0;
            if (rawd > Bfull) { mag = (1u << c) - rawd; dneg = 1; }
            const uint32_t j = (i - i0) * SUBS + e;
            uint32_t packed = 0xffffffffu;
            if (mag) {
                packed = j | ((dneg ^ sneg[e]) << 13) | ((mag - 1) << 14);
                atomicAdd(&hist[mag - 1], 1u);
            }
            raw[j] = packed;
        }
    }
    __syncthreads();
    if (tid < SMALL_MAX_B) cursor[tid] = tid < B ? hist[tid] : 0;
    __syncthreads();
    for (uint32_t d = 1; d < B; d <<= 1) {
        uint32_t v = 0;
        if (tid < B && tid >= d) v = cursor[tid - d];
        __syncthreads();
        if (tid < B) cursor[tid] += v;
        __syncthreads();
    }
    if (tid < B) cursor[tid] -= hist[tid];
    __syncthreads();
    const uint32_t T = SMALL_THREADS / B;
    const uint32_t my_b = tid / T, my_t = tid % T;
    const uint32_t my_start = cursor[my_b], my_cnt = hist[my_b];
    __syncthreads();
    for (uint32_t j = tid; j < (i1 - i0) * SUBS; j += SMALL_THREADS) {
        const uint32_t p = raw[j];
        if (p != 0xffffffffu) {
            const uint32_t pos = atomicAdd(&cursor[p >> 14], 1u);
            ent[pos] = (i0 * SUBS + (p & 0x1fffu)) | (((p >> 13) & 1u) << 31);
        }
    }
    __syncthreads();

    // ---- 2. accumulate: lane (bucket, t) takes entries t, t + T, ... of its bucket
    {
        XYZZ30<M> acc;
        acc.inf = true;
        bool flip = false;
        uint32_t en = 0;
        Affine<M> nx;
        if (my_t < my_cnt) {
            en = ent[my_start + my_t];
            const uint32_t i = g.glv ? (en & 0x7fffffffu) >> 1 : (en & 0x7fffffffu);
            load_be256(nx.x.v, points + (size_t)i * 64);
            load_be256(nx.y.v, points + (size_t)i * 64 + 32);
        }
        for (uint32_t e = my_t; e < my_cnt; e += T) {
            const uint32_t cur = en;
            Affine<M> a = nx;
            if (e + T < my_cnt) {
                en = ent[my_start + e + T];
                const uint32_t i = g.glv ? (en & 0x7fffffffu) >> 1 : (en & 0x7fffffffu);
                load_be256(nx.x.v, points + (size_t)i * 64);
                load_be256(nx.y.v, points + (size_t)i * 64 + 32);
            }
            fe_reduce_plain<M>(a.x.v, 6);
            fe_reduce_plain<M>(a.y.v, 6);
            if (aff_is_inf<M>(a)) continue;
            a = aff_neg_if<M>(a, xyzz30_flip_neg<M>((cur >> 31) != 0, flip));
            F30<M> ax = f30_from_fe<M>(a.x), ay = f30_from_fe<M>(a.y);
            if constexpr (!M::PSEUDO_MERSENNE) {
                ax = f30_mul<M>(ax, f30_const<M>(M::RR_30));
                ay = f30_mul<M>(ay, f30_const<M>(M::RR_30));
            }
            if (g.glv && (cur & 1u)) ax = f30_mul<M>(ax, f30_const<M>(C::Glv::BETA_30));
            xyzz30_madd_flip<M>(acc, flip, ax, ay);
        }
        xyzz30_flip_finish<M>(acc, flip);
        xyzz30_store_lazy<M>(&pts[tid], acc);
    }
    __syncthreads();

    // ---- 3a. fold the T lane sums of every bucket
    for (uint32_t h = 1; h < T; h <<= 1) {
        const bool last = (h << 1) == T;
        small_quad_adds<M>(SMALL_THREADS / (2 * h), [&](uint32_t t, const XYZZ<M>*& pa, const XYZZ<M>*& pb, XYZZ<M>*& out) {
            pa = &pts[t * 2 * h]; pb = pa + h;
            out = last ? &bk[t] : &pts[t * 2 * h];
        });
        __syncthreads();
    }
    // ---- 3b. bucket reduction: the bit-sliced tree on the window's B buckets, in LDS
    const uint32_t nlev = (uint32_t)(cw - 1);
    auto s_level = [&](uint32_t l) { return slev + (B - (B >> l)); };
    auto m_half = [&](uint32_t h) { return mlev + (h & 1u) * (SMALL_MAX_B / 4 + 1); };
    for (uint32_t l = 0; l < nlev; l++) {
        const uint32_t nl = B >> (l + 1);
        const XYZZ<M>* sp = l ? s_level(l - 1) : bk;
        const XYZZ<M>* sp2 = l >= 2 ? s_level(l - 2) : bk;
        const XYZZ<M>* mp = m_half(l + 1);
        XYZZ<M>* so = s_level(l);
        XYZZ<M>* mo = m_half(l);
        small_quad_adds<M>((l + 1) * nl, [&](uint32_t t, const XYZZ<M>*& pa, const XYZZ<M>*& pb, XYZZ<M>*& out) {
            const uint32_t sl = t / nl, i = t % nl;
            if (sl == l) { pa = sp + 2 * i; pb = pa + 1; out = so + i; }
            else if (sl + 1 == l) { pa = sp2 + 4 * i + 1; pb = pa + 2; out = mo + sl * nl + i; }
            else { pa = mp + sl * 2 * nl + 2 * i; pb = pa + 1; out = mo + sl * nl + i; }
        });
        __syncthreads();
    }
    XYZZ<M>* mine = part + (size_t)(E.base + bx) * SMALL_MAX_C;
    if (tid < (uint32_t)c * 8) {
        const uint32_t kk = tid >> 3, q = tid & 7;
        const XYZZ<M>* src = nullptr;
        if (kk == 0) src = nlev ? s_level(nlev - 1) : bk;
        else if (kk > nlev) src = nullptr;
        else if (kk == nlev) src = (nlev >= 2 ? s_level(nlev - 2) : bk) + 1;
        else src = m_half(nlev - 1) + (kk - 1);
        reinterpret_cast<uint4*>(mine + kk)[q] = src ? reinterpret_cast<const uint4*>(src)[q] : make_uint4(0, 0, 0, 0);
    }
    // ---- 4. the last block of the window folds the slices into the entry's window sums
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const uint32_t old = atomicAdd(&counters[E.base + w], 1u);
        last_flag = (old == (uint32_t)g.S - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last_flag) return;
    __threadfence();
    {
        const uint4* src = reinterpret_cast<const uint4*>(part + (size_t)(E.base + w * g.S) * SMALL_MAX_C);
        uint4* dst = reinterpret_cast<uint4*>(pts);
        const uint32_t total = (uint32_t)g.S * (uint32_t)c * 8;
        for (uint32_t x = tid; x < total; x += SMALL_THREADS) {
            const uint32_t e = x >> 3, q = x & 7;
            dst[x] = src[(size_t)((e / (uint32_t)c) * SMALL_MAX_C + e % (uint32_t)c) * 8 + q];
        }
    }
    __syncthreads();
    for (uint32_t cnt = (uint32_t)g.S; cnt > 1;) {
        const uint32_t half = (cnt + 1) / 2, pairs = cnt - half;
        small_quad_adds<M>(pairs * (uint32_t)c, [&](uint32_t t, const XYZZ<M>*& pa, const XYZZ<M>*& pb, XYZZ<M>*& out) {
            const uint32_t sl = t / (uint32_t)c, kk = t % (uint32_t)c;
            pa = &pts[sl * c + kk]; pb = &pts[(sl + half) * c + kk];
            out = &pts[sl * c + kk];
        });
        __syncthreads();
        cnt = half;
    }
    if (tid < (uint32_t)c * 8) {
        const uint32_t kk = tid >> 3, q = tid & 7;
        reinterpret_cast<uint4*>(fin + (size_t)E.base * SMALL_MAX_C + w * (uint32_t)c + kk)[q] = reinterpret_cast<const uint4*>(&pts[kk])[q];
    }
}

// ---------------------------------------------------------------- the window fold of the bucket entries: one quad per entry
// fold[i] = entry; its W x c window sums at fin[base * SMALL_MAX_C ..] (memory form), the sum goes to sums[entry] (2^256 form).
// The Horner fold of host_fold64.hpp:h_fold_tree64, in the same order.
template <class C>
__global__ void __launch_bounds__(4 * BATCH_QUADS)
k_batch_fold(const BatchEntry* __restrict__ ents, const uint32_t* __restrict__ fold, uint32_t nf, const XYZZ<typename C::Fp>* __restrict__ fin,
             const uint32_t* __restrict__ shape, XYZZ<typename C::Fp>* __restrict__ sums) {
    using M = typename C::Fp;
    __shared__ XYZZ<M> sa[BATCH_QUADS], sb[BATCH_QUADS];
    const uint32_t tid = threadIdx.x, q = tid >> 2, r = tid & 3u, lane = tid & 63u;
    const uint32_t i = blockIdx.x * BATCH_QUADS + q;
    if (i >= nf) return;                                     // whole quads leave together
    const uint32_t e = fold[i];
    const uint32_t sh = shape[e];
    int W = (int)(sh & 0xffu);
    const int c = (int)((sh >> 8) & 0xffu);
    const BatchEntry E = ents[e];
    if (c < 1 || c > SMALL_MAX_C || W > (int)E.blocks) W = 0;          // (never: the bucket kernel writes a shape inside its allotment)
    const XYZZ<M>* f0 = fin + (size_t)E.base * SMALL_MAX_C;
    F30<M> acc;
    bool inf = true;
#pragma unroll 1
    for (int w = W - 1; w >= 0; w--) {
        const XYZZ<M>* f = f0 + (size_t)w * c;
        if (!inf) xyzz30_dbl_quadreg<M>(acc, r);             // bit c-1 of the bucket index does not exist
#pragma unroll 1
        for (int k = c - 2; k >= 0; k--) {
            if (!inf) xyzz30_dbl_quadreg<M>(acc, r);
            batch_add_maybe_inf<M>(acc, inf, f + 1 + k, &sa[q], &sb[q], r, lane);
        }
        batch_add_maybe_inf<M>(acc, inf, f, &sa[q], &sb[q], r, lane);
    }
    batch_store_point<M>(sums + e, acc, inf, r, true);
}

}  // namespace porla

// Host helpers shared by the ICC data encode (icc.hip), the MAC-side encode (mac_fft.hip) and the batched calls built on them.
#pragma once
#include "host_curve.hpp"
#include "icc.hip.h"
#include "../../include/porla_gpu.h"

namespace porla {

inline int ilog2u(size_t n) { int l = 0; while (n >>= 1) l++; return l; }
inline uint64_t rev_bits(uint64_t x, int n) { uint64_t r = 0; for (int i = 0; i < n; i++) { r = (r << 1) | (x & 1); x >>= 1; } return r; }

// w = GENERATOR^((p_icc - 1)/(2N)) mod p_icc (Server.hpp:214-216), Montgomery form
inline Fe<IccFp> icc_root(size_t n) {
    Fe<IccFp> g;
    for (int i = 0; i < 8; i++) g.v[i] = IccGen::G[i];
    g = fe_to_mont<IccFp>(g);
    // (p-1)/(2N) = 207 * 2^(247 - log2 N)
    int sh = 247 - ilog2u(n);
    uint32_t e[8] = {0};
    uint64_t v = 207;
    int limb = sh >> 5, off = sh & 31;
    uint64_t lo = v << off;
    e[limb] = (uint32_t)lo;
    if (limb + 1 < 8) e[limb + 1] = (uint32_t)(lo >> 32);
    return h_fe_pow<IccFp>(g, e);
}


// wt = w^reverse_bits(write_step % N, height-1) mod p_icc (Server.hpp:1494), Montgomery form mod p_icc
inline Fe<IccFp> icc_wt(size_t n, unsigned long long write_step) {
    const int logn = ilog2u(n);
    const int height = logn + 1;
    uint64_t ex = rev_bits(write_step % n, height - 1);
    uint32_t e[8] = {(uint32_t)ex, (uint32_t)(ex >> 32), 0, 0, 0, 0, 0, 0};
    return h_fe_pow<IccFp>(icc_root(n), e);
}

// a group as the ICC code sees it: Q = the CRT partner of p_icc (the group's order), id = the `curve` argument of the C ABI
template <class C> struct IccCurve;
template <> struct IccCurve<Bn254G1> { using Q = IccBn254Fr; static constexpr int id = 0; };
template <> struct IccCurve<Secp256k1G> { using Q = IccSecp256k1Fn; static constexpr int id = 1; };

// The passes of the data network over n = 2^logn rows of ncols symbols: ceil(logn / (ICC_TILE_LOG - 1)) passes of (almost) equal
// stage counts -- a tile keeps two columns of a row side by side, so 2^9 rows are one pass, 2^10 .. 2^18 two, beyond that three.
// Pass z runs stages s .. s + ns - 1 on tiles of 2^ns rows x 2^cc_log columns = ICC_TILE_ELEMS symbols, no wider than the row; its
// grid is col_tiles * (n >> ns) blocks.
struct IccPass { int s, ns, cc_log; size_t col_tiles; };
constexpr int ICC_MAX_PASSES = 8;
inline int icc_pass_plan(int logn, size_t ncols, IccPass out[ICC_MAX_PASSES]) {
    constexpr int max_ns = ICC_TILE_LOG - 1;
    const int passes = (logn + max_ns - 1) / max_ns;
    int s = 1;
    for (int pz = 0; pz < passes; pz++) {
        const int ns = (logn - (s - 1) + (passes - pz) - 1) / (passes - pz);
        int cc_log = ICC_TILE_LOG - ns;
        while (cc_log > 0 && ((size_t)1 << (cc_log - 1)) >= ncols) cc_log--;
        out[pz] = IccPass{s, ns, cc_log, (ncols + ((size_t)1 << cc_log) - 1) >> cc_log};
        s += ns;
    }
    return passes;
}

// icc_decode.hip: porla_icc_decode_batch_device's body in the EXACT form for a caller that has made the refusals itself (the batched
// retrieval): the decode's workspace under its lock and fence, every launch on `stream`
int icc_decode_exact_enqueue(const porla_icc_decode_req* reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int curve,
                             hipStream_t stream);
// ... and in any of the three forms (the aligned retrieval: the residue forms carry the requests' d_write_steps through)
int icc_decode_form_enqueue(const porla_icc_decode_req* reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int curve, int form,
                            hipStream_t stream);
// ... and levels of UNEQUAL sizes (porla_icc_decode_ragged_batch_device's body; the file extraction): one upload, one lock, fence and
// table lease, launches by the pass classes present.  n_rows of every request: a power of two, 2 .. n_total
int icc_decode_ragged_enqueue(const porla_icc_decode_ragged_req* reqs, size_t k, size_t n_cols, size_t n_total, int curve, int form,
                              hipStream_t stream);
// ... and levels of ONE row in the form RESIDUE64 (below the decode's smallest level: level 0's Y row of the file extraction): d_out =
// the row's symbols times wt^-1 mod p_icc, canonical; d_write_steps points to the row's one write step, d_bad is not read
int icc_decode_row0_enqueue(const porla_icc_decode_req* reqs, size_t k, size_t n_cols, size_t n_total, int curve, hipStream_t stream);

}  // namespace porla

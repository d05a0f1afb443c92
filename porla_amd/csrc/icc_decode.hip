// The batched ICC decode (include/porla_gpu.h: porla_icc_decode_batch_device / porla_icc_decode_host): the coded rows of K levels
// back to their blocks in ONE asynchronous call.  Kernels and arithmetic: icc_decode.hip.h.  Every step is on the caller's stream
// and the launch sequence depends on n_rows, never on K:
//
//   upload          one copy of the requests (the kernels read them as they are: IcdDesc)
//   k_icd_clear     EXACT: the counters of the requests that have one
//   k_icd_exact /   ceil(log2 n_rows / 9) passes over 1 024-symbol tiles, the encode's plan in reverse order, grid.y = request, under
//   k_icd_residue   the data side's table lease; the first reads the rows, the last writes the blocks; between them the residue
//                   planes travel through this workspace
//
// porla_icc_decode_ragged_batch_device, further down, is the same decode for levels of unequal sizes: n_rows per request, launches by
// the pass classes present (kernels: icc_decode_ragged.hip.h).
#include "batch_host.hpp"
#include "icc_decode.hip.h"
#include "icc_decode_ragged.hip.h"
#include "icc_host.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>

namespace porla {

struct IccDecodeWs {
    std::mutex mu;
    int device = -1;
    Buf list, planes;
    Buf io_rows, io_out, io_steps, io_bad;     // the host form's device images
    PinnedList h_list;
    UseFence fence;
    IcdScale rag_scales[2][ICD_RAG_MAX_LOG + 1];   // the ragged call's n_rows^-1 table per curve, made on first use
    bool rag_scales_made[2] = {false, false};
};
static PerDevice<IccDecodeWs> g_icd_ws;

static const char* const ICD_WHO = "porla_icc_decode_batch_device";

static inline size_t icd_symbol_bytes(int form) { return form == PORLA_ICC_DECODE_RESIDUE32 ? 32 : 64; }

// the refusals that concern the shape of the call
static int icd_check_shape(const char* who, size_t n_rows, size_t n_cols, size_t n_total, int curve, int form) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (int rc = check_n_total(who, n_total, 16)) return rc;
    if (n_rows < 2 || (n_rows & (n_rows - 1)) != 0 || n_rows > n_total) return bad("n_rows must be a power of two, 2 .. n_total");
    if (n_cols == 0) return bad("n_cols is 0");
    if (curve != 0 && curve != 1) return bad("curve must be 0 (BN254 / KZG) or 1 (secp256k1 / IPA)");
    if (form != PORLA_ICC_DECODE_EXACT && form != PORLA_ICC_DECODE_RESIDUE64 && form != PORLA_ICC_DECODE_RESIDUE32)
        return bad("form must be PORLA_ICC_DECODE_EXACT, _RESIDUE64 or _RESIDUE32");
    size_t t;
    if (!mul_ok(n_rows, n_cols, &t) || !mul_ok(t, 64, &t) || !mul_ok(t, 2, &t))
        return bad("a byte size overflows: n_rows * n_cols symbols do not fit a buffer");
    if (n_cols > 0xffffu) return bad("n_cols above 65535");
    return PORLA_OK;
}

// the byte ranges of a call's requests, for the overlap rule
struct IcdRange { uintptr_t lo, hi; bool out; };

// the refusals that concern ONE request of n_rows rows (`at`: "request a: "), and its ranges
static int icd_check_request(const char* who, const std::string& at, const void* d_rows, const void* d_out, const unsigned long long* d_write_steps,
                             const unsigned int* d_bad, size_t n_rows, size_t n_cols, int form, std::vector<IcdRange>& ranges) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    const size_t symbols = n_rows * n_cols;
    const size_t in_b = symbols * icd_symbol_bytes(form), out_b = symbols * 32;
    if (!d_rows || !d_out) return bad(at + "a NULL d_rows or d_out");
    if (((uintptr_t)d_rows | (uintptr_t)d_out) & 15u) return bad(at + "d_rows or d_out is not 16-byte aligned");
    if ((uintptr_t)d_write_steps & 7u) return bad(at + "d_write_steps is not 8-byte aligned");
    if ((uintptr_t)d_bad & 3u) return bad(at + "d_bad is not 4-byte aligned");
    if (d_write_steps && form == PORLA_ICC_DECODE_EXACT) return bad(at + "d_write_steps with PORLA_ICC_DECODE_EXACT: the unscale is the residue forms'");
    if (d_bad && form != PORLA_ICC_DECODE_EXACT) return bad(at + "d_bad with a residue form: only PORLA_ICC_DECODE_EXACT counts");
    if ((uintptr_t)d_rows + in_b < (uintptr_t)d_rows || (uintptr_t)d_out + out_b < (uintptr_t)d_out)
        return bad(at + "a byte size overflows: a buffer wraps around the address space");
    ranges.push_back(IcdRange{(uintptr_t)d_rows, (uintptr_t)d_rows + in_b, false});
    ranges.push_back(IcdRange{(uintptr_t)d_out, (uintptr_t)d_out + out_b, true});
    if (d_write_steps) ranges.push_back(IcdRange{(uintptr_t)d_write_steps, (uintptr_t)d_write_steps + n_rows * 8, false});
    if (d_bad) ranges.push_back(IcdRange{(uintptr_t)d_bad, (uintptr_t)d_bad + 4, true});
    return PORLA_OK;
}

// an output may overlap nothing, inputs may be shared: sorted by start, an output must begin at or after the end of everything
// before it and an input at or after the end of every output before it
static int icd_check_overlap(const char* who, std::vector<IcdRange>& ranges) {
    std::sort(ranges.begin(), ranges.end(), [](const IcdRange& x, const IcdRange& y) { return x.lo < y.lo; });
    uintptr_t end_any = 0, end_out = 0;
    for (const IcdRange& r : ranges) {
        if (r.lo < (r.out ? end_any : end_out))
            return bad_arg(who, "an output (d_out or d_bad) overlaps an input or output of this call: outputs must be disjoint from everything");
        end_any = std::max(end_any, r.hi);
        if (r.out) end_out = std::max(end_out, r.hi);
    }
    return PORLA_OK;
}

// the checks made before the device is touched
static int icd_check(const porla_icc_decode_req* reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int curve, int form) {
    auto bad = [&](const std::string& what) { return bad_arg(ICD_WHO, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = icd_check_shape(ICD_WHO, n_rows, n_cols, n_total, curve, form)) return rc;
    if (int rc = check_request_count(ICD_WHO, k)) return rc;
    size_t t;
    if (k && (!mul_ok(n_rows * n_cols * 2 * ICC30_PLANE_WORDS * 4, k, &t)))
        return bad("a byte size overflows: the residue planes of k requests do not fit a buffer");
    std::vector<IcdRange> ranges;
    ranges.reserve(4 * k);
    for (size_t a = 0; a < k; a++) {
        const porla_icc_decode_req& R = reqs[a];
        if (int rc = icd_check_request(ICD_WHO, "request " + std::to_string(a) + ": ", R.d_rows, R.d_out, R.d_write_steps, R.d_bad, n_rows, n_cols,
                                       form, ranges))
            return rc;
    }
    return icd_check_overlap(ICD_WHO, ranges);
}

// 2^e mod the modulus of M as a plain integer (e >= 0): e doublings of 1
template <class M>
static void icd_pow2(int e, uint32_t out[8]) {
    Fe<M> x = fe_zero<M>();
    x.v[0] = 1;
    for (int i = 0; i < e; i++) x = fe_add<M>(x, x);
    for (int k = 0; k < 8; k++) out[k] = x.v[k];
}

// ws->mu held, ws->fence entered; arguments checked
template <class Q>
static int icd_enqueue(IccDecodeWs* ws, int curve, const porla_icc_decode_req* reqs, size_t k, size_t n, size_t ncols, size_t n_total, int form,
                       hipStream_t stream) {
    int rc;
    const int logn = ilog2u(n);
    const bool exact = form == PORLA_ICC_DECODE_EXACT;
    IccPass plan[ICC_MAX_PASSES];
    const int passes = icc_pass_plan(logn, ncols, plan);
    const size_t plane_words = n * ncols * ICC30_PLANE_WORDS;
    const size_t desc_b = k * sizeof(IcdDesc);
    static_assert(sizeof(IcdDesc) == sizeof(porla_icc_decode_req), "the requests are uploaded as they are");
    if ((rc = ws->h_list.stage(desc_b))) return rc;
    if ((rc = ws->list.ensure(desc_b))) return rc;
    if (passes > 1 && (rc = ws->planes.ensure(k * (exact ? 2 : 1) * plane_words * 4))) return rc;
    memcpy(ws->h_list.h, reqs, desc_b);
    if ((rc = ws->h_list.send(ws->list.p, desc_b, stream))) return rc;
    const IcdDesc* d_desc = (const IcdDesc*)ws->list.p;
    IcdScale sc;
    icd_pow2<IccFp>(270 - logn, sc.p);
    icd_pow2<Q>(270 - logn, sc.q);
    if (exact) {
        hipLaunchKernelGGL(k_icd_clear, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, stream, d_desc, (uint32_t)k);
        PORLA_HIP(hipGetLastError());
    }
    const uint32_t *twp = nullptr, *twqi = nullptr;
    if ((rc = icc_decode_tables_acquire(curve, n_total, exact, stream, &twp, &twqi))) return rc;
    uint32_t* planes = (uint32_t*)ws->planes.p;
    for (int pz = passes - 1; pz >= 0; pz--) {
        const int s = plan[pz].s, ns = plan[pz].ns, cc_log = plan[pz].cc_log;
        const dim3 grid((unsigned)(plan[pz].col_tiles * (n >> ns)), (unsigned)k);
        const dim3 block(ICC30_SPLIT_THREADS);
        const bool first = pz == passes - 1, last = pz == 0;
        ProfScope ps("icc_decode", stream);
#define PORLA_ICD_EXACT(F, L)                                                                                                       \
    hipLaunchKernelGGL((k_icd_exact<Q, F, L>), grid, block, 0, stream, d_desc, planes, plane_words, twp, twqi, (uint32_t)n_total,   \
                       (uint32_t)n, (uint32_t)ncols, s, ns, cc_log, sc)
#define PORLA_ICD_RESIDUE(S, L)                                                                                                     \
    hipLaunchKernelGGL((k_icd_residue<S, L>), grid, block, 0, stream, d_desc, planes, plane_words, twp, (uint32_t)n_total,          \
                       ilog2u(n_total), (uint32_t)n, (uint32_t)ncols, s, ns, cc_log, sc)
        if (exact) {
            if (first && last) PORLA_ICD_EXACT(true, true);
            else if (first) PORLA_ICD_EXACT(true, false);
            else if (last) PORLA_ICD_EXACT(false, true);
            else PORLA_ICD_EXACT(false, false);
        } else if (!first) {
            if (last) PORLA_ICD_RESIDUE(ICD_WORK, true);
            else PORLA_ICD_RESIDUE(ICD_WORK, false);
        } else if (form == PORLA_ICC_DECODE_RESIDUE64) {
            if (last) PORLA_ICD_RESIDUE(ICD_ROWS64, true);
            else PORLA_ICD_RESIDUE(ICD_ROWS64, false);
        } else {
            if (last) PORLA_ICD_RESIDUE(ICD_ROWS32, true);
            else PORLA_ICD_RESIDUE(ICD_ROWS32, false);
        }
#undef PORLA_ICD_EXACT
#undef PORLA_ICD_RESIDUE
    }
    if (hipGetLastError() != hipSuccess) { set_last_error("porla: ICC decode batch: a launch failed"); rc = PORLA_ERR_HIP; }
    const int r1 = icc_mix_tables_release(stream);
    return rc ? rc : r1;
}

static int icd_run(IccDecodeWs* ws, const porla_icc_decode_req* reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int curve, int form,
                   hipStream_t stream) {
    return curve == 0 ? icd_enqueue<IccBn254Fr>(ws, 0, reqs, k, n_rows, n_cols, n_total, form, stream)
                      : icd_enqueue<IccSecp256k1Fn>(ws, 1, reqs, k, n_rows, n_cols, n_total, form, stream);
}

int icc_decode_form_enqueue(const porla_icc_decode_req* reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int curve, int form,
                            hipStream_t stream) {
    IccDecodeWs* ws = nullptr;
    if (int rc = g_icd_ws.get(&ws)) return rc;
    return FencedCall(ws, stream).run([&] { return icd_run(ws, reqs, k, n_rows, n_cols, n_total, curve, form, stream); });
}
// levels of ONE row in the form RESIDUE64: k_icd_row0 under the workspace's lock and fence and the data side's table lease
int icc_decode_row0_enqueue(const porla_icc_decode_req* reqs, size_t k, size_t n_cols, size_t n_total, int curve, hipStream_t stream) {
    IccDecodeWs* ws = nullptr;
    if (int rc = g_icd_ws.get(&ws)) return rc;
    return FencedCall(ws, stream).run([&] {
        int rc;
        const size_t desc_b = k * sizeof(IcdDesc);
        if ((rc = ws->h_list.stage(desc_b))) return rc;
        if ((rc = ws->list.ensure(desc_b))) return rc;
        memcpy(ws->h_list.h, reqs, desc_b);
        if ((rc = ws->h_list.send(ws->list.p, desc_b, stream))) return rc;
        const uint32_t *twp = nullptr, *twqi = nullptr;
        if ((rc = icc_decode_tables_acquire(curve, n_total, false, stream, &twp, &twqi))) return rc;
        {
            ProfScope ps("icc_decode_row0", stream);
            hipLaunchKernelGGL(k_icd_row0, dim3((unsigned)((n_cols + 255) / 256), (unsigned)k), dim3(256), 0, stream, (const IcdDesc*)ws->list.p,
                               twp, (uint32_t)n_total, ilog2u(n_total), (uint32_t)n_cols);
        }
        if (hipGetLastError() != hipSuccess) { set_last_error("porla: ICC decode of one-row levels: a launch failed"); rc = PORLA_ERR_HIP; }
        const int r1 = icc_mix_tables_release(stream);
        return rc ? rc : r1;
    });
}
int icc_decode_exact_enqueue(const porla_icc_decode_req* reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int curve,
                             hipStream_t stream) {
    return icc_decode_form_enqueue(reqs, k, n_rows, n_cols, n_total, curve, PORLA_ICC_DECODE_EXACT, stream);
}

// ---- the ragged decode (porla_icc_decode_ragged_batch_device): levels of unequal sizes, kernels in icc_decode_ragged.hip.h.  The
// launch sequence depends on the pass classes present, never on K or on which sizes are present:
//
//   upload              one copy: the requests with their shapes (IcdRagDesc), LARGEST FIRST so that a launch ends in small tiles and the
//                       requests of one pass count are neighbours; the n_rows^-1 table; per launch the tile starts
//   k_icd_clear_ragged  EXACT: the counters of the requests that have one
//   k_icd_exact_ragged / k_icd_residue_ragged    per pass count P present (n_rows <= 2^9: 1; else 2), P launches over ALL requests of
//                       that count, grid.x = their tiles; the residue planes of the requests of two passes sit one behind the other in
//                       this workspace's planes
static const char* const ICR_WHO = "porla_icc_decode_ragged_batch_device";
constexpr size_t ICR_MAX_TILES = 0xffffffu;               // one launch's grid.x: 256 lanes a block, 2^32 lanes a grid

// one launch: pass pz of the requests [first, first + count) of the sorted list, whose tile starts begin at starts[at]
struct IcrLaunch { int passes, pz; size_t first, count, at; uint32_t tiles; };
struct IcrPlan {
    std::vector<IcdRagDesc> desc;
    std::vector<uint32_t> starts;
    std::vector<IcrLaunch> launches;
    size_t plane_words = 0;
    bool logn_used[ICD_RAG_MAX_LOG + 1] = {};
};

// the plan of a call, on the host alone; arguments checked but for the tile count, which is refused here
static int icr_plan(const porla_icc_decode_ragged_req* reqs, size_t k, size_t ncols, int form, IcrPlan* out) {
    static_assert(ICD_RAG_MAX_PASSES * (ICC_TILE_LOG - 1) >= ICD_RAG_MAX_LOG, "a level of 2^16 rows has at most ICD_RAG_MAX_PASSES passes");
    const size_t planes_per = form == PORLA_ICC_DECODE_EXACT ? 2 : 1;
    std::vector<uint32_t> order(k);
    for (size_t a = 0; a < k; a++) order[a] = (uint32_t)a;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return reqs[x].n_rows > reqs[y].n_rows; });
    out->desc.resize(k);
    std::vector<int> passes_of(k);
    std::vector<IccPass> plans(k * ICD_RAG_MAX_PASSES);
    for (size_t i = 0; i < k; i++) {
        const porla_icc_decode_ragged_req& R = reqs[order[i]];
        const int logn = ilog2u((size_t)R.n_rows);
        IccPass plan[ICC_MAX_PASSES];
        passes_of[i] = icc_pass_plan(logn, ncols, plan);
        IcdRagDesc& D = out->desc[i];
        memset(&D, 0, sizeof D);
        D.d = IcdDesc{(const uint8_t*)R.d_rows, (uint8_t*)R.d_out, R.d_write_steps, R.d_bad};
        D.logn = (uint32_t)logn;
        for (int z = 0; z < passes_of[i]; z++) {
            plans[i * ICD_RAG_MAX_PASSES + z] = plan[z];
            D.shape[z] = (uint32_t)plan[z].s | (uint32_t)plan[z].ns << 8 | (uint32_t)plan[z].cc_log << 16;
        }
        if (passes_of[i] > 1) {
            D.work = out->plane_words;
            out->plane_words += planes_per * ((size_t)R.n_rows * ncols * ICC30_PLANE_WORDS);
        }
        out->logn_used[logn] = true;
    }
    // the requests of one pass count are neighbours (the count grows with n_rows): the highest pass of each group first
    for (size_t first = 0; first < k;) {
        size_t end = first;
        while (end < k && passes_of[end] == passes_of[first]) end++;
        for (int pz = passes_of[first] - 1; pz >= 0; pz--) {
            IcrLaunch L{passes_of[first], pz, first, end - first, out->starts.size(), 0};
            size_t tiles = 0;
            for (size_t i = first; i < end; i++) {
                const IccPass& p = plans[i * ICD_RAG_MAX_PASSES + pz];
                out->starts.push_back((uint32_t)tiles);
                tiles += p.col_tiles * ((size_t)reqs[order[i]].n_rows >> p.ns);
                if (tiles > ICR_MAX_TILES)
                    return bad_arg(ICR_WHO, "more than 2^24 - 1 tiles in one launch: the levels of this call do not fit a grid, split it");
            }
            out->starts.push_back((uint32_t)tiles);
            L.tiles = (uint32_t)tiles;
            out->launches.push_back(L);
        }
        first = end;
    }
    return PORLA_OK;
}

// the checks made before the device is touched
static int icr_check(const porla_icc_decode_ragged_req* reqs, size_t k, size_t n_cols, size_t n_total, int curve, int form) {
    auto bad = [&](const std::string& what) { return bad_arg(ICR_WHO, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = icd_check_shape(ICR_WHO, 2, n_cols, n_total, curve, form)) return rc;          // the call's own arguments
    if (int rc = check_request_count(ICR_WHO, k)) return rc;
    std::vector<IcdRange> ranges;
    ranges.reserve(4 * k);
    for (size_t a = 0; a < k; a++) {
        const porla_icc_decode_ragged_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        const size_t n = (size_t)R.n_rows;
        if (R.n_rows < 2 || (R.n_rows & (R.n_rows - 1)) != 0 || R.n_rows > n_total) return bad(at + "n_rows must be a power of two, 2 .. n_total");
        // (n <= 2^16 and n_cols <= 65535: no byte size of one request overflows; all planes together stay below 2^56)
        if (int rc = icd_check_request(ICR_WHO, at, R.d_rows, R.d_out, R.d_write_steps, R.d_bad, n, n_cols, form, ranges)) return rc;
    }
    return icd_check_overlap(ICR_WHO, ranges);
}

// ws->mu held, ws->fence entered; arguments checked, the plan made
template <class Q>
static int icr_enqueue(IccDecodeWs* ws, int curve, const IcrPlan& plan, size_t ncols, size_t n_total, int form, hipStream_t stream) {
    int rc;
    const bool exact = form == PORLA_ICC_DECODE_EXACT;
    const size_t k = plan.desc.size();
    if (!ws->rag_scales_made[curve]) {
        for (int l = 0; l <= ICD_RAG_MAX_LOG; l++) {
            icd_pow2<IccFp>(270 - l, ws->rag_scales[curve][l].p);
            icd_pow2<Q>(270 - l, ws->rag_scales[curve][l].q);
        }
        ws->rag_scales_made[curve] = true;
    }
    const size_t desc_b = k * sizeof(IcdRagDesc), scales_b = sizeof ws->rag_scales[curve], starts_b = plan.starts.size() * 4;
    const size_t list_b = desc_b + scales_b + starts_b;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    if ((rc = ws->list.ensure(list_b))) return rc;
    if (plan.plane_words && (rc = ws->planes.ensure(plan.plane_words * 4))) return rc;
    uint8_t* h = (uint8_t*)ws->h_list.h;
    memcpy(h, plan.desc.data(), desc_b);
    memcpy(h + desc_b, ws->rag_scales[curve], scales_b);
    memcpy(h + desc_b + scales_b, plan.starts.data(), starts_b);
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const uint8_t* d = (const uint8_t*)ws->list.p;
    const IcdRagDesc* d_desc = (const IcdRagDesc*)d;
    const IcdScale* d_scales = (const IcdScale*)(d + desc_b);
    const uint32_t* d_starts = (const uint32_t*)(d + desc_b + scales_b);
    if (exact) {
        hipLaunchKernelGGL(k_icd_clear_ragged, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, stream, d_desc, (uint32_t)k);
        PORLA_HIP(hipGetLastError());
    }
    const uint32_t *twp = nullptr, *twqi = nullptr;
    if ((rc = icc_decode_tables_acquire(curve, n_total, exact, stream, &twp, &twqi))) return rc;
    uint32_t* planes = (uint32_t*)ws->planes.p;
    for (const IcrLaunch& L : plan.launches) {
        const dim3 grid(L.tiles), block(ICC30_SPLIT_THREADS);
        const bool first = L.pz == L.passes - 1, last = L.pz == 0;
        const IcdRagDesc* desc = d_desc + L.first;
        const uint32_t* starts = d_starts + L.at;
        ProfScope ps("icc_decode_ragged", stream);
#define PORLA_ICR_EXACT(F, L_)                                                                                                      \
    hipLaunchKernelGGL((k_icd_exact_ragged<Q, F, L_>), grid, block, 0, stream, desc, starts, (uint32_t)L.count, L.pz, d_scales, planes, \
                       twp, twqi, (uint32_t)n_total, (uint32_t)ncols)
#define PORLA_ICR_RESIDUE(S, L_)                                                                                                    \
    hipLaunchKernelGGL((k_icd_residue_ragged<S, L_>), grid, block, 0, stream, desc, starts, (uint32_t)L.count, L.pz, d_scales, planes,  \
                       twp, (uint32_t)n_total, ilog2u(n_total), (uint32_t)ncols)
        if (exact) {
            if (first && last) PORLA_ICR_EXACT(true, true);
            else if (first) PORLA_ICR_EXACT(true, false);
            else if (last) PORLA_ICR_EXACT(false, true);
            else if constexpr (2 * (ICC_TILE_LOG - 1) < ICD_RAG_MAX_LOG) PORLA_ICR_EXACT(false, false);    // (a third pass: small tiles only)
        } else if (!first) {
            if (last) PORLA_ICR_RESIDUE(ICD_WORK, true);
            else if constexpr (2 * (ICC_TILE_LOG - 1) < ICD_RAG_MAX_LOG) PORLA_ICR_RESIDUE(ICD_WORK, false);
        } else if (form == PORLA_ICC_DECODE_RESIDUE64) {
            if (last) PORLA_ICR_RESIDUE(ICD_ROWS64, true);
            else PORLA_ICR_RESIDUE(ICD_ROWS64, false);
        } else {
            if (last) PORLA_ICR_RESIDUE(ICD_ROWS32, true);
            else PORLA_ICR_RESIDUE(ICD_ROWS32, false);
        }
#undef PORLA_ICR_EXACT
#undef PORLA_ICR_RESIDUE
    }
    if (hipGetLastError() != hipSuccess) { set_last_error("porla: ragged ICC decode batch: a launch failed"); rc = PORLA_ERR_HIP; }
    const int r1 = icc_mix_tables_release(stream);
    return rc ? rc : r1;
}

static int icr_run(const IcrPlan& plan, size_t n_cols, size_t n_total, int curve, int form, hipStream_t stream) {
    IccDecodeWs* ws = nullptr;
    if (int rc = g_icd_ws.get(&ws)) return rc;
    return FencedCall(ws, stream).run([&] {
        return curve == 0 ? icr_enqueue<IccBn254Fr>(ws, 0, plan, n_cols, n_total, form, stream)
                          : icr_enqueue<IccSecp256k1Fn>(ws, 1, plan, n_cols, n_total, form, stream);
    });
}

int icc_decode_ragged_enqueue(const porla_icc_decode_ragged_req* reqs, size_t k, size_t n_cols, size_t n_total, int curve, int form,
                              hipStream_t stream) {
    if (k == 0) return PORLA_OK;
    IcrPlan plan;
    if (int rc = icr_plan(reqs, k, n_cols, form, &plan)) return rc;
    return icr_run(plan, n_cols, n_total, curve, form, stream);
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_icc_decode_req) == PORLA_ICC_DECODE_REQ_BYTES, "porla_icc_decode_req size");
static_assert(offsetof(porla_icc_decode_req, d_rows) == 0 && offsetof(porla_icc_decode_req, d_out) == 8 &&
              offsetof(porla_icc_decode_req, d_write_steps) == 16 && offsetof(porla_icc_decode_req, d_bad) == 24,
              "porla_icc_decode_req offsets (include/porla_gpu.h)");
static_assert(offsetof(IcdDesc, rows) == 0 && offsetof(IcdDesc, out) == 8 && offsetof(IcdDesc, steps) == 16 && offsetof(IcdDesc, bad) == 24,
              "IcdDesc is porla_icc_decode_req field for field");

extern "C" int porla_icc_decode_batch_device(const porla_icc_decode_req* reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total,
                                             int curve, int form, void* hip_stream) {
    int rc = icd_check(reqs, k, n_rows, n_cols, n_total, curve, form);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    IccDecodeWs* ws = nullptr;
    if ((rc = g_icd_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return icd_run(ws, reqs, k, n_rows, n_cols, n_total, curve, form, stream); });
}

static_assert(sizeof(porla_icc_decode_ragged_req) == PORLA_ICC_DECODE_RAGGED_REQ_BYTES, "porla_icc_decode_ragged_req size");
static_assert(offsetof(porla_icc_decode_ragged_req, d_rows) == 0 && offsetof(porla_icc_decode_ragged_req, d_out) == 8 &&
              offsetof(porla_icc_decode_ragged_req, d_write_steps) == 16 && offsetof(porla_icc_decode_ragged_req, d_bad) == 24 &&
              offsetof(porla_icc_decode_ragged_req, n_rows) == 32,
              "porla_icc_decode_ragged_req offsets (include/porla_gpu.h): porla_icc_decode_req field for field, then n_rows");
static_assert(offsetof(IcdRagDesc, d) == 0 && offsetof(IcdRagDesc, logn) == 32 && offsetof(IcdRagDesc, shape) == 36 &&
              offsetof(IcdRagDesc, work) == 48, "IcdRagDesc: the request's pointers, its shape, its planes");

extern "C" int porla_icc_decode_ragged_batch_device(const porla_icc_decode_ragged_req* reqs, size_t k, size_t n_cols, size_t n_total, int curve,
                                                    int form, void* hip_stream) {
    int rc = icr_check(reqs, k, n_cols, n_total, curve, form);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    IcrPlan plan;
    if ((rc = icr_plan(reqs, k, n_cols, form, &plan))) return rc;
    if ((rc = ensure_device())) return rc;
    return icr_run(plan, n_cols, n_total, curve, form, (hipStream_t)hip_stream);
}

// one level from host memory: upload, the batch of one request on the engine's stream, download
extern "C" int porla_icc_decode_host(const uint8_t* rows, size_t n_rows, size_t n_cols, size_t n_total, int curve, int form,
                                     const unsigned long long* write_steps, uint8_t* out, unsigned int* bad) {
    static const char* const who = "porla_icc_decode_host";
    if (!rows || !out) return bad_arg(who, "rows or out is NULL");
    int rc = icd_check_shape(who, n_rows, n_cols, n_total, curve, form);
    if (rc) return rc;
    if (write_steps && form == PORLA_ICC_DECODE_EXACT) return bad_arg(who, "write_steps with PORLA_ICC_DECODE_EXACT: the unscale is the residue forms'");
    if (bad && form != PORLA_ICC_DECODE_EXACT) return bad_arg(who, "bad with a residue form: only PORLA_ICC_DECODE_EXACT counts");
    if ((rc = ensure_device())) return rc;
    IccDecodeWs* ws = nullptr;
    if ((rc = g_icd_ws.get(&ws))) return rc;
    const size_t symbols = n_rows * n_cols, in_b = symbols * icd_symbol_bytes(form), out_b = symbols * 32;
    hipStream_t s = engine_stream();
    FencedCall call(ws, s);
    rc = call.run([&] {
        int r;
        if ((r = ws->io_rows.ensure(in_b)) || (r = ws->io_out.ensure(out_b))) return r;
        if (write_steps && (r = ws->io_steps.ensure(n_rows * 8))) return r;
        if (bad && (r = ws->io_bad.ensure(4))) return r;
        PORLA_HIP(hipMemcpyAsync(ws->io_rows.p, rows, in_b, hipMemcpyHostToDevice, s));
        if (write_steps) PORLA_HIP(hipMemcpyAsync(ws->io_steps.p, write_steps, n_rows * 8, hipMemcpyHostToDevice, s));
        porla_icc_decode_req R;
        R.d_rows = ws->io_rows.p;
        R.d_out = ws->io_out.p;
        R.d_write_steps = write_steps ? (const unsigned long long*)ws->io_steps.p : nullptr;
        R.d_bad = bad ? (unsigned int*)ws->io_bad.p : nullptr;
        if ((r = icd_run(ws, &R, 1, n_rows, n_cols, n_total, curve, form, s))) return r;
        PORLA_HIP(hipMemcpyAsync(out, ws->io_out.p, out_b, hipMemcpyDeviceToHost, s));
        if (bad) PORLA_HIP(hipMemcpyAsync(bad, ws->io_bad.p, 4, hipMemcpyDeviceToHost, s));
        return (int)PORLA_OK;
    });
    if (rc) return rc;
    PORLA_HIP(hipStreamSynchronize(s));        // (the lock is held to here: the images are this call's until the copies are done)
    return PORLA_OK;
}

// The batched verified retrieval (include/porla_gpu.h: porla_kzg_retrieve_batch_device / porla_ipa_retrieve_batch_device, the aligned
// calls porla_{kzg,ipa}_retrieve_aligned_batch_device that take a half's alignment store, and the host forms of the four): the coded
// rows of K halves checked row by row against their stored MAC rows, then decoded, in ONE asynchronous call.  The exact call is the
// aligned one without alignment stores in the form PORLA_ICC_DECODE_EXACT: its requests are widened on the way to the device.
// Kernels and the relation: retrieve_batch.hip.h.  Every step is on the caller's stream and the launch sequence depends on n_rows,
// never on K (IPA: as long as the call's coefficient rows fit the workspace bound RT_COEFF_BYTES; beyond it the rows go through in groups):
//
//   upload                the requests as they are (RtDesc)
//   k_rt_clear            both counters of every request that has them
//   KZG:  k_rt_eval_lazy / k_rt_eval_horner    alpha f_g(tau) | PRF per row into the KZG state's d_eval
//         fb_gh commit    the two-coefficient commitment against (G1[0], h_MAC) -> the expected MACs
//   IPA:  k_rt_pack       sym mod n as coefficient rows, the PRF values as rows of the h pass
//         client_block_pass, client_h_pass       the two commitments of porla_ipa_client_update_batch_device's step 1
//   k_rt_compare          (IPA: block commitment + hiding multiple, then) 64 bytes against d_macs -> status, failures counted
//     or k_rt_compare_aligned   when a request of the call has a d_align: ... minus alpha * A_j first (a quad of lanes per row)
//   the data decode in the call's form (icc_decode.hip: icc_decode_form_enqueue) of the requests that have a d_out; EXACT: d_bad =
//   d_counts + 1
// The check between k_rt_clear and the decode is rt_check_rows, written over the kernels' row -> request map: the retrieval calls run
// it with RtMapShift, the file extraction (extract_batch.hip) through rt_check_starts_{kzg,ipa} with RtMapStarts on halves of unequal sizes.
#include "retrieve_batch.hip.h"
#include "write_batch_host.hpp"
#include "../../include/porla_gpu.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

namespace porla {

struct RetrieveWs {
    std::mutex mu;
    int device = -1;
    Buf list, exp, coeffs, scalars, hpts;
    Buf io_rows, io_macs, io_prf, io_align, io_steps, io_out, io_status, io_counts;     // the host forms' device images
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<RetrieveWs> g_rt_ws;

// the IPA build's coefficient rows of one group: 2^16 rows of 128 coefficients
constexpr size_t RT_COEFF_BYTES = (size_t)256 << 20;

// the refusals that concern the shape of the call
static int rt_check_shape(const char* who, size_t n_rows, size_t n_total) {
    if (int rc = check_n_total(who, n_total, 16)) return rc;
    if (n_rows < 2 || (n_rows & (n_rows - 1)) != 0 || n_rows > n_total) return bad_arg(who, "n_rows must be a power of two, 2 .. n_total");
    return PORLA_OK;
}

// The requests of a call: porla_retrieve_aligned_req (wide), or porla_retrieve_req read as one without d_align and d_write_steps
struct RtReqs {
    const void* p;
    bool wide;
    porla_retrieve_aligned_req at(size_t a) const {
        if (wide) return static_cast<const porla_retrieve_aligned_req*>(p)[a];
        const porla_retrieve_req& R = static_cast<const porla_retrieve_req*>(p)[a];
        return porla_retrieve_aligned_req{R.d_rows, R.d_macs, R.d_prf, nullptr, nullptr, R.d_out, R.d_status, R.d_counts};
    }
};

static inline bool rt_form_ok(int form) {
    return form == PORLA_ICC_DECODE_EXACT || form == PORLA_ICC_DECODE_RESIDUE64 || form == PORLA_ICC_DECODE_RESIDUE32;
}
static inline size_t rt_symbol_bytes(int form) { return form == PORLA_ICC_DECODE_RESIDUE32 ? 32 : 64; }
static int rt_check_form(const char* who, int form) {
    return rt_form_ok(form) ? (int)PORLA_OK : bad_arg(who, "form must be PORLA_ICC_DECODE_EXACT, _RESIDUE64 or _RESIDUE32");
}

// the checks made before the device is touched; n_cols: the row width the buffers are sized by, form: the symbol width
static int rt_check(const char* who, const RtReqs& reqs, size_t k, size_t n_rows, size_t n_cols, size_t n_total, int form) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs.p) return bad("reqs is NULL");
    if (int rc = rt_check_shape(who, n_rows, n_total)) return rc;
    if (int rc = rt_check_form(who, form)) return rc;
    if (int rc = check_request_count(who, k)) return rc;
    size_t in_b, t;
    // (the kernels number the rows of the call through in 32 bits)
    if (!mul_ok(n_rows, n_cols, &t) || !mul_ok(t, 64, &in_b) || (k && (!mul_ok(n_rows, k, &t) || t > 0xffffffffull)))
        return bad("a byte size overflows: the rows of the call do not fit a buffer");
    const size_t out_b = in_b / 2;
    in_b = out_b / 32 * rt_symbol_bytes(form);
    struct Range { uintptr_t lo, hi; bool out; };
    std::vector<Range> ranges;
    ranges.reserve(8 * k);
    for (size_t a = 0; a < k; a++) {
        const porla_retrieve_aligned_req R = reqs.at(a);
        const std::string at = "request " + std::to_string(a) + ": ";
        if (!R.d_rows || !R.d_macs || !R.d_prf || !R.d_status) return bad(at + "a NULL d_rows, d_macs, d_prf or d_status");
        if (((uintptr_t)R.d_rows | (uintptr_t)R.d_macs | (uintptr_t)R.d_prf | (uintptr_t)R.d_out) & 15u)
            return bad(at + "d_rows, d_macs, d_prf or d_out is not 16-byte aligned");
        if ((uintptr_t)R.d_counts & 3u) return bad(at + "d_counts is not 4-byte aligned");
        if ((uintptr_t)R.d_align & 15u) return bad(at + "d_align is not 16-byte aligned");
        if ((uintptr_t)R.d_write_steps & 7u) return bad(at + "d_write_steps is not 8-byte aligned");
        if (R.d_write_steps && form == PORLA_ICC_DECODE_EXACT)
            return bad(at + "d_write_steps with PORLA_ICC_DECODE_EXACT: the unscale is the residue forms'");
        if ((uintptr_t)R.d_rows + in_b < (uintptr_t)R.d_rows || (R.d_out && (uintptr_t)R.d_out + out_b < (uintptr_t)R.d_out) ||
            (uintptr_t)R.d_macs + n_rows * 64 < (uintptr_t)R.d_macs || (uintptr_t)R.d_prf + n_rows * 16 < (uintptr_t)R.d_prf ||
            (uintptr_t)R.d_status + n_rows < (uintptr_t)R.d_status || (R.d_counts && (uintptr_t)R.d_counts + 8 < (uintptr_t)R.d_counts) ||
            (R.d_align && (uintptr_t)R.d_align + n_rows * 64 < (uintptr_t)R.d_align) ||
            (R.d_write_steps && (uintptr_t)R.d_write_steps + n_rows * 8 < (uintptr_t)R.d_write_steps))
            return bad(at + "a byte size overflows: a buffer wraps around the address space");
        if (R.d_align) ranges.push_back(Range{(uintptr_t)R.d_align, (uintptr_t)R.d_align + n_rows * 64, false});
        if (R.d_write_steps) ranges.push_back(Range{(uintptr_t)R.d_write_steps, (uintptr_t)R.d_write_steps + n_rows * 8, false});
        ranges.push_back(Range{(uintptr_t)R.d_rows, (uintptr_t)R.d_rows + in_b, false});
        ranges.push_back(Range{(uintptr_t)R.d_macs, (uintptr_t)R.d_macs + n_rows * 64, false});
        ranges.push_back(Range{(uintptr_t)R.d_prf, (uintptr_t)R.d_prf + n_rows * 16, false});
        if (R.d_out) ranges.push_back(Range{(uintptr_t)R.d_out, (uintptr_t)R.d_out + out_b, true});
        ranges.push_back(Range{(uintptr_t)R.d_status, (uintptr_t)R.d_status + n_rows, true});
        if (R.d_counts) ranges.push_back(Range{(uintptr_t)R.d_counts, (uintptr_t)R.d_counts + 8, true});
    }
    // an output may overlap nothing, inputs may be shared (icc_decode.hip: the same walk)
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uintptr_t end_any = 0, end_out = 0;
    for (const Range& r : ranges) {
        if (r.lo < (r.out ? end_any : end_out))
            return bad("an output (d_out, d_status or d_counts) overlaps an input or output of this call: outputs must be disjoint from everything");
        end_any = std::max(end_any, r.hi);
        if (r.out) end_out = std::max(end_out, r.hi);
    }
    return PORLA_OK;
}

// KZG: the expected MACs of all rows into d_exp -- the evaluation into the state's d_eval, then the two-coefficient commitment against
// the table of (G1[0], h_MAC), under the state's and the table's mutexes and the tables' fences as client_batch_device takes them
// symb: the symbol width of the rows.  alpha_sc (or nullptr): the key as the plain scalar of the aligned compare's ladder, read under
// the same lock as the evaluation's
template <class Map>
static int rt_kzg_expected(const RtDesc* d_desc, const Map& map, size_t rows, size_t n_coeffs, size_t symb, uint8_t* d_exp, uint32_t* alpha_sc,
                           hipStream_t stream) {
    using Fr = Bn254Fr;
    int rc;
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    if (!g_kzg.have_key || g_kzg.srs.empty()) { set_last_error("porla: init_key / init_SRS first"); return PORLA_ERR_STATE; }
    if ((size_t)g_kzg.n_samples != n_coeffs) { set_last_error("porla: the SRS changed during the call"); return PORLA_ERR_STATE; }
    if (alpha_sc) h_fe_to_plain<Fr>(alpha_sc, g_kzg.alpha);
    KzgDev* kd;
    if ((rc = current_dev(&kd))) return rc;
    FixedBase<Bn254G1>& fb = kd->fb_gh;
    if ((rc = kzg_small_table(fb, kd->gh_version, {g_kzg.srs[0], g_kzg.h_mac}))) return rc;
    std::lock_guard<std::mutex> lk2(fb.mu);
    if ((rc = kd->d_eval.ensure(rows * 64))) return rc;              // a hipFree in there waits for the work that still uses it
    // d_eval is shared by the three client-side tables: a previous batch on another stream must have finished with it
    if ((rc = kd->fb_g.fence.enter(stream))) return rc;
    if ((rc = kd->fb_gh.fence.enter(stream))) return rc;
    const uint32_t nc = (uint32_t)n_coeffs;
    if (nc <= KZG_LAZY_MAX_COEFFS) {
        const uint32_t entries = (nc + 7) / 8 * 8;
        const size_t entry_words = 2 * KZG_LAZY_ENTRY_WORDS;
        if (!kd->d_tau29w.p || kd->tau29w_n != nc || memcmp(kd->tau29w_tau.v, g_kzg.tau.v, sizeof(g_kzg.tau.v)) != 0) {
            const std::vector<uint32_t> tab = kzg_tau29_table(nc, true);     // per power: tau^i, then 2^256 tau^i mod r
            kd->d_tau29w.release();                                  // the hipFree waits for the evaluations that still read the old table
            kd->tau29w_n = 0;
            if ((rc = kd->d_tau29w.ensure(tab.size() * 4))) return rc;
            PORLA_HIP(hipMemcpy(kd->d_tau29w.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
            kd->tau29w_tau = g_kzg.tau;
            kd->tau29w_n = nc;
        }
        KzgAlpha270 A;
        kzg_to270(g_kzg.alpha, A.w);
        static LdsOnce once;                                         // dynamic LDS above 64 KiB (more than 682 coefficients): told once per device
        once.set({lds_kernel(&k_rt_eval_lazy<64, Map>, (size_t)KZG_LAZY_MAX_COEFFS * entry_words * 4),
                  lds_kernel(&k_rt_eval_lazy<32, Map>, (size_t)KZG_LAZY_MAX_COEFFS * entry_words * 2)});
        ProfScope ps("retrieve_eval", stream);
        constexpr size_t lazy_grid = 2048;                           // k_kzg_eval_rows_lazy's
        const size_t groups = (rows + 31) / 32;
        const dim3 grid((unsigned)std::min(groups, lazy_grid));
        if (symb == 64)
            hipLaunchKernelGGL((k_rt_eval_lazy<64, Map>), grid, dim3(256), (size_t)entries * entry_words * 4, stream, d_desc, map,
                               (uint32_t)rows, nc, (const uint32_t*)kd->d_tau29w.p, A, (uint8_t*)kd->d_eval.p);
        else                                                         // (the tau^i half of every entry of the same table)
            hipLaunchKernelGGL((k_rt_eval_lazy<32, Map>), grid, dim3(256), (size_t)entries * entry_words * 2, stream, d_desc, map,
                               (uint32_t)rows, nc, (const uint32_t*)kd->d_tau29w.p, A, (uint8_t*)kd->d_eval.p);
    } else {
        KzgEvalConsts K;
        Fe<Fr> pw = fe_one<Fr>();
        for (int jj = 0; jj < 8; jj++) { kzg_to270(pw, K.tj[jj]); pw = fe_mul<Fr>(pw, g_kzg.tau); }
        kzg_to270(pw, K.t8);
        kzg_to270(g_kzg.alpha, K.alpha);
        ProfScope ps("retrieve_eval", stream);
        const dim3 grid((unsigned)((8 * rows + 255) / 256));
        if (symb == 64)
            hipLaunchKernelGGL((k_rt_eval_horner<64, Map>), grid, dim3(256), 0, stream, d_desc, map, (uint32_t)rows, nc, K,
                               (uint8_t*)kd->d_eval.p);
        else
            hipLaunchKernelGGL((k_rt_eval_horner<32, Map>), grid, dim3(256), 0, stream, d_desc, map, (uint32_t)rows, nc, K,
                               (uint8_t*)kd->d_eval.p);
    }
    PORLA_HIP(hipGetLastError());
    return fb.commit_device((const uint8_t*)kd->d_eval.p, rows, 2, 64, d_exp, stream);
}

// the aligned compare: its dynamic LDS is the quad ladder's, told once per device
template <class C, bool ADD, class Map, class Act>
static void rt_compare_aligned_launch(const RtDesc* d_desc, const Map& map, size_t g0, size_t m, uint8_t* d_exp, const uint8_t* d_hpts,
                                      const MacScalar& alpha, hipStream_t stream) {
    static LdsOnce once;
    once.set({lds_kernel(&k_rt_compare_aligned<C, ADD, Map, Act>, macq_lds_bytes<C>())});
    hipLaunchKernelGGL((k_rt_compare_aligned<C, ADD, Map, Act>), dim3((unsigned)((m + RT_ALIGNED_ROWS - 1) / RT_ALIGNED_ROWS)), dim3(4 * MACQ_BF),
                       macq_lds_bytes<C>(), stream, d_desc, map, (uint32_t)g0, (uint32_t)m, d_exp, d_hpts, alpha);
}

// the IPA build's rows of one group (all of them while their coefficient rows fit the bound); the KZG build takes all rows at once
template <class C>
static size_t rt_group_rows(size_t rows, size_t ncols) {
    return std::is_same<C, Bn254G1>::value ? rows : std::min(rows, std::max<size_t>(RT_COEFF_BYTES / (ncols * 32), 1));
}
// the workspace of a check of `rows` rows
template <class C>
static int rt_ensure(RetrieveWs* ws, size_t rows, size_t ncols) {
    int rc;
    const size_t group = rt_group_rows<C>(rows, ncols);
    if ((rc = ws->exp.ensure(group * 64))) return rc;
    if (!std::is_same<C, Bn254G1>::value) {
        if ((rc = ws->coeffs.ensure(group * ncols * 32))) return rc;
        if ((rc = ws->scalars.ensure(group * 32))) return rc;
        if ((rc = ws->hpts.ensure(group * 64))) return rc;
    }
    return PORLA_OK;
}

// The check of the rows 0 .. rows - 1 of the requests at d_desc under `map`: expected MACs, then the compare -> status bytes, failures
// counted.  ws->mu held, ws->fence entered, rt_ensure done.  alpha: the IPA build's, for the aligned compare (the KZG build reads its key)
// Act = RtActWrite: the same stages, and the last kernel writes the selected rows' MAC bytes instead of judging (the top-level repair)
template <class C, class Map, class Act = RtActCompare>
static int rt_check_rows(RetrieveWs* ws, FixedBase<C>* fb_alpha, FixedBase<C>* fb_h, MacScalar alpha, bool aligned, const RtDesc* d_desc,
                         const Map& map, size_t rows, size_t ncols, size_t symb, hipStream_t stream) {
    using Q = typename IccCurve<C>::Q;
    constexpr bool kzg = std::is_same<C, Bn254G1>::value;
    int rc;
    const size_t group = rt_group_rows<C>(rows, ncols);
    uint8_t* d_exp = (uint8_t*)ws->exp.p;
    for (size_t g0 = 0; g0 < rows; g0 += group) {
        const size_t m = std::min(group, rows - g0);
        if constexpr (kzg) {
            if ((rc = rt_kzg_expected(d_desc, map, rows, ncols, symb, d_exp, aligned ? alpha.v : nullptr, stream))) return rc;
        } else {
            {
                ProfScope ps("retrieve_pack", stream);
                const size_t items = m * ncols + m;
                const dim3 grid((unsigned)((items + 255) / 256));
                if (symb == 64)
                    hipLaunchKernelGGL((k_rt_pack<Q, 64, Map>), grid, dim3(256), 0, stream, d_desc, map, (uint32_t)g0, (uint32_t)m,
                                       (uint32_t)ncols, (uint8_t*)ws->coeffs.p, (uint8_t*)ws->scalars.p);
                else
                    hipLaunchKernelGGL((k_rt_pack<Q, 32, Map>), grid, dim3(256), 0, stream, d_desc, map, (uint32_t)g0, (uint32_t)m,
                                       (uint32_t)ncols, (uint8_t*)ws->coeffs.p, (uint8_t*)ws->scalars.p);
                PORLA_HIP(hipGetLastError());
            }
            if ((rc = client_block_pass<C>(fb_alpha, (const uint8_t*)ws->coeffs.p, m, ncols, d_exp, stream))) return rc;
            if ((rc = client_h_pass<C>(fb_h, (const uint8_t*)ws->scalars.p, m, (uint8_t*)ws->hpts.p, stream))) return rc;
        }
        ProfScope ps(std::is_same<Act, RtActCompare>::value ? "retrieve_compare" : "retrieve_write", stream);
        if (aligned)
            rt_compare_aligned_launch<C, !kzg, Map, Act>(d_desc, map, g0, m, d_exp, (const uint8_t*)ws->hpts.p, alpha, stream);
        else
            hipLaunchKernelGGL((k_rt_compare<C, !kzg, Map, Act>), dim3((unsigned)((m + 63) / 64)), dim3(64), 0, stream, d_desc, map,
                               (uint32_t)g0, (uint32_t)m, d_exp, (const uint8_t*)ws->hpts.p);
        PORLA_HIP(hipGetLastError());
    }
    return PORLA_OK;
}

// ws->mu held, ws->fence entered; arguments checked.  fb_alpha == nullptr: the KZG build (the resident key, SRS and hiding base).
// alpha_ipa: the IPA build's alpha, reduced, little-endian words (the KZG build reads its key under the state's lock)
template <class C>
static int rt_enqueue(RetrieveWs* ws, FixedBase<C>* fb_alpha, FixedBase<C>* fb_h, const uint32_t* alpha_ipa, const RtReqs& reqs, size_t k,
                      size_t n_rows, size_t ncols, size_t n_total, int form, hipStream_t stream) {
    constexpr bool kzg = std::is_same<C, Bn254G1>::value;
    int rc;
    const int logn = ilog2u(n_rows);
    const size_t rows = k * n_rows, desc_b = k * sizeof(RtDesc);
    static_assert(sizeof(RtDesc) == sizeof(porla_retrieve_aligned_req), "the requests are uploaded in the aligned call's layout");
    const size_t symb = rt_symbol_bytes(form);
    bool aligned = false;                                                // a request with an alignment store: the quad compare
    if ((rc = ws->h_list.stage(desc_b))) return rc;
    if ((rc = ws->list.ensure(desc_b))) return rc;
    if ((rc = rt_ensure<C>(ws, rows, ncols))) return rc;
    for (size_t a = 0; a < k; a++) {
        const porla_retrieve_aligned_req R = reqs.at(a);
        aligned = aligned || R.d_align;
        memcpy((uint8_t*)ws->h_list.h + a * sizeof(RtDesc), &R, sizeof(RtDesc));
    }
    if ((rc = ws->h_list.send(ws->list.p, desc_b, stream))) return rc;
    MacScalar alpha{};
    if (!kzg && aligned) memcpy(alpha.v, alpha_ipa, sizeof(alpha.v));
    const RtDesc* d_desc = (const RtDesc*)ws->list.p;
    hipLaunchKernelGGL(k_rt_clear, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, stream, d_desc, (uint32_t)k);
    PORLA_HIP(hipGetLastError());
    if ((rc = rt_check_rows<C>(ws, fb_alpha, fb_h, alpha, aligned, d_desc, RtMapShift{(uint32_t)logn}, rows, ncols, symb, stream))) return rc;
    // the data decode of the requests that want their blocks, whatever the statuses are
    std::vector<porla_icc_decode_req> dec;
    dec.reserve(k);
    const bool exact = form == PORLA_ICC_DECODE_EXACT;                  // (only the EXACT decode counts: d_counts[1] stays 0 otherwise)
    for (size_t a = 0; a < k; a++) {
        const porla_retrieve_aligned_req R = reqs.at(a);
        if (R.d_out) dec.push_back(porla_icc_decode_req{R.d_rows, R.d_out, R.d_write_steps, exact && R.d_counts ? R.d_counts + 1 : nullptr});
    }
    if (dec.empty()) return PORLA_OK;
    return icc_decode_form_enqueue(dec.data(), dec.size(), n_rows, ncols, n_total, IccCurve<C>::id, form, stream);
}

// The same check for halves of unequal sizes (the extraction, extract_batch.hip): the requests at d_desc, row numbering by `map`,
// `rows` rows of `symb`-byte symbols; under this file's workspace, its lock and fence
template <class C, class Act = RtActCompare>
static int rt_check_starts(FixedBase<C>* fb_alpha, FixedBase<C>* fb_h, const uint32_t* alpha_ipa, bool aligned, const RtDesc* d_desc,
                           const RtMapStarts& map, size_t rows, size_t ncols, size_t symb, hipStream_t stream) {
    RetrieveWs* ws = nullptr;
    int rc;
    if ((rc = g_rt_ws.get(&ws))) return rc;
    MacScalar alpha{};
    if (alpha_ipa && aligned) memcpy(alpha.v, alpha_ipa, sizeof(alpha.v));
    return FencedCall(ws, stream).run([&] {
        if (int r = rt_ensure<C>(ws, rows, ncols)) return r;
        return rt_check_rows<C, RtMapStarts, Act>(ws, fb_alpha, fb_h, alpha, aligned, d_desc, map, rows, ncols, symb, stream);
    });
}
int rt_check_starts_kzg(bool aligned, const RtDesc* d_desc, const RtMapStarts& map, size_t rows, size_t ncols, size_t symb, hipStream_t stream) {
    return rt_check_starts<Bn254G1>(nullptr, nullptr, nullptr, aligned, d_desc, map, rows, ncols, symb, stream);
}
int rt_check_starts_ipa(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint32_t alpha[8], bool aligned, const RtDesc* d_desc,
                        const RtMapStarts& map, size_t rows, size_t symb, hipStream_t stream) {
    return rt_check_starts<Secp256k1G>(&alpha_generators_fb->secp, &h_fb->secp, alpha, aligned, d_desc, map, rows, IPA_COLS, symb, stream);
}

// The repair's second pass over the same halves (repair_batch.hip): the expected-MAC stages again, over the rows as they lie now, and
// the last kernel writes (RtActWrite, retrieve_batch.hip.h: what the requests' members mean there)
int rt_write_starts_kzg(bool aligned, const RtDesc* d_desc, const RtMapStarts& map, size_t rows, size_t ncols, size_t symb, hipStream_t stream) {
    return rt_check_starts<Bn254G1, RtActWrite>(nullptr, nullptr, nullptr, aligned, d_desc, map, rows, ncols, symb, stream);
}
int rt_write_starts_ipa(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint32_t alpha[8], bool aligned, const RtDesc* d_desc,
                        const RtMapStarts& map, size_t rows, size_t symb, hipStream_t stream) {
    return rt_check_starts<Secp256k1G, RtActWrite>(&alpha_generators_fb->secp, &h_fb->secp, alpha, aligned, d_desc, map, rows, IPA_COLS, symb,
                                                   stream);
}

// one level from host memory: upload, the batch of one request on the engine's stream, download; `run` enqueues that batch
template <class Run>
static int rt_host(const char* who, const uint8_t* rows, const uint8_t* macs, const uint8_t* prf, const uint8_t* align,
                   const unsigned long long* write_steps, size_t n_rows, size_t ncols, int form, uint8_t* out, uint8_t* status,
                   unsigned int* counts, Run run) {
    RetrieveWs* ws = nullptr;
    int rc;
    if ((rc = g_rt_ws.get(&ws))) return rc;
    size_t in_b;
    if (!mul_ok(n_rows * 64, ncols, &in_b)) return bad_arg(who, "a byte size overflows: n_rows * n_cols symbols do not fit a buffer");
    const size_t out_b = in_b / 2;
    in_b = out_b / 32 * rt_symbol_bytes(form);
    hipStream_t s = engine_stream();
    FencedCall call(ws, s);
    rc = call.run([&] {
        int r;
        if ((r = ws->io_rows.ensure(in_b)) || (r = ws->io_macs.ensure(n_rows * 64)) || (r = ws->io_prf.ensure(n_rows * 16)) ||
            (r = ws->io_status.ensure(n_rows)) || (r = ws->io_counts.ensure(8)))
            return r;
        if (out && (r = ws->io_out.ensure(out_b))) return r;
        if (align && (r = ws->io_align.ensure(n_rows * 64))) return r;
        if (write_steps && (r = ws->io_steps.ensure(n_rows * 8))) return r;
        PORLA_HIP(hipMemcpyAsync(ws->io_rows.p, rows, in_b, hipMemcpyHostToDevice, s));
        PORLA_HIP(hipMemcpyAsync(ws->io_macs.p, macs, n_rows * 64, hipMemcpyHostToDevice, s));
        PORLA_HIP(hipMemcpyAsync(ws->io_prf.p, prf, n_rows * 16, hipMemcpyHostToDevice, s));
        if (align) PORLA_HIP(hipMemcpyAsync(ws->io_align.p, align, n_rows * 64, hipMemcpyHostToDevice, s));
        if (write_steps) PORLA_HIP(hipMemcpyAsync(ws->io_steps.p, write_steps, n_rows * 8, hipMemcpyHostToDevice, s));
        porla_retrieve_aligned_req R;
        R.d_rows = ws->io_rows.p; R.d_macs = ws->io_macs.p; R.d_prf = ws->io_prf.p;
        R.d_align = align ? ws->io_align.p : nullptr;
        R.d_write_steps = write_steps ? (const unsigned long long*)ws->io_steps.p : nullptr;
        R.d_out = out ? ws->io_out.p : nullptr;
        R.d_status = (unsigned char*)ws->io_status.p;
        R.d_counts = (unsigned int*)ws->io_counts.p;
        if ((r = run(ws, &R, s))) return r;
        if (out) PORLA_HIP(hipMemcpyAsync(out, ws->io_out.p, out_b, hipMemcpyDeviceToHost, s));
        PORLA_HIP(hipMemcpyAsync(status, ws->io_status.p, n_rows, hipMemcpyDeviceToHost, s));
        if (counts) PORLA_HIP(hipMemcpyAsync(counts, ws->io_counts.p, 8, hipMemcpyDeviceToHost, s));
        return (int)PORLA_OK;
    });
    if (rc) return rc;
    PORLA_HIP(hipStreamSynchronize(s));        // (the lock is held to here: the images are this call's until the copies are done)
    return PORLA_OK;
}

// the KZG build's row width for the refusals: the SRS size, or one column while there is no SRS (the call then ends in PORLA_ERR_STATE,
// or PORLA_ERR_NO_DEVICE, and the refusals that do not depend on the width have been made)
static size_t rt_kzg_width_for_checks() { return std::max<size_t>(kzg_n_samples(), 1); }

static int rt_ipa_bases(const char* who, porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb) {
    if (int rc = ipa_check_generators(who, "alpha_generators_fb", alpha_generators_fb)) return rc;
    return ipa_check_hiding_base(who, "h_fb", h_fb);
}

// the IPA build's alpha: 32 big-endian bytes -> reduced mod n, little-endian words
static void rt_ipa_alpha(const uint8_t alpha_be[32], uint32_t sc[8]) {
    h_load_be(sc, alpha_be);
    fe_reduce_plain<IccCurve<Secp256k1G>::Q>(sc, 8);
}

// the bodies of the device calls, exact (wide == false, form EXACT) and aligned
static int rt_kzg_device(const char* who, const RtReqs& reqs, size_t k, size_t n_rows, size_t n_total, int form, void* hip_stream) {
    const size_t width = rt_kzg_width_for_checks();
    int rc = rt_check(who, reqs, k, n_rows, width, n_total, form);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = client_kzg_row_width(&n))) return rc;
    if (n != width && (rc = rt_check(who, reqs, k, n_rows, n, n_total, form))) return rc;       // (an SRS made since the first look)
    RetrieveWs* ws = nullptr;
    if ((rc = g_rt_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return rt_enqueue<Bn254G1>(ws, nullptr, nullptr, nullptr, reqs, k, n_rows, n, n_total, form, stream); });
}

static int rt_ipa_device(const char* who, porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t* alpha_be,
                         const RtReqs& reqs, size_t k, size_t n_rows, size_t n_total, int form, void* hip_stream) {
    int rc = rt_check(who, reqs, k, n_rows, IPA_COLS, n_total, form);
    if (rc) return rc;
    if (reqs.wide && !alpha_be) return bad_arg(who, "alpha_be is NULL");
    if (k == 0) return PORLA_OK;
    if (!alpha_generators_fb || !h_fb) return bad_arg(who, "a NULL base");
    if ((rc = ensure_device())) return rc;
    if ((rc = rt_ipa_bases(who, alpha_generators_fb, h_fb))) return rc;
    uint32_t alpha[8] = {0};
    if (alpha_be) rt_ipa_alpha(alpha_be, alpha);
    RetrieveWs* ws = nullptr;
    if ((rc = g_rt_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        return rt_enqueue<Secp256k1G>(ws, &alpha_generators_fb->secp, &h_fb->secp, alpha, reqs, k, n_rows, IPA_COLS, n_total, form, stream);
    });
}

static int rt_kzg_host(const char* who, const uint8_t* rows, const uint8_t* macs, const uint8_t* prf, const uint8_t* align,
                       const unsigned long long* write_steps, size_t n_rows, size_t n_total, int form, uint8_t* out, uint8_t* status,
                       unsigned int* counts) {
    if (!rows || !macs || !prf || !status) return bad_arg(who, "rows, macs, prf or status is NULL");
    int rc = rt_check_shape(who, n_rows, n_total);
    if (rc) return rc;
    if ((rc = rt_check_form(who, form))) return rc;
    if (write_steps && form == PORLA_ICC_DECODE_EXACT) return bad_arg(who, "write_steps with PORLA_ICC_DECODE_EXACT: the unscale is the residue forms'");
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = client_kzg_row_width(&n))) return rc;
    return rt_host(who, rows, macs, prf, align, write_steps, n_rows, n, form, out, status, counts,
                   [&](RetrieveWs* ws, const porla_retrieve_aligned_req* R, hipStream_t s) {
                       return rt_enqueue<Bn254G1>(ws, nullptr, nullptr, nullptr, RtReqs{R, true}, 1, n_rows, n, n_total, form, s);
                   });
}

static int rt_ipa_host(const char* who, bool wide, porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t* alpha_be,
                       const uint8_t* rows, const uint8_t* macs, const uint8_t* prf, const uint8_t* align, const unsigned long long* write_steps,
                       size_t n_rows, size_t n_total, int form, uint8_t* out, uint8_t* status, unsigned int* counts) {
    if (!rows || !macs || !prf || !status) return bad_arg(who, "rows, macs, prf or status is NULL");
    int rc = rt_check_shape(who, n_rows, n_total);
    if (rc) return rc;
    if ((rc = rt_check_form(who, form))) return rc;
    if (write_steps && form == PORLA_ICC_DECODE_EXACT) return bad_arg(who, "write_steps with PORLA_ICC_DECODE_EXACT: the unscale is the residue forms'");
    if (wide && !alpha_be) return bad_arg(who, "alpha_be is NULL");
    if (!alpha_generators_fb || !h_fb) return bad_arg(who, "a NULL base");
    if ((rc = ensure_device())) return rc;
    if ((rc = rt_ipa_bases(who, alpha_generators_fb, h_fb))) return rc;
    uint32_t alpha[8] = {0};
    if (alpha_be) rt_ipa_alpha(alpha_be, alpha);
    return rt_host(who, rows, macs, prf, align, write_steps, n_rows, IPA_COLS, form, out, status, counts,
                   [&](RetrieveWs* ws, const porla_retrieve_aligned_req* R, hipStream_t s) {
                       return rt_enqueue<Secp256k1G>(ws, &alpha_generators_fb->secp, &h_fb->secp, alpha, RtReqs{R, true}, 1, n_rows, IPA_COLS,
                                                     n_total, form, s);
                   });
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_retrieve_req) == PORLA_RETRIEVE_REQ_BYTES, "porla_retrieve_req size");
static_assert(offsetof(porla_retrieve_req, d_rows) == 0 && offsetof(porla_retrieve_req, d_macs) == 8 && offsetof(porla_retrieve_req, d_prf) == 16 &&
              offsetof(porla_retrieve_req, d_out) == 24 && offsetof(porla_retrieve_req, d_status) == 32 &&
              offsetof(porla_retrieve_req, d_counts) == 40,
              "porla_retrieve_req offsets (include/porla_gpu.h)");
static_assert(sizeof(porla_retrieve_aligned_req) == PORLA_RETRIEVE_ALIGNED_REQ_BYTES, "porla_retrieve_aligned_req size");
static_assert(offsetof(porla_retrieve_aligned_req, d_rows) == 0 && offsetof(porla_retrieve_aligned_req, d_macs) == 8 &&
              offsetof(porla_retrieve_aligned_req, d_prf) == 16 && offsetof(porla_retrieve_aligned_req, d_align) == 24 &&
              offsetof(porla_retrieve_aligned_req, d_write_steps) == 32 && offsetof(porla_retrieve_aligned_req, d_out) == 40 &&
              offsetof(porla_retrieve_aligned_req, d_status) == 48 && offsetof(porla_retrieve_aligned_req, d_counts) == 56,
              "porla_retrieve_aligned_req offsets (include/porla_gpu.h)");
static_assert(offsetof(RtDesc, rows) == 0 && offsetof(RtDesc, macs) == 8 && offsetof(RtDesc, prf) == 16 && offsetof(RtDesc, align) == 24 &&
              offsetof(RtDesc, steps) == 32 && offsetof(RtDesc, out) == 40 && offsetof(RtDesc, status) == 48 && offsetof(RtDesc, counts) == 56,
              "RtDesc is porla_retrieve_aligned_req field for field");

extern "C" int porla_kzg_retrieve_batch_device(const porla_retrieve_req* reqs, size_t k, size_t n_rows, size_t n_total, void* hip_stream) {
    return rt_kzg_device("porla_kzg_retrieve_batch_device", RtReqs{reqs, false}, k, n_rows, n_total, PORLA_ICC_DECODE_EXACT, hip_stream);
}

extern "C" int porla_ipa_retrieve_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const porla_retrieve_req* reqs,
                                               size_t k, size_t n_rows, size_t n_total, void* hip_stream) {
    return rt_ipa_device("porla_ipa_retrieve_batch_device", alpha_generators_fb, h_fb, nullptr, RtReqs{reqs, false}, k, n_rows, n_total,
                         PORLA_ICC_DECODE_EXACT, hip_stream);
}

extern "C" int porla_kzg_retrieve_host(const uint8_t* rows, const uint8_t* macs, const uint8_t* prf, size_t n_rows, size_t n_total, uint8_t* out,
                                       uint8_t* status, unsigned int* counts) {
    return rt_kzg_host("porla_kzg_retrieve_host", rows, macs, prf, nullptr, nullptr, n_rows, n_total, PORLA_ICC_DECODE_EXACT, out, status, counts);
}

extern "C" int porla_ipa_retrieve_host(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t* rows, const uint8_t* macs,
                                       const uint8_t* prf, size_t n_rows, size_t n_total, uint8_t* out, uint8_t* status, unsigned int* counts) {
    return rt_ipa_host("porla_ipa_retrieve_host", false, alpha_generators_fb, h_fb, nullptr, rows, macs, prf, nullptr, nullptr, n_rows, n_total,
                       PORLA_ICC_DECODE_EXACT, out, status, counts);
}

extern "C" int porla_kzg_retrieve_aligned_batch_device(const porla_retrieve_aligned_req* reqs, size_t k, size_t n_rows, size_t n_total, int form,
                                                       void* hip_stream) {
    return rt_kzg_device("porla_kzg_retrieve_aligned_batch_device", RtReqs{reqs, true}, k, n_rows, n_total, form, hip_stream);
}

extern "C" int porla_ipa_retrieve_aligned_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32],
                                                       const porla_retrieve_aligned_req* reqs, size_t k, size_t n_rows, size_t n_total,
                                                       int form, void* hip_stream) {
    return rt_ipa_device("porla_ipa_retrieve_aligned_batch_device", alpha_generators_fb, h_fb, alpha_be, RtReqs{reqs, true}, k, n_rows, n_total,
                         form, hip_stream);
}

extern "C" int porla_kzg_retrieve_aligned_host(const uint8_t* rows, const uint8_t* macs, const uint8_t* prf, const uint8_t* align,
                                               const unsigned long long* write_steps, size_t n_rows, size_t n_total, int form, uint8_t* out,
                                               uint8_t* status, unsigned int* counts) {
    return rt_kzg_host("porla_kzg_retrieve_aligned_host", rows, macs, prf, align, write_steps, n_rows, n_total, form, out, status, counts);
}

extern "C" int porla_ipa_retrieve_aligned_host(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32],
                                               const uint8_t* rows, const uint8_t* macs, const uint8_t* prf, const uint8_t* align,
                                               const unsigned long long* write_steps, size_t n_rows, size_t n_total, int form, uint8_t* out,
                                               uint8_t* status, unsigned int* counts) {
    return rt_ipa_host("porla_ipa_retrieve_aligned_host", true, alpha_generators_fb, h_fb, alpha_be, rows, macs, prf, align, write_steps, n_rows,
                       n_total, form, out, status, counts);
}

// The verified file extraction (include/porla_gpu.h: porla_{kzg,ipa}_extract_batch_device and, with the lower levels' Y halves as a
// second source, porla_{kzg,ipa}_extract_xy_batch_device, and with the top level's Y half row by row,
// porla_{kzg,ipa}_extract_xyt_batch_device): every resident level of K files checked row by row against its stored MAC
// rows, the halves decoded, and the decoded blocks merged into each file's block store by "newest authentic copy wins", in ONE
// asynchronous call.  Kernels and the layout of a file's rows: extract_batch.hip.h.  All three pairs of entry points go through ex_check
// and ex_enqueue; a request of the first pair is one of the second without Y stores, one of the second one of the third with top_y =
// 0.  Every step is on the caller's stream.  The launch sequence depends on the symbol widths and the pass classes present in the call
// (levels of up to 2^9 rows, larger ones; among the X halves, among the tried Y halves) and on whether a top level's Y half is tried
// at all, never on K and never on which levels are resident:
//
//   upload                the files (ExFile), the halves as requests of the row check (RtDesc) and their start rows, one copy
//   k_ex_clear            counters, failed-level masks, decode counters, the ranks and doubts of all slots, the untried Y statuses
//   k_ex_ysteps           a Y half tried: the write steps of the lower-level entries, for the unscale
//   the row check         retrieve_batch.hip: rt_check_starts_{kzg,ipa}, the aligned retrieval's launches with the search map -- one
//                         pass over ALL halves of 64-byte symbols (the lower levels' X and tried Y halves, an exact top level and
//                         its tried Y half), one over the RESIDUE32 top levels and their tried Y halves
//   k_ex_top_patch        a top level's Y half tried: the half its decode reads, X rows where they checked OK, wt^-1 Y rows elsewhere
//   the decodes           icc_decode_ragged_enqueue ONCE over the lower levels' X halves of two rows and more (into d_work) and the
//                         exact top levels (into d_blocks): at most three pass launches whatever sizes are present; the uniform
//                         icc_decode_form_enqueue for RESIDUE32 top levels; k_ex_level0 for the one-row level; the tried Y halves of
//                         two rows and more in the form RESIDUE64 into d_work_y, one ragged call again, icc_decode_row0_enqueue for
//                         level 0's Y row
//   k_ex_verdict, k_ex_rank, k_ex_gather       the merge
#include "extract_batch.hip.h"
#include "write_batch_host.hpp"
#include "../../include/porla_gpu.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

namespace porla {

// retrieve_batch.hip: the row check of halves of unequal sizes, under the retrieval's workspace
int rt_check_starts_kzg(bool aligned, const RtDesc* d_desc, const RtMapStarts& map, size_t rows, size_t ncols, size_t symb, hipStream_t stream);
int rt_check_starts_ipa(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint32_t alpha[8], bool aligned, const RtDesc* d_desc,
                        const RtMapStarts& map, size_t rows, size_t symb, hipStream_t stream);

struct ExtractWs {
    std::mutex mu;
    int device = -1;
    Buf list, scratch, doubt, ysteps;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<ExtractWs> g_ex_ws;

// the requests of a call: an array of porla_extract_req (kind 0), of porla_extract_xy_req (1) or of porla_extract_xyt_req (2), read as
// the widest -- the first has no Y stores, the second no top-level Y half
struct ExReqs {
    const void* p;
    int kind;
    size_t stride() const {
        return kind == 2 ? sizeof(porla_extract_xyt_req) : kind == 1 ? sizeof(porla_extract_xy_req) : sizeof(porla_extract_req);
    }
    porla_extract_xyt_req at(size_t a) const {
        porla_extract_xyt_req R;
        memset(&R, 0, sizeof R);
        memcpy(&R, (const uint8_t*)p + a * stride(), stride());
        return R;
    }
    size_t counts_bytes() const { return kind == 2 ? 32 : kind == 1 ? 24 : 16; }
};

static inline uint32_t ex_t(const porla_extract_xyt_req& R, size_t n_total) { return (uint32_t)(R.write_step % n_total); }
static inline uint32_t ex_tried(const porla_extract_xyt_req& R, size_t n_total) { return (uint32_t)(R.y_levels & ex_t(R, n_total)); }
// the top level's Y half is tried
static inline bool ex_top_tried(const porla_extract_xyt_req& R) { return R.top_y == 1 && R.d_top_rows != nullptr; }

// the checks made before the device is touched; n_cols: the row width the buffers are sized by
static int ex_check(const char* who, const ExReqs& reqs, size_t k, size_t n_cols, size_t n_total, int top_form) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs.p) return bad("reqs is NULL");
    if (int rc = check_n_total(who, n_total, 16)) return rc;
    if (top_form != PORLA_ICC_DECODE_EXACT && top_form != PORLA_ICC_DECODE_RESIDUE32)
        return bad("top_form must be PORLA_ICC_DECODE_EXACT or PORLA_ICC_DECODE_RESIDUE32");
    if (int rc = check_request_count(who, k)) return rc;
    size_t bb, top_b, blocks_b, rows_all;
    // (the kernels number the rows of the call through in 32 bits)
    if (!mul_ok(n_cols, 64, &bb) || !mul_ok(bb, n_total, &top_b) ||
        (k && (!mul_ok((size_t)(2 + reqs.kind) * n_total, k, &rows_all) || rows_all > 0xffffffffull)))
        return bad("a byte size overflows: the rows of the call do not fit a buffer");
    bb /= 2;                                                                 // a decoded block
    blocks_b = top_b / 2;
    top_b = top_form == PORLA_ICC_DECODE_RESIDUE32 ? blocks_b : top_b;
    const int logn = ilog2u(n_total);
    struct Range { uintptr_t lo, hi; bool out; };
    std::vector<Range> ranges;
    bool wraps = false;
    auto add = [&](const void* p, size_t bytes, bool out) {
        const uintptr_t lo = (uintptr_t)p;
        if (lo + bytes < lo) wraps = true;
        ranges.push_back(Range{lo, lo + bytes, out});
    };
    for (size_t a = 0; a < k; a++) {
        const porla_extract_xyt_req R = reqs.at(a);
        const std::string at = "request " + std::to_string(a) + ": ";
        const uint32_t t = ex_t(R, n_total), ym = ex_tried(R, n_total);
        const bool ty = ex_top_tried(R);
        if (R.top_y > 1) return bad(at + "top_y must be 0 or 1");
        if (ty && (!R.d_top_rows_y || !R.d_top_macs_y || !R.d_prf_top_y || !R.d_top_patch || !R.d_row_status_top_y))
            return bad(at + "a NULL d_top_rows_y, d_top_macs_y, d_prf_top_y, d_top_patch or d_row_status_top_y with the top level's Y half to try");
        if (((uintptr_t)R.d_top_rows_y | (uintptr_t)R.d_top_macs_y | (uintptr_t)R.d_top_align_y | (uintptr_t)R.d_prf_top_y |
             (uintptr_t)R.d_top_patch | (uintptr_t)R.d_row_status_top_y) & 15u)
            return bad(at + "d_top_rows_y, d_top_macs_y, d_top_align_y, d_prf_top_y, d_top_patch or d_row_status_top_y is not 16-byte aligned");
        const size_t rows = t + (R.d_top_rows ? n_total : 0);
        if (!R.d_blocks || !R.d_steps || !R.d_flags) return bad(at + "a NULL d_blocks, d_steps or d_flags");
        if (rows && (!R.d_prf || !R.d_row_status)) return bad(at + "a NULL d_prf or d_row_status");
        if (R.d_top_rows && !R.d_top_macs) return bad(at + "a NULL d_top_macs");
        if (t && (!R.data_x || !R.mac_x || !R.d_work)) return bad(at + "a NULL data_x, mac_x or d_work with resident lower levels");
        if (ym && (!R.data_y || !R.mac_y || !R.align_y || !R.d_prf_y || !R.d_work_y || !R.d_row_status_y))
            return bad(at + "a NULL data_y, mac_y, align_y, d_prf_y, d_work_y or d_row_status_y with a Y half to try");
        if (((uintptr_t)R.d_top_rows | (uintptr_t)R.d_top_macs | (uintptr_t)R.d_top_align | (uintptr_t)R.d_prf | (uintptr_t)R.d_work |
             (uintptr_t)R.d_blocks) & 15u)
            return bad(at + "d_top_rows, d_top_macs, d_top_align, d_prf, d_work or d_blocks is not 16-byte aligned");
        if (((uintptr_t)R.d_prf_y | (uintptr_t)R.d_work_y) & 15u) return bad(at + "d_prf_y or d_work_y is not 16-byte aligned");
        if (((uintptr_t)R.d_steps | (uintptr_t)R.d_counts) & 3u) return bad(at + "d_steps or d_counts is not 4-byte aligned");
        for (int i = 0; i < logn; i++) {
            if (!(t >> i & 1u)) continue;
            const void *dx = R.data_x[i], *mx = R.mac_x[i];
            if (!dx || !mx) return bad(at + "resident level " + std::to_string(i) + " has a NULL pointer in data_x or mac_x");
            if (((uintptr_t)dx | (uintptr_t)mx) & 15u) return bad(at + "a level pointer of data_x or mac_x is not 16-byte aligned");
            add(dx, ((size_t)2 * bb) << i, false);
            add(mx, (size_t)64 << i, false);
            if (!(ym >> i & 1u)) continue;
            const void *dy = R.data_y[i], *my = R.mac_y[i], *ay = R.align_y[i];
            if (!dy || !my) return bad(at + "tried level " + std::to_string(i) + " has a NULL pointer in data_y or mac_y");
            if (((uintptr_t)dy | (uintptr_t)my | (uintptr_t)ay) & 15u)
                return bad(at + "a level pointer of data_y, mac_y or align_y is not 16-byte aligned");
            add(dy, ((size_t)2 * bb) << i, false);
            add(my, (size_t)64 << i, false);
            if (ay) add(ay, (size_t)64 << i, false);
        }
        if (R.d_top_rows) {
            add(R.d_top_rows, top_b, false);
            add(R.d_top_macs, 64 * n_total, false);
            if (R.d_top_align) add(R.d_top_align, 64 * n_total, false);
        }
        if (ty) {
            add(R.d_top_rows_y, top_b, false);
            add(R.d_top_macs_y, 64 * n_total, false);
            if (R.d_top_align_y) add(R.d_top_align_y, 64 * n_total, false);
            add(R.d_prf_top_y, 16 * n_total, false);
            add(R.d_top_patch, top_b, true);
        }
        if (R.d_row_status_top_y) add(R.d_row_status_top_y, n_total, true);               // (untried: filled with NOT_TRIED)
        if (rows) {
            add(R.d_prf, 16 * rows, false);
            add(R.d_row_status, rows, true);
        }
        if (t) add(R.d_work, (size_t)t * bb, true);
        if (t && R.d_prf_y) add(R.d_prf_y, (size_t)16 * t, false);
        if (t && R.d_work_y) add(R.d_work_y, (size_t)t * bb, true);
        if (t && R.d_row_status_y) add(R.d_row_status_y, t, true);
        add(R.d_blocks, blocks_b, true);
        add(R.d_steps, 4 * n_total, true);
        add(R.d_flags, n_total, true);
        if (R.d_counts) add(R.d_counts, reqs.counts_bytes(), true);
        if (wraps) return bad(at + "a byte size overflows: a buffer wraps around the address space");
    }
    // an output may overlap nothing, inputs may be shared (retrieve_batch.hip: the same walk)
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uintptr_t end_any = 0, end_out = 0;
    for (const Range& r : ranges) {
        if (r.lo < (r.out ? end_any : end_out))
            return bad(std::string("an output (d_work, d_blocks, d_steps, d_flags, d_row_status") +
                       (reqs.kind ? ", d_work_y, d_row_status_y" : "") + (reqs.kind == 2 ? ", d_top_patch, d_row_status_top_y" : "") +
                       " or d_counts) overlaps an input or output of this call: outputs must be disjoint from everything");
        end_any = std::max(end_any, r.hi);
        if (r.out) end_out = std::max(end_out, r.hi);
    }
    return PORLA_OK;
}

// ws->mu held, ws->fence entered; arguments checked.  fb_alpha == nullptr: the KZG build
static int ex_enqueue(ExtractWs* ws, porla_fixed_base* fb_alpha, porla_fixed_base* fb_h, const uint32_t* alpha_ipa, const ExReqs& reqs, size_t k,
                      size_t ncols, size_t n_total, int top_form, hipStream_t stream) {
    int rc;
    const bool kzg = fb_alpha == nullptr, residue = top_form == PORLA_ICC_DECODE_RESIDUE32;
    const int logn = ilog2u(n_total), curve = kzg ? 0 : 1;
    const size_t bb = ncols * 32;
    // the halves as requests of the row check, per symbol width, and the files
    std::vector<RtDesc> desc[2];
    std::vector<uint32_t> starts[2];
    uint32_t rows_of[2] = {0, 0};
    bool aligned[2] = {false, false};
    std::vector<ExFile> files(k);
    std::vector<porla_icc_decode_ragged_req> dec, dec_y;               // the EXACT decodes; the tried Y halves of two rows and more
    std::vector<porla_icc_decode_req> dec_top32, dec_y0;               // RESIDUE32 top levels; level 0's Y rows
    uint32_t t_max = 0, rows_max = 0;
    bool level0 = false, any_y = false, any_top_y = false;
    for (size_t a = 0; a < k; a++) {
        any_y = any_y || ex_tried(reqs.at(a), n_total) != 0;
        any_top_y = any_top_y || ex_top_tried(reqs.at(a));
    }
    if ((rc = ws->scratch.ensure(k * EX_SCRATCH_WORDS * 4))) return rc;
    if (any_y && ((rc = ws->doubt.ensure(k * n_total * 4)) || (rc = ws->ysteps.ensure(k * n_total * 8)))) return rc;
    for (size_t a = 0; a < k; a++) {
        const porla_extract_xyt_req R = reqs.at(a);
        const uint32_t t = ex_t(R, n_total), ym = ex_tried(R, n_total);
        const bool ty = ex_top_tried(R);
        uint32_t* scratch = (uint32_t*)ws->scratch.p + a * EX_SCRATCH_WORDS;
        unsigned long long* ysteps = ym ? (unsigned long long*)ws->ysteps.p + a * n_total : nullptr;
        ExFile& F = files[a];
        F.level0 = (t & 1u) ? (const uint8_t*)R.data_x[0] : nullptr;
        F.status = R.d_row_status;
        F.work = (uint8_t*)R.d_work;
        F.blocks = (uint8_t*)R.d_blocks;
        F.steps = R.d_steps;
        F.flags = R.d_flags;
        F.counts = R.d_counts;
        F.scratch = scratch;
        F.status_y = t ? R.d_row_status_y : nullptr;
        F.work_y = (const uint8_t*)R.d_work_y;
        F.doubt = ym ? (uint32_t*)ws->doubt.p + a * n_total : nullptr;
        F.ysteps = ysteps;
        F.epoch = R.write_step - t;
        F.t = t;
        F.has_top = R.d_top_rows != nullptr;
        F.y_tried = ym;
        F.n_counts = (uint32_t)(reqs.counts_bytes() / 4);
        F.status_top_y = R.d_row_status_top_y;
        F.top_x = (const uint8_t*)R.d_top_rows;
        F.top_rows_y = (const uint8_t*)R.d_top_rows_y;
        F.top_patch = (uint8_t*)R.d_top_patch;
        F.top_y = ty ? 1u : 0u;
        F.top_e = (uint32_t)rev_bits(R.top_step % n_total, logn);
        level0 = level0 || (t & 1u);
        t_max = std::max(t_max, t);
        rows_max = std::max(rows_max, t + (F.has_top ? (uint32_t)n_total : 0u));
        auto half = [&](int w, const RtDesc& D, size_t n) {
            desc[w].push_back(D);
            starts[w].push_back(rows_of[w]);
            rows_of[w] += (uint32_t)n;
            aligned[w] = aligned[w] || D.align;
        };
        auto half_x = [&](int w, const void* rows, const void* macs, const void* align, size_t off, size_t n) {
            half(w, RtDesc{(const uint8_t*)rows, (const uint8_t*)macs, (const uint8_t*)R.d_prf + 16 * off, (const uint8_t*)align, nullptr, nullptr,
                           R.d_row_status + off, R.d_counts}, n);
        };
        for (int i = 0; i < logn; i++) {
            if (!(t >> i & 1u)) continue;
            const size_t off = t & ((1u << i) - 1u);
            half_x(0, R.data_x[i], R.mac_x[i], nullptr, off, (size_t)1 << i);
            if (i) dec.push_back(porla_icc_decode_ragged_req{R.data_x[i], (uint8_t*)R.d_work + off * bb, nullptr, scratch + 1 + i, 1ull << i});
        }
        // the tried Y halves: further halves of the 64-byte pass, their failures counted in d_counts[4]
        for (int i = 0; i < logn; i++) {
            if (!(ym >> i & 1u)) continue;
            const size_t off = t & ((1u << i) - 1u);
            half(0, RtDesc{(const uint8_t*)R.data_y[i], (const uint8_t*)R.mac_y[i], (const uint8_t*)R.d_prf_y + 16 * off, (const uint8_t*)R.align_y[i],
                           nullptr, nullptr, R.d_row_status_y + off, R.d_counts ? R.d_counts + 4 : nullptr}, (size_t)1 << i);
            if (i) dec_y.push_back(porla_icc_decode_ragged_req{R.data_y[i], (uint8_t*)R.d_work_y + off * bb, ysteps + off, nullptr, 1ull << i});
            else dec_y0.push_back(porla_icc_decode_req{R.data_y[i], (uint8_t*)R.d_work_y + off * bb, ysteps + off, nullptr});
        }
        if (F.has_top) {
            half_x(residue ? 1 : 0, R.d_top_rows, R.d_top_macs, R.d_top_align, t, n_total);
            // the top level's tried Y half: one more half of the same pass, its failures counted in d_counts[6]; the decode then reads
            // the patched half
            if (ty)
                half(residue ? 1 : 0, RtDesc{(const uint8_t*)R.d_top_rows_y, (const uint8_t*)R.d_top_macs_y, (const uint8_t*)R.d_prf_top_y,
                                             (const uint8_t*)R.d_top_align_y, nullptr, nullptr, R.d_row_status_top_y,
                                             R.d_counts ? R.d_counts + 6 : nullptr}, n_total);
            const void* top_rows = ty ? R.d_top_patch : R.d_top_rows;
            if (residue) dec_top32.push_back(porla_icc_decode_req{top_rows, R.d_blocks, nullptr, nullptr});
            else dec.push_back(porla_icc_decode_ragged_req{top_rows, R.d_blocks, nullptr, scratch + 1 + logn, (unsigned long long)n_total});
        }
    }
    // one upload: files, requests of both widths, start rows of both widths
    const size_t files_b = k * sizeof(ExFile), d0_b = desc[0].size() * sizeof(RtDesc), d1_b = desc[1].size() * sizeof(RtDesc);
    const size_t s0_b = starts[0].size() * 4, s1_b = starts[1].size() * 4, list_b = files_b + d0_b + d1_b + s0_b + s1_b;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    if ((rc = ws->list.ensure(list_b))) return rc;
    uint8_t* h = (uint8_t*)ws->h_list.h;
    memcpy(h, files.data(), files_b);
    if (d0_b) memcpy(h + files_b, desc[0].data(), d0_b);
    if (d1_b) memcpy(h + files_b + d0_b, desc[1].data(), d1_b);
    if (s0_b) memcpy(h + files_b + d0_b + d1_b, starts[0].data(), s0_b);
    if (s1_b) memcpy(h + files_b + d0_b + d1_b + s0_b, starts[1].data(), s1_b);
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const uint8_t* d = (const uint8_t*)ws->list.p;
    const ExFile* d_files = (const ExFile*)d;
    const RtDesc* d_desc[2] = {(const RtDesc*)(d + files_b), (const RtDesc*)(d + files_b + d0_b)};
    const uint32_t* d_starts[2] = {(const uint32_t*)(d + files_b + d0_b + d1_b), (const uint32_t*)(d + files_b + d0_b + d1_b + s0_b)};
    const unsigned ky = (unsigned)k;
    auto blocks_of = [](size_t items) { return (unsigned)std::max<size_t>((items + 255) / 256, 1); };
    {
        ProfScope ps("extract_clear", stream);
        hipLaunchKernelGGL(k_ex_clear, dim3(blocks_of(n_total), ky), dim3(256), 0, stream, d_files, (uint32_t)n_total);
        PORLA_HIP(hipGetLastError());
    }
    if (any_y) {
        ProfScope ps("extract_ysteps", stream);
        hipLaunchKernelGGL(k_ex_ysteps, dim3(blocks_of(t_max), ky), dim3(256), 0, stream, d_files);
        PORLA_HIP(hipGetLastError());
    }
    // the row check: one pass per symbol width present
    for (int w = 0; w < 2; w++) {
        if (!rows_of[w]) continue;
        const RtMapStarts map{d_starts[w], (uint32_t)desc[w].size()};
        const size_t symb = w ? 32 : 64;
        rc = kzg ? rt_check_starts_kzg(aligned[w], d_desc[w], map, rows_of[w], ncols, symb, stream)
                 : rt_check_starts_ipa(fb_alpha, fb_h, alpha_ipa, aligned[w], d_desc[w], map, rows_of[w], symb, stream);
        if (rc) return rc;
    }
    // the patched top halves, under the data side's table lease
    if (any_top_y) {
        const uint32_t *twp = nullptr, *twqi = nullptr;
        if ((rc = icc_decode_tables_acquire(curve, n_total, !residue, stream, &twp, &twqi))) return rc;
        {
            ProfScope ps("extract_top_patch", stream);
            const dim3 grid(blocks_of(n_total * ncols), ky), block(256);
            if (residue)
                hipLaunchKernelGGL((k_ex_top_patch<PORLA_ICC_DECODE_RESIDUE32, IccBn254Fr>), grid, block, 0, stream, d_files, twp, twqi,
                                   (uint32_t)n_total, (uint32_t)ncols);
            else if (kzg)
                hipLaunchKernelGGL((k_ex_top_patch<PORLA_ICC_DECODE_EXACT, IccBn254Fr>), grid, block, 0, stream, d_files, twp, twqi,
                                   (uint32_t)n_total, (uint32_t)ncols);
            else
                hipLaunchKernelGGL((k_ex_top_patch<PORLA_ICC_DECODE_EXACT, IccSecp256k1Fn>), grid, block, 0, stream, d_files, twp, twqi,
                                   (uint32_t)n_total, (uint32_t)ncols);
        }
        if (hipGetLastError() != hipSuccess) { set_last_error("porla: extraction: the top-level patch launch failed"); rc = PORLA_ERR_HIP; }
        const int r1 = icc_mix_tables_release(stream);
        if (rc || r1) return rc ? rc : r1;
    }
    // the decodes: one ragged call over every size present; RESIDUE32 top levels are of one size and keep the uniform call
    if (level0) {
        ProfScope ps("extract_level0", stream);
        hipLaunchKernelGGL(k_ex_level0, dim3(blocks_of(ncols), ky), dim3(256), 0, stream, d_files, (uint32_t)ncols);
        PORLA_HIP(hipGetLastError());
    }
    if ((rc = icc_decode_ragged_enqueue(dec.data(), dec.size(), ncols, n_total, curve, PORLA_ICC_DECODE_EXACT, stream))) return rc;
    if (!dec_top32.empty() &&
        (rc = icc_decode_form_enqueue(dec_top32.data(), dec_top32.size(), n_total, ncols, n_total, curve, PORLA_ICC_DECODE_RESIDUE32, stream)))
        return rc;
    // ... and the tried Y halves
    if (!dec_y0.empty() && (rc = icc_decode_row0_enqueue(dec_y0.data(), dec_y0.size(), ncols, n_total, curve, stream))) return rc;
    if ((rc = icc_decode_ragged_enqueue(dec_y.data(), dec_y.size(), ncols, n_total, curve, PORLA_ICC_DECODE_RESIDUE64, stream))) return rc;
    // the merge
    ProfScope ps("extract_merge", stream);
    hipLaunchKernelGGL(k_ex_verdict, dim3(blocks_of(rows_max), ky), dim3(256), 0, stream, d_files, (uint32_t)n_total, (uint32_t)logn);
    hipLaunchKernelGGL(k_ex_rank, dim3(blocks_of(t_max), ky), dim3(256), 0, stream, d_files, (uint32_t)n_total, (uint32_t)ncols);
    hipLaunchKernelGGL(k_ex_gather, dim3((unsigned)n_total, ky), dim3(64), 0, stream, d_files, (uint32_t)ncols, (uint32_t)logn,
                       residue ? 1u : 0u);
    PORLA_HIP(hipGetLastError());
    return PORLA_OK;
}

static int ex_kzg(const char* who, const ExReqs& reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    // the row width for the refusals: the SRS size, or one column while there is no SRS (the call then ends in PORLA_ERR_STATE or
    // PORLA_ERR_NO_DEVICE, and the refusals that do not depend on the width have been made)
    const size_t width = std::max<size_t>(kzg_n_samples(), 1);
    int rc = ex_check(who, reqs, k, width, n_total, top_form);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = client_kzg_row_width(&n))) return rc;
    if (n != width && (rc = ex_check(who, reqs, k, n, n_total, top_form))) return rc;         // (an SRS made since the first look)
    ExtractWs* ws = nullptr;
    if ((rc = g_ex_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return ex_enqueue(ws, nullptr, nullptr, nullptr, reqs, k, n, n_total, top_form, stream); });
}

static int ex_ipa(const char* who, porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32], const ExReqs& reqs,
                  size_t k, size_t n_total, int top_form, void* hip_stream) {
    int rc = ex_check(who, reqs, k, IPA_COLS, n_total, top_form);
    if (rc) return rc;
    if (!alpha_be) return bad_arg(who, "alpha_be is NULL");
    if (k == 0) return PORLA_OK;
    if (!alpha_generators_fb || !h_fb) return bad_arg(who, "a NULL base");
    if ((rc = ensure_device())) return rc;
    if ((rc = ipa_check_generators(who, "alpha_generators_fb", alpha_generators_fb))) return rc;
    if ((rc = ipa_check_hiding_base(who, "h_fb", h_fb))) return rc;
    uint32_t alpha[8];
    h_load_be(alpha, alpha_be);
    fe_reduce_plain<IccCurve<Secp256k1G>::Q>(alpha, 8);
    ExtractWs* ws = nullptr;
    if ((rc = g_ex_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run(
        [&] { return ex_enqueue(ws, alpha_generators_fb, h_fb, alpha, reqs, k, IPA_COLS, n_total, top_form, stream); });
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_extract_req) == PORLA_EXTRACT_REQ_BYTES, "porla_extract_req size");
static_assert(offsetof(porla_extract_req, write_step) == 0 && offsetof(porla_extract_req, data_x) == 8 && offsetof(porla_extract_req, mac_x) == 16 &&
              offsetof(porla_extract_req, d_top_rows) == 24 && offsetof(porla_extract_req, d_top_macs) == 32 &&
              offsetof(porla_extract_req, d_top_align) == 40 && offsetof(porla_extract_req, d_prf) == 48 &&
              offsetof(porla_extract_req, d_work) == 56 && offsetof(porla_extract_req, d_blocks) == 64 &&
              offsetof(porla_extract_req, d_steps) == 72 && offsetof(porla_extract_req, d_flags) == 80 &&
              offsetof(porla_extract_req, d_row_status) == 88 && offsetof(porla_extract_req, d_counts) == 96,
              "porla_extract_req offsets (include/porla_gpu.h)");
static_assert(sizeof(porla_extract_xy_req) == PORLA_EXTRACT_XY_REQ_BYTES, "porla_extract_xy_req size");
static_assert(offsetof(porla_extract_xy_req, write_step) == 0 && offsetof(porla_extract_xy_req, data_x) == 8 &&
              offsetof(porla_extract_xy_req, mac_x) == 16 && offsetof(porla_extract_xy_req, d_top_rows) == 24 &&
              offsetof(porla_extract_xy_req, d_top_macs) == 32 && offsetof(porla_extract_xy_req, d_top_align) == 40 &&
              offsetof(porla_extract_xy_req, d_prf) == 48 && offsetof(porla_extract_xy_req, d_work) == 56 &&
              offsetof(porla_extract_xy_req, d_blocks) == 64 && offsetof(porla_extract_xy_req, d_steps) == 72 &&
              offsetof(porla_extract_xy_req, d_flags) == 80 && offsetof(porla_extract_xy_req, d_row_status) == 88 &&
              offsetof(porla_extract_xy_req, d_counts) == 96 && offsetof(porla_extract_xy_req, data_y) == 104 &&
              offsetof(porla_extract_xy_req, mac_y) == 112 && offsetof(porla_extract_xy_req, align_y) == 120 &&
              offsetof(porla_extract_xy_req, d_prf_y) == 128 && offsetof(porla_extract_xy_req, d_work_y) == 136 &&
              offsetof(porla_extract_xy_req, d_row_status_y) == 144 && offsetof(porla_extract_xy_req, y_levels) == 152,
              "porla_extract_xy_req offsets (include/porla_gpu.h): porla_extract_req field for field, then the Y stores");

static_assert(sizeof(porla_extract_xyt_req) == PORLA_EXTRACT_XYT_REQ_BYTES, "porla_extract_xyt_req size");
static_assert(offsetof(porla_extract_xyt_req, write_step) == 0 && offsetof(porla_extract_xyt_req, data_x) == 8 &&
              offsetof(porla_extract_xyt_req, mac_x) == 16 && offsetof(porla_extract_xyt_req, d_top_rows) == 24 &&
              offsetof(porla_extract_xyt_req, d_top_macs) == 32 && offsetof(porla_extract_xyt_req, d_top_align) == 40 &&
              offsetof(porla_extract_xyt_req, d_prf) == 48 && offsetof(porla_extract_xyt_req, d_work) == 56 &&
              offsetof(porla_extract_xyt_req, d_blocks) == 64 && offsetof(porla_extract_xyt_req, d_steps) == 72 &&
              offsetof(porla_extract_xyt_req, d_flags) == 80 && offsetof(porla_extract_xyt_req, d_row_status) == 88 &&
              offsetof(porla_extract_xyt_req, d_counts) == 96 && offsetof(porla_extract_xyt_req, data_y) == 104 &&
              offsetof(porla_extract_xyt_req, mac_y) == 112 && offsetof(porla_extract_xyt_req, align_y) == 120 &&
              offsetof(porla_extract_xyt_req, d_prf_y) == 128 && offsetof(porla_extract_xyt_req, d_work_y) == 136 &&
              offsetof(porla_extract_xyt_req, d_row_status_y) == 144 && offsetof(porla_extract_xyt_req, y_levels) == 152 &&
              offsetof(porla_extract_xyt_req, d_top_rows_y) == 160 && offsetof(porla_extract_xyt_req, d_top_macs_y) == 168 &&
              offsetof(porla_extract_xyt_req, d_top_align_y) == 176 && offsetof(porla_extract_xyt_req, d_prf_top_y) == 184 &&
              offsetof(porla_extract_xyt_req, d_top_patch) == 192 && offsetof(porla_extract_xyt_req, d_row_status_top_y) == 200 &&
              offsetof(porla_extract_xyt_req, top_step) == 208 && offsetof(porla_extract_xyt_req, top_y) == 216,
              "porla_extract_xyt_req offsets (include/porla_gpu.h): porla_extract_xy_req field for field, then the top level's Y half");

extern "C" int porla_kzg_extract_batch_device(const porla_extract_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    return ex_kzg("porla_kzg_extract_batch_device", ExReqs{reqs, 0}, k, n_total, top_form, hip_stream);
}

extern "C" int porla_ipa_extract_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32],
                                              const porla_extract_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    return ex_ipa("porla_ipa_extract_batch_device", alpha_generators_fb, h_fb, alpha_be, ExReqs{reqs, 0}, k, n_total, top_form, hip_stream);
}

extern "C" int porla_kzg_extract_xy_batch_device(const porla_extract_xy_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    return ex_kzg("porla_kzg_extract_xy_batch_device", ExReqs{reqs, 1}, k, n_total, top_form, hip_stream);
}

extern "C" int porla_ipa_extract_xy_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32],
                                                 const porla_extract_xy_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    return ex_ipa("porla_ipa_extract_xy_batch_device", alpha_generators_fb, h_fb, alpha_be, ExReqs{reqs, 1}, k, n_total, top_form,
                  hip_stream);
}

extern "C" int porla_kzg_extract_xyt_batch_device(const porla_extract_xyt_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    return ex_kzg("porla_kzg_extract_xyt_batch_device", ExReqs{reqs, 2}, k, n_total, top_form, hip_stream);
}

extern "C" int porla_ipa_extract_xyt_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32],
                                                  const porla_extract_xyt_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    return ex_ipa("porla_ipa_extract_xyt_batch_device", alpha_generators_fb, h_fb, alpha_be, ExReqs{reqs, 2}, k, n_total, top_form,
                  hip_stream);
}

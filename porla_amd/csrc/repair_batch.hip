// The top-level repair (include/porla_gpu.h: porla_{kzg,ipa}_repair_top_batch_device): the rows of K files' top levels that fail
// their check while their sibling in the other half passes are written back IN PLACE, data row and MAC row, in ONE asynchronous call.
// Kernels: repair_batch.hip.h.  Every step is on the caller's stream, and the launch sequence depends neither on K nor on which rows
// are damaged nor on whether any are:
//
//   upload                the files (RpFile), the halves as requests of the row check and of the write pass (RtDesc), their start rows
//   k_rp_clear            the action bytes and the counters
//   the row check         retrieve_batch.hip: rt_check_starts_{kzg,ipa} -- both halves of all files are halves of ONE pass
//   k_rp_patch            the data rows, both directions: wt^-1 Y_j over a repairable X row, wt X_j over a repairable Y row
//   the write pass        retrieve_batch.hip: rt_write_starts_{kzg,ipa} -- the check's expected-MAC stages over all rows of both halves
//                         as they lie now; the last kernel writes the repairable rows' MAC bytes instead of comparing
#include "repair_batch.hip.h"
#include "write_batch_host.hpp"
#include "../../include/porla_gpu.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

namespace porla {

// retrieve_batch.hip: the row check of halves of unequal sizes and its writing twin, under the retrieval's workspace
int rt_check_starts_kzg(bool aligned, const RtDesc* d_desc, const RtMapStarts& map, size_t rows, size_t ncols, size_t symb, hipStream_t stream);
int rt_check_starts_ipa(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint32_t alpha[8], bool aligned, const RtDesc* d_desc,
                        const RtMapStarts& map, size_t rows, size_t symb, hipStream_t stream);
int rt_write_starts_kzg(bool aligned, const RtDesc* d_desc, const RtMapStarts& map, size_t rows, size_t ncols, size_t symb, hipStream_t stream);
int rt_write_starts_ipa(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint32_t alpha[8], bool aligned, const RtDesc* d_desc,
                        const RtMapStarts& map, size_t rows, size_t symb, hipStream_t stream);

struct RepairWs {
    std::mutex mu;
    int device = -1;
    Buf list;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<RepairWs> g_rp_ws;

// the checks made before the device is touched; n_cols: the row width the buffers are sized by
static int rp_check(const char* who, const porla_repair_top_req* reqs, size_t k, size_t n_cols, size_t n_total, int top_form) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = check_n_total(who, n_total, 16)) return rc;
    if (top_form != PORLA_ICC_DECODE_EXACT && top_form != PORLA_ICC_DECODE_RESIDUE32)
        return bad("top_form must be PORLA_ICC_DECODE_EXACT or PORLA_ICC_DECODE_RESIDUE32");
    if (int rc = check_request_count(who, k)) return rc;
    size_t half_b, rows_all;
    // (the kernels number the rows of the call through in 32 bits)
    if (!mul_ok(n_cols, 64, &half_b) || !mul_ok(half_b, n_total, &half_b) || (k && (!mul_ok(2 * n_total, k, &rows_all) || rows_all > 0xffffffffull)))
        return bad("a byte size overflows: the rows of the call do not fit a buffer");
    if (top_form == PORLA_ICC_DECODE_RESIDUE32) half_b /= 2;
    struct Range { uintptr_t lo, hi; bool out; };
    std::vector<Range> ranges;
    ranges.reserve(13 * k);
    bool wraps = false;
    auto add = [&](const void* p, size_t bytes, bool out) {
        const uintptr_t lo = (uintptr_t)p;
        if (lo + bytes < lo) wraps = true;
        ranges.push_back(Range{lo, lo + bytes, out});
    };
    for (size_t a = 0; a < k; a++) {
        const porla_repair_top_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        if (!R.d_rows_x || !R.d_macs_x || !R.d_rows_y || !R.d_macs_y) return bad(at + "a NULL d_rows_x, d_macs_x, d_rows_y or d_macs_y");
        if (!R.d_prf_x || !R.d_prf_y) return bad(at + "a NULL d_prf_x or d_prf_y");
        if (!R.d_status_x || !R.d_status_y) return bad(at + "a NULL d_status_x or d_status_y");
        if (!R.d_action_x || !R.d_action_y) return bad(at + "a NULL d_action_x or d_action_y");
        if (((uintptr_t)R.d_rows_x | (uintptr_t)R.d_macs_x | (uintptr_t)R.d_align_x | (uintptr_t)R.d_prf_x | (uintptr_t)R.d_rows_y |
             (uintptr_t)R.d_macs_y | (uintptr_t)R.d_align_y | (uintptr_t)R.d_prf_y) & 15u)
            return bad(at + "a store, alignment or PRF pointer is not 16-byte aligned");
        if ((uintptr_t)R.d_counts & 3u) return bad(at + "d_counts is not 4-byte aligned");
        if (R.reserved != 0) return bad(at + "reserved must be 0");
        add(R.d_rows_x, half_b, true);
        add(R.d_macs_x, 64 * n_total, true);
        add(R.d_rows_y, half_b, true);
        add(R.d_macs_y, 64 * n_total, true);
        if (R.d_align_x) add(R.d_align_x, 64 * n_total, false);
        if (R.d_align_y) add(R.d_align_y, 64 * n_total, false);
        add(R.d_prf_x, 16 * n_total, false);
        add(R.d_prf_y, 16 * n_total, false);
        add(R.d_status_x, n_total, true);
        add(R.d_status_y, n_total, true);
        add(R.d_action_x, n_total, true);
        add(R.d_action_y, n_total, true);
        if (R.d_counts) add(R.d_counts, 32, true);
        if (wraps) return bad(at + "a byte size overflows: a buffer wraps around the address space");
    }
    // an output may overlap nothing, inputs may be shared (retrieve_batch.hip: the same walk); the stores are written: outputs
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uintptr_t end_any = 0, end_out = 0;
    for (const Range& r : ranges) {
        if (r.lo < (r.out ? end_any : end_out))
            return bad("an output (d_rows_x, d_macs_x, d_rows_y, d_macs_y, d_status_x, d_status_y, d_action_x, d_action_y or d_counts) overlaps an "
                       "input or output of this call: the stores are written, outputs must be disjoint from everything");
        end_any = std::max(end_any, r.hi);
        if (r.out) end_out = std::max(end_out, r.hi);
    }
    return PORLA_OK;
}

// ws->mu held, ws->fence entered; arguments checked.  fb_alpha == nullptr: the KZG build
static int rp_enqueue(RepairWs* ws, porla_fixed_base* fb_alpha, porla_fixed_base* fb_h, const uint32_t* alpha_ipa, const porla_repair_top_req* reqs,
                      size_t k, size_t ncols, size_t n_total, int top_form, hipStream_t stream) {
    int rc;
    const bool kzg = fb_alpha == nullptr, residue = top_form == PORLA_ICC_DECODE_RESIDUE32;
    const int logn = ilog2u(n_total), curve = kzg ? 0 : 1;
    const size_t symb = residue ? 32 : 64, halves = 2 * k, rows = halves * n_total;
    // the files; the halves as requests of the check pass and of the write pass (RtActWrite: what its members mean); their start rows
    std::vector<RpFile> files(k);
    std::vector<RtDesc> check(halves), write(halves);
    std::vector<uint32_t> starts(halves);
    bool aligned = false;
    for (size_t a = 0; a < k; a++) {
        const porla_repair_top_req& R = reqs[a];
        RpFile& F = files[a];
        F.rows[0] = (uint8_t*)R.d_rows_x; F.rows[1] = (uint8_t*)R.d_rows_y;
        F.status[0] = R.d_status_x; F.status[1] = R.d_status_y;
        F.action[0] = R.d_action_x; F.action[1] = R.d_action_y;
        F.counts = R.d_counts;
        F.e = (uint32_t)rev_bits(R.top_step % n_total, logn);
        F.pad = 0;
        const uint8_t* macs[2] = {(const uint8_t*)R.d_macs_x, (const uint8_t*)R.d_macs_y};
        const uint8_t* prf[2] = {(const uint8_t*)R.d_prf_x, (const uint8_t*)R.d_prf_y};
        const uint8_t* align[2] = {(const uint8_t*)R.d_align_x, (const uint8_t*)R.d_align_y};
        for (int h = 0; h < 2; h++) {
            check[2 * a + h] = RtDesc{F.rows[h], macs[h], prf[h], align[h], nullptr, nullptr, (uint8_t*)F.status[h],
                                      R.d_counts ? R.d_counts + h : nullptr};
            write[2 * a + h] = RtDesc{F.rows[h], macs[h], prf[h], align[h], (const unsigned long long*)F.status[h ^ 1], F.action[h],
                                      (uint8_t*)F.status[h], R.d_counts ? R.d_counts + 2 + 2 * h : nullptr};
            starts[2 * a + h] = (uint32_t)((2 * a + h) * n_total);
            aligned = aligned || align[h];
        }
    }
    // one upload
    const size_t files_b = k * sizeof(RpFile), desc_b = halves * sizeof(RtDesc), starts_b = halves * 4, list_b = files_b + 2 * desc_b + starts_b;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    if ((rc = ws->list.ensure(list_b))) return rc;
    uint8_t* h = (uint8_t*)ws->h_list.h;
    memcpy(h, files.data(), files_b);
    memcpy(h + files_b, check.data(), desc_b);
    memcpy(h + files_b + desc_b, write.data(), desc_b);
    memcpy(h + files_b + 2 * desc_b, starts.data(), starts_b);
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const uint8_t* d = (const uint8_t*)ws->list.p;
    const RpFile* d_files = (const RpFile*)d;
    const RtDesc *d_check = (const RtDesc*)(d + files_b), *d_write = (const RtDesc*)(d + files_b + desc_b);
    const RtMapStarts map{(const uint32_t*)(d + files_b + 2 * desc_b), (uint32_t)halves};
    const unsigned ky = (unsigned)k;
    auto blocks_of = [](size_t items) { return (unsigned)std::max<size_t>((items + 255) / 256, 1); };
    {
        ProfScope ps("repair_clear", stream);
        hipLaunchKernelGGL(k_rp_clear, dim3(blocks_of(n_total), ky), dim3(256), 0, stream, d_files, (uint32_t)n_total);
        PORLA_HIP(hipGetLastError());
    }
    // the statuses of all rows of both halves
    rc = kzg ? rt_check_starts_kzg(aligned, d_check, map, rows, ncols, symb, stream)
             : rt_check_starts_ipa(fb_alpha, fb_h, alpha_ipa, aligned, d_check, map, rows, symb, stream);
    if (rc) return rc;
    // the data rows, under the data side's table lease
    {
        const uint32_t *twp = nullptr, *twq = nullptr, *twqi = nullptr;
        if ((rc = icc_scale_tables_acquire(curve, n_total, !residue, stream, &twp, &twq, &twqi))) return rc;
        {
            ProfScope ps("repair_patch", stream);
            const dim3 grid(blocks_of(2 * n_total * ncols), ky), block(256);
            if (residue)
                hipLaunchKernelGGL((k_rp_patch<PORLA_ICC_DECODE_RESIDUE32, IccBn254Fr>), grid, block, 0, stream, d_files, twp, twq, twqi,
                                   (uint32_t)n_total, (uint32_t)ncols);
            else if (kzg)
                hipLaunchKernelGGL((k_rp_patch<PORLA_ICC_DECODE_EXACT, IccBn254Fr>), grid, block, 0, stream, d_files, twp, twq, twqi,
                                   (uint32_t)n_total, (uint32_t)ncols);
            else
                hipLaunchKernelGGL((k_rp_patch<PORLA_ICC_DECODE_EXACT, IccSecp256k1Fn>), grid, block, 0, stream, d_files, twp, twq, twqi,
                                   (uint32_t)n_total, (uint32_t)ncols);
        }
        if (hipGetLastError() != hipSuccess) { set_last_error("porla: repair: the data-row patch launch failed"); rc = PORLA_ERR_HIP; }
        const int r1 = icc_mix_tables_release(stream);
        if (rc || r1) return rc ? rc : r1;
    }
    // the MAC rows: the expected MACs of the rows as repaired, written over the repairable rows'
    return kzg ? rt_write_starts_kzg(aligned, d_write, map, rows, ncols, symb, stream)
               : rt_write_starts_ipa(fb_alpha, fb_h, alpha_ipa, aligned, d_write, map, rows, symb, stream);
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_repair_top_req) == PORLA_REPAIR_TOP_REQ_BYTES, "porla_repair_top_req size");
static_assert(offsetof(porla_repair_top_req, d_rows_x) == 0 && offsetof(porla_repair_top_req, d_macs_x) == 8 &&
              offsetof(porla_repair_top_req, d_align_x) == 16 && offsetof(porla_repair_top_req, d_prf_x) == 24 &&
              offsetof(porla_repair_top_req, d_rows_y) == 32 && offsetof(porla_repair_top_req, d_macs_y) == 40 &&
              offsetof(porla_repair_top_req, d_align_y) == 48 && offsetof(porla_repair_top_req, d_prf_y) == 56 &&
              offsetof(porla_repair_top_req, d_status_x) == 64 && offsetof(porla_repair_top_req, d_status_y) == 72 &&
              offsetof(porla_repair_top_req, d_action_x) == 80 && offsetof(porla_repair_top_req, d_action_y) == 88 &&
              offsetof(porla_repair_top_req, d_counts) == 96 && offsetof(porla_repair_top_req, top_step) == 104 &&
              offsetof(porla_repair_top_req, reserved) == 112,
              "porla_repair_top_req offsets (include/porla_gpu.h)");

extern "C" int porla_kzg_repair_top_batch_device(const porla_repair_top_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    const char* who = "porla_kzg_repair_top_batch_device";
    // the row width for the refusals: the SRS size, or one column while there is no SRS (the call then ends in PORLA_ERR_STATE or
    // PORLA_ERR_NO_DEVICE, and the refusals that do not depend on the width have been made)
    const size_t width = std::max<size_t>(kzg_n_samples(), 1);
    int rc = rp_check(who, reqs, k, width, n_total, top_form);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = client_kzg_row_width(&n))) return rc;
    if (n != width && (rc = rp_check(who, reqs, k, n, n_total, top_form))) return rc;            // (an SRS made since the first look)
    RepairWs* ws = nullptr;
    if ((rc = g_rp_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return rp_enqueue(ws, nullptr, nullptr, nullptr, reqs, k, n, n_total, top_form, stream); });
}

extern "C" int porla_ipa_repair_top_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32],
                                                 const porla_repair_top_req* reqs, size_t k, size_t n_total, int top_form, void* hip_stream) {
    const char* who = "porla_ipa_repair_top_batch_device";
    int rc = rp_check(who, reqs, k, IPA_COLS, n_total, top_form);
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
    RepairWs* ws = nullptr;
    if ((rc = g_rp_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run(
        [&] { return rp_enqueue(ws, alpha_generators_fb, h_fb, alpha, reqs, k, IPA_COLS, n_total, top_form, stream); });
}

// The lower-level repair (include/porla_gpu.h: porla_{kzg,ipa}_repair_levels_batch_device): the rows of K files' lower-level Y halves
// that fail their check are rebuilt from the levels' X halves and written back IN PLACE -- data row, alignment row and MAC row -- in
// ONE asynchronous call.  Kernels, layouts and the state word of a level: repair_levels_batch.hip.h.  Every step is on the caller's
// stream, and the launch sequence depends on which level sizes are named in the call, never on K, on which rows are damaged or on
// whether any are:
//
//   upload                the files (RlFile), the halves as requests of the row check and of the write pass (RtDesc), their start rows,
//                         the named levels of two rows and more as items of the data passes (RlItem), grouped by size
//   fill                  the rows of alignment scalars: zero (the commitment pass runs over all named rows)
//   k_rl_clear            actions, verdicts, counters, states, row words, permits; NOT_TRIED for the rows of unnamed levels
//   the row check         retrieve_batch.hip: rt_check_starts_{kzg,ipa} -- the X and Y halves of all named levels are halves of ONE pass
//   k_rl_plan             the state word of every named level                              (stages marked * read it and leave at once
//   the X decode          icc_decode.hip: icc_decode_ragged_enqueue, EXACT, into d_work     for a level that is not under repair)
//   k_rl_hadd *           y_p over the chunks, c_p beside them; level 0's candidate row and row of scalars
//   k_rl_data *           per level size: the passes over the rows y_p -> the candidate data rows, then over the rows c_p on the q plane
//                         -> the rows of alignment scalars; blockIdx.y = the named level
//   the commitment pass   kzg_state.hpp: commit_rows_then over all named rows, and k_rl_align under the table's lock: the candidate
//                         alignment rows as affine bytes
//   k_rl_compare *        the witnesses
//   k_rl_write *          data and alignment bytes of the failed rows of the repaired levels; their permits
//   the write pass        retrieve_batch.hip: rt_write_starts_{kzg,ipa} over the Y halves -- the expected MACs of the rows as they lie now,
//                         written over the permitted rows' MAC bytes
//   k_rl_tally            action bytes, counters, verdicts
#include "repair_levels_batch.hip.h"
#include "kzg_state.hpp"
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

struct RepairLevelsWs {
    std::mutex mu;
    int device = -1;
    Buf list, scalars, align, rowstate;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<RepairLevelsWs> g_rl_ws;

constexpr size_t RL_ROWS_CEIL = (size_t)1 << 18;        // named rows of one call: their rows of alignment scalars are one workspace
constexpr size_t RL_WORK_PER_SYMBOL = 200;              // d_work: 32 (chunk, then y_p) + 32 (c_p) + 64 (candidate) + 72 (two residue planes)

static inline uint32_t rl_t(const porla_repair_levels_req& R, size_t n_total) { return (uint32_t)(R.write_step % n_total); }
static inline uint32_t rl_named(const porla_repair_levels_req& R, size_t n_total) { return (uint32_t)(R.levels & rl_t(R, n_total)); }

// the checks made before the device is touched; n_cols: the row width the buffers are sized by
static int rl_check(const char* who, const porla_repair_levels_req* reqs, size_t k, size_t n_cols, size_t n_total) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = check_n_total(who, n_total, 16)) return rc;
    if (int rc = check_request_count(who, k)) return rc;
    size_t row_b, t_;
    if (!mul_ok(n_cols, 64, &row_b) || !mul_ok(row_b, n_total, &t_) || !mul_ok(n_cols * n_total, RL_WORK_PER_SYMBOL, &t_))
        return bad("a byte size overflows: the rows of a level do not fit a buffer");
    const int logn = ilog2u(n_total);
    struct Range { uintptr_t lo, hi; bool out; };
    std::vector<Range> ranges;
    bool wraps = false;
    auto add = [&](const void* p, size_t bytes, bool out) {
        const uintptr_t lo = (uintptr_t)p;
        if (lo + bytes < lo) wraps = true;
        ranges.push_back(Range{lo, lo + bytes, out});
    };
    size_t named_rows = 0;
    for (size_t a = 0; a < k; a++) {
        const porla_repair_levels_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        const uint32_t t = rl_t(R, n_total), m = rl_named(R, n_total);
        if (R.reserved != 0) return bad(at + "reserved must be 0");
        if (!R.d_level) return bad(at + "a NULL d_level");
        if (t && (!R.d_status_x || !R.d_status_y || !R.d_action_y)) return bad(at + "a NULL d_status_x, d_status_y or d_action_y with resident lower levels");
        if (m && (!R.data_x || !R.mac_x || !R.data_y || !R.mac_y || !R.align_y))
            return bad(at + "a NULL data_x, mac_x, data_y, mac_y or align_y with a named level");
        if (m && (!R.d_prf_x || !R.d_prf_y || !R.d_work)) return bad(at + "a NULL d_prf_x, d_prf_y or d_work with a named level");
        if (((uintptr_t)R.d_prf_x | (uintptr_t)R.d_prf_y | (uintptr_t)R.d_work) & 15u) return bad(at + "d_prf_x, d_prf_y or d_work is not 16-byte aligned");
        if ((uintptr_t)R.d_counts & 3u) return bad(at + "d_counts is not 4-byte aligned");
        for (int i = 0; i < logn; i++) {
            if (!(m >> i & 1u)) continue;
            const void* fam[5] = {R.data_x[i], R.mac_x[i], R.data_y[i], R.mac_y[i], R.align_y[i]};
            uintptr_t bits = 0;
            for (const void* p : fam) {
                if (!p) return bad(at + "named level " + std::to_string(i) + " has a NULL pointer in data_x, mac_x, data_y, mac_y or align_y");
                bits |= (uintptr_t)p;
            }
            if (bits & 15u) return bad(at + "a level pointer of data_x, mac_x, data_y, mac_y or align_y is not 16-byte aligned");
            add(fam[0], row_b << i, false);
            add(fam[1], (size_t)64 << i, false);
            add(fam[2], row_b << i, true);
            add(fam[3], (size_t)64 << i, true);
            add(fam[4], (size_t)64 << i, true);
        }
        if (m) {
            add(R.d_prf_x, (size_t)16 * t, false);
            add(R.d_prf_y, (size_t)16 * t, false);
            add(R.d_work, (size_t)m * n_cols * RL_WORK_PER_SYMBOL, true);
        }
        if (t) {
            add(R.d_status_x, t, true);
            add(R.d_status_y, t, true);
            add(R.d_action_y, t, true);
        }
        add(R.d_level, RL_MAX_LEVELS, true);
        if (R.d_counts) add(R.d_counts, 32, true);
        if (wraps) return bad(at + "a byte size overflows: a buffer wraps around the address space");
        named_rows += m;
    }
    if (named_rows > RL_ROWS_CEIL) return bad("more than 2^18 named rows in one call: the workspace of alignment scalars stops there");
    // an output may overlap nothing, inputs may be shared (retrieve_batch.hip: the same walk); the Y stores are written: outputs
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uintptr_t end_any = 0, end_out = 0;
    for (const Range& r : ranges) {
        if (r.lo < (r.out ? end_any : end_out))
            return bad("an output (a level of data_y, mac_y or align_y, d_work, d_status_x, d_status_y, d_action_y, d_level or d_counts) overlaps an "
                       "input or output of this call: the Y stores are written, outputs must be disjoint from everything");
        end_any = std::max(end_any, r.hi);
        if (r.out) end_out = std::max(end_out, r.hi);
    }
    return PORLA_OK;
}

// the passes of the data network over the named levels of 2^lg rows (items d_items[0 .. count)): the rows y_p on both planes, then
// the rows c_p on the q plane.  The data side's table lease is held.
template <class Q>
static void rl_launch_size(const RlItem* d_items, size_t count, int lg, size_t ncols, size_t n_total, const uint32_t* twp, const uint32_t* twq,
                           hipStream_t stream) {
    IccPass plan[ICC_MAX_PASSES];
    const int passes = icc_pass_plan(lg, ncols, plan);
    const size_t plane_words = (ncols << lg) * ICC30_PLANE_WORDS;
    for (int data = 1; data >= 0; data--) {
        for (int pz = 0; pz < passes; pz++) {
            const int s = plan[pz].s, ns = plan[pz].ns, cc_log = plan[pz].cc_log;
            const dim3 grid((unsigned)(plan[pz].col_tiles * (((size_t)1 << lg) >> ns)), (unsigned)count);
            const bool first = pz == 0, last = pz == passes - 1;
            ProfScope ps(data ? "repair_levels_data" : "repair_levels_scalars", stream);
#define PORLA_RL_LAUNCH(F, L, D)                                                                                                      \
    hipLaunchKernelGGL((k_rl_data<Q, F, L, D>), grid, dim3(ICC30_SPLIT_THREADS), 0, stream, d_items, plane_words, twp, twq, (uint32_t)n_total, \
                       (uint32_t)ncols, s, ns, cc_log)
            if (data) {
                if (first && last) PORLA_RL_LAUNCH(true, true, true);
                else if (first) PORLA_RL_LAUNCH(true, false, true);
                else if (last) PORLA_RL_LAUNCH(false, true, true);
                else PORLA_RL_LAUNCH(false, false, true);
            } else {
                if (first && last) PORLA_RL_LAUNCH(true, true, false);
                else if (first) PORLA_RL_LAUNCH(true, false, false);
                else if (last) PORLA_RL_LAUNCH(false, true, false);
                else PORLA_RL_LAUNCH(false, false, false);
            }
#undef PORLA_RL_LAUNCH
        }
    }
}

// ws->mu held, ws->fence entered; arguments checked.  kzg: fb == nullptr (the resident SRS), fb_alpha / fb_h / alpha_ipa unused
template <class C>
static int rl_enqueue(RepairLevelsWs* ws, FixedBase<C>* fb, porla_fixed_base* fb_alpha, porla_fixed_base* fb_h, const uint32_t* alpha_ipa,
                      const RlScale& scale, const porla_repair_levels_req* reqs, size_t k, size_t ncols, size_t n_total, hipStream_t stream) {
    using Q = typename IccCurve<C>::Q;
    using M = typename C::Fp;
    constexpr bool kzg = std::is_same<C, Bn254G1>::value;
    int rc;
    const int logn = ilog2u(n_total), curve = IccCurve<C>::id;
    const size_t B = ncols * 32;
    size_t rows_t = 0, rows_m = 0;
    uint32_t t_max = 0, m_max = 0;
    for (size_t a = 0; a < k; a++) {
        const uint32_t t = rl_t(reqs[a], n_total), m = rl_named(reqs[a], n_total);
        rows_t += t; rows_m += m;
        t_max = std::max(t_max, t); m_max = std::max(m_max, m);
    }
    // the workspace: the rows of alignment scalars and the candidate alignment rows of all named rows, files end to end; per file the
    // state words, per row of the t layouts a word and a permit byte
    const size_t state_b = k * RL_STATE_WORDS * 4, bits_b = rows_t * 4;
    if ((rc = ws->rowstate.ensure(state_b + bits_b + rows_t))) return rc;
    if ((rc = ws->scalars.ensure(rows_m * B))) return rc;
    if ((rc = ws->align.ensure(rows_m * 64))) return rc;
    uint8_t* const d_scalars = (uint8_t*)ws->scalars.p;
    uint8_t* const d_align = (uint8_t*)ws->align.p;
    uint32_t* const d_state = (uint32_t*)ws->rowstate.p;
    uint32_t* const d_bits = (uint32_t*)((uint8_t*)ws->rowstate.p + state_b);
    uint8_t* const d_permit = (uint8_t*)ws->rowstate.p + state_b + bits_b;
    std::vector<RlFile> files(k);
    std::vector<RtDesc> check_x, check_y, write;
    std::vector<uint32_t> starts_w;
    std::vector<std::vector<RlItem>> items(logn);
    std::vector<porla_icc_decode_ragged_req> dec;
    size_t at_t = 0, at_m = 0;
    for (size_t a = 0; a < k; a++) {
        const porla_repair_levels_req& R = reqs[a];
        const uint32_t t = rl_t(R, n_total), m = rl_named(R, n_total);
        RlFile& F = files[a];
        memset(&F, 0, sizeof F);
        F.status_x = R.d_status_x; F.status_y = R.d_status_y; F.action_y = R.d_action_y;
        F.verdict = R.d_level; F.counts = R.d_counts; F.work = (uint8_t*)R.d_work;
        F.state = d_state + a * RL_STATE_WORDS;
        F.rowbits = d_bits + at_t;
        F.permit = d_permit + at_t;
        F.epoch = R.write_step - t;
        F.t = t; F.m = m; F.row0 = (uint32_t)at_m;
        for (int i = 0; i < logn; i++) {
            if (!(m >> i & 1u)) continue;
            const size_t off_t = t & ((1u << i) - 1u), off_m = m & ((1u << i) - 1u), n = (size_t)1 << i;
            F.data_y[i] = (uint8_t*)R.data_y[i];
            F.align_y[i] = (uint8_t*)R.align_y[i];
            if (i == 0) F.level0_x = (const uint8_t*)R.data_x[0];
            check_x.push_back(RtDesc{(const uint8_t*)R.data_x[i], (const uint8_t*)R.mac_x[i], (const uint8_t*)R.d_prf_x + 16 * off_t, nullptr, nullptr,
                                     nullptr, R.d_status_x + off_t, R.d_counts});
            check_y.push_back(RtDesc{(const uint8_t*)R.data_y[i], (const uint8_t*)R.mac_y[i], (const uint8_t*)R.d_prf_y + 16 * off_t,
                                     (const uint8_t*)R.align_y[i], nullptr, nullptr, R.d_status_y + off_t, R.d_counts ? R.d_counts + 1 : nullptr});
            // the write pass (RtActWrite): `steps` the row permits, `out` the action bytes; the tally counts, not this pass
            write.push_back(RtDesc{(const uint8_t*)R.data_y[i], (const uint8_t*)R.mac_y[i], (const uint8_t*)R.d_prf_y + 16 * off_t,
                                   (const uint8_t*)R.align_y[i], (const unsigned long long*)(F.permit + off_t), R.d_action_y + off_t,
                                   R.d_status_y + off_t, nullptr});
            starts_w.push_back((uint32_t)(at_m + off_m));
            if (i == 0) continue;
            uint8_t* const w = (uint8_t*)R.d_work;
            dec.push_back(porla_icc_decode_ragged_req{R.data_x[i], w + off_m * B, nullptr, F.state + RL_MAX_LEVELS + i, (unsigned long long)n});
            items[i].push_back(RlItem{w + off_m * B, w + (m + off_m) * B, w + (2 * (size_t)m + 2 * off_m) * B,
                                      d_scalars + (at_m + off_m) * B,
                                      (uint32_t*)(w + 4 * (size_t)m * B + off_m * ncols * 2 * ICC30_PLANE_WORDS * 4), F.state + i});
        }
        at_t += t; at_m += m;
    }
    const unsigned ky = (unsigned)k;
    auto blocks_of = [](size_t n) { return (unsigned)std::max<size_t>((n + 255) / 256, 1); };
    // the check's requests: the X halves, then the Y halves; both kinds in the m layout's order, so the Y starts are the write pass's + rows_m
    const size_t halves = check_x.size();
    std::vector<uint32_t> starts_c(2 * halves);
    for (size_t h = 0; h < halves; h++) { starts_c[h] = starts_w[h]; starts_c[halves + h] = (uint32_t)rows_m + starts_w[h]; }
    size_t n_items = 0;
    for (const auto& v : items) n_items += v.size();
    // one upload
    const size_t files_b = k * sizeof(RlFile), half_b = halves * sizeof(RtDesc), items_b = n_items * sizeof(RlItem);
    const size_t list_b = files_b + 3 * half_b + items_b + 3 * halves * 4;
    if ((rc = ws->h_list.stage(list_b))) return rc;
    if ((rc = ws->list.ensure(list_b))) return rc;
    {
        uint8_t* h = (uint8_t*)ws->h_list.h;
        memcpy(h, files.data(), files_b); h += files_b;
        if (half_b) {
            memcpy(h, check_x.data(), half_b); h += half_b;
            memcpy(h, check_y.data(), half_b); h += half_b;
            memcpy(h, write.data(), half_b); h += half_b;
        }
        for (const auto& v : items)
            if (!v.empty()) { memcpy(h, v.data(), v.size() * sizeof(RlItem)); h += v.size() * sizeof(RlItem); }
        if (halves) {
            memcpy(h, starts_c.data(), 2 * halves * 4); h += 2 * halves * 4;
            memcpy(h, starts_w.data(), halves * 4);
        }
    }
    if ((rc = ws->h_list.send(ws->list.p, list_b, stream))) return rc;
    const uint8_t* d = (const uint8_t*)ws->list.p;
    const RlFile* d_files = (const RlFile*)d;
    const RtDesc *d_check = (const RtDesc*)(d + files_b), *d_write = (const RtDesc*)(d + files_b + 2 * half_b);
    const RlItem* d_items = (const RlItem*)(d + files_b + 3 * half_b);
    const uint32_t* d_starts_c = (const uint32_t*)(d + files_b + 3 * half_b + items_b);
    const RtMapStarts map_c{d_starts_c, (uint32_t)(2 * halves)}, map_w{d_starts_c + 2 * halves, (uint32_t)halves};
    if (rows_m) PORLA_HIP(hipMemsetAsync(d_scalars, 0, rows_m * B, stream));
    {
        ProfScope ps("repair_levels_clear", stream);
        hipLaunchKernelGGL(k_rl_clear, dim3(blocks_of(std::max<size_t>(t_max, RL_STATE_WORDS)), ky), dim3(256), 0, stream, d_files);
        PORLA_HIP(hipGetLastError());
    }
    if (!rows_m) return PORLA_OK;
    // the statuses of all named rows of both halves
    rc = kzg ? rt_check_starts_kzg(true, d_check, map_c, 2 * rows_m, ncols, 64, stream)
             : rt_check_starts_ipa(fb_alpha, fb_h, alpha_ipa, true, d_check, map_c, 2 * rows_m, 64, stream);
    if (rc) return rc;
    {
        ProfScope ps("repair_levels_plan", stream);
        hipLaunchKernelGGL(k_rl_plan, dim3(blocks_of(t_max), ky), dim3(256), 0, stream, d_files);
        PORLA_HIP(hipGetLastError());
    }
    // the chunks of the named X halves of two rows and more (under the decode's own lease of the data side's tables)
    if ((rc = icc_decode_ragged_enqueue(dec.data(), dec.size(), ncols, n_total, curve, PORLA_ICC_DECODE_EXACT, stream))) return rc;
    // y_p, c_p and the two networks, under the data side's table lease
    {
        const uint32_t *twp = nullptr, *twq = nullptr;
        if ((rc = icc_encode_tables_acquire(curve, n_total, stream, &twp, &twq))) return rc;
        {
            ProfScope ps("repair_levels_hadd", stream);
            hipLaunchKernelGGL((k_rl_hadd<Q>), dim3(blocks_of((size_t)m_max * ncols), ky), dim3(256), 0, stream, d_files, twp, twq, (uint32_t)n_total,
                               logn, (uint32_t)ncols, d_scalars, scale);
        }
        const RlItem* at = d_items;
        for (int i = 1; i < logn; i++) {
            if (items[i].empty()) continue;
            rl_launch_size<Q>(at, items[i].size(), i, ncols, n_total, twp, twq, stream);
            at += items[i].size();
        }
        if (hipGetLastError() != hipSuccess) { set_last_error("porla: lower-level repair: a data launch failed"); rc = PORLA_ERR_HIP; }
        const int r1 = icc_mix_tables_release(stream);
        if (rc || r1) return rc ? rc : r1;
    }
    // the candidate alignment rows: one commitment per named row
    auto affine = [&](const XYZZ<M>* sums, uint32_t S) {
        ProfScope ps("repair_levels_align", stream);
        hipLaunchKernelGGL((k_rl_align<C>), dim3(blocks_of(rows_m)), dim3(256), 0, stream, sums, S, (uint32_t)rows_m, d_align);
        PORLA_HIP(hipGetLastError());
        return (int)PORLA_OK;
    };
    if ((rc = commit_rows_then(fb, d_scalars, rows_m, ncols, stream, affine))) return rc;
    {
        ProfScope ps("repair_levels_compare", stream);
        hipLaunchKernelGGL(k_rl_compare, dim3(blocks_of((size_t)m_max * ncols), ky), dim3(256), 0, stream, d_files, (uint32_t)ncols, d_align);
        PORLA_HIP(hipGetLastError());
    }
    {
        ProfScope ps("repair_levels_write", stream);
        hipLaunchKernelGGL(k_rl_write, dim3(blocks_of((size_t)m_max * ncols), ky), dim3(256), 0, stream, d_files, (uint32_t)ncols, d_align);
        PORLA_HIP(hipGetLastError());
    }
    // the MAC rows: the expected MACs of the Y rows as they lie now, written over the permitted rows'
    rc = kzg ? rt_write_starts_kzg(true, d_write, map_w, rows_m, ncols, 64, stream)
             : rt_write_starts_ipa(fb_alpha, fb_h, alpha_ipa, true, d_write, map_w, rows_m, 64, stream);
    if (rc) return rc;
    ProfScope ps("repair_levels_tally", stream);
    hipLaunchKernelGGL(k_rl_tally, dim3(blocks_of(t_max), ky), dim3(256), 0, stream, d_files);
    PORLA_HIP(hipGetLastError());
    return PORLA_OK;
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_repair_levels_req) == PORLA_REPAIR_LEVELS_REQ_BYTES, "porla_repair_levels_req size");
static_assert(offsetof(porla_repair_levels_req, write_step) == 0 && offsetof(porla_repair_levels_req, levels) == 8 &&
              offsetof(porla_repair_levels_req, data_x) == 16 && offsetof(porla_repair_levels_req, mac_x) == 24 &&
              offsetof(porla_repair_levels_req, d_prf_x) == 32 && offsetof(porla_repair_levels_req, d_prf_y) == 40 &&
              offsetof(porla_repair_levels_req, data_y) == 48 && offsetof(porla_repair_levels_req, mac_y) == 56 &&
              offsetof(porla_repair_levels_req, align_y) == 64 && offsetof(porla_repair_levels_req, d_work) == 72 &&
              offsetof(porla_repair_levels_req, d_status_x) == 80 && offsetof(porla_repair_levels_req, d_status_y) == 88 &&
              offsetof(porla_repair_levels_req, d_action_y) == 96 && offsetof(porla_repair_levels_req, d_level) == 104 &&
              offsetof(porla_repair_levels_req, d_counts) == 112 && offsetof(porla_repair_levels_req, reserved) == 120,
              "porla_repair_levels_req offsets (include/porla_gpu.h)");
static_assert(RL_MAX_LEVELS == 16, "d_level is 16 bytes (include/porla_gpu.h)");

extern "C" size_t porla_repair_levels_work_bytes(size_t n_total, size_t n_cols, unsigned long long write_step, unsigned long long levels) {
    if (n_total < 2 || (n_total & (n_total - 1)) != 0 || n_total > ((size_t)1 << 16)) return 0;
    const size_t m = (size_t)(levels & (write_step % n_total));
    size_t b;
    if (!mul_ok(n_cols, RL_WORK_PER_SYMBOL, &b) || !mul_ok(b, m, &b)) return 0;
    return b;
}

extern "C" int porla_kzg_repair_levels_batch_device(const porla_repair_levels_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    const char* who = "porla_kzg_repair_levels_batch_device";
    // the row width for the refusals: the SRS size, or one column while there is no SRS (the call then ends in PORLA_ERR_STATE or
    // PORLA_ERR_NO_DEVICE, and the refusals that do not depend on the width have been made)
    const size_t width = std::max<size_t>(kzg_n_samples(), 1);
    int rc = rl_check(who, reqs, k, width, n_total);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    size_t n;
    if ((rc = client_kzg_row_width(&n))) return rc;
    if (n != width && (rc = rl_check(who, reqs, k, n, n_total))) return rc;                     // (an SRS made since the first look)
    RepairLevelsWs* ws = nullptr;
    if ((rc = g_rl_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const RlScale scale{{0, 0, 0, 0, 0, 0, 0, 0}, 0};
    return FencedCall(ws, stream).run([&] {
        return rl_enqueue<Bn254G1>(ws, (FixedBase<Bn254G1>*)nullptr, nullptr, nullptr, nullptr, scale, reqs, k, n, n_total, stream);
    });
}

extern "C" int porla_ipa_repair_levels_batch_device(porla_fixed_base* alpha_generators_fb, porla_fixed_base* h_fb, const uint8_t alpha_be[32],
                                                    const porla_repair_levels_req* reqs, size_t k, size_t n_total, void* hip_stream) {
    using Q = IccCurve<Secp256k1G>::Q;
    const char* who = "porla_ipa_repair_levels_batch_device";
    int rc = rl_check(who, reqs, k, IPA_COLS, n_total);
    if (rc) return rc;
    if (!alpha_be) return bad_arg(who, "alpha_be is NULL");
    if (k == 0) return PORLA_OK;
    if (!alpha_generators_fb || !h_fb) return bad_arg(who, "a NULL base");
    uint32_t alpha[8];
    h_load_be(alpha, alpha_be);
    fe_reduce_plain<Q>(alpha, 8);
    // the alignment rows are commitments against the generators and the call holds the alpha generators: the scalars carry alpha^-1
    Fe<Q> am;
    uint32_t any = 0;
    for (int i = 0; i < 8; i++) { am.v[i] = alpha[i]; any |= alpha[i]; }
    if (!any) return bad_arg(who, "alpha is 0 mod the group order: no alignment row can be formed from the alpha generators");
    if ((rc = ensure_device())) return rc;
    if ((rc = ipa_check_generators(who, "alpha_generators_fb", alpha_generators_fb))) return rc;
    if ((rc = ipa_check_hiding_base(who, "h_fb", h_fb))) return rc;
    const Fe<Q> inv = h_fe_inv<Q>(fe_to_mont<Q>(am));
    RlScale scale;
    for (int i = 0; i < 8; i++) scale.inv[i] = inv.v[i];
    scale.on = 1;
    RepairLevelsWs* ws = nullptr;
    if ((rc = g_rl_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] {
        return rl_enqueue<Secp256k1G>(ws, &alpha_generators_fb->secp, alpha_generators_fb, h_fb, alpha, scale, reqs, k, IPA_COLS, n_total, stream);
    });
}

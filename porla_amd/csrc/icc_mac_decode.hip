// The batched ICC MAC decode (include/porla_gpu.h: porla_icc_mac_decode_batch_device / porla_icc_mac_decode_host): the coded MAC rows
// of K levels back to their per-block MACs in ONE asynchronous call.  Kernels and arithmetic: icc_mac_decode.hip.h.  Every step is on
// the caller's stream and the launch sequence depends on n_rows, never on K:
//
//   upload               one copy of the requests (the kernels read them as they are: ImdDesc)
//   (tables)             when (n_total, curve) changed: the plain inverse twiddles from the data decode's table, their digit codes
//   k_imd_row_scalars    n_rows^-1 wt_i^-1 mod q for the K n_rows rows
//   k_imd_load           the rows (minus d_sub) into one work array, the K tables end to end
//   k_imd_stage_quad     stages log2 n_rows .. 2, one launch each over all K n_rows / 2 butterflies (wave-uniform while n_rows >> s >= 16)
//   k_imd_stage1_quad    stage 1
//   k_imd_close_quad     the per-row scalar multiplication and the affine bytes
#include "batch_host.hpp"
#include "icc_mac_decode.hip.h"
#include "icc_host.hpp"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>

namespace porla {

struct IccMacDecodeWs {
    std::mutex mu;
    int device = -1;
    Buf list, work, scal, itws, codes;
    Buf io_macs, io_out, io_steps, io_sub;     // the host form's device images
    uint32_t tw_n = 0;                          // the (n_total, curve) itws / codes were derived for
    int tw_curve = -1;
    PinnedList h_list;
    UseFence fence;
};
static PerDevice<IccMacDecodeWs> g_imd_ws;

static const char* const IMD_WHO = "porla_icc_mac_decode_batch_device";

// the refusals that concern the shape of the call
static int imd_check_shape(const char* who, size_t n_rows, size_t n_total, int curve) {
    auto bad = [&](const std::string& what) { return bad_arg(who, what); };
    if (int rc = check_n_total(who, n_total, 16)) return rc;
    if (n_rows < 2 || (n_rows & (n_rows - 1)) != 0 || n_rows > n_total) return bad("n_rows must be a power of two, 2 .. n_total");
    if (curve != 0 && curve != 1) return bad("curve must be 0 (BN254 / KZG) or 1 (secp256k1 / IPA)");
    return PORLA_OK;
}

// the checks made before the device is touched
static int imd_check(const porla_icc_mac_decode_req* reqs, size_t k, size_t n_rows, size_t n_total, int curve) {
    auto bad = [&](const std::string& what) { return bad_arg(IMD_WHO, what); };
    if (k && !reqs) return bad("reqs is NULL");
    if (int rc = imd_check_shape(IMD_WHO, n_rows, n_total, curve)) return rc;
    if (int rc = check_request_count(IMD_WHO, k)) return rc;
    size_t t;
    // the work array: k * n_rows points of 128 bytes; its row index is a 32-bit number in the kernels
    if (k && (!mul_ok(n_rows, k, &t) || t > 0xffffffffull || !mul_ok(t, 128, &t)))
        return bad("a byte size overflows: the work array of k requests does not fit a buffer");
    const size_t row_b = n_rows * 64;
    struct Range { uintptr_t lo, hi; bool out; };
    std::vector<Range> ranges;
    ranges.reserve(4 * k);
    for (size_t a = 0; a < k; a++) {
        const porla_icc_mac_decode_req& R = reqs[a];
        const std::string at = "request " + std::to_string(a) + ": ";
        if (!R.d_macs || !R.d_out) return bad(at + "a NULL d_macs or d_out");
        if (((uintptr_t)R.d_macs | (uintptr_t)R.d_out | (uintptr_t)R.d_sub) & 15u) return bad(at + "d_macs, d_out or d_sub is not 16-byte aligned");
        if ((uintptr_t)R.d_write_steps & 7u) return bad(at + "d_write_steps is not 8-byte aligned");
        if ((uintptr_t)R.d_macs + row_b < (uintptr_t)R.d_macs || (uintptr_t)R.d_out + row_b < (uintptr_t)R.d_out ||
            (R.d_sub && (uintptr_t)R.d_sub + row_b < (uintptr_t)R.d_sub))
            return bad(at + "a byte size overflows: a buffer wraps around the address space");
        ranges.push_back(Range{(uintptr_t)R.d_macs, (uintptr_t)R.d_macs + row_b, false});
        ranges.push_back(Range{(uintptr_t)R.d_out, (uintptr_t)R.d_out + row_b, true});
        if (R.d_sub) ranges.push_back(Range{(uintptr_t)R.d_sub, (uintptr_t)R.d_sub + row_b, false});
        if (R.d_write_steps) ranges.push_back(Range{(uintptr_t)R.d_write_steps, (uintptr_t)R.d_write_steps + n_rows * 8, false});
    }
    // an output may overlap nothing, inputs may be shared (icc_decode.hip: the same walk)
    std::sort(ranges.begin(), ranges.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uintptr_t end_any = 0, end_out = 0;
    for (const Range& r : ranges) {
        if (r.lo < (r.out ? end_any : end_out))
            return bad("an output (d_out) overlaps an input, sub or output of this call: outputs must be disjoint from everything");
        end_any = std::max(end_any, r.hi);
        if (r.out) end_out = std::max(end_out, r.hi);
    }
    return PORLA_OK;
}

// 2^e mod q as a plain integer (e >= 0): e doublings of 1
template <class Q>
static void imd_pow2(int e, uint32_t out[8]) {
    Fe<Q> x = fe_zero<Q>();
    x.v[0] = 1;
    for (int i = 0; i < e; i++) x = fe_add<Q>(x, x);
    for (int k = 0; k < 8; k++) out[k] = x.v[k];
}

// ws->mu held, ws->fence entered; arguments checked
template <class C, class Q>
static int imd_enqueue(IccMacDecodeWs* ws, int curve, const porla_icc_mac_decode_req* reqs, size_t k, size_t n, size_t n_total,
                       hipStream_t stream) {
    using M = typename C::Fp;
    int rc;
    const int logn = ilog2u(n);
    const size_t rows = k * n, desc_b = k * sizeof(ImdDesc);
    const uint32_t rows32 = (uint32_t)rows, half32 = (uint32_t)(rows / 2), n32 = (uint32_t)n, nt32 = (uint32_t)n_total;
    static_assert(sizeof(ImdDesc) == sizeof(porla_icc_mac_decode_req), "the requests are uploaded as they are");
    if ((rc = ws->h_list.stage(desc_b))) return rc;
    if ((rc = ws->list.ensure(desc_b))) return rc;
    if ((rc = ws->work.ensure(rows * sizeof(XYZZ<M>)))) return rc;
    if ((rc = ws->scal.ensure(rows * 32))) return rc;
    const size_t code_entries = n_total >> MACQ_CODES_EXP_SHIFT;
    if ((rc = ws->itws.ensure(n_total * 32))) return rc;
    if (code_entries && (rc = ws->codes.ensure(code_entries * MACQ_CODES_STRIDE * sizeof(uint16_t)))) return rc;
    memcpy(ws->h_list.h, reqs, desc_b);
    if ((rc = ws->h_list.send(ws->list.p, desc_b, stream))) return rc;
    const ImdDesc* d_desc = (const ImdDesc*)ws->list.p;
    XYZZ<M>* work = (XYZZ<M>*)ws->work.p;
    uint32_t* itws = (uint32_t*)ws->itws.p;
    uint16_t* codes = (uint16_t*)ws->codes.p;
    ImdScale ninv;
    imd_pow2<Q>(270 - logn, ninv.q);
    {
        // under the ICC workspace's lock and fence: the derived tables (when stale) and the rows' scalars read the resident tables
        const uint32_t *twp = nullptr, *twqi = nullptr;
        if ((rc = icc_decode_tables_acquire(curve, n_total, true, stream, &twp, &twqi))) return rc;
        ProfScope ps("icc_mac_decode_tables", stream);
        if (ws->tw_n != nt32 || ws->tw_curve != curve) {
            ws->tw_n = 0;
            hipLaunchKernelGGL((k_imd_twiddles_plain<Q>), dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, stream, twqi, nt32, itws);
            if (code_entries)
                hipLaunchKernelGGL((k_mac_wnaf_codes<C>), dim3((unsigned)((code_entries + 63) / 64)), dim3(64), 0, stream, (const uint32_t*)itws,
                                   (uint32_t)code_entries, codes);
            if (hipGetLastError() == hipSuccess) { ws->tw_n = nt32; ws->tw_curve = curve; }
            else { set_last_error("porla: ICC MAC decode batch: a table launch failed"); rc = PORLA_ERR_HIP; }
        }
        if (!rc) {
            hipLaunchKernelGGL((k_imd_row_scalars<Q>), dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, stream, d_desc, rows32, n32, twp, nt32,
                               ilog2u(n_total), ninv, (uint32_t*)ws->scal.p);
            if (hipGetLastError() != hipSuccess) { set_last_error("porla: ICC MAC decode batch: a launch failed"); rc = PORLA_ERR_HIP; }
        }
        const int r1 = icc_mix_tables_release(stream);
        if (rc || r1) return rc ? rc : r1;
    }
    imd_lds_attributes<C>();
    {
        ProfScope ps("icc_mac_decode_load", stream);
        hipLaunchKernelGGL((k_imd_load<C>), dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, stream, d_desc, rows32, n32, work);
    }
    for (int s = logn; s >= 2; s--) {
        ProfScope ps("icc_mac_decode_stage", stream);
        imd_launch_stage<C>(imd_stage_uniform(n, s), work, itws, nt32, s, codes, half32, stream);
    }
    {
        ProfScope ps("icc_mac_decode_stage", stream);
        hipLaunchKernelGGL((k_imd_stage1_quad<C>), dim3((unsigned)((rows / 2 + 63) / 64)), dim3(256), 0, stream, work, rows32);
    }
    {
        ProfScope ps("icc_mac_decode_close", stream);
        hipLaunchKernelGGL((k_imd_close_quad<C>), dim3((unsigned)((rows + MACQ_BF - 1) / MACQ_BF)), dim3(4 * MACQ_BF), macq_lds_bytes<C>(), stream,
                           (const XYZZ<M>*)work, (const uint32_t*)ws->scal.p, rows32, n32, d_desc);
    }
    if (hipGetLastError() != hipSuccess) { set_last_error("porla: ICC MAC decode batch: a launch failed"); return PORLA_ERR_HIP; }
    return PORLA_OK;
}

static int imd_run(IccMacDecodeWs* ws, const porla_icc_mac_decode_req* reqs, size_t k, size_t n_rows, size_t n_total, int curve,
                   hipStream_t stream) {
    return curve == 0 ? imd_enqueue<Bn254G1, IccBn254Fr>(ws, 0, reqs, k, n_rows, n_total, stream)
                      : imd_enqueue<Secp256k1G, IccSecp256k1Fn>(ws, 1, reqs, k, n_rows, n_total, stream);
}

}  // namespace porla

using namespace porla;

static_assert(sizeof(porla_icc_mac_decode_req) == PORLA_ICC_MAC_DECODE_REQ_BYTES, "porla_icc_mac_decode_req size");
static_assert(offsetof(porla_icc_mac_decode_req, d_macs) == 0 && offsetof(porla_icc_mac_decode_req, d_out) == 8 &&
              offsetof(porla_icc_mac_decode_req, d_write_steps) == 16 && offsetof(porla_icc_mac_decode_req, d_sub) == 24,
              "porla_icc_mac_decode_req offsets (include/porla_gpu.h)");
static_assert(offsetof(ImdDesc, macs) == 0 && offsetof(ImdDesc, out) == 8 && offsetof(ImdDesc, steps) == 16 && offsetof(ImdDesc, sub) == 24,
              "ImdDesc is porla_icc_mac_decode_req field for field");

extern "C" int porla_icc_mac_decode_batch_device(const porla_icc_mac_decode_req* reqs, size_t k, size_t n_rows, size_t n_total, int curve,
                                                 void* hip_stream) {
    int rc = imd_check(reqs, k, n_rows, n_total, curve);
    if (rc) return rc;
    if (k == 0) return PORLA_OK;
    if ((rc = ensure_device())) return rc;
    IccMacDecodeWs* ws = nullptr;
    if ((rc = g_imd_ws.get(&ws))) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    return FencedCall(ws, stream).run([&] { return imd_run(ws, reqs, k, n_rows, n_total, curve, stream); });
}

// one level from host memory: upload, the batch of one request on the engine's stream, download
extern "C" int porla_icc_mac_decode_host(const uint8_t* macs, size_t n_rows, size_t n_total, int curve, const unsigned long long* write_steps,
                                         const uint8_t* sub, uint8_t* out) {
    static const char* const who = "porla_icc_mac_decode_host";
    if (!macs || !out) return bad_arg(who, "macs or out is NULL");
    int rc = imd_check_shape(who, n_rows, n_total, curve);
    if (rc) return rc;
    if ((rc = ensure_device())) return rc;
    IccMacDecodeWs* ws = nullptr;
    if ((rc = g_imd_ws.get(&ws))) return rc;
    const size_t row_b = n_rows * 64;
    hipStream_t s = engine_stream();
    FencedCall call(ws, s);
    rc = call.run([&] {
        int r;
        if ((r = ws->io_macs.ensure(row_b)) || (r = ws->io_out.ensure(row_b))) return r;
        if (write_steps && (r = ws->io_steps.ensure(n_rows * 8))) return r;
        if (sub && (r = ws->io_sub.ensure(row_b))) return r;
        PORLA_HIP(hipMemcpyAsync(ws->io_macs.p, macs, row_b, hipMemcpyHostToDevice, s));
        if (write_steps) PORLA_HIP(hipMemcpyAsync(ws->io_steps.p, write_steps, n_rows * 8, hipMemcpyHostToDevice, s));
        if (sub) PORLA_HIP(hipMemcpyAsync(ws->io_sub.p, sub, row_b, hipMemcpyHostToDevice, s));
        porla_icc_mac_decode_req R;
        R.d_macs = ws->io_macs.p;
        R.d_out = ws->io_out.p;
        R.d_write_steps = write_steps ? (const unsigned long long*)ws->io_steps.p : nullptr;
        R.d_sub = sub ? ws->io_sub.p : nullptr;
        if ((r = imd_run(ws, &R, 1, n_rows, n_total, curve, s))) return r;
        PORLA_HIP(hipMemcpyAsync(out, ws->io_out.p, row_b, hipMemcpyDeviceToHost, s));
        return (int)PORLA_OK;
    });
    if (rc) return rc;
    PORLA_HIP(hipStreamSynchronize(s));        // (the lock is held to here: the images are this call's until the copies are done)
    return PORLA_OK;
}

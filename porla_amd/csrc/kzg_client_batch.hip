// The client side of the KZG build, batched: compute_digest (main.go:70-89), compute_digest_complement (main.go:91-101) and the MAC
// the client forms from the two, over many rows in one call (include/porla_gpu.h: porla_kzg_{digest,complement,mac}_batch_{device,host}).
// The two evaluation kernels and their table of powers; the three batches on device pointers and on caller-owned host buffers.
#include "kzg_state.hpp"
#include "kzg_eval.hip.h"

#include <cstring>
#include <initializer_list>
#include <mutex>
#include <vector>

using namespace porla;
using Fp = Bn254Fp;
using Fr = Bn254Fr;

// a table of one or two points, rebuilt from `points` if it was built from an older state (g_kzg.mu held)
int porla::kzg_small_table(FixedBase<Bn254G1>& fb, unsigned long long& built_version, std::initializer_list<Affine<Fp>> points) {
    if (built_version == g_kzg.version) return PORLA_OK;
    uint8_t be[128];
    size_t n = 0;
    for (const Affine<Fp>& p : points) h_affine_to_bytes<Fp>(be + 64 * n++, p);
    std::lock_guard<std::mutex> lk(fb.mu);
    int rc = fb.build_from_host_bytes(be, n, 0, engine_stream());
    if (rc) return rc;
    built_version = g_kzg.version;
    return PORLA_OK;
}

// x * 2^270 mod r as canonical words, x in the Montgomery form: from_mont(x R * (2^270 R) / R)
void porla::kzg_to270(const Fe<Fr>& xm, uint32_t dst[8]) {
    static constexpr uint32_t C270[8] = {0x0ffead6fu, 0x36c69455u, 0x37577218u, 0xb1e9be3cu, 0xdf11f427u, 0x9e7d8ca3u, 0xed6d3304u, 0x279be39au};   // 2^270 mod r
    Fe<Fr> c270;
    for (int w = 0; w < 8; w++) c270.v[w] = C270[w];
    const Fe<Fr> v = fe_from_mont<Fr>(fe_mul<Fr>(xm, fe_to_mont<Fr>(c270)));
    for (int w = 0; w < 8; w++) dst[w] = v.v[w];
}

// the table of powers of the dot-product evaluations (g_kzg.mu held): per power i < n_coeffs, padded to a multiple of eight entries with
// zeros, tau^i as 29-bit limbs in KZG_LAZY_ENTRY_WORDS words and, with `wide`, 2^256 tau^i mod r behind it (the Montgomery form of tau^i
// read as a plain value is exactly that)
std::vector<uint32_t> porla::kzg_tau29_table(uint32_t n_coeffs, bool wide) {
    const size_t entry_words = (wide ? 2 : 1) * KZG_LAZY_ENTRY_WORDS;
    std::vector<uint32_t> tab((size_t)((n_coeffs + 7) / 8 * 8) * entry_words, 0u);
    Fe<Fr> pw = fe_one<Fr>();
    for (uint32_t i = 0; i < n_coeffs; i++) {
        kzg_unpack29(fe_from_mont<Fr>(pw).v, &tab[(size_t)i * entry_words]);
        if (wide) kzg_unpack29(pw.v, &tab[(size_t)i * entry_words + KZG_LAZY_ENTRY_WORDS]);
        pw = fe_mul<Fr>(pw, g_kzg.tau);
    }
    return tab;
}

namespace {

__global__ void __launch_bounds__(256)
k_kzg_eval_rows30(const uint8_t* __restrict__ rows, uint32_t n_rows, uint32_t n_coeffs, KzgEvalConsts K, uint8_t* __restrict__ out,
                  uint32_t out_stride, const uint8_t* __restrict__ second) {
    using Q = IccBn254Fr;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t & 7u;
    const bool live = (t >> 3) < n_rows;
    const uint32_t r = live ? (t >> 3) : n_rows - 1;          // idle lanes redo the last row (the lane sum below is wave-wide)
    const uint8_t* row = rows + (size_t)r * n_coeffs * 32;
    const F30<Q> T8 = f30_unpack<Q>(K.t8);
    F30<Q> acc;
#pragma unroll
    for (int l = 0; l < 9; l++) acc.v[l] = 0;
    // (issuing the loads of four steps ahead of their products changes nothing: the chain is bound by its products, not its reads)
    for (uint32_t k = (n_coeffs + 7) / 8; k-- > 0;) {
        const uint32_t i = 8 * k + j;
        uint32_t c[8];
#pragma unroll
        for (int w = 0; w < 8; w++) c[w] = 0;
        if (i < n_coeffs) load_be256(c, row + (size_t)i * 32);
        acc = icc30_add<Q>(icc30_mul<Q>(acc, T8), f30_unpack<Q>(c));
    }
    uint32_t tj[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
        tj[w] = K.tj[0][w];
#pragma unroll
        for (int jj = 1; jj < 8; jj++) tj[w] = j == (uint32_t)jj ? K.tj[jj][w] : tj[w];
    }
    acc = icc30_mul<Q>(acc, f30_unpack<Q>(tj));
    kzg_eval_finish<Q>(acc, live, j, r, K.alpha, out, out_stride, second);
}

// the dot-product form (kzg_eval.hip.h) on 32-byte big-endian coefficients
__global__ void __launch_bounds__(256)
k_kzg_eval_rows_lazy(const uint8_t* __restrict__ rows, uint32_t n_rows, uint32_t n_coeffs, const uint32_t* __restrict__ tau29,
                     KzgAlpha270 A, uint8_t* __restrict__ out, uint32_t out_stride, const uint8_t* __restrict__ second) {
    using Q = IccBn254Fr;
    extern __shared__ uint4 kzg_lds_tau[];            // [8 * steps][KZG_LAZY_ENTRY_WORDS] words, zero beyond n_coeffs
    const uint32_t steps = (n_coeffs + 7) / 8;
    for (uint32_t i = threadIdx.x; i < steps * 8u * (KZG_LAZY_ENTRY_WORDS / 4); i += blockDim.x)
        kzg_lds_tau[i] = reinterpret_cast<const uint4*>(tau29)[i];
    __syncthreads();
    const uint32_t j = threadIdx.x & 7u;
    // a block takes 32 rows at a time, grid-strided: the table above is staged once per block, not once per 32 rows
    for (uint32_t r0 = blockIdx.x * (blockDim.x >> 3); r0 < n_rows; r0 += gridDim.x * (blockDim.x >> 3)) {
        const uint32_t rr = r0 + (threadIdx.x >> 3);
        const bool live = rr < n_rows;
        const uint32_t r = live ? rr : n_rows - 1;            // idle lanes redo the last row (the lane sum below is wave-wide)
        const uint8_t* row = rows + (size_t)r * n_coeffs * 32;
        uint64_t col[19];
#pragma unroll
        for (int k = 0; k < 19; k++) col[k] = 0;
        uint32_t since = 0;
        uint4 nhi = make_uint4(0, 0, 0, 0), nlo = nhi;        // the next step's coefficient, read one step ahead of its products
        if (j < n_coeffs) { nhi = reinterpret_cast<const uint4*>(row + (size_t)j * 32)[0]; nlo = reinterpret_cast<const uint4*>(row + (size_t)j * 32)[1]; }
        for (uint32_t k = 0; k < steps; k++) {
            const uint32_t i = 8 * k + j;
            const uint4 chi = nhi, clo = nlo;
            nhi = make_uint4(0, 0, 0, 0); nlo = nhi;
            if (i + 8 < n_coeffs) {
                const uint4* q = reinterpret_cast<const uint4*>(row + (size_t)(i + 8) * 32);
                nhi = q[0]; nlo = q[1];
            }
            const uint32_t c[8] = {__builtin_bswap32(clo.w), __builtin_bswap32(clo.z), __builtin_bswap32(clo.y), __builtin_bswap32(clo.x),
                                   __builtin_bswap32(chi.w), __builtin_bswap32(chi.z), __builtin_bswap32(chi.y), __builtin_bswap32(chi.x)};
            uint32_t x[9];
            kzg_unpack29(c, x);
            const uint4* tp = kzg_lds_tau + (size_t)i * (KZG_LAZY_ENTRY_WORDS / 4);
            const uint4 t0 = tp[0], t1 = tp[1], t2 = tp[2];
            const uint32_t y[9] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x};
#pragma unroll
            for (int a = 0; a < 9; a++)
#pragma unroll
                for (int b = 0; b < 9; b++) col[a + b] += (uint64_t)x[a] * y[b];
            if (++since == KZG_LAZY_GROUP) { kzg_ripple29(col); since = 0; }
        }
        kzg_ripple29(col);
        const F30<Q> acc = kzg_columns_join<Q>(col);          // (the sum is below 2^517 for 1024 coefficients)
        kzg_eval_finish<Q>(acc, live, j, r, A.w, out, out_stride, second);
    }
}

// alpha * f_r(tau) of n_rows rows into kd->d_eval at out_stride bytes per row (32, or 64 with a second scalar copied beside it).
// g_kzg.mu and the mutex of the table whose commit reads d_eval are held by the caller.
int kzg_eval_rows_launch(KzgDev* kd, const void* d_rows, size_t n_rows, uint32_t out_stride, const void* d_second, hipStream_t stream) {
    int rc;
    if ((rc = kd->d_eval.ensure(n_rows * out_stride))) return rc;      // a hipFree in there waits for the work that still uses it
    // d_eval is read by the commit that follows: a previous batch on another stream must have finished with it (each table's
    // fence is recorded after its commit's last kernel; the three client-side tables share d_eval, so enter all of them)
    if ((rc = kd->fb_g.fence.enter(stream))) return rc;
    if ((rc = kd->fb_gh.fence.enter(stream))) return rc;
    const uint32_t n_coeffs = (uint32_t)g_kzg.n_samples;
    if (n_coeffs <= KZG_LAZY_MAX_COEFFS) {
        const uint32_t entries = (n_coeffs + 7) / 8 * 8;
        if (!kd->d_tau29.p || kd->tau29_n != n_coeffs || memcmp(kd->tau29_tau.v, g_kzg.tau.v, sizeof(g_kzg.tau.v)) != 0) {
            const std::vector<uint32_t> tab = kzg_tau29_table(n_coeffs, false);
            kd->d_tau29.release();                                // the hipFree waits for the evaluations that still read the old table
            kd->tau29_n = 0;
            if ((rc = kd->d_tau29.ensure(tab.size() * 4))) return rc;
            PORLA_HIP(hipMemcpy(kd->d_tau29.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
            kd->tau29_tau = g_kzg.tau;
            kd->tau29_n = n_coeffs;
        }
        KzgAlpha270 A;
        kzg_to270(g_kzg.alpha, A.w);
        ProfScope ps("kzg_eval_rows", stream);
        constexpr size_t lazy_grid = 2048;        // 1024 .. 16384 blocks measure the same (profiles/r03_zw_bench_digest_lazy_grid.log)
        const size_t groups = (n_rows + 31) / 32;
        hipLaunchKernelGGL(k_kzg_eval_rows_lazy, dim3((unsigned)(groups < lazy_grid ? groups : lazy_grid)), dim3(256),
                           (size_t)entries * KZG_LAZY_ENTRY_WORDS * 4, stream, (const uint8_t*)d_rows, (uint32_t)n_rows, n_coeffs,
                           (const uint32_t*)kd->d_tau29.p, A, (uint8_t*)kd->d_eval.p, out_stride, (const uint8_t*)d_second);
        return PORLA_OK;
    }
    ProfScope ps("kzg_eval_rows", stream);
    // longer rows: Horner with eight lanes per row; tau^j, tau^8 and alpha in the 2^270 form
    KzgEvalConsts K;
    Fe<Fr> pw = fe_one<Fr>();
    for (int jj = 0; jj < 8; jj++) { kzg_to270(pw, K.tj[jj]); pw = fe_mul<Fr>(pw, g_kzg.tau); }
    kzg_to270(pw, K.t8);
    kzg_to270(g_kzg.alpha, K.alpha);
    hipLaunchKernelGGL(k_kzg_eval_rows30, dim3((unsigned)((8 * n_rows + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)d_rows,
                       (uint32_t)n_rows, n_coeffs, K, (uint8_t*)kd->d_eval.p, out_stride, (const uint8_t*)d_second);
    return PORLA_OK;
}

// The three batches on device pointers.  kind 0, the digests: out[r] = alpha * f_r(tau) * G1[0].  Kind 1, the complements:
// out[r] = s_r * h_MAC.  Kind 2, the MAC of a block as the client forms it (Client.hpp:229/471 compute_commitment, :424-455
// compute_MAC_complement, then add_point): out[r] = alpha * f_r(tau) * G1[0] + s_r * h_MAC as ONE two-coefficient commitment per
// row against the table of (G1[0], h_MAC): one affine conversion per block where the two batches spend two and the host one more
// for the sum.
int client_batch_device(int kind /* 0 digest, 1 complement, 2 MAC */, const void* d_rows, const void* d_scalars, size_t n, void* d_out,
                        hipStream_t stream) {
    if (n && (!d_out || (kind != 1 && !d_rows) || (kind != 0 && !d_scalars))) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    int rc = ensure_device();
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_kzg.mu);
    if (kind == 1 && g_kzg.srs.empty()) { set_last_error("porla: init_SRS first (it draws the MAC hiding base)"); return PORLA_ERR_STATE; }
    if (kind != 1 && (!g_kzg.have_key || g_kzg.srs.empty())) { set_last_error("porla: init_key / init_SRS first"); return PORLA_ERR_STATE; }
    if (n == 0) return PORLA_OK;
    KzgDev* kd;
    if ((rc = current_dev(&kd))) return rc;
    FixedBase<Bn254G1>& fb = kind == 0 ? kd->fb_g : kind == 1 ? kd->fb_h : kd->fb_gh;
    if (kind == 0) rc = kzg_small_table(fb, kd->g_version, {g_kzg.srs[0]});
    else if (kind == 1) rc = kzg_small_table(fb, kd->h_version, {g_kzg.h_mac});
    else rc = kzg_small_table(fb, kd->gh_version, {g_kzg.srs[0], g_kzg.h_mac});
    if (rc) return rc;
    std::lock_guard<std::mutex> lk2(fb.mu);
    if (kind == 1) return fb.commit_device((const uint8_t*)d_scalars, n, 1, 32, (uint8_t*)d_out, stream);
    const uint32_t coeffs = kind == 2 ? 2 : 1;                // per row of d_eval: the evaluation, and the MAC's scalar beside it
    if ((rc = kzg_eval_rows_launch(kd, d_rows, n, 32 * coeffs, kind == 2 ? d_scalars : nullptr, stream))) return rc;
    return fb.commit_device((const uint8_t*)kd->d_eval.p, n, coeffs, 32 * coeffs, (uint8_t*)d_out, stream);
}

// ---- the same three batches on caller-owned host buffers: staged into a device buffer kept between calls, computed by the
// device entry on the engine's stream, copied back; blocking.  (The copies dominate: 4 KiB per block over PCIe.)
struct ClientIo {
    std::mutex mu;                 // one host batch per device at a time: the staging buffer is shared
    int device = -1;
    Buf d;
};
PerDevice<ClientIo> g_client_io;

int client_batch_host(int kind /* 0 digest, 1 complement, 2 MAC */, const uint8_t* rows, const uint8_t* scalars, size_t n, uint8_t* out) {
    if (n && (!out || (kind != 1 && !rows) || (kind != 0 && !scalars))) { set_last_error("porla: null argument"); return PORLA_ERR_ARG; }
    int rc = ensure_device();
    if (rc) return rc;
    if (n == 0) return PORLA_OK;
    const size_t row_bytes = kzg_n_samples() * 32;
    if (kind != 1 && row_bytes == 0) { set_last_error("porla: init_key / init_SRS first"); return PORLA_ERR_STATE; }
    ClientIo* io;
    if ((rc = g_client_io.get(&io))) return rc;
    std::lock_guard<std::mutex> lk(io->mu);
    // chunks of 16 384 blocks (64 MiB of rows): a pageable copy of that size runs at 44 GB/s, one of 512 MiB at 15
    // (tools/bench_client_host.py); one stream, so the chunks follow each other through the same staging buffer
    constexpr size_t CHUNK = 16384;
    const size_t per = n < CHUNK ? n : CHUNK;
    const size_t rows_b = kind != 1 ? per * row_bytes : 0, sc_b = kind != 0 ? per * 32 : 0, out_b = per * 64;
    if ((rc = io->d.ensure(((rows_b + 255) & ~(size_t)255) + ((sc_b + 255) & ~(size_t)255) + ((out_b + 255) & ~(size_t)255)))) return rc;
    hipStream_t stream = engine_stream();
    for (size_t lo = 0; lo < n; lo += CHUNK) {
        const size_t m = n - lo < CHUNK ? n - lo : CHUNK;
        uint8_t* d_rows = (uint8_t*)io->d.p;
        uint8_t* d_sc = d_rows + ((rows_b + 255) & ~(size_t)255);
        uint8_t* d_out = d_sc + ((sc_b + 255) & ~(size_t)255);
        if (rows_b) PORLA_HIP(hipMemcpyAsync(d_rows, rows + lo * row_bytes, m * row_bytes, hipMemcpyHostToDevice, stream));
        if (sc_b) PORLA_HIP(hipMemcpyAsync(d_sc, scalars + lo * 32, m * 32, hipMemcpyHostToDevice, stream));
        rc = client_batch_device(kind, d_rows, d_sc, m, d_out, stream);
        if (rc) { (void)hipStreamSynchronize(stream); return rc; }
        PORLA_HIP(hipMemcpyAsync(out + lo * 64, d_out, m * 64, hipMemcpyDeviceToHost, stream));
    }
    PORLA_HIP(hipStreamSynchronize(stream));
    return PORLA_OK;
}

}  // namespace

void porla::kzg_client_staging_release() {
    for (ClientIo* io : g_client_io.snapshot()) {
        std::lock_guard<std::mutex> lio(io->mu);
        io->d.release();
    }
}

extern "C" {

int porla_kzg_digest_batch_device(const void* d_rows, size_t n_rows, void* d_out, void* hip_stream) {
    return client_batch_device(0, d_rows, nullptr, n_rows, d_out, (hipStream_t)hip_stream);
}
int porla_kzg_complement_batch_device(const void* d_scalars, size_t n, void* d_out, void* hip_stream) {
    return client_batch_device(1, nullptr, d_scalars, n, d_out, (hipStream_t)hip_stream);
}
int porla_kzg_mac_batch_device(const void* d_rows, const void* d_scalars, size_t n_rows, void* d_out, void* hip_stream) {
    return client_batch_device(2, d_rows, d_scalars, n_rows, d_out, (hipStream_t)hip_stream);
}
int porla_kzg_digest_batch_host(const uint8_t* rows, size_t n_rows, uint8_t* out) { return client_batch_host(0, rows, nullptr, n_rows, out); }
int porla_kzg_complement_batch_host(const uint8_t* scalars, size_t n, uint8_t* out) { return client_batch_host(1, nullptr, scalars, n, out); }
int porla_kzg_mac_batch_host(const uint8_t* rows, const uint8_t* scalars, size_t n_rows, uint8_t* out) {
    return client_batch_host(2, rows, scalars, n_rows, out);
}

}  // extern "C"

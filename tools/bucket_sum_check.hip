// Driver for the bucket accumulation of porla_amd/csrc/msm.hip.h on bucket lists the caller wrote: k_points_to_mont, then per pass
// k_size_hist / k_size_scan / k_size_order, k_bucket_sum30 and k_bucket_combine, the product's own kernels with the grid, block and
// buffer sizes of msm_impl.hip.h:msm_launch.  The counting sort in front of them is left out, so the ORDER of a bucket's entries is
// the file's: an exceptional operand can be pinned to a position.  A pure transformer: no reference arithmetic lives here, nothing
// is normalised -- the bucket array comes back as the raw memory form, the scheduling arrays as they are.  The one piece of host
// arithmetic is starts[] = the plain prefix sum of counts[].  Expected values are computed by tests/bucket_vectors.py.
// Built by porla_amd/csrc/Makefile as porla_amd/bucket_sum_check; run by tests/test_bucket_sum_gpu.py.
//
//   bucket_sum_check <bn254|secp256k1> <in> <out>
//
// Input (uint32 words, little endian):
//   [0, 8)   header: magic 0x4d55534b, n_points, glv (0 | 1), n_buckets, n_passes, 0, 0, 0
//   then     n_points points of 16 words: the 64-byte big-endian wire form X || Y as the bytes lie, all zero = infinity
//   then per pass:  n_entries, counts[n_buckets], entries[n_entries] -- the buckets' entries concatenated in bucket order, point index in
//            bits 0..30, sign in bit 31; with glv the index addresses the doubled table (2i the point, 2i + 1 its endomorphism image)
// Pass 0 runs with accumulate = 0, every later pass with accumulate = 1 into the same bucket array (k_size_order then gets no bucket
// array: empty buckets keep their sums).  ctrl is cleared before every pass as k_digits_partition clears it.
// Output, per pass:  buckets[n_buckets][32], ctrl[CTRL_WORDS], order[ctrl[3]][2], chunk_base[n_buckets], heavy_list[ctrl[2]]
// The file is validated on the host before the first launch (indices below the table size, counts summing to n_entries, totals within
// the buffers); a file that fails, and any HIP error, ends the run with a message and a non-zero status.
#include "msm.hip.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr uint32_t MAGIC = 0x4d55534bu, HDR = 8;
constexpr uint32_t MAX_POINTS = 1u << 20, MAX_BUCKETS = 1u << 20, MAX_PASSES = 8, MAX_ENTRIES = 1u << 24;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "bucket_sum_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define BAD(...) do { fprintf(stderr, "bucket_sum_check: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

struct Pass {
    size_t counts_at, entries_at;    // word offsets into the file
    uint32_t n_entries;
};

static int read_file(const char* path, std::vector<uint32_t>& v) {
    FILE* fp = fopen(path, "rb");
    if (!fp) BAD("cannot read %s", path);
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (sz < 0 || sz % 4 != 0) { fclose(fp); BAD("%s is not a whole number of words", path); }
    v.resize((size_t)sz / 4);
    const size_t got = v.empty() ? 0 : fread(v.data(), 4, v.size(), fp);
    fclose(fp);
    if (got != v.size()) BAD("short read of %s", path);
    return 0;
}

template <class T>
static int dev_alloc(T** p, size_t count) {
    CK(hipMalloc((void**)p, (count ? count : 1) * sizeof(T)));
    return 0;
}

template <class C>
static int run(const std::vector<uint32_t>& in, const char* out_path) {
    using M = typename C::Fp;
    // ---- validation: nothing below reaches the device unless every index and every total is inside its buffer
    if (in.size() < HDR || in[0] != MAGIC) BAD("not a bucket_sum_check file");
    const uint32_t n_points = in[1], glv = in[2], nb = in[3], n_passes = in[4];
    if (glv > 1 || n_points == 0 || n_points > MAX_POINTS || nb == 0 || nb > MAX_BUCKETS || n_passes == 0 || n_passes > MAX_PASSES)
        BAD("header out of range (points %u, glv %u, buckets %u, passes %u)", n_points, glv, nb, n_passes);
    const uint32_t table = glv ? 2 * n_points : n_points;
    size_t at = HDR + (size_t)16 * n_points;
    if (in.size() < at) BAD("file ends inside the points");
    std::vector<Pass> passes;
    size_t max_entries = 0;
    for (uint32_t p = 0; p < n_passes; p++) {
        if (in.size() < at + 1 + (size_t)nb) BAD("pass %u: file ends inside the counts", p);
        Pass ps;
        ps.n_entries = in[at];
        ps.counts_at = at + 1;
        ps.entries_at = at + 1 + nb;
        if (ps.n_entries > MAX_ENTRIES) BAD("pass %u: %u entries", p, ps.n_entries);
        if (in.size() < ps.entries_at + ps.n_entries) BAD("pass %u: file ends inside the entries", p);
        uint64_t sum = 0;
        for (uint32_t b = 0; b < nb; b++) {
            if (in[ps.counts_at + b] > ps.n_entries) BAD("pass %u: bucket %u counts %u entries of %u", p, b, in[ps.counts_at + b], ps.n_entries);
            sum += in[ps.counts_at + b];
        }
        if (sum != ps.n_entries) BAD("pass %u: the counts sum to %llu, the pass holds %u entries", p, (unsigned long long)sum, ps.n_entries);
        for (uint32_t k = 0; k < ps.n_entries; k++)
            if ((in[ps.entries_at + k] & 0x7fffffffu) >= table) BAD("pass %u: entry %u addresses point %u of %u", p, k, in[ps.entries_at + k] & 0x7fffffffu, table);
        if (ps.n_entries > max_entries) max_entries = ps.n_entries;
        passes.push_back(ps);
        at = ps.entries_at + ps.n_entries;
    }
    if (at != in.size()) BAD("%zu words behind the last pass", in.size() - at);
    // the buffer sizes of msm_launch
    const uint32_t nblk = (nb + 1023) / 1024;
    const size_t max_items = nb + max_entries / CHUNK;
    const size_t max_chunk_out = 2 * (max_entries / CHUNK) + 2;
    const size_t max_heavy = max_entries / CHUNK + 2;
    for (uint32_t p = 0; p < n_passes; p++) {
        size_t items = 0, chunk_items = 0, heavy = 0;
        for (uint32_t b = 0; b < nb; b++) {
            const size_t it = ((size_t)in[passes[p].counts_at + b] + CHUNK - 1) / CHUNK;
            items += it;
            if (it > 1) { chunk_items += it; heavy++; }
        }
        if (items > max_items || chunk_items > max_chunk_out || heavy > max_heavy)
            BAD("pass %u: %zu items, %zu item sums of %zu multi-item buckets exceed the buffers (%zu, %zu, %zu)", p, items, chunk_items, heavy,
                max_items, max_chunk_out, max_heavy);
    }

    // ---- device buffers
    uint8_t* d_points_be = nullptr;
    Affine<M>* d_pts = nullptr;
    XYZZ<M>*d_buckets = nullptr, *d_chunk_out = nullptr;
    uint32_t *d_entries = nullptr, *d_counts = nullptr, *d_starts = nullptr, *d_chunk_base = nullptr, *d_ctrl = nullptr, *d_heavy = nullptr,
             *d_blk_hist = nullptr, *d_blk_off = nullptr;
    uint2* d_order = nullptr;
    if (dev_alloc(&d_points_be, (size_t)64 * n_points) || dev_alloc(&d_pts, table) || dev_alloc(&d_buckets, nb) ||
        dev_alloc(&d_chunk_out, max_chunk_out) || dev_alloc(&d_entries, max_entries) || dev_alloc(&d_counts, nb) || dev_alloc(&d_starts, nb) ||
        dev_alloc(&d_chunk_base, nb) || dev_alloc(&d_ctrl, CTRL_WORDS) || dev_alloc(&d_heavy, max_heavy) ||
        dev_alloc(&d_blk_hist, (size_t)CHUNK * nblk) || dev_alloc(&d_blk_off, (size_t)CHUNK * nblk) || dev_alloc(&d_order, max_items))
        return 1;
    CK(hipMemcpy(d_points_be, in.data() + HDR, (size_t)64 * n_points, hipMemcpyHostToDevice));
    // what no launch has written yet reads as a pattern, not as a plausible value
    CK(hipMemset(d_buckets, 0xa5, (size_t)nb * sizeof(XYZZ<M>)));
    CK(hipMemset(d_chunk_out, 0xa5, max_chunk_out * sizeof(XYZZ<M>)));
    if (glv) hipLaunchKernelGGL((k_points_to_mont<C, true, C::F30_BUCKETS>), dim3((n_points + 255) / 256), dim3(256), 0, 0, d_points_be, d_pts, n_points);
    else hipLaunchKernelGGL((k_points_to_mont<C, false, C::F30_BUCKETS>), dim3((n_points + 255) / 256), dim3(256), 0, 0, d_points_be, d_pts, n_points);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());

    FILE* fp = fopen(out_path, "wb");
    if (!fp) BAD("cannot write %s", out_path);
    std::vector<uint32_t> h_buckets((size_t)nb * 32), h_ctrl(CTRL_WORDS), h_order(2 * max_items), h_chunk_base(nb), h_heavy(max_heavy), starts(nb);
    for (uint32_t p = 0; p < n_passes; p++) {
        const Pass& ps = passes[p];
        const uint32_t* counts = in.data() + ps.counts_at;
        uint32_t run_at = 0;
        for (uint32_t b = 0; b < nb; b++) { starts[b] = run_at; run_at += counts[b]; }
        const uint32_t accumulate = p > 0 ? 1u : 0u;
        CK(hipMemcpy(d_counts, counts, (size_t)nb * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_starts, starts.data(), (size_t)nb * 4, hipMemcpyHostToDevice));
        if (ps.n_entries) CK(hipMemcpy(d_entries, in.data() + ps.entries_at, (size_t)ps.n_entries * 4, hipMemcpyHostToDevice));
        CK(hipMemset(d_ctrl, 0, CTRL_WORDS * 4));
        hipLaunchKernelGGL(k_size_hist, dim3(nblk), dim3(1024), 0, 0, (const uint32_t*)d_counts, nb, d_blk_hist, nblk, d_ctrl);
        hipLaunchKernelGGL(k_size_scan, dim3(CHUNK), dim3(1024), 0, 0, (const uint32_t*)d_blk_hist, d_blk_off, nblk, d_ctrl);
        hipLaunchKernelGGL(k_size_order, dim3(nblk), dim3(1024), 0, 0, (const uint32_t*)d_counts, nb, (const uint32_t*)d_blk_off, nblk, d_order,
                           d_chunk_base, d_heavy, d_ctrl, accumulate ? (uint4*)nullptr : (uint4*)d_buckets);
        hipLaunchKernelGGL((k_bucket_sum30<C>), dim3((unsigned)((max_items + 255) / 256)), dim3(256), 0, 0, (const Affine<M>*)d_pts,
                           (const uint32_t*)d_entries, (const uint32_t*)d_starts, (const uint32_t*)d_counts, (const uint2*)d_order,
                           (const uint32_t*)d_chunk_base, (const uint32_t*)d_ctrl, d_buckets, d_chunk_out, accumulate);
        hipLaunchKernelGGL((k_bucket_combine<C>), dim3(2048), dim3(64), 0, 0, (const uint32_t*)d_heavy, (const uint32_t*)d_chunk_base,
                           (const uint32_t*)d_counts, (const uint32_t*)d_ctrl, (const XYZZ<M>*)d_chunk_out, d_buckets, accumulate);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(h_ctrl.data(), d_ctrl, CTRL_WORDS * 4, hipMemcpyDeviceToHost));
        const uint32_t n_items = h_ctrl[3], n_heavy = h_ctrl[2];
        if (n_items > max_items || n_heavy > max_heavy) { fclose(fp); BAD("pass %u: ctrl reports %u items, %u multi-item buckets", p, n_items, n_heavy); }
        CK(hipMemcpy(h_buckets.data(), d_buckets, (size_t)nb * sizeof(XYZZ<M>), hipMemcpyDeviceToHost));
        if (n_items) CK(hipMemcpy(h_order.data(), d_order, (size_t)n_items * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(h_chunk_base.data(), d_chunk_base, (size_t)nb * 4, hipMemcpyDeviceToHost));
        if (n_heavy) CK(hipMemcpy(h_heavy.data(), d_heavy, (size_t)n_heavy * 4, hipMemcpyDeviceToHost));
        size_t put = fwrite(h_buckets.data(), 4, h_buckets.size(), fp) + fwrite(h_ctrl.data(), 4, CTRL_WORDS, fp);
        put += fwrite(h_order.data(), 4, (size_t)2 * n_items, fp) + fwrite(h_chunk_base.data(), 4, nb, fp) + fwrite(h_heavy.data(), 4, n_heavy, fp);
        if (put != h_buckets.size() + CTRL_WORDS + (size_t)2 * n_items + nb + n_heavy) { fclose(fp); BAD("short write of %s", out_path); }
    }
    if (fclose(fp) != 0) BAD("short write of %s", out_path);
    CK(hipFree(d_points_be)); CK(hipFree(d_pts)); CK(hipFree(d_buckets)); CK(hipFree(d_chunk_out)); CK(hipFree(d_entries)); CK(hipFree(d_counts));
    CK(hipFree(d_starts)); CK(hipFree(d_chunk_base)); CK(hipFree(d_ctrl)); CK(hipFree(d_heavy)); CK(hipFree(d_blk_hist)); CK(hipFree(d_blk_off));
    CK(hipFree(d_order));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: bucket_sum_check <bn254|secp256k1> <in> <out>\n");
        return 2;
    }
    const std::string curve = argv[1];
    if (curve != "bn254" && curve != "secp256k1") { fprintf(stderr, "bucket_sum_check: unknown curve %s\n", curve.c_str()); return 2; }
    static_assert(sizeof(XYZZ<Bn254Fp>) == 128 && sizeof(Affine<Bn254Fp>) == 64, "the memory forms the output format states");
    std::vector<uint32_t> in;
    if (read_file(argv[2], in)) return 1;
    return curve == "bn254" ? run<Bn254G1>(in, argv[3]) : run<Secp256k1G>(in, argv[3]);
}

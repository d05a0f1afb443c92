// Stage-by-stage driver for the fixed-base commitment of porla_amd/csrc/fixed_base.hip.h: k_fb_base_powers, k_fb_multiples,
// k_fb_normalize, k_fb_commit (both template forms), k_fb_commit_small, k_fb_fold_quad and k_fb_finish<C, 1 | 2 | 4>, the product's
// own kernels, in the launch shapes FixedBase<C> gives them (fb_table_plan; the grids of fixed_base_impl.hip.h), on bases, rows and
// partials the caller wrote.  A pure transformer: no reference arithmetic lives here and nothing is normalised on the host -- the
// table, the partials, the sums and the output bytes come back as they lie.  Expected values are computed by tests/fb_vectors.py.
// (k_fb_fold and fe_inv_dev are instantiated for neither curve -- both have F30_BUCKETS and F30_LAZY -- and are left out.)
// Built by porla_amd/csrc/Makefile as porla_amd/fb_check; run by tests/test_fb_gpu.py and tests/test_fb_vectors_cpu.py.
//
//   fb_check <bn254|secp256k1> <in> <out>
//
// Input (uint32 words, little endian): one or more sections, each a header of 16 words and its payload
//   header  0 magic 0x46424b31, 1 op, 2 c, 3 n_points (table) | n_coeffs, 4 n_rows, 5 S | SL, 6 row_stride in bytes,
//           7 table: length of the index list (0 = the whole table); commit: 1 = k_fb_commit<C, true>; finish: rows per lane (1, 2, 4),
//           8, 9 table: scratch budget in bytes, low and high word (0 = the product's default), 10 sentinel rows, 11 .. 15 zero
//           W is the product's: ceil((SCALAR_BITS + 1) / c)
//   op 1 table         payload: n_points affine points of 16 words (Montgomery form, all-zero = infinity), then the index list.
//                      Runs the three construction kernels batched as FixedBase<C>::build batches them.  Output: the table's entries of
//                      16 words, all of them or those the list names.  The table stays resident for the sections that follow.
//   op 2 commit        payload: n_rows * row_stride bytes of rows.  Output: partial, (n_rows + sentinel rows) * S entries of 32 words.
//   op 3 commit_small  payload: n_rows * row_stride bytes of rows (device memory).  Output: part (n_rows * SL entries), out_sums (n_rows
//                      entries), the FB_SMALL_MAX_ROWS + 1 counters (zeroed before the launch), hdr[0] (seq = 1 is published there).
//   op 4 fold          payload: n_rows * S partials of 32 words in the lazy memory form.  Output: (n_rows + sentinel rows) * S entries.
//   op 5 finish        payload: n_rows * S partials of 32 words.  Output: (n_rows + sentinel rows) * 64 bytes.
// Every output area is filled with the word 0xA5A5A5A5 before the launch.
// Every section is validated on the host before the FIRST launch: magic, 2 <= c <= 20, the counts within the kernels' own limits (S a
// power of two in 2 .. 128 for the fold, SL <= FB_SMALL_MAX_SLICES and n_rows <= FB_SMALL_MAX_ROWS for the single-launch kernel,
// n_coeffs <= the resident table's points, at most 2^23 table entries) and the file's length.  A file that fails, and any HIP error,
// ends the run with a message and status 1.
//
//   fb_check --plan <bn254|secp256k1> [c <c> ...] [commit <n_rows> <n_coeffs> <W> ...] [rows <n_rows> ...]
//
// prints the launch shapes (fb_table_plan for the 128-point base, fb_commit_slices and fb_small_slices, fb_finish_rows); no HIP call.
#include "fixed_base.hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr uint32_t MAGIC = 0x46424b31u, HDR = 16, FILL = 0xA5A5A5A5u;
enum { OP_TABLE = 1, OP_COMMIT, OP_SMALL, OP_FOLD, OP_FINISH };
constexpr size_t MAX_ENTRIES = (size_t)1 << 23, MAX_PARTIALS = (size_t)1 << 20, MAX_POINTS = 4096, MAX_SENTINEL = 64;
constexpr size_t SMALL_ROW_BYTES = 8192;             // fixed_base_impl.hip.h: FB_SMALL_ROW_BYTES

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "fb_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define BAD(...) do { fprintf(stderr, "fb_check: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

struct Section {
    uint32_t op, c, W, n, n_rows, S, flag, sentinel;
    size_t row_stride, budget, payload_at, payload_words, out_words;
    FbTablePlan tp;
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

template <class C>
static int parse(const std::vector<uint32_t>& in, std::vector<Section>& secs) {
    using M = typename C::Fp;
    size_t at = 0;
    uint32_t table_c = 0, table_points = 0;          // the table resident when a section runs
    do {
        if (in.size() < at + HDR || in[at] != MAGIC) BAD("not an fb_check file (section at word %zu)", at);
        const uint32_t* h = in.data() + at;
        Section s{};
        s.op = h[1]; s.c = h[2]; s.n = h[3]; s.n_rows = h[4]; s.S = h[5]; s.row_stride = h[6]; s.flag = h[7];
        s.budget = ((size_t)h[9] << 32) | h[8]; s.sentinel = h[10];
        for (int k = 11; k < 16; k++) if (h[k]) BAD("header word %d is not zero", k);
        if (s.c < 2 || s.c > 20) BAD("c = %u is outside 2 .. 20", s.c);
        if (s.sentinel > MAX_SENTINEL) BAD("too many sentinel rows (%u)", s.sentinel);
        s.W = (uint32_t)((C::SCALAR_BITS + 1 + s.c - 1) / s.c);
        const size_t H = (size_t)1 << (s.c - 1);
        s.payload_at = at + HDR;
        if (s.op == OP_TABLE) {
            if (s.n < 1 || s.n > MAX_POINTS || s.n_rows || s.S || s.row_stride || s.sentinel) BAD("table: header out of range (n_points %u)", s.n);
            const size_t pairs = (size_t)s.n * s.W, entries = pairs * H;
            if (entries > MAX_ENTRIES) BAD("table: %zu entries are more than 2^23", entries);
            if (s.budget == 0) s.budget = FB_SCRATCH_BUDGET;
            if (s.budget > FB_SCRATCH_BUDGET) BAD("table: the scratch budget is above the product's");
            s.tp = fb_table_plan((int)s.c, pairs, sizeof(XYZZ<M>), s.budget);
            if (s.tp.batch_pairs < 1 || s.tp.lanes * s.tp.K * s.tp.runs != s.tp.H || s.tp.lanes * s.tp.groups_per_wave != 64)
                BAD("table: the plan does not tile the table");
            s.payload_words = (size_t)s.n * 16 + s.flag;
            if (in.size() < s.payload_at + s.payload_words) BAD("file ends inside a table section");
            for (uint32_t k = 0; k < s.flag; k++)
                if (in[s.payload_at + (size_t)s.n * 16 + k] >= entries) BAD("table: index %u is outside the table", in[s.payload_at + (size_t)s.n * 16 + k]);
            s.out_words = (s.flag ? (size_t)s.flag : entries) * 16;
            table_c = s.c; table_points = s.n;
        } else if (s.op == OP_COMMIT || s.op == OP_SMALL) {
            const char* name = s.op == OP_COMMIT ? "commit" : "commit_small";
            if (table_c != s.c) BAD("%s: no resident table with c = %u", name, s.c);
            if (s.n < 1 || s.n > table_points) BAD("%s: n_coeffs %u is outside 1 .. the table's %u points", name, s.n, table_points);
            if (s.row_stride < (size_t)s.n * 32 || s.row_stride % 4 || s.row_stride > ((size_t)1 << 20)) BAD("%s: row_stride %zu", name, s.row_stride);
            if (s.op == OP_COMMIT) {
                if (s.S < 1 || s.S > 128) BAD("commit: S = %u is outside 1 .. 128", s.S);
                if (s.n_rows < 1 || (size_t)(s.n_rows + s.sentinel) * s.S > MAX_PARTIALS) BAD("commit: n_rows %u", s.n_rows);
                if (s.flag > 1) BAD("commit: form %u", s.flag);
                s.out_words = (size_t)(s.n_rows + s.sentinel) * s.S * 32;
            } else {
                if (s.S < 1 || s.S > (uint32_t)FB_SMALL_MAX_SLICES) BAD("commit_small: SL = %u is outside 1 .. %d", s.S, FB_SMALL_MAX_SLICES);
                if (s.n_rows < 1 || s.n_rows > (uint32_t)FB_SMALL_MAX_ROWS) BAD("commit_small: n_rows = %u is outside 1 .. %d", s.n_rows, FB_SMALL_MAX_ROWS);
                if ((size_t)s.n * 32 > SMALL_ROW_BYTES || s.flag || s.sentinel) BAD("commit_small: header out of range");
                s.out_words = (size_t)s.n_rows * s.S * 32 + (size_t)s.n_rows * 32 + FB_SMALL_MAX_ROWS + 1 + 1;
            }
            if ((size_t)s.n_rows * s.row_stride > ((size_t)1 << 28)) BAD("%s: the rows are too large", name);
            s.payload_words = (size_t)s.n_rows * s.row_stride / 4;
            if (in.size() < s.payload_at + s.payload_words) BAD("file ends inside the rows");
        } else if (s.op == OP_FOLD || s.op == OP_FINISH) {
            if (s.n || s.row_stride) BAD("fold / finish: header out of range");
            if (s.op == OP_FOLD) {
                if (s.S < 2 || s.S > 128 || (s.S & (s.S - 1))) BAD("fold: S = %u is no power of two in 2 .. 128", s.S);
                if (s.flag) BAD("fold: header out of range");
                if (!(C::F30_BUCKETS && C::F30_LAZY)) BAD("fold: the curve has no reduced-radix memory form");
            } else {
                if (s.S < 1 || s.S > 128) BAD("finish: S = %u is outside 1 .. 128", s.S);
                if (s.flag != 1 && s.flag != 2 && s.flag != 4) BAD("finish: %u rows per lane", s.flag);
            }
            if (s.n_rows < 1 || (size_t)(s.n_rows + s.sentinel) * s.S > MAX_PARTIALS) BAD("fold / finish: n_rows %u", s.n_rows);
            s.payload_words = (size_t)s.n_rows * s.S * 32;
            if (in.size() < s.payload_at + s.payload_words) BAD("file ends inside the partials");
            s.out_words = s.op == OP_FOLD ? (size_t)(s.n_rows + s.sentinel) * s.S * 32 : (size_t)(s.n_rows + s.sentinel) * 16;
        } else {
            BAD("unknown operation %u", s.op);
        }
        at = s.payload_at + s.payload_words;
        secs.push_back(s);
    } while (at < in.size());
    return 0;
}

static int put(FILE* fp, const void* p, size_t words) {
    if (words && fwrite(p, 4, words, fp) != words) BAD("short write");
    return 0;
}

template <class C>
static int run(const std::vector<uint32_t>& in, const char* out_path) {
    using M = typename C::Fp;
    std::vector<Section> secs;
    if (parse<C>(in, secs)) return 1;                // ---- nothing below runs unless every section stands
    FILE* fp = fopen(out_path, "wb");
    if (!fp) BAD("cannot write %s", out_path);
    Affine<M>* table = nullptr;
    std::vector<uint32_t> host;
    for (const Section& s : secs) {
        const uint32_t* pay = in.data() + s.payload_at;
        const int c = (int)s.c, W = (int)s.W;
        host.assign(s.out_words, 0);
        if (s.op == OP_TABLE) {
            const FbTablePlan& tp = s.tp;
            const size_t n = s.n, pairs = n * (size_t)W, H = tp.H, entries = pairs * H, batch_pairs = tp.batch_pairs;
            Affine<M>* d_base = nullptr;
            XYZZ<M>*pow = nullptr, *scratch = nullptr;
            if (table) CK(hipFree(table));
            table = nullptr;
            CK(hipMalloc((void**)&table, entries * sizeof(Affine<M>)));
            CK(hipMalloc((void**)&d_base, n * sizeof(Affine<M>)));
            CK(hipMalloc((void**)&pow, pairs * sizeof(XYZZ<M>)));
            CK(hipMalloc((void**)&scratch, batch_pairs * H * sizeof(XYZZ<M>)));
            CK(hipMemcpy(d_base, pay, n * sizeof(Affine<M>), hipMemcpyHostToDevice));
            CK(hipMemsetD32((hipDeviceptr_t)table, (int)FILL, entries * 16));
            CK(hipMemsetD32((hipDeviceptr_t)pow, (int)FILL, pairs * 32));
            CK(hipMemsetD32((hipDeviceptr_t)scratch, (int)FILL, batch_pairs * H * 32));
            CK(hipDeviceSynchronize());
            hipLaunchKernelGGL((k_fb_base_powers<C>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, (const Affine<M>*)d_base, (uint32_t)n, c, W, pow);
            for (size_t p0 = 0; p0 < pairs; p0 += batch_pairs) {
                const size_t np = pairs - p0 < batch_pairs ? pairs - p0 : batch_pairs;
                hipLaunchKernelGGL((k_fb_multiples<C>), dim3((unsigned)((np * tp.runs + tp.groups_per_wave - 1) / tp.groups_per_wave)), dim3(64), 0,
                                   0, (const XYZZ<M>*)pow, (uint32_t)p0, (uint32_t)np, tp.H, tp.lanes, tp.K, scratch);
                const size_t cnt = np * H;
                hipLaunchKernelGGL((k_fb_normalize<C>), dim3((unsigned)((cnt + 64 * 32 - 1) / (64 * 32))), dim3(64), 0, 0,
                                   (const XYZZ<M>*)scratch, cnt, table + p0 * H);
            }
            CK(hipGetLastError());
            CK(hipDeviceSynchronize());
            if (s.flag == 0) {
                CK(hipMemcpy(host.data(), table, entries * sizeof(Affine<M>), hipMemcpyDeviceToHost));
            } else {
                const uint32_t* idx = pay + n * 16;
                for (uint32_t k = 0; k < s.flag; k++)
                    CK(hipMemcpy(host.data() + (size_t)k * 16, table + idx[k], sizeof(Affine<M>), hipMemcpyDeviceToHost));
            }
            CK(hipFree(d_base)); CK(hipFree(pow)); CK(hipFree(scratch));
        } else if (s.op == OP_COMMIT) {
            uint8_t* d_rows = nullptr;
            XYZZ<M>* partial = nullptr;
            const size_t n_rows = s.n_rows;
            CK(hipMalloc((void**)&d_rows, s.payload_words * 4));
            CK(hipMalloc((void**)&partial, s.out_words * 4));
            CK(hipMemcpy(d_rows, pay, s.payload_words * 4, hipMemcpyHostToDevice));
            CK(hipMemsetD32((hipDeviceptr_t)partial, (int)FILL, s.out_words));
            CK(hipDeviceSynchronize());
            if (s.flag)
                hipLaunchKernelGGL((k_fb_commit<C, true>), dim3((unsigned)((n_rows + 255) / 256), s.S), dim3(256), 0, 0, (const uint8_t*)d_rows,
                                   (uint32_t)n_rows, s.n, s.row_stride, (const Affine<M>*)table, c, W, s.S, partial);
            else
                hipLaunchKernelGGL((k_fb_commit<C>), dim3((unsigned)((n_rows + 255) / 256), s.S), dim3(256), 0, 0, (const uint8_t*)d_rows,
                                   (uint32_t)n_rows, s.n, s.row_stride, (const Affine<M>*)table, c, W, s.S, partial);
            CK(hipGetLastError());
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(host.data(), partial, s.out_words * 4, hipMemcpyDeviceToHost));
            CK(hipFree(d_rows)); CK(hipFree(partial));
        } else if (s.op == OP_SMALL) {
            uint8_t* d_rows = nullptr;
            uint32_t* d_small = nullptr;                 // part | counters, as FixedBase<C>::commit_small lays them out
            uint32_t* d_pub = nullptr;                   // hdr (32 words) | out_sums
            const size_t part_words = (size_t)FB_SMALL_MAX_ROWS * FB_SMALL_MAX_SLICES * 32, pub_words = 32 + (size_t)FB_SMALL_MAX_ROWS * 32;
            CK(hipMalloc((void**)&d_rows, s.payload_words * 4));
            CK(hipMalloc((void**)&d_small, part_words * 4 + 1024));
            CK(hipMalloc((void**)&d_pub, pub_words * 4));
            CK(hipMemcpy(d_rows, pay, s.payload_words * 4, hipMemcpyHostToDevice));
            CK(hipMemsetD32((hipDeviceptr_t)d_small, (int)FILL, part_words));
            CK(hipMemset(d_small + part_words, 0, 1024));
            CK(hipMemsetD32((hipDeviceptr_t)d_pub, (int)FILL, pub_words));
            CK(hipDeviceSynchronize());
            hipLaunchKernelGGL((k_fb_commit_small<C>), dim3((unsigned)(s.n_rows * s.S)), dim3(SMALL_THREADS), 0, 0, (const uint8_t*)d_rows,
                               s.n_rows, s.n, s.row_stride, (const Affine<M>*)table, c, W, s.S, (XYZZ<M>*)d_small, d_small + part_words, d_pub,
                               (XYZZ<M>*)(d_pub + 32), 1u);
            CK(hipGetLastError());
            CK(hipDeviceSynchronize());
            size_t at = 0;
            CK(hipMemcpy(host.data() + at, d_small, (size_t)s.n_rows * s.S * 128, hipMemcpyDeviceToHost)); at += (size_t)s.n_rows * s.S * 32;
            CK(hipMemcpy(host.data() + at, d_pub + 32, (size_t)s.n_rows * 128, hipMemcpyDeviceToHost)); at += (size_t)s.n_rows * 32;
            CK(hipMemcpy(host.data() + at, d_small + part_words, (FB_SMALL_MAX_ROWS + 1) * 4, hipMemcpyDeviceToHost)); at += FB_SMALL_MAX_ROWS + 1;
            CK(hipMemcpy(host.data() + at, d_pub, 4, hipMemcpyDeviceToHost));
            CK(hipFree(d_rows)); CK(hipFree(d_small)); CK(hipFree(d_pub));
        } else {
            XYZZ<M>* partial = nullptr;
            uint8_t* d_out = nullptr;
            const size_t n_rows = s.n_rows, area = (size_t)(s.n_rows + s.sentinel) * s.S * 32;
            CK(hipMalloc((void**)&partial, area * 4));
            CK(hipMemsetD32((hipDeviceptr_t)partial, (int)FILL, area));
            CK(hipMemcpy(partial, pay, s.payload_words * 4, hipMemcpyHostToDevice));
            if (s.op == OP_FOLD) {
                if constexpr (C::F30_BUCKETS && C::F30_LAZY) {
                    const uint32_t rows_per_block = 128 / s.S;          // S / 2 quads per row, 64 quads per block
                    CK(hipDeviceSynchronize());
                    hipLaunchKernelGGL((k_fb_fold_quad<C>), dim3((unsigned)((n_rows + rows_per_block - 1) / rows_per_block)), dim3(256), 0, 0,
                                       partial, (uint32_t)n_rows, s.S);
                    CK(hipGetLastError());
                    CK(hipDeviceSynchronize());
                    CK(hipMemcpy(host.data(), partial, area * 4, hipMemcpyDeviceToHost));
                }
            } else {
                CK(hipMalloc((void**)&d_out, s.out_words * 4));
                CK(hipMemsetD32((hipDeviceptr_t)d_out, (int)FILL, s.out_words));
                CK(hipDeviceSynchronize());
                if (s.flag == 1)
                    hipLaunchKernelGGL((k_fb_finish<C, 1>), dim3((unsigned)((n_rows + 63) / 64)), dim3(64), 0, 0,
                                       (const XYZZ<M>*)partial, (uint32_t)n_rows, s.S, d_out);
                else if (s.flag == 2)
                    hipLaunchKernelGGL((k_fb_finish<C, 2>), dim3((unsigned)((n_rows + 127) / 128)), dim3(64), 0, 0,
                                       (const XYZZ<M>*)partial, (uint32_t)n_rows, s.S, d_out);
                else
                    hipLaunchKernelGGL((k_fb_finish<C, FB_FINISH_ROWS_MAX>),
                                       dim3((unsigned)((n_rows + 64 * FB_FINISH_ROWS_MAX - 1) / (64 * FB_FINISH_ROWS_MAX))), dim3(64), 0, 0,
                                       (const XYZZ<M>*)partial, (uint32_t)n_rows, s.S, d_out);
                CK(hipGetLastError());
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(host.data(), d_out, s.out_words * 4, hipMemcpyDeviceToHost));
                CK(hipFree(d_out));
            }
            CK(hipFree(partial));
        }
        if (put(fp, host.data(), host.size())) { fclose(fp); return 1; }
    }
    if (fclose(fp) != 0) BAD("short write of %s", out_path);
    if (table) CK(hipFree(table));
    return 0;
}

template <class C>
static int plan_dump(const char* curve, int argc, char** argv) {
    using M = typename C::Fp;
    printf("curve %s\n", curve);
    int mode = 0;
    auto num = [](const char* s, unsigned long long lo, unsigned long long hi, unsigned long long* v) {
        char* end = nullptr;
        *v = strtoull(s, &end, 10);
        return *s && !*end && *v >= lo && *v <= hi;
    };
    for (int i = 3; i < argc;) {
        if (!strcmp(argv[i], "c")) { mode = 1; i++; continue; }
        if (!strcmp(argv[i], "commit")) { mode = 2; i++; continue; }
        if (!strcmp(argv[i], "rows")) { mode = 3; i++; continue; }
        unsigned long long a = 0, b = 0, w = 0;
        if (mode == 1) {
            if (!num(argv[i], 2, 20, &a)) BAD("--plan: c = %s is outside 2 .. 20", argv[i]);
            const int c = (int)a, W = (C::SCALAR_BITS + 1 + c - 1) / c;
            const size_t pairs = (size_t)128 * W;
            const FbTablePlan p = fb_table_plan(c, pairs, sizeof(XYZZ<M>));
            printf("table c=%d W=%d H=%u lanes=%u K=%u runs=%u groups_per_wave=%u pairs=%zu batch_pairs=%zu\n", c, W, p.H, p.lanes, p.K, p.runs,
                   p.groups_per_wave, pairs, p.batch_pairs);
            i++;
        } else if (mode == 2) {
            if (i + 2 >= argc || !num(argv[i], 1, 0xfffffff0ull, &a) || !num(argv[i + 1], 1, 0xffff, &b) || !num(argv[i + 2], 1, 257, &w))
                BAD("--plan: commit takes groups of n_rows n_coeffs W");
            printf("commit n_rows=%zu n_coeffs=%zu W=%d S=%u SL=%u\n", (size_t)a, (size_t)b, (int)w, fb_commit_slices((size_t)a, (size_t)b, (int)w),
                   fb_small_slices((size_t)b, (int)w));
            i += 3;
        } else if (mode == 3) {
            if (!num(argv[i], 1, 0xfffffff0ull, &a)) BAD("--plan: n_rows = %s", argv[i]);
            printf("finish n_rows=%zu rows_per_lane=%d\n", (size_t)a, fb_finish_rows((size_t)a));
            i++;
        } else {
            BAD("--plan: expected c, commit or rows before %s", argv[i]);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(XYZZ<Bn254Fp>) == 128 && sizeof(XYZZ<Secp256k1Fp>) == 128 && sizeof(Affine<Bn254Fp>) == 64 &&
                  sizeof(Affine<Secp256k1Fp>) == 64, "the memory forms the file format states");
    const bool plan = argc >= 2 && strcmp(argv[1], "--plan") == 0;
    if (plan ? argc < 3 : argc != 4) {
        fprintf(stderr, "usage: fb_check <bn254|secp256k1> <in> <out>\n       fb_check --plan <bn254|secp256k1> [c <c> ...] [commit <n_rows> <n_coeffs> <W> ...] [rows <n_rows> ...]\n");
        return 2;
    }
    const std::string curve = argv[plan ? 2 : 1];
    if (curve != "bn254" && curve != "secp256k1") { fprintf(stderr, "fb_check: unknown curve %s\n", curve.c_str()); return 2; }
    if (plan) return curve == "bn254" ? plan_dump<Bn254G1>("bn254", argc, argv) : plan_dump<Secp256k1G>("secp256k1", argc, argv);
    std::vector<uint32_t> in;
    if (read_file(argv[2], in)) return 1;
    return curve == "bn254" ? run<Bn254G1>(in, argv[3]) : run<Secp256k1G>(in, argv[3]);
}

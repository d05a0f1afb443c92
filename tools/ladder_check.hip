// Per-form driver for the scalar-multiplication ladders of the MAC side and their digit recoders (porla_amd/csrc/mac_fft.hip.h,
// quad30.hip.h, glv.hip.h): launches the product's OWN kernels on scalars and points the test chose and writes back what they left.
// A pure transformer: no reference arithmetic lives here and no kernel body is copied -- the recoder ops call the header's device
// functions, the stage ops launch the header's kernels with the grid, block, dynamic LDS and function attributes mac_fft.hip's
// mac_stages / mac_encode_core give them (macq_lds_bytes, maco_lds_bytes, mac_lds_attributes).  Expected values are computed by
// tests/ladder_vectors.py from Python integers.
// Built by porla_amd/csrc/Makefile as porla_amd/ladder_check; run by tests/test_ladder_gpu.py.
//
//   ladder_check <curve> <op> <in> <out> [<op> <in> <out> ...]        curve: bn254 | secp256k1
//
// RECODER OPS -- a file of records of REC = 192 words (uint32, little endian), one lane per record; the output file holds the same
// records after the operation:
//   [  0,  16)  flags in: 1 flip (mac_wnaf5_step)
//   [ 16,  32)  A: the 128-bit magnitude m (4 words) or the 256-bit scalar k (8 words, below the group order)
//   [ 32, 192)  O: results; what the operation does not write stays as the test wrote it
//   mac_signed_digit    O[i] = digit i of m as int32, i = 0 .. 32
//   mac_wnaf5_step      O[i] = code of position i of (m, flip), i = 0 .. 128;  O[129, 134) = the five words left of {m, 0}
//   glv_split           O[0, 4) = |k1|, O[4] = k1 negative, O[5, 9) = |k2|, O[9] = k2 negative
//
// STAGE OPS -- a file of LAUNCHES, each a header of HDR = 32 words followed by its arrays:
//   header   0 magic, 1 n, 2 s, 3 total, 4 rows, 5 entries, [8, 16) wt (the scalar the by-value forms take as an argument)
//   stage forms: `rows` points of 32 words (the work array in the lazy memory form: rows / n tables of n rows), then `entries` = n
//       scalars of 8 words IN PLACE OF THE TWIDDLE TABLE (stage s reads entry e = j * (n >> (s-1)): mac_stage_index).  Output: the
//       work array after the launch; the forms that read digit codes run k_mac_wnaf_codes on the same table first, as
//       ensure_mac_codes does, and append its n / 32 entries of MACQ_CODES_STRIDE 16-bit words.
//         stage30, stage30_quad, stage30_oct                          per-butterfly scalars; total <= rows / 2 butterflies
//         stage30_uniform, stage30_quad_uniform, stage30_oct_uniform  one table, total = n / 2, the launch rules of mac_stages
//   inverse stage forms (icc_mac_decode.hip.h: k_imd_stage_quad, (A, B) -> (A + B, sc (A - B)) on the rows k, k + 2^(s-1)): the same
//       file layout as the stage forms, the table IN PLACE OF THE INVERSE TWIDDLES; s >= 2 (stage 1 has no ladder)
//         istage1_quad                                                k_imd_stage1_quad: (A, B) -> (A + B, A - B) on the rows 2 t, 2 t + 1;
//                                                                     s = 1, total = rows / 2, the table is not read
//         istage_quad                                                 per-butterfly scalars; total <= rows / 2 butterflies
//         istage_quad_uniform                                         whole tables, total = rows / 2, n >> s >= 16; the digit codes of
//                                                                     the table are made first and appended as for the stage forms
//   by-value forms: out[i] = wt * in[i] for i < n; `rows` >= n input rows follow the header (32 words each: memory form; 16 words:
//       64-byte big-endian affine), entries = 0.  Output: `rows` rows of 32 words, filled with 0xA5 bytes before the launch.  The
//       launches of a file have a slice each of one input and one output buffer and go out over a few streams, waited for once.
//         scale30 (k_mac_scale30, memory form), load30_wt (k_mac_load30<C, true>, affine), load30_quad (k_mac_load30_quad<C, false>,
//         affine), load30_quad_work (k_mac_load30_quad<C, true>, memory form)
// Every launch is checked against the rows and entries its file holds before it runs: a malformed file is refused, not launched.
#include "mac_fft.hip.h"
#include "icc_mac_decode.hip.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr int REC = 192, FI = 0, A0 = 16, O0 = 32, F_FLIP = 1;
constexpr int HDR = 32, H_MAGIC = 0, H_N = 1, H_S = 2, H_TOTAL = 3, H_ROWS = 4, H_ENTRIES = 5, H_WT = 8;
constexpr uint32_t MAGIC = 0x4c414444u;
constexpr uint32_t MAX_ROWS = 1u << 20;
constexpr int CODE_WORDS = MACQ_CODES_STRIDE / 2;                 // 32-bit words of one entry of the code table

enum Op {
    OP_DIGIT, OP_WNAF, OP_SPLIT,
    OP_STAGE, OP_STAGE_U, OP_QUAD, OP_QUAD_U, OP_OCT, OP_OCT_U,
    OP_SCALE, OP_LOAD_WT, OP_LOAD_QUAD, OP_LOAD_QUAD_WORK,
    OP_IQUAD, OP_IQUAD_U, OP_ISTAGE1,
    OP_COUNT
};
static const char* const OP_NAMES[OP_COUNT] = {
    "mac_signed_digit", "mac_wnaf5_step", "glv_split",
    "stage30", "stage30_uniform", "stage30_quad", "stage30_quad_uniform", "stage30_oct", "stage30_oct_uniform",
    "scale30", "load30_wt", "load30_quad", "load30_quad_work",
    "istage_quad", "istage_quad_uniform", "istage1_quad"};
static bool op_is_recoder(int op) { return op <= OP_SPLIT; }
static bool op_is_value(int op) { return op >= OP_SCALE && op <= OP_LOAD_QUAD_WORK; }
static bool op_is_uniform_stage(int op) { return op == OP_STAGE_U || op == OP_QUAD_U || op == OP_OCT_U; }
static bool op_affine_in(int op) { return op == OP_LOAD_WT || op == OP_LOAD_QUAD; }

template <class G, int OP>
__global__ void k_recode(uint32_t* io, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* rec = io + (size_t)i * REC;
    const uint32_t* A = rec + A0;
    uint32_t* O = rec + O0;
    if constexpr (OP == OP_DIGIT) {
        const uint32_t m[4] = {A[0], A[1], A[2], A[3]};
#pragma unroll 1
        for (int w = 0; w <= 32; w++) O[w] = (uint32_t)mac_signed_digit(m, w);
    } else if constexpr (OP == OP_WNAF) {
        uint32_t k[5] = {A[0], A[1], A[2], A[3], 0u};
        const bool flip = rec[FI + F_FLIP] != 0;
#pragma unroll 1
        for (int w = 0; w < MACQ_WNAF_LEN; w++) O[w] = mac_wnaf5_step(k, flip);
        for (int w = 0; w < 5; w++) O[MACQ_WNAF_LEN + w] = k[w];
    } else {
        uint32_t k[8], m1[4], m2[4];
        bool n1, n2;
        for (int w = 0; w < 8; w++) k[w] = A[w];
        glv_split<G>(k, m1, n1, m2, n2);
        for (int w = 0; w < 4; w++) { O[w] = m1[w]; O[5 + w] = m2[w]; }
        O[4] = n1 ? 1u : 0u;
        O[9] = n2 ? 1u : 0u;
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "ladder_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static int read_file(const char* path, std::vector<uint32_t>& v) {
    FILE* fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "ladder_check: cannot read %s\n", path); return 1; }
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (sz < 0 || sz % 4 != 0) { fprintf(stderr, "ladder_check: %s is not a whole number of words\n", path); fclose(fp); return 1; }
    v.resize((size_t)sz / 4);
    const size_t got = v.empty() ? 0 : fread(v.data(), 4, v.size(), fp);
    fclose(fp);
    if (got != v.size()) { fprintf(stderr, "ladder_check: short read of %s\n", path); return 1; }
    return 0;
}
static int write_file(const char* path, const uint32_t* v, size_t words) {
    FILE* fp = fopen(path, "wb");
    if (!fp) { fprintf(stderr, "ladder_check: cannot write %s\n", path); return 1; }
    const size_t put = words ? fwrite(v, 4, words, fp) : 0;
    if (fclose(fp) != 0 || put != words) { fprintf(stderr, "ladder_check: short write of %s\n", path); return 1; }
    return 0;
}

template <class C>
static int run_recoder(int op, std::vector<uint32_t>& io) {
    using G = typename C::Glv;
    if (io.size() % REC != 0) { fprintf(stderr, "ladder_check: not a whole number of %d-word records\n", REC); return 1; }
    const int n = (int)(io.size() / REC);
    if (n == 0) return 0;
    uint32_t* d_io = nullptr;
    const size_t bytes = io.size() * 4;
    CK(hipMalloc(&d_io, bytes));
    CK(hipMemcpy(d_io, io.data(), bytes, hipMemcpyHostToDevice));
    const dim3 grid((n + 63) / 64), block(64);
    if (op == OP_DIGIT) hipLaunchKernelGGL((k_recode<G, OP_DIGIT>), grid, block, 0, 0, d_io, n);
    else if (op == OP_WNAF) hipLaunchKernelGGL((k_recode<G, OP_WNAF>), grid, block, 0, 0, d_io, n);
    else hipLaunchKernelGGL((k_recode<G, OP_SPLIT>), grid, block, 0, 0, d_io, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(io.data(), d_io, bytes, hipMemcpyDeviceToHost));
    CK(hipFree(d_io));
    return 0;
}

struct Launch {
    uint32_t n, s, total, rows, entries;
    MacScalar wt;
    size_t at_rows, at_tws;                                       // word offsets into the input file
};
static int ilog2(uint32_t v) { int l = 0; while ((1u << l) < v) l++; return l; }
static int refuse(const char* why) { fprintf(stderr, "ladder_check: refused: %s\n", why); return 1; }

// the launches of a file, each checked against what the kernel of `op` reads and writes
static int parse_launches(int op, const std::vector<uint32_t>& in, std::vector<Launch>& out) {
    const size_t row_words = op_affine_in(op) ? 16 : 32;
    size_t at = 0;
    while (at < in.size()) {
        if (in.size() - at < (size_t)HDR || in[at + H_MAGIC] != MAGIC) return refuse("no launch header");
        Launch l;
        l.n = in[at + H_N]; l.s = in[at + H_S]; l.total = in[at + H_TOTAL]; l.rows = in[at + H_ROWS]; l.entries = in[at + H_ENTRIES];
        for (int i = 0; i < 8; i++) l.wt.v[i] = in[at + H_WT + i];
        if (l.rows == 0 || l.rows > MAX_ROWS || l.entries > MAX_ROWS) return refuse("row or entry count");
        l.at_rows = at + HDR;
        l.at_tws = l.at_rows + (size_t)l.rows * row_words;
        at = l.at_tws + (size_t)l.entries * 8;
        if (at > in.size()) return refuse("the file ends inside a launch");
        if (op_is_value(op)) {
            if (l.n == 0 || l.n > l.rows || l.entries != 0) return refuse("a by-value form needs 1 <= n <= rows and no table");
        } else {
            if (l.n < 2 || l.n > MAX_ROWS) return refuse("n must be 2 .. 2^20");
            const int logn = ilog2(l.n);
            if ((1u << logn) != l.n || l.s < 1 || (int)l.s > logn) return refuse("n must be a power of two and 1 <= s <= log2 n");
            if (l.rows % l.n != 0 || l.entries != l.n) return refuse("rows must be whole tables of n rows and entries = n");
            if (l.total == 0 || l.total > l.rows / 2) return refuse("total must be 1 .. rows / 2");
            if (op == OP_IQUAD || op == OP_IQUAD_U) {
                if (l.s < 2) return refuse("stage 1 of the decode has no ladder (istage1_quad)");
                if (op == OP_IQUAD_U && (l.total != l.rows / 2 || !imd_stage_uniform(l.n, (int)l.s)))
                    return refuse("the wave-uniform inverse stage runs on whole tables, total = rows / 2, n >> s >= 16");
            }
            if (op == OP_ISTAGE1 && (l.s != 1 || l.total != l.rows / 2)) return refuse("istage1_quad runs stage 1 on every pair: s = 1, total = rows / 2");
            if (op_is_uniform_stage(op)) {
                // the launch rules of mac_stages for the wave-uniform forms
                if (l.rows != l.n || l.total != l.n / 2 || l.n < 128) return refuse("a wave-uniform form runs on one table of n >= 128 rows, total = n / 2");
                if (l.s < 2) return refuse("stage 1 is never a wave-uniform launch (its twiddles are all 1: k_mac_stage1_quad, or no ladder)");
                const uint32_t share = op == OP_STAGE_U ? 64u : 16u;
                if ((l.n >> l.s) < share) return refuse("n >> s is below the butterflies a wave shares a twiddle among");
                if (op == OP_STAGE_U && (l.total & 255u) != 0) return refuse("n / 2 must be a multiple of 256");
                if (op == OP_OCT_U && l.total > MACO_MAX_BUTTERFLIES) return refuse("too many butterflies for eight lanes each");
            }
        }
        out.push_back(l);
    }
    return 0;
}

// The by-value forms: one launch per scalar, each a single short block whose time is a ladder's latency.  Every launch has its own
// slice of one input and one output buffer, so the launches go out back to back over a few streams and are waited for once.
constexpr int VALUE_STREAMS = 4;
template <class C>
static int run_value_launches(int op, const std::vector<uint32_t>& in, const std::vector<Launch>& ls, std::vector<uint32_t>& result) {
    using M = typename C::Fp;
    const size_t row_words = op_affine_in(op) ? 16 : 32;
    size_t rows = 0;
    for (const Launch& l : ls) rows += l.rows;
    std::vector<uint32_t> packed(rows * row_words);
    size_t at = 0;
    for (const Launch& l : ls) {
        memcpy(packed.data() + at * row_words, in.data() + l.at_rows, (size_t)l.rows * row_words * 4);
        at += l.rows;
    }
    uint32_t *d_in = nullptr, *d_out = nullptr;
    CK(hipMalloc(&d_in, packed.size() * 4));
    CK(hipMalloc(&d_out, rows * 128));
    CK(hipMemcpy(d_in, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xA5, rows * 128));
    CK(hipDeviceSynchronize());
    mac_lds_attributes<C>();
    hipStream_t streams[VALUE_STREAMS];
    for (int i = 0; i < VALUE_STREAMS; i++) CK(hipStreamCreate(&streams[i]));
    at = 0;
    for (size_t i = 0; i < ls.size(); i++) {
        const Launch& l = ls[i];
        const uint32_t n = l.n;                                           // (n <= l.rows: parse_launches)
        hipStream_t st = streams[i % VALUE_STREAMS];
        const uint32_t* src32 = d_in + at * row_words;
        const uint8_t* src = reinterpret_cast<const uint8_t*>(src32);
        XYZZ<M>* out = reinterpret_cast<XYZZ<M>*>(d_out) + at;
        if (op == OP_SCALE)
            hipLaunchKernelGGL((k_mac_scale30<C>), dim3((n + 63) / 64), dim3(64), 0, st, reinterpret_cast<const XYZZ<M>*>(src32), n, out, l.wt);
        else if (op == OP_LOAD_WT)
            hipLaunchKernelGGL((k_mac_load30<C, true>), dim3((n + 63) / 64), dim3(64), 0, st, src, n, out, l.wt);
        else if (op == OP_LOAD_QUAD)
            hipLaunchKernelGGL((k_mac_load30_quad<C>), dim3((n + MACQ_BF - 1) / MACQ_BF), dim3(4 * MACQ_BF), macq_lds_bytes<C>(), st, src, n, out, l.wt);
        else
            hipLaunchKernelGGL((k_mac_load30_quad<C, true>), dim3((n + MACQ_BF - 1) / MACQ_BF), dim3(4 * MACQ_BF), macq_lds_bytes<C>(), st, src, n, out, l.wt);
        at += l.rows;
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    for (int i = 0; i < VALUE_STREAMS; i++) CK(hipStreamDestroy(streams[i]));
    result.resize(rows * 32);
    CK(hipMemcpy(result.data(), d_out, rows * 128, hipMemcpyDeviceToHost));
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    return 0;
}

template <class C>
static int run_launches(int op, const std::vector<uint32_t>& in, std::vector<uint32_t>& result) {
    using M = typename C::Fp;
    static_assert(sizeof(XYZZ<M>) == 128, "a memory-form point is 32 words");
    std::vector<Launch> ls;
    if (parse_launches(op, in, ls)) return 1;
    if (ls.empty()) return 0;
    if (op_is_value(op)) return run_value_launches<C>(op, in, ls, result);
    size_t max_rows = 1, max_entries = 1;
    for (const Launch& l : ls) { if (l.rows > max_rows) max_rows = l.rows; if (l.entries > max_entries) max_entries = l.entries; }
    uint32_t *d_work = nullptr, *d_tws = nullptr;
    uint16_t* d_codes = nullptr;
    const size_t codes_bytes = (max_entries / 32 + 1) * MACQ_CODES_STRIDE * sizeof(uint16_t);
    CK(hipMalloc(&d_work, max_rows * 128));
    CK(hipMalloc(&d_tws, max_entries * 32));
    CK(hipMalloc(&d_codes, codes_bytes));
    mac_lds_attributes<C>();
    imd_lds_attributes<C>();
    for (const Launch& l : ls) {
        XYZZ<M>* work = reinterpret_cast<XYZZ<M>*>(d_work);
        const uint32_t n = l.n, total = l.total;
        const int s = (int)l.s;
        bool with_codes = false;
        CK(hipMemcpy(d_work, in.data() + l.at_rows, (size_t)l.rows * 128, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_tws, in.data() + l.at_tws, (size_t)l.entries * 32, hipMemcpyHostToDevice));
        const uint32_t* tws = d_tws;
        const uint16_t* none = nullptr;
        if (op_is_uniform_stage(op) || op == OP_IQUAD_U) {             // the digit codes of the table, as ensure_mac_codes makes them
            with_codes = true;
            const uint32_t entries = n >> MACQ_CODES_EXP_SHIFT;
            CK(hipMemset(d_codes, 0xA5, codes_bytes));
            hipLaunchKernelGGL((k_mac_wnaf_codes<C>), dim3((entries + 63) / 64), dim3(64), 0, 0, tws, entries, d_codes);
        }
        if (op == OP_ISTAGE1)
            hipLaunchKernelGGL((k_imd_stage1_quad<C>), dim3((total + 63) / 64), dim3(256), 0, 0, work, l.rows);
        else if (op == OP_IQUAD || op == OP_IQUAD_U)
            imd_launch_stage<C>(op == OP_IQUAD_U, work, tws, n, s, d_codes, total, 0);
        else if (op == OP_OCT_U)
            hipLaunchKernelGGL((k_mac_stage30_oct_uniform<C>), dim3(total / MACO_BF), dim3(8 * MACO_BF), maco_lds_bytes<C>(), 0, work, tws, n, s, d_codes);
        else if (op == OP_QUAD_U)
            hipLaunchKernelGGL((k_mac_stage30_quad<C, true>), dim3((total + MACQ_BF - 1) / MACQ_BF), dim3(4 * MACQ_BF), macq_lds_bytes<C>(), 0, work, tws, n, s,
                               d_codes);
        else if (op == OP_OCT)
            hipLaunchKernelGGL((k_mac_stage30_oct<C>), dim3((total + MACO_BF - 1) / MACO_BF), dim3(8 * MACO_BF), maco_lds_bytes<C>(), 0, work, tws, n, total, s);
        else if (op == OP_QUAD)
            hipLaunchKernelGGL((k_mac_stage30_quad<C, false, uint32_t>), dim3((total + MACQ_BF - 1) / MACQ_BF), dim3(4 * MACQ_BF), macq_lds_bytes<C>(), 0, work,
                               tws, n, s, none, total);
        else if (op == OP_STAGE_U)
            hipLaunchKernelGGL((k_mac_stage30<C, true>), dim3((total + 255) / 256), dim3(256), 0, 0, work, tws, n, s, d_codes);
        else
            hipLaunchKernelGGL((k_mac_stage30<C, false, uint32_t>), dim3((total + 255) / 256), dim3(256), 0, 0, work, tws, n, s, none, total);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        const size_t at = result.size();
        result.resize(at + (size_t)l.rows * 32);
        CK(hipMemcpy(result.data() + at, d_work, (size_t)l.rows * 128, hipMemcpyDeviceToHost));
        if (with_codes) {
            const size_t words = (size_t)(n >> MACQ_CODES_EXP_SHIFT) * CODE_WORDS, at2 = result.size();
            result.resize(at2 + words);
            CK(hipMemcpy(result.data() + at2, d_codes, words * 4, hipMemcpyDeviceToHost));
        }
    }
    CK(hipFree(d_work));
    CK(hipFree(d_tws));
    CK(hipFree(d_codes));
    return 0;
}

template <class C>
static int run(int op, const char* in, const char* out) {
    std::vector<uint32_t> io;
    if (read_file(in, io)) return 1;
    if (op_is_recoder(op)) {
        if (run_recoder<C>(op, io)) return 1;
        return write_file(out, io.data(), io.size());
    }
    std::vector<uint32_t> result;
    if (run_launches<C>(op, io, result)) return 1;
    return write_file(out, result.data(), result.size());
}

int main(int argc, char** argv) {
    if (argc < 5 || (argc - 2) % 3 != 0) {
        fprintf(stderr, "usage: ladder_check <bn254|secp256k1> <op> <in> <out> [<op> <in> <out> ...]\nops:");
        for (int i = 0; i < OP_COUNT; i++) fprintf(stderr, " %s", OP_NAMES[i]);
        fprintf(stderr, "\n");
        return 2;
    }
    const std::string curve = argv[1];
    if (curve != "bn254" && curve != "secp256k1") { fprintf(stderr, "ladder_check: unknown curve %s\n", curve.c_str()); return 2; }
    for (int at = 2; at + 2 < argc; at += 3) {
        int op = -1;
        for (int i = 0; i < OP_COUNT; i++) if (!strcmp(argv[at], OP_NAMES[i])) op = i;
        if (op < 0) { fprintf(stderr, "ladder_check: unknown operation %s\n", argv[at]); return 2; }
        const int rc = curve == "bn254" ? run<Bn254G1>(op, argv[at + 1], argv[at + 2]) : run<Secp256k1G>(op, argv[at + 1], argv[at + 2]);
        if (rc) return rc;
    }
    return 0;
}

// Driver for the sort front of porla_amd/csrc/msm.hip.h on scalars the caller wrote: k_scalar_or, k_points_to_mont, k_digits_partition
// and k_partition_sort, the product's own kernels in the launch shape of msm.hip.h:sort_front_plan (or with the partition width, the
// half-size instantiation and the blocks per tile forced by the file).  A pure transformer: no reference arithmetic lives here --
// every array comes back as it lies in memory, over the fill word 0xA5A5A5A5 wherever no kernel wrote.  Expected values are computed
// by tests/sort_vectors.py.  Built by porla_amd/csrc/Makefile as porla_amd/sort_check; run by tests/test_sort_gpu.py and
// tests/test_sort_vectors_cpu.py.
//
//   sort_check <bn254|secp256k1> <in> <out>
//   sort_check --plan <n> <glv> <c> <W> ...          sort_front_plan's fields, one line per group of four numbers; no HIP call
//
// Input (uint32 words, little endian): a sequence of sections
//   [0, 12)  header: magic 0x534f5254, n, glv (0 | 1), c, W, lowbits, sort_half, wg, n_points, 0, 0, 0
//            0xffffffff for lowbits, sort_half or wg: the value of sort_front_plan(n, glv, c, W)
//   then     n scalars of 8 words: 32 bytes big endian, as the bytes lie
//   then     n_points points of 16 words: the 64-byte big-endian wire form X || Y; n_points = 0: no points stage
// Output per section, SUBS = glv ? 2 : 1, T = ceil(n / 4096), B = 2^(c-1):
//   or[8]  pts[n_points SUBS][16]  tile_off[W T 129] (16-bit, padded to a whole word)  tile_items[W T 4096 SUBS]  counts[W B]
//   starts[W B]  entries[W n SUBS]  ctrl[CTRL_WORDS]
// Every header is validated on the host before the first launch, so that no kernel leaves its LDS arrays or its buffers; a file that
// fails, and any HIP error, ends the run with a message and status 1.
#include "msm.hip.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr uint32_t MAGIC = 0x534f5254u, HDR = 12, DEFAULT = 0xffffffffu, FILL = 0xA5A5A5A5u;
constexpr uint32_t MAX_N = 1u << 18, MAX_BUCKETS = 1u << 21;
constexpr size_t MAX_WORDS = (size_t)1 << 26;         // tile_items and entries of one section: 256 MiB each at the most

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "sort_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define BAD(...) do { fprintf(stderr, "sort_check: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

struct Section {
    uint32_t n, glv, c, W, n_points;
    SortFrontPlan plan;
    size_t scalars_at, points_at;                     // word offsets into the file
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

// the shape limits of the two kernels: the LDS arrays of k_digits_partition (MAX_PARTS counters) and of k_partition_sort (MAX_LOW
// counters, `per` <= 4 of them per thread), the 13-bit local index beside lowbits + 1 bits in an item
static int check_shape(uint32_t n, uint32_t glv, uint32_t c, uint32_t W) {
    if (glv > 1 || n == 0 || n > MAX_N) BAD("header out of range (n %u, glv %u)", n, glv);
    if (c < 2 || c > 20 || W < 1) BAD("shape out of range (c %u, W %u)", c, W);
    if (((uint64_t)W << (c - 1)) > MAX_BUCKETS) BAD("shape out of range (%u windows of %u buckets)", W, 1u << (c - 1));
    const size_t T = (n + TILE - 1) / TILE, cap = glv ? 2 * TILE : TILE;
    if ((size_t)W * T * cap > MAX_WORDS) BAD("shape out of range (%u windows of %zu tiles)", W, T);
    return 0;
}

static int make_section(Section& sc, const uint32_t* h) {
    sc.n = h[1]; sc.glv = h[2]; sc.c = h[3]; sc.W = h[4]; sc.n_points = h[8];
    if (check_shape(sc.n, sc.glv, sc.c, sc.W)) return 1;
    if (sc.n_points > MAX_N || h[9] || h[10] || h[11]) BAD("header out of range (points %u, reserved %u %u %u)", sc.n_points, h[9], h[10], h[11]);
    sc.plan = sort_front_plan(sc.n, sc.glv != 0, (int)sc.c, (int)sc.W);
    const int c = (int)sc.c;
    if (h[6] != DEFAULT) {
        if (h[6] > 1) BAD("sort_half must be 0 or 1");
        sc.plan.sort_half = h[6] != 0;
    }
    if (h[5] != DEFAULT) {
        if (h[5] > (uint32_t)(c - 1)) BAD("lowbits %u above c - 1", h[5]);
        sc.plan.lowbits = (int)h[5];
        sc.plan.P = 1 << (c - 1 - sc.plan.lowbits);
    }
    if (h[7] != DEFAULT) sc.plan.wg = h[7];
    const int lb = sc.plan.lowbits;
    if (lb > (sc.plan.sort_half ? 11 : 12)) BAD("lowbits %d above the %s sort's counters", lb, sc.plan.sort_half ? "half" : "full");
    if (c - 1 - lb > 7) BAD("c - 1 - lowbits = %d: more than %d partitions", c - 1 - lb, MAX_PARTS);
    if (sc.plan.wg < 1 || sc.plan.wg > 16 || sc.plan.wg > sc.W) BAD("wg %u outside 1 .. min(16, W)", sc.plan.wg);
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
    // ---- validation: nothing below reaches the device unless every section's shape is inside the kernels' limits
    std::vector<Section> secs;
    size_t at = 0, max_n = 0, max_pts = 0, max_items = 0, max_off = 0, max_nb = 0, max_entries = 0;
    if (in.empty()) BAD("not a sort_check file");
    do {
        if (in.size() < at + HDR || in[at] != MAGIC) BAD("section %zu: not a sort_check file", secs.size());
        Section sc;
        if (make_section(sc, in.data() + at)) return 1;
        sc.scalars_at = at + HDR;
        sc.points_at = sc.scalars_at + (size_t)8 * sc.n;
        at = sc.points_at + (size_t)16 * sc.n_points;
        if (in.size() < sc.points_at) BAD("section %zu: file ends inside the scalars", secs.size());
        if (in.size() < at) BAD("section %zu: file ends inside the points", secs.size());
        const size_t subs = sc.glv ? 2 : 1, T = sc.plan.T_tiles;
        max_n = std::max(max_n, (size_t)sc.n);
        max_pts = std::max(max_pts, subs * sc.n_points);
        max_items = std::max(max_items, (size_t)sc.W * T * sc.plan.tile_cap);
        max_off = std::max(max_off, ((size_t)sc.W * T * (MAX_PARTS + 1) + 1) / 2);       // words
        max_nb = std::max(max_nb, (size_t)sc.W << (sc.c - 1));
        max_entries = std::max(max_entries, (size_t)sc.W * subs * sc.n);
        secs.push_back(sc);
    } while (at < in.size());

    // ---- device buffers
    uint8_t *d_scalars = nullptr, *d_points_be = nullptr;
    Affine<M>* d_pts = nullptr;
    uint32_t *d_or = nullptr, *d_items = nullptr, *d_off = nullptr, *d_counts = nullptr, *d_starts = nullptr, *d_entries = nullptr, *d_ctrl = nullptr;
    if (dev_alloc(&d_scalars, 32 * max_n) || dev_alloc(&d_points_be, 64 * max_pts) || dev_alloc(&d_pts, max_pts) || dev_alloc(&d_or, 8) ||
        dev_alloc(&d_items, max_items) || dev_alloc(&d_off, max_off) || dev_alloc(&d_counts, max_nb) || dev_alloc(&d_starts, max_nb) ||
        dev_alloc(&d_entries, max_entries) || dev_alloc(&d_ctrl, CTRL_WORDS))
        return 1;
    FILE* fp = fopen(out_path, "wb");
    if (!fp) BAD("cannot write %s", out_path);
    std::vector<uint32_t> host;
    for (const Section& sc : secs) {
        const SortFrontPlan& pl = sc.plan;
        const uint32_t n = sc.n, T = pl.T_tiles;
        const int c = (int)sc.c, W = (int)sc.W;
        const size_t subs = sc.glv ? 2 : 1, nb = (size_t)W << (c - 1);
        struct { void* d; size_t words; } areas[8] = {
            {d_or, 8}, {d_pts, subs * sc.n_points * 16}, {d_off, ((size_t)W * T * (MAX_PARTS + 1) + 1) / 2}, {d_items, (size_t)W * T * pl.tile_cap},
            {d_counts, nb}, {d_starts, nb}, {d_entries, (size_t)W * subs * n}, {d_ctrl, (size_t)CTRL_WORDS}};
        // what no launch has written reads as a pattern, not as a plausible value
        for (auto& a : areas)
            if (a.words) CK(hipMemsetD32((hipDeviceptr_t)a.d, (int)FILL, a.words));
        CK(hipMemcpy(d_scalars, in.data() + sc.scalars_at, (size_t)32 * n, hipMemcpyHostToDevice));
        if (sc.n_points) CK(hipMemcpy(d_points_be, in.data() + sc.points_at, (size_t)64 * sc.n_points, hipMemcpyHostToDevice));
        CK(hipMemset(d_or, 0, 32));
        CK(hipDeviceSynchronize());
        unsigned blocks = (unsigned)(((size_t)n + 255) / 256);       // the grid rule of msm_launch
        if (blocks > 512) blocks = 512;
        hipLaunchKernelGGL(k_scalar_or, dim3(blocks), dim3(256), 0, 0, (const uint8_t*)d_scalars, n, d_or);
        if (sc.n_points) {
            const uint32_t np = sc.n_points;
            if (sc.glv) hipLaunchKernelGGL((k_points_to_mont<C, true, C::F30_BUCKETS>), dim3((np + 255) / 256), dim3(256), 0, 0, (const uint8_t*)d_points_be, d_pts, np);
            else hipLaunchKernelGGL((k_points_to_mont<C, false, C::F30_BUCKETS>), dim3((np + 255) / 256), dim3(256), 0, 0, (const uint8_t*)d_points_be, d_pts, np);
        }
        if (sc.glv)
            hipLaunchKernelGGL((k_digits_partition<C, true>), dim3(T, pl.wg), dim3(TILE_THREADS), 0, 0, (const uint8_t*)d_scalars, n, c, W, pl.lowbits,
                               d_items, (uint16_t*)d_off, d_ctrl);
        else
            hipLaunchKernelGGL((k_digits_partition<C, false>), dim3(T, pl.wg), dim3(TILE_THREADS), 0, 0, (const uint8_t*)d_scalars, n, c, W, pl.lowbits,
                               d_items, (uint16_t*)d_off, d_ctrl);
        sort_launch(pl, c, W, 0, (const uint32_t*)d_items, (const uint16_t*)d_off, d_counts, d_starts, d_entries, d_ctrl);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        for (auto& a : areas) {
            if (!a.words) continue;
            host.resize(a.words);
            CK(hipMemcpy(host.data(), a.d, a.words * 4, hipMemcpyDeviceToHost));
            if (fwrite(host.data(), 4, host.size(), fp) != host.size()) { fclose(fp); BAD("short write of %s", out_path); }
        }
    }
    if (fclose(fp) != 0) BAD("short write of %s", out_path);
    CK(hipFree(d_scalars)); CK(hipFree(d_points_be)); CK(hipFree(d_pts)); CK(hipFree(d_or)); CK(hipFree(d_items)); CK(hipFree(d_off));
    CK(hipFree(d_counts)); CK(hipFree(d_starts)); CK(hipFree(d_entries)); CK(hipFree(d_ctrl));
    return 0;
}

static bool parse_u32(const char* s, uint32_t* v) {
    char* end = nullptr;
    const unsigned long long x = strtoull(s, &end, 10);
    if (!*s || *end || x >= DEFAULT) return false;
    *v = (uint32_t)x;
    return true;
}

static int plan_dump(int argc, char** argv) {
    const int count = argc - 2;
    if (count < 4 || count % 4 != 0) { fprintf(stderr, "usage: sort_check --plan <n> <glv> <c> <W> ...\n"); return 2; }
    for (int g = 0; g < count; g += 4) {
        uint32_t v[4];
        for (int k = 0; k < 4; k++)
            if (!parse_u32(argv[2 + g + k], &v[k])) BAD("not a number: %s", argv[2 + g + k]);
        // --plan reaches no kernel: any n the product takes in one launch, the shape limits as for a file
        if (v[1] > 1 || v[0] == 0 || v[0] >= (1u << 30)) BAD("header out of range (n %u, glv %u)", v[0], v[1]);
        if (v[2] < 2 || v[2] > 20 || v[3] < 1 || v[3] > 4096) BAD("shape out of range (c %u, W %u)", v[2], v[3]);
        const SortFrontPlan pl = sort_front_plan(v[0], v[1] != 0, (int)v[2], (int)v[3]);
        printf("n=%u glv=%u c=%u W=%u tile_cap=%u T_tiles=%u lowbits=%d sort_half=%d P=%d wg=%u\n", v[0], v[1], v[2], v[3], pl.tile_cap, pl.T_tiles,
               pl.lowbits, pl.sort_half ? 1 : 0, pl.P, pl.wg);
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(Affine<Bn254Fp>) == 64 && sizeof(Affine<Secp256k1Fp>) == 64, "the memory form the output format states");
    if (argc >= 2 && strcmp(argv[1], "--plan") == 0) return plan_dump(argc, argv);
    if (argc != 4) {
        fprintf(stderr, "usage: sort_check <bn254|secp256k1> <in> <out>\n       sort_check --plan <n> <glv> <c> <W> ...\n");
        return 2;
    }
    const std::string curve = argv[1];
    if (curve != "bn254" && curve != "secp256k1") { fprintf(stderr, "sort_check: unknown curve %s\n", curve.c_str()); return 2; }
    std::vector<uint32_t> in;
    if (read_file(argv[2], in)) return 1;
    return curve == "bn254" ? run<Bn254G1>(in, argv[3]) : run<Secp256k1G>(in, argv[3]);
}

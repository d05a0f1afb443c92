// Driver for the bucket reduction tree of porla_amd/csrc/msm.hip.h on bucket arrays the caller wrote: k_tree_front2, k_tree_level,
// k_tree_level_quad and k_tree_tail, the product's own kernels, issued by the product's own schedule (msm_tree.hip.h: tree_plan and
// tree_enqueue, the two halves of msm_impl.hip.h:msm_tree_launch).  A pure transformer: no reference arithmetic lives here and nothing
// is normalised -- fin and the three scratch areas come back as they lie.  Expected values are computed by tests/tree_vectors.py.
// Built by porla_amd/csrc/Makefile as porla_amd/tree_check; run by tests/test_tree_gpu.py and tests/test_tree_vectors_cpu.py.
//
//   tree_check <bn254|secp256k1> <in> <out>
//
// Input (uint32 words, little endian): one or more sections, each
//   [0, 12)  header: magic 0x54524545, c, W, lone (0 | 1), parts, front2, quad_max_tasks, l0, n_runs, 0, 0, 0
//            parts .. l0 are the fields of TreeOptions, 0xffffffff = the product's default
//   then per run  W * 2^(c-1) buckets of 32 words in the lazy memory form, as they lie (window w's bucket b at (w * 2^(c-1) + b) * 32)
// Per run the three scratch areas and fin are filled with the word 0xA5A5A5A5 (not zero: zero reads as infinity, and a node read
// before it is written would go unnoticed among sparse sums), the plan is enqueued, the device synchronised.
// Output, per run:  fin[W][c][32], the S area [s_entries][32], the M area [m_entries][32], the tail's area [mt_entries][32] -- the
//            sizes are the plan's, slack included.
// Every section is validated on the host before the first launch: ranges (c <= 17, W * 2^(c-1) <= 2^18), the file's length and the
// plan's own refusals.  A file that fails, and any HIP error, ends the run with a message and status 1.
//
//   tree_check --plan <bn254|secp256k1> <c> <W> <lone> [<parts> <front2> <quad_max_tasks> <l0>] ...
//
// prints the plan (sizes, launches, offsets; tree_plan_text) of every group of arguments, - = the product's default; no HIP call.
#include "msm_tree.hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr uint32_t MAGIC = 0x54524545u, HDR = 12, DEFAULT = 0xffffffffu, FILL = 0xA5A5A5A5u;
constexpr uint32_t MAX_C = 17, MAX_BUCKETS = 1u << 18, MAX_RUNS = 4096;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "tree_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define BAD(...) do { fprintf(stderr, "tree_check: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

struct Section {
    TreePlan plan;
    size_t buckets_at;     // word offset of the first run
    uint32_t n_runs;
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

static TreeOptions options(uint32_t parts, uint32_t front2, uint32_t quad_max, uint32_t l0) {
    TreeOptions o;
    if (parts != DEFAULT) o.parts = (int)(parts & 0x7fffffffu);
    if (front2 != DEFAULT) o.front2 = (int)(front2 & 0x7fffffffu);
    if (quad_max != DEFAULT) o.quad_max_tasks = (long long)quad_max;
    if (l0 != DEFAULT) o.l0 = (int)(l0 & 0x7fffffffu);
    return o;
}

// the header's ranges (device: the driver's caps on top) and the plan's own refusals
static int make_plan(TreePlan& plan, uint32_t c, uint32_t W, uint32_t lone, const TreeOptions& o, bool lazy, bool device) {
    if (lone > 1 || o.front2 > 1) BAD("header out of range (lone %u, front2 %d)", lone, o.front2);
    if (device && (c < 2 || c > MAX_C || W < 1 || W > MAX_BUCKETS || ((size_t)W << (c - 1)) > MAX_BUCKETS))
        BAD("header out of range (c %u, W %u)", c, W);
    if (c > 64 || W > (1u << 30)) BAD("header out of range (c %u, W %u)", c, W);
    const std::string refused = tree_plan(plan, (int)c, (int)W, lone != 0, lazy, o);
    if (!refused.empty()) BAD("the plan is refused: %s", refused.c_str());
    return 0;
}

template <class C>
static int run(const std::vector<uint32_t>& in, const char* out_path) {
    using M = typename C::Fp;
    // ---- validation: nothing below reaches the device unless every section's plan stands and the file holds its runs
    std::vector<Section> secs;
    size_t at = 0, max_nb = 0, max_s = 0, max_m = 0, max_mt = 0, max_fin = 0;
    do {
        if (in.size() < at + HDR || in[at] != MAGIC) BAD("not a tree_check file (section at word %zu)", at);
        const uint32_t* h = in.data() + at;
        Section sc;
        if (make_plan(sc.plan, h[1], h[2], h[3], options(h[4], h[5], h[6], h[7]), C::F30_LAZY, true)) return 1;
        sc.n_runs = h[8];
        if (sc.n_runs == 0 || sc.n_runs > MAX_RUNS || h[9] || h[10] || h[11]) BAD("header out of range (runs %u)", sc.n_runs);
        sc.buckets_at = at + HDR;
        const size_t nb = (size_t)sc.plan.W * sc.plan.B;
        if (in.size() < sc.buckets_at + (size_t)sc.n_runs * nb * 32) BAD("file ends inside the buckets");
        at = sc.buckets_at + (size_t)sc.n_runs * nb * 32;
        if (nb > max_nb) max_nb = nb;
        if (sc.plan.s_entries > max_s) max_s = sc.plan.s_entries;
        if (sc.plan.m_entries > max_m) max_m = sc.plan.m_entries;
        if (sc.plan.mt_entries > max_mt) max_mt = sc.plan.mt_entries;
        if (sc.plan.fin_entries > max_fin) max_fin = sc.plan.fin_entries;
        secs.push_back(std::move(sc));
    } while (at < in.size());

    // ---- device buffers: exactly the plan's sizes are filled, used and read back
    XYZZ<M>*d_bk = nullptr, *d_s = nullptr, *d_m = nullptr, *d_mt = nullptr, *d_fin = nullptr;
    CK(hipMalloc((void**)&d_bk, max_nb * sizeof(XYZZ<M>)));
    CK(hipMalloc((void**)&d_s, max_s * sizeof(XYZZ<M>)));
    CK(hipMalloc((void**)&d_m, max_m * sizeof(XYZZ<M>)));
    CK(hipMalloc((void**)&d_mt, max_mt * sizeof(XYZZ<M>)));
    CK(hipMalloc((void**)&d_fin, max_fin * sizeof(XYZZ<M>)));
    hipStream_t st[2];
    CK(hipStreamCreateWithFlags(&st[0], hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&st[1], hipStreamNonBlocking));
    FILE* fp = fopen(out_path, "wb");
    if (!fp) BAD("cannot write %s", out_path);
    std::vector<uint32_t> host;
    for (const Section& sc : secs) {
        const TreePlan& p = sc.plan;
        const size_t nb = (size_t)p.W * p.B;
        struct { XYZZ<M>* d; size_t entries; } areas[4] = {{d_fin, p.fin_entries}, {d_s, p.s_entries}, {d_m, p.m_entries}, {d_mt, p.mt_entries}};
        for (uint32_t r = 0; r < sc.n_runs; r++) {
            CK(hipMemcpy(d_bk, in.data() + sc.buckets_at + (size_t)r * nb * 32, nb * sizeof(XYZZ<M>), hipMemcpyHostToDevice));
            for (auto& a : areas) CK(hipMemsetD32((hipDeviceptr_t)a.d, (int)FILL, a.entries * 32));
            CK(hipDeviceSynchronize());
            CK((tree_enqueue<C>(p, d_bk, d_s, d_m, d_mt, d_fin, st[0], st[1])));
            CK(hipDeviceSynchronize());
            for (auto& a : areas) {
                host.resize(a.entries * 32);
                CK(hipMemcpy(host.data(), a.d, a.entries * sizeof(XYZZ<M>), hipMemcpyDeviceToHost));
                if (fwrite(host.data(), 4, host.size(), fp) != host.size()) { fclose(fp); BAD("short write of %s", out_path); }
            }
        }
    }
    if (fclose(fp) != 0) BAD("short write of %s", out_path);
    CK(hipStreamDestroy(st[0])); CK(hipStreamDestroy(st[1]));
    CK(hipFree(d_bk)); CK(hipFree(d_s)); CK(hipFree(d_m)); CK(hipFree(d_mt)); CK(hipFree(d_fin));
    return 0;
}

static bool parse_u32(const char* s, uint32_t* v) {
    if (strcmp(s, "-") == 0) { *v = DEFAULT; return true; }
    char* end = nullptr;
    const unsigned long long x = strtoull(s, &end, 10);
    if (!*s || *end || x >= DEFAULT) return false;
    *v = (uint32_t)x;
    return true;
}

static int plan_dump(int argc, char** argv, bool lazy) {
    // groups of 7 numbers (c W lone parts front2 quad_max_tasks l0); a lone group may stop after lone
    const int n = argc - 3;
    if (n != 3 && (n < 7 || n % 7 != 0)) { fprintf(stderr, "usage: tree_check --plan <curve> <c> <W> <lone> [<parts> <front2> <quad_max_tasks> <l0>] ...\n"); return 2; }
    for (int g = 0; g < n; g += 7) {
        uint32_t v[7] = {0, 0, 0, DEFAULT, DEFAULT, DEFAULT, DEFAULT};
        for (int k = 0; k < 7 && g + k < n; k++)
            if (!parse_u32(argv[3 + g + k], &v[k])) BAD("not a number: %s", argv[3 + g + k]);
        TreePlan plan;
        if (make_plan(plan, v[0], v[1], v[2], options(v[3], v[4], v[5], v[6]), lazy, false)) return 1;
        fputs(tree_plan_text(plan).c_str(), stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(XYZZ<Bn254Fp>) == 128 && sizeof(XYZZ<Secp256k1Fp>) == 128, "the memory form the file formats state");
    const bool plan = argc >= 2 && strcmp(argv[1], "--plan") == 0;
    if (plan ? argc < 6 : argc != 4) {
        fprintf(stderr, "usage: tree_check <bn254|secp256k1> <in> <out>\n       tree_check --plan <bn254|secp256k1> <c> <W> <lone> [overrides]\n");
        return 2;
    }
    const std::string curve = argv[plan ? 2 : 1];
    if (curve != "bn254" && curve != "secp256k1") { fprintf(stderr, "tree_check: unknown curve %s\n", curve.c_str()); return 2; }
    if (plan) return plan_dump(argc, argv, curve == "bn254" ? Bn254G1::F30_LAZY : Secp256k1G::F30_LAZY);
    std::vector<uint32_t> in;
    if (read_file(argv[2], in)) return 1;
    return curve == "bn254" ? run<Bn254G1>(in, argv[3]) : run<Secp256k1G>(in, argv[3]);
}

// Block-by-block driver for the single-launch MSM of porla_amd/csrc/msm_small.hip.h: launches k_small_msm itself, the product's own
// kernel, in the product's launch shapes (blocks x sets, c_flags, bits_hint, the pair's region stride) on scalars and points the caller
// wrote, and returns everything the launch left behind as it lies.  A pure transformer: no reference arithmetic lives here.  Expected
// values are computed by tests/small_vectors.py.
// Built by porla_amd/csrc/Makefile as porla_amd/small_check; run by tests/test_small_block_gpu.py.
//
//   small_check <bn254|secp256k1> <in> <out>
//
// Input (uint32 words, little endian): one or more sections, each a header of 16 words and its payload
//   header  0 magic 0x534d4b31, 1 n, 2 blocks per point set (gridDim.x), 3 sets (1 lone, 2 pair), 4 c_flags (forced window bits in the
//           low byte, 0x100 = never split), 5 bits_hint (0 = the kernel scans), 6 region stride in bytes, 7 first sequence number,
//           8 launches (1 .. 3, one after the other on ONE workspace, sequence number + 1 each), 9 1 = the shape does not fit and the
//           kernel is expected to refuse it, 10 .. 15 zero
//   payload n scalars of 32 bytes (big endian, as the entry points take them), then sets * n points of 64 bytes (x || y big endian).
// Output, once per launch: part (sets * blocks * SMALL_MAX_C entries of 32 words, then SENTINEL_ENTRIES more that nothing owns), the
// 512 + 1 counters, the pinned result regions (sets * stride bytes: header words, window sums, and whatever lies behind them), then
// SENTINEL_ENTRIES * 32 words behind the last region.
// Before the FIRST launch of a section every area is filled with the word 0xA5A5A5A5, the counters with zero and word 0 of each
// region's header with zero (the product clears it before every launch; so does the driver).  Nothing is refilled between the launches
// of one section.
// Every section is validated on the host before the first launch of the file: magic, the counts within the kernel's limits, the
// scalars within bits_hint, the file's length -- and the shape: the host derives it from the scalars' bit length as the kernel does
// (small_cfg) and asks small_fits.  A section whose shape does not fit is run only where word 9 says so: the kernel's own admit is the
// same predicate and leaves without a write.  A file that fails, and any HIP error, ends the run with a message and status 1.
#include "msm_small.hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr uint32_t MAGIC = 0x534d4b31u, HDR = 16, FILL = 0xA5A5A5A5u;
constexpr size_t SENTINEL_ENTRIES = 8, COUNTER_WORDS = 512 + 1;
constexpr size_t MIN_STRIDE = SMALL_HDR_WORDS * 4 + (size_t)33 * SMALL_MAX_C * 128;      // the widest shape: W = 33 windows of c = 8

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "small_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)
#define BAD(...) do { fprintf(stderr, "small_check: " __VA_ARGS__); fprintf(stderr, "\n"); return 1; } while (0)

struct Section {
    uint32_t n, blocks, sets, c_flags, hint, seq, launches, refusal;
    size_t stride, payload_at, payload_words, part_words, pin_words, out_words;
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

// bit length of the OR of n big-endian 32-byte scalars
static int used_bits(const uint8_t* sc, size_t n) {
    uint8_t acc[32] = {0};
    for (size_t i = 0; i < n; i++)
        for (int b = 0; b < 32; b++) acc[b] |= sc[32 * i + b];
    for (int b = 0; b < 32; b++)
        if (acc[b]) { int l = 8; while (!(acc[b] >> (l - 1))) l--; return 8 * (31 - b) + l; }
    return 0;
}

template <class C>
static int parse(const std::vector<uint32_t>& in, std::vector<Section>& secs) {
    size_t at = 0;
    do {
        if (in.size() < at + HDR || in[at] != MAGIC) BAD("not a small_check file (section at word %zu)", at);
        const uint32_t* h = in.data() + at;
        Section s{};
        s.n = h[1]; s.blocks = h[2]; s.sets = h[3]; s.c_flags = h[4]; s.hint = h[5]; s.stride = h[6]; s.seq = h[7]; s.launches = h[8]; s.refusal = h[9];
        for (int k = 10; k < 16; k++) if (h[k]) BAD("header word %d is not zero", k);
        if (s.n < 1 || s.n > SMALL_MAX_N) BAD("n = %u is outside 1 .. %u", s.n, SMALL_MAX_N);
        if (s.blocks < 1 || s.blocks > (uint32_t)SMALL_BLOCKS) BAD("blocks = %u is outside 1 .. %d", s.blocks, SMALL_BLOCKS);
        if (s.sets < 1 || s.sets > 2) BAD("sets = %u", s.sets);
        if ((s.c_flags & ~0x1ffu) || (s.c_flags & 0xffu) > (uint32_t)SMALL_MAX_C) BAD("c_flags = %#x", s.c_flags);
        if (s.hint > 256) BAD("bits_hint = %u", s.hint);
        if (s.stride < MIN_STRIDE || s.stride % 128 || s.stride > ((size_t)1 << 20)) BAD("region stride %zu", s.stride);
        if (s.launches < 1 || s.launches > 3 || s.seq == 0 || s.seq > 0xfffffff0u || s.refusal > 1) BAD("launches %u, sequence %u, refusal %u", s.launches, s.seq, s.refusal);
        s.payload_at = at + HDR;
        s.payload_words = (size_t)s.n * 8 + (size_t)s.sets * s.n * 16;
        if (in.size() < s.payload_at + s.payload_words) BAD("file ends inside a section's payload");
        const int used = used_bits((const uint8_t*)(in.data() + s.payload_at), s.n);
        if (s.hint && used > (int)s.hint) BAD("a scalar of %d bits under bits_hint = %u", used, s.hint);
        const SmallCfg g = small_cfg<C>(s.n, s.hint ? (int)s.hint : used, (int)s.c_flags, (int)s.blocks);
        const bool fits = small_fits(g, (int)s.blocks);
        if (fits == (s.refusal != 0))
            BAD("n = %u on %u blocks: shape c = %d, W = %d, S = %d %s", s.n, s.blocks, g.c, g.W, g.S,
                fits ? "fits, the section expects a refusal" : "does not fit the launch");
        s.part_words = ((size_t)s.sets * s.blocks * SMALL_MAX_C + SENTINEL_ENTRIES) * 32;
        s.pin_words = (size_t)s.sets * s.stride / 4 + SENTINEL_ENTRIES * 32;
        s.out_words = (s.part_words + COUNTER_WORDS + s.pin_words) * s.launches;
        at = s.payload_at + s.payload_words;
        secs.push_back(s);
    } while (at < in.size());
    return 0;
}

template <class C>
static int run(const std::vector<uint32_t>& in, const char* out_path) {
    using M = typename C::Fp;
    std::vector<Section> secs;
    if (parse<C>(in, secs)) return 1;                // ---- nothing below runs unless every section stands
    FILE* fp = fopen(out_path, "wb");
    if (!fp) BAD("cannot write %s", out_path);
    std::vector<uint32_t> host;
    for (const Section& s : secs) {
        const uint32_t* pay = in.data() + s.payload_at;
        const size_t n = s.n;
        uint8_t *d_sc = nullptr, *d_pts = nullptr;
        uint32_t *d_part = nullptr, *d_cnt = nullptr, *h_pin = nullptr;
        void* pin_dev = nullptr;
        CK(hipMalloc((void**)&d_sc, n * 32));
        CK(hipMalloc((void**)&d_pts, (size_t)s.sets * n * 64));
        CK(hipMalloc((void**)&d_part, s.part_words * 4));
        CK(hipMalloc((void**)&d_cnt, COUNTER_WORDS * 4));
        CK(hipHostMalloc((void**)&h_pin, s.pin_words * 4, hipHostMallocMapped | hipHostMallocCoherent));   // as the workspace's h_windows
        CK(hipHostGetDevicePointer(&pin_dev, h_pin, 0));
        CK(hipMemcpy(d_sc, pay, n * 32, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_pts, pay + n * 8, (size_t)s.sets * n * 64, hipMemcpyHostToDevice));
        CK(hipMemsetD32((hipDeviceptr_t)d_part, (int)FILL, s.part_words));
        CK(hipMemset(d_cnt, 0, COUNTER_WORDS * 4));
        for (size_t k = 0; k < s.pin_words; k++) h_pin[k] = FILL;
        CK(hipDeviceSynchronize());
        for (uint32_t l = 0; l < s.launches; l++) {
            for (uint32_t set = 0; set < s.sets; set++) ((volatile uint32_t*)((uint8_t*)h_pin + set * s.stride))[0] = 0;
            hipLaunchKernelGGL((k_small_msm<C>), dim3(s.blocks, s.sets), dim3(SMALL_THREADS), 0, 0, (const uint8_t*)d_sc, (const uint8_t*)d_pts,
                               (uint32_t)n, (int)(s.c_flags | (s.hint << 16)), (XYZZ<M>*)d_part, d_cnt, (uint32_t*)pin_dev,
                               (XYZZ<M>*)((uint8_t*)pin_dev + SMALL_HDR_WORDS * 4), s.seq + l, s.sets == 2 ? (const uint8_t*)(d_pts + n * 64) : nullptr,
                               (uint32_t)s.stride);
            CK(hipGetLastError());
            CK(hipDeviceSynchronize());
            host.assign(s.part_words + COUNTER_WORDS + s.pin_words, 0);
            CK(hipMemcpy(host.data(), d_part, s.part_words * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(host.data() + s.part_words, d_cnt, COUNTER_WORDS * 4, hipMemcpyDeviceToHost));
            memcpy(host.data() + s.part_words + COUNTER_WORDS, h_pin, s.pin_words * 4);
            if (fwrite(host.data(), 4, host.size(), fp) != host.size()) { fclose(fp); BAD("short write"); }
        }
        CK(hipFree(d_sc)); CK(hipFree(d_pts)); CK(hipFree(d_part)); CK(hipFree(d_cnt)); CK(hipHostFree(h_pin));
    }
    if (fclose(fp) != 0) BAD("short write of %s", out_path);
    return 0;
}

int main(int argc, char** argv) {
    static_assert(sizeof(XYZZ<Bn254Fp>) == 128 && sizeof(XYZZ<Secp256k1Fp>) == 128, "the memory form the file format states");
    static_assert(MIN_STRIDE <= SMALL_PAIR_STRIDE, "the product's stride holds the widest shape");
    if (argc != 4) { fprintf(stderr, "usage: small_check <bn254|secp256k1> <in> <out>\n"); return 2; }
    const std::string curve = argv[1];
    if (curve != "bn254" && curve != "secp256k1") { fprintf(stderr, "small_check: unknown curve %s\n", curve.c_str()); return 2; }
    std::vector<uint32_t> in;
    if (read_file(argv[2], in)) return 1;
    return curve == "bn254" ? run<Bn254G1>(in, argv[3]) : run<Secp256k1G>(in, argv[3]);
}

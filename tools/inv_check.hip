// Driver for the division-step inversion of porla_amd/csrc/inv30.hip.h: runs the product's OWN f30_inv_safegcd_raw / fe_inv_safegcd, one
// lane per record, in the block sizes and with the two ways of treating a lane without work that the product's callers have, and writes
// back what the functions returned.  A pure transformer: no reference arithmetic lives here and the loop is not copied.  Expected
// values are computed by tests/inv_vectors.py from Python integers.
// Built by porla_amd/csrc/Makefile as porla_amd/inv_check; run by tests/test_inv_gpu.py.
//
//   inv_check <modulus> <op> <block> <policy> <in> <out> [<op> <block> <policy> <in> <out> ...]
//       modulus: bn254_fp | secp256k1_fp | icc_bn254_fr | icc_secp256k1_fn
//       op:      raw   O[0, 9) = the nine limbs of f30_inv_safegcd_raw<M>(V) exactly as returned          (all four moduli)
//                fe    O[0, 8) = the eight words of fe_inv_safegcd<M>(V)                                   (the two base fields: only they
//                                                                                                           have an INV_OUT_30)
//       block:   64 | 256 -- the two block sizes the product calls the inversion with
//       policy:  leave   a lane whose record is not active returns before the call (fixed_base.hip.h:k_fb_normalize after its bounds
//                        check, mac_fft.hip.h:store_affine_be with the infinity lanes gone)
//                stay    such a lane runs the call on the value 1 and skips the store (icc_mac_decode.hip.h:k_imd_row_scalars,
//                        icc_decode.hip.h:k_icd_twiddles_qinv)
//
// A file is records of REC = 24 words (uint32, little endian); record i belongs to lane i of ONE launch of records / block blocks, so
// the record count is a whole number of blocks.  The output file holds the same records after the launch:
//   [ 0,  8)  V, any 256-bit value that is not 0 modulo the modulus (the functions' contract; the test's business)
//   [ 8]      flags: bit 0 = active
//   [ 9, 12)  not read
//   [12, 24)  O: filled with 0xA5A5A5A5 by this program before the launch, whatever the file held; an active lane writes its result
#include "inv30.hip.h"
#include "icc.hip.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr int REC = 24, V0 = 0, FLAGS = 8, O0 = 12, F_ACTIVE = 1;
constexpr uint32_t SENTINEL = 0xA5A5A5A5u;
constexpr size_t MAX_RECORDS = 1u << 20;
enum Op { OP_RAW, OP_FE };

template <class M> struct HasFeForm { static constexpr bool value = false; };
template <> struct HasFeForm<Bn254Fp> { static constexpr bool value = true; };
template <> struct HasFeForm<Secp256k1Fp> { static constexpr bool value = true; };

template <class M, int OP>
__device__ __forceinline__ void invert_and_store(const Fe<M>& v, uint32_t* O, bool store) {
    if constexpr (OP == OP_RAW) {
        const F30<M> r = f30_inv_safegcd_raw<M>(v);
        if (store) for (int k = 0; k < 9; k++) O[k] = r.v[k];
    } else {
        const Fe<M> r = fe_inv_safegcd<M>(v);
        if (store) for (int k = 0; k < 8; k++) O[k] = r.v[k];
    }
}

template <class M, int OP, bool STAY>
__global__ void __launch_bounds__(256) k_inv(uint32_t* io, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;                                            // (never taken: n is a whole number of blocks)
    uint32_t* rec = io + (size_t)i * REC;
    const bool active = (rec[FLAGS] & F_ACTIVE) != 0;
    Fe<M> v;
    if constexpr (STAY) {
        for (int k = 0; k < 8; k++) v.v[k] = active ? rec[V0 + k] : (k == 0 ? 1u : 0u);
        invert_and_store<M, OP>(v, rec + O0, active);
    } else {
        if (!active) return;
        for (int k = 0; k < 8; k++) v.v[k] = rec[V0 + k];
        invert_and_store<M, OP>(v, rec + O0, true);
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "inv_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

static int read_file(const char* path, std::vector<uint32_t>& v) {
    FILE* fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "inv_check: cannot read %s\n", path); return 1; }
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (sz < 0 || sz % 4 != 0) { fprintf(stderr, "inv_check: %s is not a whole number of words\n", path); fclose(fp); return 1; }
    v.resize((size_t)sz / 4);
    const size_t got = v.empty() ? 0 : fread(v.data(), 4, v.size(), fp);
    fclose(fp);
    if (got != v.size()) { fprintf(stderr, "inv_check: short read of %s\n", path); return 1; }
    return 0;
}
static int write_file(const char* path, const uint32_t* v, size_t words) {
    FILE* fp = fopen(path, "wb");
    if (!fp) { fprintf(stderr, "inv_check: cannot write %s\n", path); return 1; }
    const size_t put = words ? fwrite(v, 4, words, fp) : 0;
    if (fclose(fp) != 0 || put != words) { fprintf(stderr, "inv_check: short write of %s\n", path); return 1; }
    return 0;
}
static int refuse(const char* why) { fprintf(stderr, "inv_check: refused: %s\n", why); return 2; }

template <class M, int OP>
static int launch(std::vector<uint32_t>& io, uint32_t n, int block, bool stay) {
    uint32_t* d_io = nullptr;
    const size_t bytes = io.size() * 4;
    CK(hipMalloc(&d_io, bytes));
    CK(hipMemcpy(d_io, io.data(), bytes, hipMemcpyHostToDevice));
    const dim3 grid(n / (uint32_t)block), blk((uint32_t)block);
    if (stay) hipLaunchKernelGGL((k_inv<M, OP, true>), grid, blk, 0, 0, d_io, n);
    else hipLaunchKernelGGL((k_inv<M, OP, false>), grid, blk, 0, 0, d_io, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(io.data(), d_io, bytes, hipMemcpyDeviceToHost));
    CK(hipFree(d_io));
    return 0;
}

template <class M>
static int run(int op, int block, bool stay, const char* in, const char* out) {
    std::vector<uint32_t> io;
    if (read_file(in, io)) return 1;
    if (io.size() % REC != 0) return refuse("not a whole number of 24-word records");
    const size_t n = io.size() / REC;
    if (n > MAX_RECORDS) return refuse("more than 2^20 records");
    if (n % (size_t)block != 0) return refuse("the records must fill whole blocks: record i is lane i of the launch");
    for (size_t i = 0; i < n; i++)
        for (int k = O0; k < REC; k++) io[i * REC + k] = SENTINEL;
    if (n != 0) {
        int rc;
        if (op == OP_RAW) rc = launch<M, OP_RAW>(io, (uint32_t)n, block, stay);
        else if constexpr (HasFeForm<M>::value) rc = launch<M, OP_FE>(io, (uint32_t)n, block, stay);
        else rc = refuse("fe exists for bn254_fp and secp256k1_fp only (no INV_OUT_30 elsewhere)");
        if (rc) return rc;
    }
    return write_file(out, io.data(), io.size());
}

static int usage() {
    fprintf(stderr, "usage: inv_check <bn254_fp|secp256k1_fp|icc_bn254_fr|icc_secp256k1_fn> <raw|fe> <64|256> <leave|stay> <in> <out> "
                    "[<op> <block> <policy> <in> <out> ...]\n");
    return 2;
}

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 2) % 5 != 0) return usage();
    const std::string mod = argv[1];
    int m = -1;
    const char* const names[4] = {"bn254_fp", "secp256k1_fp", "icc_bn254_fr", "icc_secp256k1_fn"};
    for (int i = 0; i < 4; i++) if (mod == names[i]) m = i;
    if (m < 0) { fprintf(stderr, "inv_check: unknown modulus %s\n", mod.c_str()); return usage(); }
    for (int at = 2; at + 4 < argc; at += 5) {
        const std::string op = argv[at], block = argv[at + 1], policy = argv[at + 2];
        if (op != "raw" && op != "fe") { fprintf(stderr, "inv_check: unknown operation %s\n", op.c_str()); return usage(); }
        if (block != "64" && block != "256") { fprintf(stderr, "inv_check: block size %s is neither 64 nor 256\n", block.c_str()); return usage(); }
        if (policy != "leave" && policy != "stay") { fprintf(stderr, "inv_check: unknown lane policy %s\n", policy.c_str()); return usage(); }
        const int o = op == "raw" ? OP_RAW : OP_FE, b = block == "64" ? 64 : 256;
        const bool stay = policy == "stay";
        const char *in = argv[at + 3], *out = argv[at + 4];
        const int rc = m == 0 ? run<Bn254Fp>(o, b, stay, in, out) : m == 1 ? run<Secp256k1Fp>(o, b, stay, in, out)
                     : m == 2 ? run<IccBn254Fr>(o, b, stay, in, out) : run<IccSecp256k1Fn>(o, b, stay, in, out);
        if (rc) return rc;
    }
    return 0;
}

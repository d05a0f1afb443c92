// Per-operation driver for the group law of porla_amd/csrc/ec30.hip.h (9 x 30-bit limbs) and ec.hip.h (8 x 32-bit words):
// reads a file of records, applies ONE named operation of the product's own headers to every record on the device and writes
// the records back.  A pure transformer: no reference arithmetic lives here, nothing is normalised on the way in or out --
// operands are raw limbs / words exactly as the test chose them (unreduced values included), results are raw limbs / words
// plus the returned bool, the `inf` flag and `flip`.  Expected values are computed by tests/ec_vectors.py from Python integers.
// Built by porla_amd/csrc/Makefile as porla_amd/ec30_check; run by tests/test_ec30_gpu.py and tests/test_ec_host_cpu.py.
//
//   ec30_check [--host] <curve> <op> <in> <out> [<op> <in> <out> ...]        curve: bn254 | secp256k1
//   --host: the PORLA_HD forms of ec.hip.h on the CPU, with no HIP call at all
//
// A record is REC = 192 words (uint32, little endian); the output file holds the same records after the operation:
//   [  0,  16)  flags in : 0 inf, 1 flip, 2 neg, 3 phi, 4 a_is_inf, 5 final, 6 live, 7 times, 8 alias (out = first operand),
//                          9 inf of the second operand, 10 separate X table (qx), 11 / 12 scalar bits of the ladder
//   [ 16,  96)  A: operands (F30 residues of 9 limbs at A + 9 i; memory-form points of 32 words at A, A + 32 or A + 40)
//   [ 96, 112)  flags out: 0 returned bool, 1 inf, 2 flip
//   [112, 192)  O: results
// Memory-form operations work in place on the record (every point sits at a multiple of 16 bytes), so the test sees what was
// written AND what was left alone.  One thread per record; the quad forms take one record per quad, 16 records per wave in file
// order, all four lanes calling.  Addresses and trip counts depend on the record index and the capped `times` field only.
#include "ec30.hip.h"
#include "glv.hip.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr int REC = 192, FI = 0, A0 = 16, FO = 96, O0 = 112, MAX_TIMES = 64;
enum Flag { F_INF = 0, F_FLIP, F_NEG, F_PHI, F_AINF, F_FINAL, F_LIVE, F_TIMES, F_ALIAS, F_INF2, F_SEPX, F_BITS0, F_BITS1 };

enum Op {
    OP_SUB2, OP_SUB3, OP_SUB4, OP_SUB5, OP_SUB6, OP_SUB_TWICE3, OP_ADD2, OP_SMALL_MUL2, OP_SMALL_MUL3, OP_RIPPLE, OP_IS_ZERO,
    OP_TO_FE, OP_PM_REDUCE, OP_UNPACK, OP_PACK, OP_CONST,
    OP_DOUBLE_AFFINE, OP_MADD_FLIP, OP_MADD_FLIP_FAST, OP_MMADD_FLIP_FAST, OP_FLIP_FINISH, OP_DOUBLE, OP_ADD, OP_TO_XYZZ,
    OP_STORE_LOAD, OP_ADD_MEM, OP_DOUBLE_MEM, OP_ADD_ONE_LANE,
    OP_ADD_QUAD, OP_DBL_QUAD, OP_DBL_QUADREG, OP_ADD_QUADREG, OP_QUADREG_LADDER,
    OP_MADD32, OP_MADD32_CALL, OP_ADD32, OP_ADD32_CALL, OP_DOUBLE32, OP_DOUBLE32_CALL, OP_DOUBLE_AFFINE32, OP_DOUBLE_AFFINE32_CALL,
    OP_COUNT
};
static const char* const OP_NAMES[OP_COUNT] = {
    "f30_sub2", "f30_sub3", "f30_sub4", "f30_sub5", "f30_sub6", "f30_sub_twice3", "f30_add2", "f30_small_mul2", "f30_small_mul3",
    "f30_ripple", "f30_product_is_zero", "f30_to_fe_canonical", "f30_pm_reduce", "f30_unpack", "f30_pack", "f30_const",
    "xyzz30_double_affine", "xyzz30_madd_flip", "xyzz30_madd_flip_fast", "xyzz30_mmadd_flip_fast", "xyzz30_flip_finish",
    "xyzz30_double", "xyzz30_add", "xyzz30_to_xyzz",
    "xyzz30_store_load_lazy", "xyzz30_add_mem", "xyzz30_double_mem", "xyzz30_add_one_lane",
    "xyzz30_add_quad", "xyzz30_dbl_quad", "xyzz30_dbl_quadreg", "xyzz30_add_quadreg", "xyzz30_quadreg_ladder",
    "xyzz_madd", "xyzz_madd_call", "xyzz_add", "xyzz_add_call", "xyzz_double", "xyzz_double_call", "xyzz_double_affine",
    "xyzz_double_affine_call"};
constexpr bool op_is_quad(int op) { return op >= OP_ADD_QUAD && op <= OP_QUADREG_LADDER; }
constexpr bool op_is_32(int op) { return op >= OP_MADD32; }

template <class M>
__device__ __forceinline__ F30<M> ld30(const uint32_t* s) {
    F30<M> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = s[i];
    return r;
}
template <class M>
__device__ __forceinline__ void st30(uint32_t* d, const F30<M>& a) {
#pragma unroll
    for (int i = 0; i < 9; i++) d[i] = a.v[i];
}
template <class M>
__device__ __forceinline__ XYZZ30<M> ldp30(const uint32_t* s, uint32_t inf) {
    XYZZ30<M> p;
    p.x = ld30<M>(s); p.y = ld30<M>(s + 9); p.zz = ld30<M>(s + 18); p.zzz = ld30<M>(s + 27);
    p.inf = inf != 0;
    return p;
}
template <class M>
__device__ __forceinline__ void stp30(uint32_t* rec, const XYZZ30<M>& p) {
    st30<M>(rec + O0, p.x); st30<M>(rec + O0 + 9, p.y); st30<M>(rec + O0 + 18, p.zz); st30<M>(rec + O0 + 27, p.zzz);
    rec[FO + 1] = p.inf ? 1u : 0u;
}
template <class M>
PORLA_HD XYZZ<M> ldp32(const uint32_t* s) {
    XYZZ<M> p;
    for (int i = 0; i < 8; i++) { p.x.v[i] = s[i]; p.y.v[i] = s[8 + i]; p.zz.v[i] = s[16 + i]; p.zzz.v[i] = s[24 + i]; }
    return p;
}
template <class M>
PORLA_HD void stp32(uint32_t* d, const XYZZ<M>& p) {
    for (int i = 0; i < 8; i++) { d[i] = p.x.v[i]; d[8 + i] = p.y.v[i]; d[16 + i] = p.zz.v[i]; d[24 + i] = p.zzz.v[i]; }
}

// the 8 x 32-bit forms of ec.hip.h: one body for the device kernel and for --host
template <class M, int OP>
PORLA_HD void run32(uint32_t* rec) {
    constexpr bool CALL = ((OP - OP_MADD32) & 1) != 0;
    XYZZ<M> p = ldp32<M>(rec + A0);
    Affine<M> a;
    for (int i = 0; i < 8; i++) { a.x.v[i] = rec[A0 + 32 + i]; a.y.v[i] = rec[A0 + 40 + i]; }
    if constexpr (OP == OP_MADD32 || OP == OP_MADD32_CALL) xyzz_madd<M, CALL>(p, a);
    else if constexpr (OP == OP_ADD32 || OP == OP_ADD32_CALL) { const XYZZ<M> q = ldp32<M>(rec + A0 + 32); xyzz_add<M, CALL>(p, q); }
    else if constexpr (OP == OP_DOUBLE32 || OP == OP_DOUBLE32_CALL) p = xyzz_double<M, CALL>(p);
    else p = xyzz_double_affine<M, CALL>(a);
    stp32<M>(rec + O0, p);
    rec[FO + 1] = xyzz_is_inf<M>(p) ? 1u : 0u;
}

template <class M, int OP>
__global__ void k_lane(uint32_t* io, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* rec = io + (size_t)i * REC;
    const uint32_t* f = rec + FI;
    uint32_t* A = rec + A0;
    uint32_t* O = rec + O0;
    if constexpr (op_is_32(OP)) { run32<M, OP>(rec); return; }
    else if constexpr (OP <= OP_SMALL_MUL3) {
        const F30<M> a = ld30<M>(A), b = ld30<M>(A + 9);
        F30<M> r;
        if constexpr (OP == OP_SUB2) r = f30_sub<M, 2>(a, b);
        else if constexpr (OP == OP_SUB3) r = f30_sub<M, 3>(a, b);
        else if constexpr (OP == OP_SUB4) r = f30_sub<M, 4>(a, b);
        else if constexpr (OP == OP_SUB5) r = f30_sub<M, 5>(a, b);
        else if constexpr (OP == OP_SUB6) r = f30_sub<M, 6>(a, b);
        else if constexpr (OP == OP_SUB_TWICE3) r = f30_sub_twice<M, 3>(a, b);
        else if constexpr (OP == OP_ADD2) r = f30_add2<M>(a, b);
        else if constexpr (OP == OP_SMALL_MUL2) r = f30_small_mul<M, 2>(a);
        else r = f30_small_mul<M, 3>(a);
        st30<M>(O, r);
    } else if constexpr (OP == OP_RIPPLE) {
        F30<M> a = ld30<M>(A);
        f30_ripple<M>(a);
        st30<M>(O, a);
    } else if constexpr (OP == OP_IS_ZERO) {
        rec[FO] = f30_product_is_zero<M>(ld30<M>(A)) ? 1u : 0u;
    } else if constexpr (OP == OP_TO_FE) {
        const Fe<M> t = f30_to_fe_canonical<M>(ld30<M>(A));
        for (int k = 0; k < 8; k++) O[k] = t.v[k];
    } else if constexpr (OP == OP_PM_REDUCE) {
        st30<M>(O, f30_pm_reduce<M>(ld30<M>(A)));
    } else if constexpr (OP == OP_UNPACK) {
        uint32_t w[8];
        for (int k = 0; k < 8; k++) w[k] = A[k];
        st30<M>(O, f30_unpack<M>(w));
    } else if constexpr (OP == OP_PACK) {
        uint32_t w[8];
        f30_pack<M>(w, ld30<M>(A));
        for (int k = 0; k < 8; k++) O[k] = w[k];
    } else if constexpr (OP == OP_CONST) {
        uint32_t w[8];
        for (int k = 0; k < 8; k++) w[k] = A[k];
        st30<M>(O, f30_const<M>(w));
    } else if constexpr (OP == OP_DOUBLE_AFFINE) {
        stp30<M>(rec, xyzz30_double_affine<M>(ld30<M>(A + 36), ld30<M>(A + 45)));
    } else if constexpr (OP == OP_MADD_FLIP || OP == OP_MADD_FLIP_FAST || OP == OP_MMADD_FLIP_FAST) {
        XYZZ30<M> p = ldp30<M>(A, f[F_INF]);
        bool flip = f[F_FLIP] != 0, ret = true;
        const F30<M> ax = ld30<M>(A + 36), ay = ld30<M>(A + 45);
        if constexpr (OP == OP_MADD_FLIP) xyzz30_madd_flip<M>(p, flip, ax, ay);
        else if constexpr (OP == OP_MADD_FLIP_FAST) ret = xyzz30_madd_flip_fast<M>(p, flip, ax, ay, f[F_AINF] != 0);
        else ret = xyzz30_mmadd_flip_fast<M>(p, flip, ax, ay, f[F_AINF] != 0);
        stp30<M>(rec, p);
        rec[FO] = ret ? 1u : 0u;
        rec[FO + 2] = flip ? 1u : 0u;
    } else if constexpr (OP == OP_FLIP_FINISH) {
        XYZZ30<M> p = ldp30<M>(A, f[F_INF]);
        xyzz30_flip_finish<M>(p, f[F_FLIP] != 0);
        stp30<M>(rec, p);
    } else if constexpr (OP == OP_DOUBLE) {
        stp30<M>(rec, xyzz30_double<M>(ld30<M>(A), ld30<M>(A + 9), ld30<M>(A + 18), ld30<M>(A + 27)));
    } else if constexpr (OP == OP_ADD) {
        XYZZ30<M> p = ldp30<M>(A, f[F_INF]);
        const XYZZ30<M> q = ldp30<M>(A + 36, f[F_INF2]);
        xyzz30_add<M>(p, q);
        stp30<M>(rec, p);
    } else if constexpr (OP == OP_TO_XYZZ) {
        stp32<M>(O, xyzz30_to_xyzz<M>(ldp30<M>(A, f[F_INF])));
    } else if constexpr (OP == OP_STORE_LOAD) {
        XYZZ<M>* mem = reinterpret_cast<XYZZ<M>*>(O);
        xyzz30_store_lazy<M>(mem, ldp30<M>(A, f[F_INF]));
        const XYZZ30<M> b = xyzz30_load_lazy<M>(mem);
        st30<M>(O + 32, b.x); st30<M>(O + 41, b.y); st30<M>(O + 50, b.zz); st30<M>(O + 59, b.zzz);
        rec[FO + 1] = b.inf ? 1u : 0u;
    } else if constexpr (OP == OP_ADD_MEM) {
        F30<M> beta30;                                            // as mac_fft.hip.h builds it: the constant of glv.hip.h
        if constexpr (M::PSEUDO_MERSENNE) beta30 = f30_const<M>(GlvSecp256k1::BETA_30);
        else beta30 = f30_const<M>(GlvBn254::BETA_30);
        xyzz30_add_mem<M>(reinterpret_cast<XYZZ<M>*>(A), reinterpret_cast<const XYZZ<M>*>(A + 32), f[F_NEG], f[F_PHI], &beta30);
    } else if constexpr (OP == OP_DOUBLE_MEM) {
        const uint32_t times = f[F_TIMES] < (uint32_t)MAX_TIMES ? f[F_TIMES] : (uint32_t)MAX_TIMES;
        xyzz30_double_mem<M>(reinterpret_cast<XYZZ<M>*>(A), (int)times);
    } else if constexpr (OP == OP_ADD_ONE_LANE) {
        xyzz30_add_one_lane<M>(reinterpret_cast<const XYZZ<M>*>(A), reinterpret_cast<const XYZZ<M>*>(A + 32),
                               reinterpret_cast<XYZZ<M>*>(O), f[F_FINAL] != 0);
    }
}

// one record per quad, 16 per wave (blocks of one wave); n is a multiple of 16 (the host pads with all-zero records: live = 0)
template <class M, int OP>
__global__ void __launch_bounds__(64) k_quad(uint32_t* io, int n) {
    const int rec_i = blockIdx.x * 16 + (int)(threadIdx.x >> 2);
    if (rec_i >= n) return;                                       // never taken: whole waves only
    const uint32_t lane = threadIdx.x & 63u, r = lane & 3u;
    uint32_t* rec = io + (size_t)rec_i * REC;
    const uint32_t* f = rec + FI;
    uint32_t* A = rec + A0;
    uint32_t* O = rec + O0;
    if constexpr (OP == OP_ADD_QUAD) {
        const XYZZ<M>* pa = reinterpret_cast<const XYZZ<M>*>(A);
        XYZZ<M>* out = f[F_ALIAS] ? reinterpret_cast<XYZZ<M>*>(A) : reinterpret_cast<XYZZ<M>*>(O);
        xyzz30_add_quad<M>(pa, reinterpret_cast<const XYZZ<M>*>(A + 32), out, f[F_FINAL] != 0, f[F_LIVE] != 0, lane);
    } else if constexpr (OP == OP_DBL_QUAD) {
        XYZZ<M>* out = f[F_ALIAS] ? reinterpret_cast<XYZZ<M>*>(A) : reinterpret_cast<XYZZ<M>*>(O);
        xyzz30_dbl_quad<M>(reinterpret_cast<const XYZZ<M>*>(A), out, f[F_LIVE] != 0, lane);
    } else if constexpr (OP == OP_DBL_QUADREG) {
        F30<M> c = ld30<M>(A + 9 * r);
        xyzz30_dbl_quadreg<M>(c, r);
        st30<M>(O + 9 * r, c);
    } else {
        F30<M> c = ld30<M>(A + 9 * r);
        const XYZZ<M>* q = reinterpret_cast<const XYZZ<M>*>(A + 40);
        const uint32_t* qx = f[F_SEPX] ? A + 72 : A + 40;
        const bool neg = f[F_NEG] != 0;
        bool ok = true;
        if constexpr (OP == OP_ADD_QUADREG) {
            ok = xyzz30_add_quadreg<M>(c, q, qx, neg, r, lane);
        } else {
            // c = k c0 for the `times` low bits of k below its leading 1 (double, add q where the bit is set), as the ladders of
            // quad30.hip.h chain the two forms; a step that meets equal x is reported, not repaired
            const uint32_t times = f[F_TIMES] < (uint32_t)MAX_TIMES ? f[F_TIMES] : (uint32_t)MAX_TIMES;
#pragma unroll 1
            for (int b = (int)times - 1; b >= 0; b--) {
                xyzz30_dbl_quadreg<M>(c, r);
                const uint32_t bit = (f[b < 32 ? F_BITS0 : F_BITS1] >> (b & 31)) & 1u;
                if (bit && !xyzz30_add_quadreg<M>(c, q, qx, neg, r, lane)) ok = false;
            }
        }
        st30<M>(O + 9 * r, c);
        if (r == 0u) rec[FO] = ok ? 1u : 0u;
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "ec30_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

template <class M, int OP>
static int launch(uint32_t* d_io, int n) {
    if constexpr (OP == OP_PM_REDUCE && !M::PSEUDO_MERSENNE) {
        fprintf(stderr, "ec30_check: f30_pm_reduce belongs to the special-form modulus (secp256k1)\n");
        return 1;
    } else {
        if constexpr (op_is_quad(OP)) hipLaunchKernelGGL((k_quad<M, OP>), dim3(n / 16), dim3(64), 0, 0, d_io, n);
        else hipLaunchKernelGGL((k_lane<M, OP>), dim3((n + 63) / 64), dim3(64), 0, 0, d_io, n);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        return 0;
    }
}
template <class M, int OP = 0>
static int dispatch(int op, uint32_t* d_io, int n) {
    if constexpr (OP < OP_COUNT) {
        if (op == OP) return launch<M, OP>(d_io, n);
        return dispatch<M, OP + 1>(op, d_io, n);
    } else {
        return 1;
    }
}
template <class M, int OP = OP_MADD32>
static int dispatch_host(int op, uint32_t* io, int n) {
    if constexpr (OP < OP_COUNT) {
        if (op == OP) {
            for (int i = 0; i < n; i++) run32<M, OP>(io + (size_t)i * REC);
            return 0;
        }
        return dispatch_host<M, OP + 1>(op, io, n);
    } else {
        return 1;
    }
}

static int read_file(const char* path, std::vector<uint32_t>& v) {
    FILE* fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "ec30_check: cannot read %s\n", path); return 1; }
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (sz < 0 || sz % (REC * 4) != 0) { fprintf(stderr, "ec30_check: %s is not a whole number of %d-word records\n", path, REC); fclose(fp); return 1; }
    v.resize((size_t)sz / 4);
    const size_t got = v.empty() ? 0 : fread(v.data(), 4, v.size(), fp);
    fclose(fp);
    if (got != v.size()) { fprintf(stderr, "ec30_check: short read of %s\n", path); return 1; }
    return 0;
}
static int write_file(const char* path, const uint32_t* v, size_t words) {
    FILE* fp = fopen(path, "wb");
    if (!fp) { fprintf(stderr, "ec30_check: cannot write %s\n", path); return 1; }
    const size_t put = words ? fwrite(v, 4, words, fp) : 0;
    if (fclose(fp) != 0 || put != words) { fprintf(stderr, "ec30_check: short write of %s\n", path); return 1; }
    return 0;
}

template <class M>
static int run(bool host, int op, const char* in, const char* out) {
    std::vector<uint32_t> io;
    if (read_file(in, io)) return 1;
    const int n = (int)(io.size() / REC);
    if (host) {
        if (!op_is_32(op)) { fprintf(stderr, "ec30_check: --host runs the ec.hip.h forms only\n"); return 1; }
        if (dispatch_host<M>(op, io.data(), n)) return 1;
        return write_file(out, io.data(), (size_t)n * REC);
    }
    const int np = op_is_quad(op) ? (n + 15) / 16 * 16 : n;      // whole waves of quads: all-zero records (live = 0) behind the last
    io.resize((size_t)np * REC, 0u);
    if (np > 0) {
        uint32_t* d_io = nullptr;
        const size_t bytes = (size_t)np * REC * 4;
        CK(hipMalloc(&d_io, bytes));
        CK(hipMemcpy(d_io, io.data(), bytes, hipMemcpyHostToDevice));
        if (dispatch<M>(op, d_io, np)) return 1;
        CK(hipMemcpy(io.data(), d_io, bytes, hipMemcpyDeviceToHost));
        CK(hipFree(d_io));
    }
    return write_file(out, io.data(), (size_t)n * REC);
}

int main(int argc, char** argv) {
    int at = 1;
    bool host = false;
    if (at < argc && !strcmp(argv[at], "--host")) { host = true; at++; }
    if (argc - at < 4 || (argc - at - 1) % 3 != 0) {
        fprintf(stderr, "usage: ec30_check [--host] <bn254|secp256k1> <op> <in> <out> [<op> <in> <out> ...]\nops:");
        for (int i = 0; i < OP_COUNT; i++) fprintf(stderr, " %s", OP_NAMES[i]);
        fprintf(stderr, "\n");
        return 2;
    }
    const std::string curve = argv[at++];
    if (curve != "bn254" && curve != "secp256k1") { fprintf(stderr, "ec30_check: unknown curve %s\n", curve.c_str()); return 2; }
    for (; at + 2 < argc; at += 3) {
        int op = -1;
        for (int i = 0; i < OP_COUNT; i++) if (!strcmp(argv[at], OP_NAMES[i])) op = i;
        if (op < 0) { fprintf(stderr, "ec30_check: unknown operation %s\n", argv[at]); return 2; }
        const int rc = curve == "bn254" ? run<Bn254Fp>(host, op, argv[at + 1], argv[at + 2]) : run<Secp256k1Fp>(host, op, argv[at + 1], argv[at + 2]);
        if (rc) return rc;
    }
    return 0;
}

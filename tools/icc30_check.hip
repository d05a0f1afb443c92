// Per-operation driver for the reduced-radix field layer of the ICC encode, porla_amd/csrc/icc30.hip.h and icc30_split.hip.h:
// reads a file of records, applies ONE named helper of the product's own headers to every record on the device and writes the
// records back.  A pure transformer: no reference arithmetic lives here, nothing is normalised on the way in or out -- operands
// are raw limbs / words exactly as the test chose them (unreduced values at the stated operand bounds included), results are raw
// limbs / words.  Expected values are computed by tests/icc_vectors.py from Python integers.
// Built by porla_amd/csrc/Makefile as porla_amd/icc30_check; run by tests/test_icc30_gpu.py.
//
//   icc30_check <modulus> <op> <in> <out> [<op> <in> <out> ...]        modulus: p_icc | bn254_r | secp256k1_n
//
// The single-plane helpers run on the named modulus.  The helpers that hold BOTH residues of a symbol (finish step, symbol load,
// icc30_from_elem, the mix, the 80-byte slot) take the named modulus as q and p_icc as the other plane; they do not exist for p_icc,
// and icc30_finish_p exists for p_icc only.
//
// A record is REC = 192 words (uint32, little endian); the output file holds the same records after the operation:
//   [  0,  16)  flags in : 0 times (icc30_chain; capped at MAX_TIMES), 1 scaled (icc30_chain: the K = 2 / K = 4 first round),
//                          2 feed (icc30_chain: 0 keeps (upper, lower) outputs in place, 1 swaps them between stages),
//                          3 outputs of the finish step (bit 0 x, 1 al, 2 sc, 3 qres), 4 scalar_le
//   [ 16,  96)  A: operands.  F30 residues of 9 limbs at A + 9 i; 64-byte symbols / IccElem of 16 words at A + 16 i; the twiddle
//               slot of the mix (20 words) at A + 32
//   [ 96, 112)  flags out (unused: stays as the test wrote it)
//   [112, 192)  O: results, as listed per operation below.  What an operation does not write stays as the test wrote it.
//
//   icc30_mul            O = a b;                 O + 18 = f30_mul_portable(a, b) in every product shape
//   icc30_mul_alias_x    x = icc30_mul(x, y):     O = x, O + 9 = y
//   icc30_mul_alias_y    y = icc30_mul(x, y):     O = x, O + 9 = y
//   icc30_mul_sqr        x = icc30_mul(x, x):     O = x
//   icc30_add, icc30_sub2                         O = a + b, a - b + 2 p
//   icc30_bfly (a, b, w at A, A + 9, A + 18)      O = a', O + 9 = b'
//   icc30_bfly_plain2|3|4|7 (a, b)                O = a', O + 9 = b'
//   icc30_reduce_top                              O = 9 limbs
//   icc30_canonical, icc30_finish_p               O = 8 words
//   icc30_finish_elem (e.p at A, e.q at A + 9)    x: O[0, 16), al: O[16, 24), sc: O[24, 32), qres: O[32, 40)
//   icc30_finish_q (P: 8 words at A + 18)         the same places
//   icc30_load_symbol (16 words at A)             O = e.p, O + 9 = e.q
//   icc30_from_elem (IccElem: 16 words at A)      O = e.p, O + 9 = e.q
//   icc30_mix_elem (a0 at A, a1 at A + 16, twiddle slot at A + 32; len = ncols = 1)    O[0, 16) = out[0], O[16, 32) = out[1]
//   icc30_slot   (e.p, e.q at A, A + 9)           st_slot at O[0, 20); ld_slot of it -> O + 32, O + 41
//   icc30_pslot  (a at A)                         st_pslot at O[0, 10); ld_pslot of it -> O + 16
//   icc30_work   (a at A)                         st_work at O[1, 10) (4-byte aligned only); ld_work of it -> O + 16
//   icc30_chain  (a0..a3 at A + 9 i, w3 at A + 36, w at A + 45)
//                the first round of icc30_split.hip.h:icc30_round on one radix-4 unit: bfly_plain<7> on (0, 1) and (2, 3), reduce_top of
//                a2 and bfly_plain<3> on (0, 2), icc30_bfly on (1, 3) with w3 (scaled: bfly_plain<2>, <2>, <4>); then times - 2
//                further icc30_bfly stages on (a1, a3) with w.  O + 9 i = a_i.
// One thread per record; addresses and trip counts depend on the record index and the capped `times` field only.
#include "icc30_split.hip.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
using namespace porla;

constexpr int REC = 192, FI = 0, A0 = 16, FO = 96, O0 = 112, MAX_TIMES = 32;
enum Flag { F_TIMES = 0, F_SCALED, F_FEED, F_OUTS, F_SCALAR_LE };

enum Op {
    OP_MUL, OP_MUL_ALIAS_X, OP_MUL_ALIAS_Y, OP_MUL_SQR, OP_ADD, OP_SUB2, OP_BFLY, OP_PLAIN2, OP_PLAIN3, OP_PLAIN4, OP_PLAIN7,
    OP_REDUCE_TOP, OP_CANONICAL, OP_PSLOT, OP_WORK, OP_CHAIN,
    OP_FINISH_P,
    OP_FINISH_ELEM, OP_FINISH_Q, OP_LOAD_SYMBOL, OP_FROM_ELEM, OP_MIX_ELEM, OP_SLOT,
    OP_COUNT
};
static const char* const OP_NAMES[OP_COUNT] = {
    "icc30_mul", "icc30_mul_alias_x", "icc30_mul_alias_y", "icc30_mul_sqr", "icc30_add", "icc30_sub2", "icc30_bfly",
    "icc30_bfly_plain2", "icc30_bfly_plain3", "icc30_bfly_plain4", "icc30_bfly_plain7",
    "icc30_reduce_top", "icc30_canonical", "icc30_pslot", "icc30_work", "icc30_chain",
    "icc30_finish_p",
    "icc30_finish_elem", "icc30_finish_q", "icc30_load_symbol", "icc30_from_elem", "icc30_mix_elem", "icc30_slot"};
constexpr bool op_is_pair(int op) { return op >= OP_FINISH_ELEM; }       // both residues of a symbol: the modulus is q

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

template <class M, int OP>
__global__ void k_lane(uint32_t* io, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* rec = io + (size_t)i * REC;
    const uint32_t* f = rec + FI;
    uint32_t* A = rec + A0;
    uint32_t* O = rec + O0;
    if constexpr (OP == OP_MUL) {
        const F30<M> a = ld30<M>(A), b = ld30<M>(A + 9);
        st30<M>(O, icc30_mul<M>(a, b));
        st30<M>(O + 18, f30_mul_portable<M>(a, b));
    } else if constexpr (OP == OP_MUL_ALIAS_X || OP == OP_MUL_ALIAS_Y || OP == OP_MUL_SQR) {
        F30<M> x = ld30<M>(A), y = ld30<M>(A + 9);
        st30<M>(O + 18, f30_mul_portable<M>(x, OP == OP_MUL_SQR ? x : y));
        if constexpr (OP == OP_MUL_ALIAS_X) x = icc30_mul<M>(x, y);
        else if constexpr (OP == OP_MUL_ALIAS_Y) y = icc30_mul<M>(x, y);
        else x = icc30_mul<M>(x, x);
        st30<M>(O, x);
        st30<M>(O + 9, y);
    } else if constexpr (OP == OP_ADD) {
        st30<M>(O, icc30_add<M>(ld30<M>(A), ld30<M>(A + 9)));
    } else if constexpr (OP == OP_SUB2) {
        st30<M>(O, icc30_sub<M, 2>(ld30<M>(A), ld30<M>(A + 9)));
    } else if constexpr (OP == OP_BFLY) {
        F30<M> a = ld30<M>(A), b = ld30<M>(A + 9);
        icc30_bfly<M>(a, b, ld30<M>(A + 18));
        st30<M>(O, a);
        st30<M>(O + 9, b);
    } else if constexpr (OP >= OP_PLAIN2 && OP <= OP_PLAIN7) {
        F30<M> a = ld30<M>(A), b = ld30<M>(A + 9);
        if constexpr (OP == OP_PLAIN2) icc30_bfly_plain<M, 2>(a, b);
        else if constexpr (OP == OP_PLAIN3) icc30_bfly_plain<M, 3>(a, b);
        else if constexpr (OP == OP_PLAIN4) icc30_bfly_plain<M, 4>(a, b);
        else icc30_bfly_plain<M, 7>(a, b);
        st30<M>(O, a);
        st30<M>(O + 9, b);
    } else if constexpr (OP == OP_REDUCE_TOP) {
        st30<M>(O, icc30_reduce_top<M>(ld30<M>(A)));
    } else if constexpr (OP == OP_CANONICAL) {
        const Fe<M> t = icc30_canonical<M>(ld30<M>(A));
        for (int k = 0; k < 8; k++) O[k] = t.v[k];
    } else if constexpr (OP == OP_PSLOT) {
        icc30_st_pslot<M>(O, ld30<M>(A));
        st30<M>(O + 16, icc30_ld_pslot<M>(O));
    } else if constexpr (OP == OP_WORK) {
        icc30_st_work<M>(O + 1, ld30<M>(A));
        st30<M>(O + 16, icc30_ld_work<M>(O + 1));
    } else if constexpr (OP == OP_CHAIN) {
        F30<M> a[4];
#pragma unroll
        for (int k = 0; k < 4; k++) a[k] = ld30<M>(A + 9 * k);
        const F30<M> w3 = ld30<M>(A + 36), w = ld30<M>(A + 45);
        const uint32_t times = f[F_TIMES] < (uint32_t)MAX_TIMES ? f[F_TIMES] : (uint32_t)MAX_TIMES;
        if (f[F_SCALED]) {
            icc30_bfly_plain<M, 2>(a[0], a[1]); icc30_bfly_plain<M, 2>(a[2], a[3]);
            icc30_bfly_plain<M, 4>(a[0], a[2]);
        } else {
            icc30_bfly_plain<M, 7>(a[0], a[1]); icc30_bfly_plain<M, 7>(a[2], a[3]);
            a[2] = icc30_reduce_top<M>(a[2]);
            icc30_bfly_plain<M, 3>(a[0], a[2]);
        }
        icc30_bfly<M>(a[1], a[3], w3);
#pragma unroll 1
        for (uint32_t s = 2; s < times; s++) {
            if (f[F_FEED]) { const F30<M> t = a[1]; a[1] = a[3]; a[3] = t; }
            icc30_bfly<M>(a[1], a[3], w);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) st30<M>(O + 9 * k, a[k]);
    } else if constexpr (OP == OP_FINISH_P) {
        const Fe<IccFp> t = icc30_finish_p(ld30<IccFp>(A));
        for (int k = 0; k < 8; k++) O[k] = t.v[k];
    } else if constexpr (OP == OP_FINISH_ELEM || OP == OP_FINISH_Q) {
        uint8_t* const out = reinterpret_cast<uint8_t*>(O);
        IccOut o;
        o.x = (f[F_OUTS] & 1u) ? out : nullptr;
        o.al = (f[F_OUTS] & 2u) ? out + 64 : nullptr;
        o.sc = (f[F_OUTS] & 4u) ? out + 96 : nullptr;
        o.qres = (f[F_OUTS] & 8u) ? out + 128 : nullptr;
        o.scalar_le = (int)f[F_SCALAR_LE];
        if constexpr (OP == OP_FINISH_ELEM) {
            IccElem30<M> e;
            e.p = ld30<IccFp>(A); e.q = ld30<M>(A + 9);
            icc30_finish_elem<M>(e, 0, o);
        } else {
            Fe<IccFp> P;
            for (int k = 0; k < 8; k++) P.v[k] = A[18 + k];
            icc30_finish_q<M>(P, ld30<M>(A + 9), 0, o);
        }
    } else if constexpr (OP == OP_LOAD_SYMBOL) {
        const IccElem30<M> e = icc30_load_symbol<M>(reinterpret_cast<const uint8_t*>(A));
        st30<IccFp>(O, e.p);
        st30<M>(O + 9, e.q);
    } else if constexpr (OP == OP_FROM_ELEM) {
        const IccElem30<M> e = icc30_from_elem<M>(ld_elem<M>(reinterpret_cast<const IccElem<M>*>(A)));
        st30<IccFp>(O, e.p);
        st30<M>(O + 9, e.q);
    } else if constexpr (OP == OP_MIX_ELEM) {
        icc30_mix_elem<M>(reinterpret_cast<const uint8_t*>(A), reinterpret_cast<const uint8_t*>(A + 16), 0, 1u, 1u, A + 32, 1u,
                          reinterpret_cast<uint8_t*>(O));
    } else if constexpr (OP == OP_SLOT) {
        IccElem30<M> e;
        e.p = ld30<IccFp>(A); e.q = ld30<M>(A + 9);
        icc30_st_slot<M>(O, e);
        const IccElem30<M> b = icc30_ld_slot<M>(O);
        st30<IccFp>(O + 32, b.p);
        st30<M>(O + 41, b.q);
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "icc30_check: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

template <class M, int OP>
static int launch(uint32_t* d_io, int n) {
    constexpr bool P_PLANE = std::is_same<M, IccFp>::value;
    if constexpr ((op_is_pair(OP) && P_PLANE) || (OP == OP_FINISH_P && !P_PLANE)) {
        fprintf(stderr, "icc30_check: %s does not exist for this modulus\n", OP_NAMES[OP]);
        return 1;
    } else {
        hipLaunchKernelGGL((k_lane<M, OP>), dim3((n + 63) / 64), dim3(64), 0, 0, d_io, n);
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

static int read_file(const char* path, std::vector<uint32_t>& v) {
    FILE* fp = fopen(path, "rb");
    if (!fp) { fprintf(stderr, "icc30_check: cannot read %s\n", path); return 1; }
    fseek(fp, 0, SEEK_END);
    const long sz = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    if (sz < 0 || sz % (REC * 4) != 0) { fprintf(stderr, "icc30_check: %s is not a whole number of %d-word records\n", path, REC); fclose(fp); return 1; }
    v.resize((size_t)sz / 4);
    const size_t got = v.empty() ? 0 : fread(v.data(), 4, v.size(), fp);
    fclose(fp);
    if (got != v.size()) { fprintf(stderr, "icc30_check: short read of %s\n", path); return 1; }
    return 0;
}
static int write_file(const char* path, const uint32_t* v, size_t words) {
    FILE* fp = fopen(path, "wb");
    if (!fp) { fprintf(stderr, "icc30_check: cannot write %s\n", path); return 1; }
    const size_t put = words ? fwrite(v, 4, words, fp) : 0;
    if (fclose(fp) != 0 || put != words) { fprintf(stderr, "icc30_check: short write of %s\n", path); return 1; }
    return 0;
}

template <class M>
static int run(int op, const char* in, const char* out) {
    std::vector<uint32_t> io;
    if (read_file(in, io)) return 1;
    const int n = (int)(io.size() / REC);
    if (n > 0) {
        uint32_t* d_io = nullptr;
        const size_t bytes = (size_t)n * REC * 4;
        CK(hipMalloc(&d_io, bytes));
        CK(hipMemcpy(d_io, io.data(), bytes, hipMemcpyHostToDevice));
        if (dispatch<M>(op, d_io, n)) return 1;
        CK(hipMemcpy(io.data(), d_io, bytes, hipMemcpyDeviceToHost));
        CK(hipFree(d_io));
    }
    return write_file(out, io.data(), (size_t)n * REC);
}

int main(int argc, char** argv) {
    int at = 1;
    if (argc - at < 4 || (argc - at - 1) % 3 != 0) {
        fprintf(stderr, "usage: icc30_check <p_icc|bn254_r|secp256k1_n> <op> <in> <out> [<op> <in> <out> ...]\nops:");
        for (int i = 0; i < OP_COUNT; i++) fprintf(stderr, " %s", OP_NAMES[i]);
        fprintf(stderr, "\n");
        return 2;
    }
    const std::string mod = argv[at++];
    if (mod != "p_icc" && mod != "bn254_r" && mod != "secp256k1_n") { fprintf(stderr, "icc30_check: unknown modulus %s\n", mod.c_str()); return 2; }
    for (; at + 2 < argc; at += 3) {
        int op = -1;
        for (int i = 0; i < OP_COUNT; i++) if (!strcmp(argv[at], OP_NAMES[i])) op = i;
        if (op < 0) { fprintf(stderr, "icc30_check: unknown operation %s\n", argv[at]); return 2; }
        const int rc = mod == "p_icc" ? run<IccFp>(op, argv[at + 1], argv[at + 2])
                     : mod == "bn254_r" ? run<IccBn254Fr>(op, argv[at + 1], argv[at + 2])
                                        : run<IccSecp256k1Fn>(op, argv[at + 1], argv[at + 2]);
        if (rc) return rc;
    }
    return 0;
}

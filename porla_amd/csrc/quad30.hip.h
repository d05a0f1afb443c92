// Quad-lane helpers shared by the kernels whose group operations run on the four lanes of a quad with the accumulator in registers
// (ec30.hip.h: xyzz30_dbl_quadreg / xyzz30_add_quadreg): the MAC-side encode's ladders (mac_fft.hip.h) and the batched MSM's tiny
// entries and window fold (msm_batch.hip.h).  The signed 4-bit recoding of a 128-bit half-scalar, the quad-private LDS ordering, the
// memory form of one residue, the general addition with its rare equal-x fallback, and the windowed ladder built on them.
// Checked per form by tools/ladder_check.hip / tests/test_ladder_gpu.py: mac_signed_digit word for word against a Python model on
// chosen 128-bit patterns, macq_ladder inside k_mac_stage30_quad on scalars built from their endomorphism halves
// (tests/ladder_vectors.py), and through the batched MSM's tiny entries by tests/test_msm_batch_gpu.py.
#pragma once
#include "ec30.hip.h"
#include "glv.hip.h"

namespace porla {

// signed 4-bit digit i (0 .. 32) of the 128-bit magnitude m: ((m >> 4i) & 15) + carry, minus 16 above 8.  The carry into
// window i is 1 exactly when the bits below it exceed 0x88..8 (the recoding with digits in (-8, 8] is unique: msm_small.hip.h).
__device__ __forceinline__ int mac_signed_digit(const uint32_t m[4], int i) {
    bool gt = false, eq = true;
#pragma unroll
    for (int q = 3; q >= 0; q--) {
        const int below = 4 * i - 32 * q;                                  // bits of limb q below the window
        const uint32_t mask = below <= 0 ? 0u : (below >= 32 ? 0xffffffffu : ((1u << below) - 1u));
        const uint32_t a = m[q] & mask, b = 0x88888888u & mask;
        gt = eq ? (a > b) : gt;
        eq = eq && (a == b);
    }
    uint32_t raw = gt ? 1u : 0u;
    if (i < 32) {
        uint32_t limb = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) limb = (q == (i >> 3)) ? m[q] : limb;
        raw += (limb >> ((i & 7) * 4)) & 15u;
    }
    return raw > 8u ? (int)raw - 16 : (int)raw;
}

// A quad's LDS state is private to its four lanes, which sit in one wave: LDS operations of a wave complete in order, so between a
// lane's store and another lane's load only the compiler has to be held back -- no s_barrier across the block's waves
__device__ __forceinline__ void macq_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// one residue in the memory form (BN254: packed as it is; secp256k1: canonical) at d
template <class M>
__device__ __forceinline__ void macq_store_residue(uint32_t* d, const F30<M>& v) {
    Fe<M> t;
    if constexpr (M::PSEUDO_MERSENNE) t = f30_to_fe_canonical<M>(f30_pm_reduce<M>(v));
    else f30_pack<M>(t.v, v);
    store_words8(d, t.v);
}
template <class M>
__device__ __forceinline__ F30<M> macq_load_residue(const uint32_t* s, bool* all_zero) {
    const uint4* q = reinterpret_cast<const uint4*>(s);
    const uint4 a = q[0], b = q[1];
    const uint32_t t[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    *all_zero = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0;
    return f30_unpack<M>(t);
}
// does any lane of this lane's quad say so?
__device__ __forceinline__ bool macq_quad_any(bool v, uint32_t lane) { return ((__ballot(v) >> (lane & 60u)) & 0xfull) != 0; }

// (c, inf) += (neg ? -1 : 1) * e, where e is a finite memory-form point whose X is read at `ex` (e's own, or the beta table's):
// the register-form addition, an accumulator at infinity (the result is the operand), and -- rare: equal x, i.e. the accumulator
// is +-e -- the ordinary one-lane addition through the two LDS slots.  All four lanes of a quad call it together.
template <class M>
__device__ __forceinline__ void macq_add(F30<M>& c, bool& inf, const XYZZ<M>* e, const uint32_t* ex, bool neg, XYZZ<M>* slot_a,
                                         XYZZ<M>* slot_b, uint32_t r, uint32_t lane) {
    if (!inf) {
        if (xyzz30_add_quadreg<M>(c, e, ex, neg, r, lane)) return;
        macq_store_residue<M>(reinterpret_cast<uint32_t*>(slot_a) + 8 * r, c);
    }
    // the operand as a point of its own: X from ex, the sign applied to Y
    bool z;
    F30<M> v = macq_load_residue<M>(r == 0u ? ex : reinterpret_cast<const uint32_t*>(e) + 8 * r, &z);
    if (neg && r == 1u) v = f30_sub<M, 4>(F30<M>{}, v);
    if (inf) { c = v; inf = false; return; }
    macq_store_residue<M>(reinterpret_cast<uint32_t*>(slot_b) + 8 * r, v);
    macq_sync();
    if (r == 0u) xyzz30_add_one_lane<M>(slot_a, slot_b, slot_a, false);
    macq_sync();
    c = macq_load_residue<M>(reinterpret_cast<const uint32_t*>(slot_a) + 8 * r, &z);
    inf = macq_quad_any(z && r == 2u, lane);
}

// (c, inf) = sc * P on the four lanes of a quad: the endomorphism split, 33 signed 4-bit windows over the table of the multiples
// 1 .. 8 of P.  Q: the quad's LDS record -- tbl[8] (memory form; P = tbl[0], written by this quad's lanes, macq_sync or a block
// barrier passed) and bx[8][8] (the table's X coordinates times beta: the endomorphism's half reads its X there, so phi(d P) costs
// no product per addition); slot_a / slot_b: the quad's two slots for the rare general addition.  Lane r ends with coordinate r
// of the product; `inf` is the same on the four lanes.
template <class C, class Q>
__device__ __forceinline__ void macq_ladder(Q& Qd, XYZZ<typename C::Fp>* slot_a, XYZZ<typename C::Fp>* slot_b, uint32_t r, uint32_t lane,
                                            const uint32_t sc[8], F30<typename C::Fp>& c, bool& inf) {
    using M = typename C::Fp;
    using G = typename C::Glv;
    inf = true;
    bool z;
    c = macq_load_residue<M>(reinterpret_cast<const uint32_t*>(&Qd.tbl[0]) + 8 * r, &z);
    if (macq_quad_any(z && r == 2u, lane)) return;                         // P is infinity: so is every multiple
    uint32_t m0[4], m1[4];
    bool ng0, ng1;
    glv_split<G>(sc, m0, ng0, m1, ng1);
    // tbl[i] = (i + 1) P: one doubling, six additions of P
    bool tinf = false;
    xyzz30_dbl_quadreg<M>(c, r);
    macq_store_residue<M>(reinterpret_cast<uint32_t*>(&Qd.tbl[1]) + 8 * r, c);
#pragma unroll 1
    for (int i = 2; i < 8; i++) {
        macq_add<M>(c, tinf, &Qd.tbl[0], reinterpret_cast<const uint32_t*>(&Qd.tbl[0]), false, slot_a, slot_b, r, lane);
        macq_store_residue<M>(reinterpret_cast<uint32_t*>(&Qd.tbl[i]) + 8 * r, c);
    }
    macq_sync();
    // beta * X of the eight entries: two per lane
    {
        const F30<M> beta30 = f30_const<M>(G::BETA_30);
#pragma unroll 1
        for (int t = 0; t < 2; t++) {
            const uint32_t e = r + 4u * (uint32_t)t;
            const F30<M> x = macq_load_residue<M>(reinterpret_cast<const uint32_t*>(&Qd.tbl[e]), &z);
            macq_store_residue<M>(&Qd.bx[e][0], f30_mul<M>(x, beta30));
        }
    }
    macq_sync();
#pragma unroll 1
    for (int i = 32; i >= 0; i--) {
        if (!inf) {
#pragma unroll 1
            for (int d = 0; d < 4; d++) xyzz30_dbl_quadreg<M>(c, r);
        }
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            uint32_t mh[4];
#pragma unroll
            for (int j = 0; j < 4; j++) mh[j] = h ? m1[j] : m0[j];
            const int dg = mac_signed_digit(mh, i);
            if (dg == 0) continue;
            const uint32_t mag = (uint32_t)(dg < 0 ? -dg : dg) - 1u;
            const XYZZ<M>* e = &Qd.tbl[mag];
            macq_add<M>(c, inf, e, h ? &Qd.bx[mag][0] : reinterpret_cast<const uint32_t*>(e), (dg < 0) != (h ? ng1 : ng0), slot_a, slot_b,
                        r, lane);
        }
    }
}

}  // namespace porla

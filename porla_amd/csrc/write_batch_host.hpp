// Host decisions the five write batches (update, client update, client rebuild, the two server rebuilds) share: wt of a write, the level
// plan, the IPA row width and bases.  Elsewhere: mac_mix_form (mac_fft.hip.h), kzg_row_width, commit_rows_then (kzg_state.hpp).
#pragma once
#include "batch_host.hpp"
#include "icc_host.hpp"
#include <algorithm>

namespace porla {

// wt of one write (icc_wt) for its descriptor.  wt_sc: the integer wt mod p_icc reduced mod the group order, little-endian words -- the
// group sees wt mod its order (convert_ZZ_to_scalar / fr.SetBytes).  wt_p, wt_q: the data side's Montgomery residue pair, where wanted.
template <class C>
static void write_wt(size_t n_total, unsigned long long write_step, uint32_t wt_sc[8], uint32_t* wt_p = nullptr, uint32_t* wt_q = nullptr) {
    uint32_t p[8], q[8];
    uint8_t be[32];
    (void)icc_wt_residues(IccCurve<C>::id, n_total, write_step, wt_p ? wt_p : p, wt_q ? wt_q : q, be);
    h_load_be(wt_sc, be);
    fe_reduce_plain<typename IccCurve<C>::Q>(wt_sc, 8);
}

// The level plan of k >= 1 requests: `order` = the requests by level, highest first (stable), so that the requests step i concerns
// (level > i) are the first active[i] of it; lmax = the highest level of the call = the number of steps.
struct LevelPlan {
    std::vector<uint32_t> order, active;
    uint32_t lmax;
    template <class LevelOf>
    LevelPlan(size_t k, LevelOf level_of) : order(k) {
        for (size_t a = 0; a < k; a++) order[a] = (uint32_t)a;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return level_of(x) > level_of(y); });
        lmax = (uint32_t)level_of(order[0]);
        active.assign(lmax, 0);
        for (size_t a = 0; a < k; a++)
            for (uint32_t i = 0; i < (uint32_t)level_of(a); i++) active[i]++;
    }
};

constexpr size_t IPA_COLS = 128;               // NUM_CHUNKS: the row width of the IPA build

// the IPA build's bases, `name` as the message says it (a handle exists only where a device does: read after ensure_device)
static inline int ipa_check_generators(const char* who, const char* name, const porla_fixed_base* fb) {
    if (fb->curve == 1 && fb->secp.n_points >= IPA_COLS) return PORLA_OK;
    return bad_arg(who, std::string(name) + " must be a secp256k1 fixed base over at least the 128 generators");
}
static inline int ipa_check_hiding_base(const char* who, const char* name, const porla_fixed_base* fb) {
    if (fb->curve == 1 && fb->secp.n_points == 1) return PORLA_OK;
    return bad_arg(who, std::string(name) + " must be a secp256k1 fixed base over exactly one point");
}

}  // namespace porla

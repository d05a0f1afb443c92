// The schedule of the bucket reduction tree (msm.hip.h: k_tree_front2, k_tree_level, k_tree_level_quad, k_tree_tail) apart from the
// Workspace: tree_plan() is the host arithmetic -- scratch sizes, the ordered launches with every offset that goes into their
// arguments -- and tree_enqueue() issues exactly a plan's launches on raw device pointers.  msm_impl.hip.h:msm_tree_launch calls
// the two with default options; tools/tree_check.hip calls them on bucket arrays a test wrote and may override the options.
#pragma once
#include "msm.hip.h"
#include <cstdio>
#include <string>
#include <vector>

namespace porla {

// threads of the per-window tail block: the tail takes over at the first level whose additions per window fit one pass (four
// lanes per addition).  Same-box sweep of a blocking 2^20-pair MSM, profiles/r05_f_tree_tail_sweep.txt: 256 threads 1.58 ms,
// 512 threads 1.53-1.55, 1 024 threads 1.55-1.64 (one block per window then holds a compute unit for eight levels).
static inline uint32_t tree_tail_threads() { return 512u; }
// quad = four lanes per addition: a pass of the tail holds threads / 4 additions
static inline bool tree_quad() { return true; }
constexpr uint32_t TREE_QUAD_MAX_TASKS = 16384;         // levels up to this many additions run four lanes per addition ...
constexpr uint32_t TREE_QUAD_MAX_TASKS_LONE = 65536;    // ... for a caller that waits for this MSM alone (idle lanes to spend on latency; same sweep)
static inline uint32_t tree_tail_start(uint32_t B, uint32_t nlev, bool quad) {
    const uint32_t cap = quad ? tree_tail_threads() / 4 : tree_tail_threads();
    uint32_t l = 0;
    while (l + 1 < nlev && (l + 1) * (B >> (l + 1)) > cap) l++;
    return l;
}

// The decisions of the schedule.  A negative value means the product's choice (the expression in tree_plan); a caller may set
// any of them within what the kernels support, tree_plan refuses the rest.
struct TreeOptions {
    int parts = -1;                 // 1 | 2: the windows as one set, or as two halves on two streams
    int front2 = -1;                // 0 | 1: levels 0 and 1 as one launch of k_tree_front2
    long long quad_max_tasks = -1;  // a level of up to this many additions runs as k_tree_level_quad, a larger one as k_tree_level
    int l0 = -1;                    // first level of the per-window tail kernel
};

enum TreeKind : uint32_t { TREE_FRONT2 = 0, TREE_LEVEL = 1, TREE_LEVEL_QUAD = 2, TREE_TAIL = 3 };
static inline const char* tree_kind_name(uint32_t k) {
    return k == TREE_FRONT2 ? "front2" : k == TREE_LEVEL ? "level" : k == TREE_LEVEL_QUAD ? "level_quad" : "tail";
}

// one launch; every offset counts entries (XYZZ) from the start of its area
struct TreeLaunch {
    uint32_t kind, part;
    uint32_t l;                     // its level (front2: 1, the upper of its two; tail: l0, it runs l0 .. nlev - 1)
    uint32_t n;                     // TreeLevelArgs::n (front2: groups of four buckets; tail: windows)
    uint32_t grid, block;
    size_t bk;                      // this part's buckets
    // front2, level, level_quad
    bool s_prev_bk, s_prev2_bk;     // s_prev / s_prev2 are the buckets (at `bk`), else S entries
    size_t s_prev, s_prev2, s_out, s1_out;   // S area (s1_out: front2 only)
    size_t m_prev, m_out;           // M area
    uint32_t m_prev_stride, m_out_stride;
    // tail
    size_t s_lev[24];               // S area, levels 0 .. nlev - 1
    size_t m_global;                // M area
    size_t m_tail[2];               // tail area
    size_t fin;                     // fin
    uint32_t per_window, nb, B, nlev;
};

struct TreePlan {
    uint32_t c, W, lone, parts, nlev, B;
    size_t s_entries, m_entries, mt_entries, fin_entries;     // scratch sizes (tree_s, tree_m, tree_mt) and W * c
    struct Part { uint32_t w0, Wp, l0, front2; unsigned long long quad_max; } part[2];
    std::vector<TreeLaunch> launches;                         // part 0's in order, then part 1's
};

// -> "" or why the plan is refused.  lazy = C::F30_LAZY: the quad forms exist for the reduced-radix memory form only.
static inline std::string tree_plan(TreePlan& p, int c, int W, bool lone, bool lazy, const TreeOptions& o = TreeOptions()) {
    if (c < 2 || c > 24 || W < 1 || ((size_t)W << (c - 1)) > ((size_t)1 << 31)) return "shape out of range";
    const uint32_t B = 1u << (c - 1);
    const size_t nb = (size_t)W * B;
    const uint32_t nlev = (uint32_t)(c - 1);
    const bool quad = lazy && tree_quad();
    // k_tree_tail<C, false> is not launched: every tail runs four lanes per addition
    if (!quad) return "the tail runs four lanes per addition: curves with the reduced-radix memory form only";
    p.c = (uint32_t)c; p.W = (uint32_t)W; p.lone = lone ? 1u : 0u; p.nlev = nlev; p.B = B;
    // (sizes for the two halves of the window set, each with its own end slack)
    p.s_entries = nb + 2;                                     // all S levels: nb/2 + nb/4 + ...
    p.m_entries = 2 * (nb / 4) + 6;                           // two ping-pong halves
    p.mt_entries = 2 * (size_t)W * (B / 4 + 1) + 4;           // the tail's private halves
    p.fin_entries = (size_t)W * c;
    // The windows are independent trees.  With enough buckets they run as TWO halves on two streams: the first levels of a tree
    // are throughput bound, the last ones (quad levels, the tail) latency bound -- side by side the latency-bound levels of one
    // half run under the large levels of the other.
    // (only for a caller that waits for this one device-resident MSM: -1.7 % at 2^18 and 2^20 pairs; with a second MSM in
    // flight -- the two-phase API -- the other MSM already fills those gaps and the extra stream costs 5 % of the pipelined rate)
    const int parts = o.parts >= 0 ? o.parts : ((lone && W >= 4 && nb >= ((size_t)1 << 18)) ? 2 : 1);
    if (parts != 1 && parts != 2) return "parts must be 1 or 2";
    if (parts == 2 && W < 2) return "two parts need at least two windows";
    const uint32_t l0 = o.l0 >= 0 ? (uint32_t)o.l0 : tree_tail_start(B, nlev, quad);
    if (l0 >= nlev) return "the tail must start below the last level (l0 < nlev)";
    // a caller that waits for this MSM alone has idle lanes to spend on latency: more levels on four lanes per
    // addition; with another MSM in flight the extra lane work would cost throughput
    const unsigned long long quad_max = o.quad_max_tasks >= 0 ? (unsigned long long)o.quad_max_tasks
                                                               : (lone ? TREE_QUAD_MAX_TASKS_LONE : TREE_QUAD_MAX_TASKS);
    p.parts = (uint32_t)parts;
    p.launches.clear();
    p.launches.reserve(2 * (size_t)c);
    size_t s_off = 0, m_off = 0, mt_off = 0;
    for (int part = 0, w0 = 0; part < parts; part++) {
        const int Wp = parts == 1 ? W : (part == 0 ? W / 2 : W - W / 2);
        const size_t nbp = (size_t)Wp * B;
        // S level l at s_off + (nbp - (nbp >> l)) (nbp/2 + ... + nbp/2^l entries before it); M slots of level l in half l & 1
        const size_t m_half[2] = {m_off, m_off + nbp / 4 + 1};
        auto s_level = [&](uint32_t l) { return s_off + (nbp - (nbp >> l)); };
        // levels 0 and 1 as one launch (k_tree_front2) where both are full-width levels and another MSM is in flight: the chip
        // time the tree takes from that MSM's accumulation is what counts there, not the tree's depth
        const bool front2 = o.front2 >= 0 ? o.front2 != 0
                                          : (!lone && l0 >= 2 && (nbp & 3) == 0 && nbp / 2 > (size_t)TREE_QUAD_MAX_TASKS);
        if (front2 && (l0 < 2 || (nbp & 3) != 0)) return "front2 needs l0 >= 2 and a bucket count per part divisible by 4";
        p.part[part] = {(uint32_t)w0, (uint32_t)Wp, l0, front2 ? 1u : 0u, quad_max};
        TreeLaunch z{};
        z.part = (uint32_t)part; z.bk = (size_t)w0 * B; z.nlev = nlev; z.B = B; z.nb = (uint32_t)nbp;
        uint32_t l_first = 0;
        if (front2) {
            TreeLaunch a = z;
            a.kind = TREE_FRONT2; a.l = 1;
            a.s_prev_bk = a.s_prev2_bk = true; a.s_prev = a.s_prev2 = 0; a.m_prev = m_half[0];
            a.s_out = s_level(0); a.s1_out = s_level(1);
            a.m_out = m_half[1];                              // M^1, slot 0
            a.n = (uint32_t)(nbp >> 2);
            a.m_prev_stride = 0; a.m_out_stride = a.n;
            a.grid = (a.n + 255) / 256; a.block = 256;
            p.launches.push_back(a);
            l_first = 2;
        }
        for (uint32_t l = l_first; l < l0; l++) {
            TreeLaunch a = z;
            a.l = l;
            a.s_prev_bk = l == 0; a.s_prev = l ? s_level(l - 1) : 0;
            a.s_prev2_bk = l < 2; a.s_prev2 = l >= 2 ? s_level(l - 2) : 0;
            a.m_prev = m_half[(l + 1) & 1];
            a.s_out = s_level(l);
            a.m_out = m_half[l & 1];
            a.n = (uint32_t)(nbp >> (l + 1));
            a.m_prev_stride = 2 * a.n; a.m_out_stride = a.n;
            const size_t tasks = (size_t)(l + 1) * a.n;
            a.block = 256;
            if (tasks <= quad_max) { a.kind = TREE_LEVEL_QUAD; a.grid = (unsigned)((4 * tasks + 255) / 256); }
            else { a.kind = TREE_LEVEL; a.grid = (unsigned)((tasks + 255) / 256); }
            p.launches.push_back(a);
        }
        {
            TreeLaunch t = z;
            t.kind = TREE_TAIL; t.l = l0; t.n = (uint32_t)Wp;
            for (uint32_t l = 0; l < 24; l++) t.s_lev[l] = l < nlev ? s_level(l) : 0;
            t.m_global = m_half[(l0 + 1) & 1];
            t.per_window = B / 4 + 1;
            t.m_tail[0] = mt_off; t.m_tail[1] = mt_off + (size_t)Wp * t.per_window + 1;
            t.fin = (size_t)w0 * c;
            uint32_t need = (l0 + 2) * (B >> (l0 + 1)) * 4u;
            uint32_t threads = (need + 63) / 64 * 64;
            if (threads > tree_tail_threads()) threads = tree_tail_threads();
            if (threads < 64) threads = 64;
            t.grid = (uint32_t)Wp; t.block = threads;
            p.launches.push_back(t);
        }
        s_off += nbp + 1; m_off += 2 * (nbp / 4) + 2; mt_off += 2 * (size_t)Wp * (B / 4 + 1) + 2;
        w0 += Wp;
    }
    return "";
}

// what tree_enqueue puts around a part's level launches and around its tail launch (msm_tree_launch: the profiler's scopes)
struct TreeNoScope { TreeNoScope(const char*, hipStream_t) {} };

// issues the plan's launches: part 0 on st0, part 1 on st1 (the caller orders the two streams around the call)
template <class C, class Scope = TreeNoScope>
static hipError_t tree_enqueue(const TreePlan& p, const XYZZ<typename C::Fp>* buckets, XYZZ<typename C::Fp>* s_area,
                               XYZZ<typename C::Fp>* m_area, XYZZ<typename C::Fp>* mt_area, XYZZ<typename C::Fp>* fin,
                               hipStream_t st0, hipStream_t st1) {
    using M = typename C::Fp;
    static_assert(C::F30_LAZY, "the tree's quad forms read the reduced-radix memory form");
    size_t at = 0;
    for (uint32_t part = 0; part < p.parts; part++) {
        hipStream_t st = part == 0 ? st0 : st1;
        {
            Scope ps("tree_levels", st);
            for (; at < p.launches.size() && p.launches[at].part == part && p.launches[at].kind != TREE_TAIL; at++) {
                const TreeLaunch& q = p.launches[at];
                TreeLevelArgs<M> a;
                a.s_prev = q.s_prev_bk ? buckets + q.bk : s_area + q.s_prev;
                a.s_prev2 = q.s_prev2_bk ? buckets + q.bk : s_area + q.s_prev2;
                a.m_prev = m_area + q.m_prev;
                a.s_out = s_area + q.s_out;
                a.m_out = m_area + q.m_out;
                a.fin = nullptr;   // only the tail holds the last level
                a.n = q.n;
                a.m_prev_stride = q.m_prev_stride; a.m_out_stride = q.m_out_stride;
                a.l = q.l; a.nlev = q.nlev; a.last = 0;
                if (q.kind == TREE_FRONT2) hipLaunchKernelGGL((k_tree_front2<C>), dim3(q.grid), dim3(q.block), 0, st, a, s_area + q.s1_out);
                else if (q.kind == TREE_LEVEL_QUAD) hipLaunchKernelGGL((k_tree_level_quad<C>), dim3(q.grid), dim3(q.block), 0, st, a);
                else hipLaunchKernelGGL((k_tree_level<C>), dim3(q.grid), dim3(q.block), 0, st, a);
            }
        }
        if (at < p.launches.size() && p.launches[at].part == part) {
            const TreeLaunch& q = p.launches[at++];
            Scope ps("tree_tail", st);
            TreeTailArgs<M> t;
            t.buckets = buckets + q.bk;
            for (uint32_t l = 0; l < 24; l++) t.s_lev[l] = l < q.nlev ? s_area + q.s_lev[l] : nullptr;
            t.m_global = m_area + q.m_global;
            t.per_window = q.per_window;
            t.m_tail[0] = mt_area + q.m_tail[0]; t.m_tail[1] = mt_area + q.m_tail[1];
            t.fin = fin + q.fin;
            t.nb = q.nb; t.B = q.B; t.l0 = q.l; t.nlev = q.nlev;
            hipLaunchKernelGGL((k_tree_tail<C, true>), dim3(q.grid), dim3(q.block), 0, st, t);
        }
        // no copy packet: the last level stores its W * c results straight into the pinned host buffer (a D2H hipMemcpyAsync
        // was seen to block the launching thread for milliseconds while another MSM is in flight)
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the plan as text, one launch per line (tools/tree_check.hip --plan; read by tests/tree_vectors.py)
static inline std::string tree_plan_text(const TreePlan& p) {
    char b[1024];
    std::string out;
    snprintf(b, sizeof b, "plan c=%u W=%u lone=%u parts=%u nlev=%u B=%u s_entries=%zu m_entries=%zu mt_entries=%zu fin_entries=%zu tail_threads=%u\n",
             p.c, p.W, p.lone, p.parts, p.nlev, p.B, p.s_entries, p.m_entries, p.mt_entries, p.fin_entries, tree_tail_threads());
    out += b;
    for (uint32_t i = 0; i < p.parts; i++) {
        snprintf(b, sizeof b, "part part=%u w0=%u Wp=%u l0=%u front2=%u quad_max=%llu\n", i, p.part[i].w0, p.part[i].Wp, p.part[i].l0,
                 p.part[i].front2, p.part[i].quad_max);
        out += b;
    }
    for (const TreeLaunch& q : p.launches) {
        if (q.kind != TREE_TAIL) {
            snprintf(b, sizeof b, "launch part=%u kind=%s l=%u n=%u grid=%u block=%u bk=%zu s_prev_bk=%d s_prev=%zu s_prev2_bk=%d s_prev2=%zu "
                     "s_out=%zu s1_out=%zu m_prev=%zu m_out=%zu m_prev_stride=%u m_out_stride=%u nb=%u nlev=%u\n",
                     q.part, tree_kind_name(q.kind), q.l, q.n, q.grid, q.block, q.bk, (int)q.s_prev_bk, q.s_prev, (int)q.s_prev2_bk, q.s_prev2,
                     q.s_out, q.s1_out, q.m_prev, q.m_out, q.m_prev_stride, q.m_out_stride, q.nb, q.nlev);
            out += b;
            continue;
        }
        snprintf(b, sizeof b, "launch part=%u kind=tail l=%u n=%u grid=%u block=%u bk=%zu m_global=%zu m_tail0=%zu m_tail1=%zu per_window=%u "
                 "fin=%zu nb=%u B=%u nlev=%u s_lev=", q.part, q.l, q.n, q.grid, q.block, q.bk, q.m_global, q.m_tail[0], q.m_tail[1],
                 q.per_window, q.fin, q.nb, q.B, q.nlev);
        out += b;
        for (uint32_t l = 0; l < q.nlev; l++) { snprintf(b, sizeof b, "%s%zu", l ? "," : "", q.s_lev[l]); out += b; }
        out += "\n";
    }
    return out;
}

}  // namespace porla

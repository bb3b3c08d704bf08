// Host-side launch policy of the persistent recurrent kernels (reccell.hip, gatedcell.hip), in one place: how one pass
// over (Bp, T, H) is cut into launches, and how a hidden size picks a kernel shape.  Plain C++17, no HIP types: a host
// compiler builds it alone (a sweep over the whole input grid needs no GPU).
//
// A persistent launch keeps the time loop inside the kernel: the workgroups of a row tile (32 virtual batch rows) hand
// their step's output to each other and wait for it, so every workgroup of the launch must be resident at once — at
// most one per CU.  The pass is therefore cut into GROUPS of row tiles that fit the machine, run one after the other,
// and into CHUNKS of L = steps_per_launch time steps.  L = T is one launch per group; L = 1 is one launch per step,
// where every wait is already satisfied at launch: any grid size runs, the safe fallback.
#pragma once
#include <algorithm>
#include <type_traits>

namespace rec_plan {

// What differs between the kinds of cell.  Everything else below is the same for all of them.
struct Policy {
    // GRU: two hand-offs inside a step, so the workgroups of a row tile must be resident at ANY L.  The groups are
    // limited at L = 1 too, and a row tile that does not fit the machine is refused (the caller takes its per-step
    // path) where the other kinds degrade to L = 1.
    bool always_resident = false;
    // Spiking kinds: ask the runtime's occupancy calculator (the `resident` callable of make_plan) instead of assuming
    // that one workgroup per CU fits.
    bool ask_occupancy = false;
    // Spiking forward with bf16 saved states: those cannot carry the exact state from one launch to the next, so an
    // occupancy answer of "no" is refused instead of degraded to L = 1.
    bool refuse_degrade = false;
    // Spiking kinds, bf16 operand mode, not streaming, kgw >= 2: the 64-column workgroups (cw = 2) exist.
    bool has_cw2 = false;
    int cw_override = 0;  // SPARCH_REC_CW: 1 forces the 32-column kernels, 2 the 64-column ones where they exist
    // Dense cell, kept as found: it decides "whole sequence" from the clamped steps_per_launch BEFORE the fallback to
    // L = 1, so a pass degraded because a row tile has more workgroups than the device has CUs still gets the agreement
    // table.  (Not reachable on 256 CUs: a row tile has at most 32 workgroups.)
    bool whole_before_degrade = false;
};

struct Plan {
    bool ok = false;        // false: refused (SPARCH_EINVAL)
    int n_rt_total = 0, T = 0;
    int L = 1;              // steps per launch, in [1, T]
    int rt_per_launch = 0;  // row tiles per group
    int cw = 1;             // 32-column groups per workgroup
    int wg_per_rt = 0;      // workgroups of one row tile = n_ct / cw
    bool whole = false;     // one launch covers the whole sequence (the XCD agreement table is per launch)
};

inline int cus_or_default(int cus) { return cus > 0 ? cus : 256; }  // an unknown CU count counts as a full MI355X

// n_ct: workgroups of one row tile at cw = 1.  resident(grid, cw): can `grid` workgroups of the kernel this plan would
// launch be resident at once?  Only called when p.ask_occupancy and L > 1.
template <class Resident>
Plan make_plan(int n_rt_total, int T, int n_ct, int steps_per_launch, int cus, const Policy& p, Resident&& resident) {
    Plan q;
    q.n_rt_total = n_rt_total; q.T = T;
    cus = cus_or_default(cus);
    int L = std::min(std::max(steps_per_launch, 1), T);
    const bool asked_whole = L >= T;
    // 64-column workgroups (bf16 operand mode): when the row tiles do not fit one persistent launch at 32 columns
    // per workgroup (512 virtual rows at H = 1024: 16 x 32 workgroups) but do at 64 (16 x 16), the whole batch runs
    // as ONE launch instead of two half-machine launches back to back — the steps are latency chains, so a launch
    // over all rows takes about as long as one over half of them.
    int cw = 1;
    if (p.has_cw2 && L > 1 && n_ct % 2 == 0 && p.cw_override != 1 &&
        (p.cw_override == 2 || ((long long)n_rt_total * n_ct > cus && (long long)n_rt_total * (n_ct / 2) <= cus)))
        cw = 2;
    const int wg = n_ct / cw;
    int rt = n_rt_total;  // L = 1: nothing waits inside a launch, any grid size is fine
    if (L > 1 || p.always_resident) {
        rt = cus / wg;  // one workgroup per CU must be co-resident
        if (rt < 1) {
            if (p.always_resident) return q;
            L = 1; rt = n_rt_total;
        }
    }
    if (L > 1 && p.ask_occupancy && !resident((unsigned)(wg * std::min(rt, n_rt_total)), cw)) {
        if (p.refuse_degrade) return q;
        L = 1; rt = n_rt_total;
    }
    if (L == 1) cw = 1;  // the per-step launches are 32-column
    q.ok = true; q.L = L; q.rt_per_launch = rt; q.cw = cw; q.wg_per_rt = n_ct / cw;
    q.whole = p.whole_before_degrade ? asked_whole : L >= T;
    return q;
}
inline Plan make_plan(int n_rt_total, int T, int n_ct, int steps_per_launch, int cus, const Policy& p) {
    return make_plan(n_rt_total, T, n_ct, steps_per_launch, cus, p, [](unsigned, int) { return true; });
}

// launch(rt0, n_rt_launch, step_begin, step_end) for every group of row tiles and chunk of steps; stops at the first
// non-zero return.  reverse: the chunks run from the end of the sequence down (the spiking backward).
template <class Launch>
int walk(const Plan& q, bool reverse, Launch&& launch) {
    for (int rt0 = 0; rt0 < q.n_rt_total; rt0 += q.rt_per_launch) {
        const int n = std::min(q.rt_per_launch, q.n_rt_total - rt0);
        if (!reverse) {
            for (int t0 = 0; t0 < q.T; t0 += q.L)
                if (int rc = launch(rt0, n, t0, std::min(q.T, t0 + q.L))) return rc;
        } else {
            for (int t1 = q.T; t1 > 0; t1 -= q.L)
                if (int rc = launch(rt0, n, std::max(0, t1 - q.L), t1)) return rc;
        }
    }
    return 0;
}

// ---- kernel shape.  kgw = k-groups of the contraction per wave class, one of 1, 2, 4, 8 (0: no kernel holds the slice).
template <int K> using kgw_c = std::integral_constant<int, K>;
// f(kgw_c<K>) for the run-time kgw; a value-initialised result for anything else
template <class F>
auto with_kgw(int kgw, F&& f) -> decltype(f(kgw_c<1>{})) {
    switch (kgw) {
        case 1: return f(kgw_c<1>{});
        case 2: return f(kgw_c<2>{});
        case 4: return f(kgw_c<4>{});
        case 8: return f(kgw_c<8>{});
        default: return {};
    }
}
template <class F>
auto with_bool(bool b, F&& f) -> decltype(f(std::true_type{})) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}
// reccell.hip's kernels: 8 waves of kgw / 2 k-groups each once there are at least 8 k-groups (kgw >= 2), else 4 waves
// of one.  (gatedcell.hip's always run 8 waves of kgw.)
constexpr int rec_kb(int kgw) { return kgw == 1 ? 1 : kgw / 2; }
constexpr int rec_nw(int kgw) { return kgw == 1 ? 4 : 8; }

}  // namespace rec_plan

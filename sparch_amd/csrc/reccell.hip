// G3/G4 (recurrent kinds): RLIF / RadLIF cells, forward and reverse-time backward, with
// the time loop inside a persistent kernel and the recurrent product on MFMA.
//
// Replaces _rlif_cell (snns.py:554-578) and _radlif_cell (696-727) — per step
//     w = beta*w + a*u + b*s ;  u = alpha*(u-s) + (1-alpha)*(Wx_t + s@V - w) ;  s = H(u-theta)
// with V = V.weight, diagonal zeroed (566/712), `s @ V` un-transposed — and their autograd
// replay (reverse recurrences in SURVEY.md §8a), including du_{t+1} @ V^T per step.
//
// Decomposition (gfx950, 256 CUs in 8 XCDs):
//   * a workgroup (256 threads, one wave per SIMD) owns a 32-row x 32-column tile of the
//     (B', H) state for the whole sequence; membrane/adaptation state lives in registers;
//   * its 1024x32 slice of V (forward) / V^T (backward) stays in VGPRs for the whole launch
//     as MFMA B-operands; the four waves split K and the partial 32x32 tiles meet in LDS in
//     a fixed order (reproducible);
//   * EXACT low-precision operands: every fp32 V element is split into three bf16 values
//     V = hi + mid + lo (8+8+8 significand bits, exact).  Spikes are 0/1, exact in bf16, so
//     s@V = s@hi + s@mid + s@lo runs on v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate) with
//     exact products and fp32 accumulation: same accuracy class as an fp32 fmaf chain at 3/16
//     of its cost.  In the backward dWx is split as well (x = t1 + t2 + t3 exactly) and the six
//     largest cross terms (t1*hi, t1*mid, t2*hi, t1*lo, t3*hi, t2*mid; the dropped ones are
//     t3*mid <= 2^-22 and t2*lo <= 2^-23 of |x||V| per product in the worst case; measured aggregate
//     3e-9 of sum|x||V| against 1e-7 for an fp32 sgemm's own rounding) are accumulated: fp32-faithful
//     at 6/16 of the fp32 MFMA cost;
//   * the 32 workgroups of one batch tile exchange the step's output every step:
//       forward  — spikes, bit-packed, as 8-byte {tag = t+1, 32 spike bits} granules written
//                  with one agent-scope (sc1, write-through) store each and polled with sc1
//                  loads: the data is the flag, no fence (MI355X guide, G16 form R2).  One slot
//                  per (step, row): never reused inside a call;
//       backward — the 32x32 tile of dWx_t as three PRE-SPLIT bf16 planes (x = t1 + t2 + t3 exactly: truncation
//                  split by v_perm / AND / SUB in the producer), stored in MFMA-FRAGMENT ORDER (16-byte piece
//                  ((ks*3 + p)*64 + h*32 + row) = plane p, k = 16 ks + 8 h + 0..7) into a depth-4 ring, and
//                  NOTHING ELSE: no drain, no tag.  The data is the flag here too: every ring slot holds a
//                  SENTINEL bit pattern (a signalling NaN, which no fp32 arithmetic result can be — and no
//                  plane word either: its upper half would be a signalling-NaN bf16) until its piece lands,
//                  and consumers simply load the tile (16-byte sc1 loads, every wave-load one contiguous
//                  1 KiB = the MFMA A fragments of one k16-step and plane) and re-load the pieces that still
//                  read as the sentinel (first and last word checked: a producer thread owns 4 consecutive k,
//                  i.e. half a piece, written with one 8-byte store per plane; 8- and 16-byte stores are
//                  observed untorn on gfx950).  A producer puts the sentinel back into its slot of step t+2
//                  while it works on step t: by then it has seen every peer's step t+1 tile, which they
//                  produced after consuming every step t+2 tile, and its next vmcnt(0) (the tile loads of
//                  step t-1) retires that store before it publishes step t-1 — the store a consumer must see
//                  before it can ask for step t-2, the slot's next content.  Against the first version (tile
//                  stores, drain, barrier, tag store; consumers poll the tag, barrier, then load): one
//                  store->load visibility hop instead of two per step and two workgroup barriers fewer.
//                  Until the XCD-local stores the wire carried fp32 (4 KB per tile) and each of the 32
//                  consumers split the same values (2.8 k VALU cycles per SIMD and step); with the tiles
//                  served by the XCD's own L2 the 6 KB plane tiles are the faster trade (1.34 -> 1.27 ms per
//                  launch; timing ablations: no split at 4 KB 1.16, no split at 6 KB 1.27);
//   * block -> tile mapping keeps a batch tile's workgroups at equal blockIdx % n_row_tiles,
//     i.e. on one XCD under round-robin dispatch.  That is a speed choice only: every
//     hand-off is agent-scope and placement-independent.  Every spin is bounded by a
//     wall-clock timeout that raises *status and unwinds the launch.
//   * steps_per_launch = T gives one persistent launch; = 1 degenerates to one launch per
//     time step, where every wait is already satisfied at launch (safe fallback, and the
//     path for shapes whose grid cannot be co-resident).
//   * host side: how a pass is cut into launches (groups of row tiles x chunks of steps, the
//     fallbacks, 32- or 64-column workgroups) is decided in ONE place for these cells and for
//     gatedcell.hip's: rec_plan.h (plain C++, no HIP).  What differs between the kinds is a
//     rec_plan::Policy; run_rec / run_ann below size, check and clear the workspace, plan, walk.
//     Which instantiation runs a call is one table per family (rec_kernel, ann_kernel), used
//     for launching and for the occupancy question alike.
#include "neuron.h"

#include "rec_common.h"

namespace {

struct RecArgs {
    int B, dirs, T, H, Bp;
    int n_ct, nkg, n_rt_total;
    int rt_base, n_rt_launch;
    int t_begin, t_end;
    const float* Wx; const float* scale; const float* shift;
    const float* alpha; const float* beta; const float* a; const float* b;
    const u32x4* vpack; const float* rec0;
    // step variants (EXT): the recurrent product of the ONE step [t_begin, t_begin+1) is supplied by the caller
    // in rec0 (Bp,H); the step's raw spikes (forward, bf16 0/1) / dWx (backward, fp32) also go to a contiguous
    // (Bp,H) buffer, the operand of the caller's next product
    uint16_t* s_step16; float* dwx_step;
    const float* u0; const float* w0; const float* s0;
    float theta, p_drop, inv_keep; uint64_t seed;
    float* s_out; uint16_t* s16_out; float* u_save; float* w_save; uint32_t* spike_count;
    // backward
    const float* g_out; const float* g_rate; float g_rate_scale;
    float* dWx; uint16_t* s_prev16; float* dparam_ws;
    // BatchNorm backward folded in (nullable): raw projection (B,T,H) + per-column statistics; the kernel then
    // also leaves sum_t dWx and sum_t dWx*xhat per (row, column) in planes 6 and 7 of dparam_ws
    const float* bn_x; const float* bn_mean; const float* bn_invstd;
    const float* bn_src;  // backward: bn_x, or (without BatchNorm) any readable (B,T,H) range — the loop loads unconditionally
    int save16;  // u_save / w_save hold bf16 (common.h save_u16); whole-sequence launches only
    // hand-off
    u64* chan; char* ring; unsigned* status;
    unsigned* xcd_tab;  // [n_rt_total][n_ct] agreement table of the XCD-local stores (whole-sequence launches), or null
};

// RecArgs itself does not grow (every kernel's argument segment would): the smooth-surrogate backward kernels take it
// with the surrogate behind it, the ragged (`_len`) kernels with the surrogate and the per-row lengths (B,), as one
// by-value argument (the kernel table's rows are KernelRef<Args>)
struct RecSgArgs : RecArgs { SurrogateArgs sg; };
struct RecLenArgs : RecSgArgs { const int* lengths; };
// the packed (`_pk`) kernels: the sorted lengths and the exclusive prefix sum (B + 1,) behind them — sequence j owns rows
// [offsets[j], offsets[j] + lengths[j]) of every (N, .) tensor; B counts sequences and T is the longest length
struct RecPkArgs : RecLenArgs { const int* offsets; };
// the stateful (`_st`) backward kernels: the gradient arriving on the final state (u_T, w_T, s_T) and the gradient of the
// initial state going out, each (Bp,H) and nullable
struct RecStArgs : RecSgArgs {
    const float* g_uT; const float* g_wT; const float* g_sT;
    float* g_u0; float* g_w0; float* g_s0;
};

// Diagnostic build only (-DSPARCH_REC_PROF, never shipped): per-workgroup sums of s_memtime
// deltas for the segments of a time step, written to a private buffer no kernel reads.
#ifdef SPARCH_REC_PROF
__device__ u64 g_rec_prof[2][512][12];
#define PROF_DECL u64 pf_t = 0, pf_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define PROF_STAMP(i)                                                                           \
    do {                                                                                        \
        u64 now_;                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                      \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_)::"memory");            \
        __builtin_amdgcn_sched_barrier(0);                                                      \
        if ((i) >= 0) pf_acc[(i) < 0 ? 0 : (i)] += now_ - pf_t;                                 \
        pf_t = now_;                                                                            \
    } while (0)
#ifdef SPARCH_REC_PROF_ALLWAVES  /* every wave of the first 64 workgroups: slot = workgroup * 8 + wave */
#define PROF_FLUSH(which)                                                                       \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 64)                                             \
        for (int i_ = 0; i_ < 10; ++i_) g_rec_prof[which][blockIdx.x * 8 + (threadIdx.x >> 6)][i_] += pf_acc[i_];
#else
#define PROF_FLUSH(which)                                                                       \
    if ((threadIdx.x == 0 || threadIdx.x == 256) && blockIdx.x < 256)  /* wave 0, and wave 4 in slots 256.. */ \
        for (int i_ = 0; i_ < 10; ++i_) g_rec_prof[which][blockIdx.x + (threadIdx.x ? 256 : 0)][i_] += pf_acc[i_];
#endif
#else
#define PROF_DECL
#define PROF_STAMP(i)
#define PROF_FLUSH(which)
#endif

// ------------------------------------------------------------------------------ forward
// NW waves per workgroup, each taking the k-groups kg = wave + NW*kk of the contraction (partial tiles
// summed through LDS); NW = 8 puts two waves on each SIMD so that one's LUT reads / poll latency sit
// under the other's MFMAs.  Pointwise update, publish and stores stay on the first 256 threads.
// NP: planes of V — 3 = exact split (default), 1 = the bf16 operand mode (V rounded once by the pack kernel).
// CW (round 3): 32-column groups per workgroup.  1: a workgroup owns 32 columns and its first 256 threads the
// pointwise state (above).  2 (bf16 operand mode, 8 waves): it owns 64 columns — with ONE plane of V the slice is
// 128 KiB, a quarter of the register file — and all 512 threads own pointwise state (thread = (column group j,
// row, column quad)); a batch of 512 virtual rows (a bidirectional B = 256 layer, BASELINE configs[4]) is then
// 16 row tiles x 16 workgroups = ONE persistent launch on 256 CUs instead of two half-filled ones run back to
// back.  The hand-off format does not change: the workgroup publishes the granules of k-groups 2 ctw and
// 2 ctw + 1, consumers read k-groups as before.
// STREAM (streaming inference, sparch_rec_cell_stream_fwd / sparch_rec_cell_step_stream_fwd): no save tensors.  u0 /
// w0 / s0 are the stream's (Bp,H) state buffers: EVERY launch starts from them (a launch per step included) and
// writes the state it ended in back behind its last step, each thread its own elements; the last step's raw spikes
// also go to s_step16 as a bf16 0/1 plane, the operand of the caller's next s @ V product.
// LEN (sparch_rec_cell_fwd_len, one direction): the output spikes of steps at or past the row's length are 0 and not
// counted — a select in the dropout block.  The spikes PUBLISHED to the peers and the saved states stay unmasked: a
// row's padded steps are garbage in, masked out, and nothing of them reaches a valid step (time runs forward only).
// PK (sparch_rec_cell_fwd_pk, with LEN; whole-sequence launches only): the packed layout.  A row tile runs t < the length
// of its first row, its longest (the rows are sorted): the bound is the same in all of the tile's workgroups, so the
// poll / publish protocol is untouched.  A shorter row keeps computing and publishing (unmasked, as with LEN) up to the
// tile's bound; its projection loads are clamped into its own packed rows and its stores happen only for t < its length
// — a store behind a row's end would land in the next sequence.
template <bool ADAPT, int KGW, int NW, bool EXT = false, int NP = 3, int CW = 1, bool STREAM = false, bool LEN = false,
          bool PK = false>
__global__ __launch_bounds__(64 * NW, 1) void rec_fwd_kernel(
    std::conditional_t<PK, RecPkArgs, std::conditional_t<LEN, RecLenArgs, RecArgs>> a) {
    static_assert(!PK || (LEN && !EXT && !STREAM), "packed: the ragged whole-sequence forward");
    static_assert(CW == 1 || (CW == 2 && NW == 8 && !EXT), "64-column workgroups: the 8-wave persistent kernels");
    static_assert(!STREAM || CW == 1, "the streaming kernels own 32 columns per workgroup");
    __shared__ __attribute__((aligned(16))) float red[2][NW][CW][RT * RED_LD4];
    __shared__ __attribute__((aligned(16))) u32x4 lut[256];  // byte of 8 spikes -> 8 bf16 (0 / 1.0)
    __shared__ int abort_flag[2];
    __shared__ int xcd_local_flag;
    __shared__ unsigned cnt_lds[2][CW * CT];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, hh = lane >> 5;
    const int rt = a.rt_base + (int)(blockIdx.x % a.n_rt_launch);
    const int ctw = (int)(blockIdx.x / a.n_rt_launch);  // the workgroup's index among its row tile's workgroups
    const int T = a.T, H = a.H, HO = a.H * a.dirs;

    // element ownership for the pointwise update: row r, 4 columns (of column group ct)
    const bool pw = tid < 256 * CW;
    const bool pw_wave = NW == 4 || CW == 2 || wave < 4;  // the same, as a scalar (wave-uniform branches)
    const int ct = ctw * CW + (CW == 2 ? tid >> 8 : 0);   // this THREAD's 32-column group
    const int r = (tid & 255) >> 3, cq = tid & 7;
    const int bp = rt * RT + r, col = ct * CT + cq * 4;
    const bool valid = pw && bp < a.Bp && col < H;
    const int bpc = min(bp, a.Bp - 1), colc = min(col, H - 4);
    const int d = bpc / a.B, b = bpc - d * a.B;

    u32x4 vb[CW][KGW][2][NP];
    if (!EXT) {
#pragma unroll
        for (int c = 0; c < CW; ++c) load_vslice<KGW, NW, NP>(vb[c], a.vpack, ctw * CW + c, a.nkg, wave, lane);
    }
    if (tid < 256) {
        u32x4 e;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            e[j] = spike_pair16(((unsigned)tid >> (2 * j)) & 1u, ((unsigned)tid >> (2 * j + 1)) & 1u);
        lut[tid] = e;
    }

    Neuron<ADAPT> p[4];
    float sc[4], sh[4], u[4], w[4], s[4];
    uint32_t cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        p[e] = neuron_load<ADAPT>(a.alpha, a.beta, a.a, a.b, colc + e);
        sc[e] = a.scale ? a.scale[colc + e] : 1.0f;
        sh[e] = a.scale ? a.shift[colc + e] : 0.0f;
        w[e] = 0.f;
    }
    {
        f32x4 v;
        if (a.t_begin == 0 || STREAM) {
            v = ld4(a.u0 + (size_t)bpc * H + colc); u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
            v = ld4(a.s0 + (size_t)bpc * H + colc); s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
            if (ADAPT) { v = ld4(a.w0 + (size_t)bpc * H + colc); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
        } else {
            const size_t o = ((size_t)bpc * T + (a.t_begin - 1)) * H + colc;
            v = ld4(a.u_save + o); u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] = spike_of(u[e], a.theta) ? 1.0f : 0.0f;
            if (ADAPT) { v = ld4(a.w_save + o); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
        }
    }
    if (tid < 2) abort_flag[tid] = 0;
    if (tid < 2 * CW * CT) cnt_lds[tid / (CW * CT)][tid % (CW * CT)] = 0;
    const unsigned my_xcc = xcc_id();
    xcd_agree((EXT || !a.xcd_tab) ? nullptr : (gu32*)a.xcd_tab + (size_t)rt * a.n_ct, 0u, a.n_ct / CW, ctw, my_xcc, tid, &xcd_local_flag);
    __syncthreads();
    const bool xcd_local = xcd_local_flag != 0;  // this row tile's workgroups share an XCD: plain hand-off stores

    const bool has_norm = a.scale != nullptr;
    const bool drop = a.p_drop > 0.0f;
    const uint64_t seed = drop ? resolve_seed(a.seed) : 0;
    int len = T;
    if constexpr (LEN) len = a.lengths[b];
    // (PK is a constant: of `PK ? :` only the live arm is compiled, and without PK that is the expression it always was)
    [[maybe_unused]] size_t row0 = 0;   // the row's first packed row
    [[maybe_unused]] int t_tile = 0;    // the tile's bound: the length of its first row
    if constexpr (PK) {
        row0 = (size_t)a.offsets[b];
        t_tile = __builtin_amdgcn_readfirstlane(a.lengths[min(rt * RT, a.Bp - 1)]);
    }
    auto wx_ptr = [&](int t) {
        const int tt = d ? (T - 1 - t) : t;
        return a.Wx + (PK ? row0 + min(t, len - 1) : (size_t)b * T + tt) * H + colc;
    };
    f32x4 x_next = {0.f, 0.f, 0.f, 0.f};
    if (pw) x_next = ld4s(wx_ptr(a.t_begin));
    // The recurrent drive of the launch's FIRST step (t = 0: s0 @ V from the host; step variants: the caller's
    // product) and the projection row of its second step are loaded HERE, not inside the loop: a global load on
    // one path of the loop body only (round 2 had `if (t == 0) rec = ld4(rec0)`) makes hipcc's wait-count pass
    // merge the two paths conservatively — an `s_waitcnt vmcnt(0)` behind the reduction barrier of EVERY step,
    // where the pointwise waves then sat out the acknowledgements of the previous step's bulk HBM stores.
    const bool first_ext = a.t_begin == 0 || EXT;
    f32x4 rec_first = {0.f, 0.f, 0.f, 0.f}, x_second = rec_first;
    if (first_ext) {
        rec_first = ld4(a.rec0 + (size_t)bpc * H + colc);
        if (pw && a.t_begin + 1 < a.t_end) x_second = ld4s(wx_ptr(a.t_begin + 1));
    }
    // Bulk HBM stores of a step are held back (12 VGPRs) and issued only after the NEXT step's poll loads:
    // vmcnt retires in order and counts stores, so stores (and the Wx prefetch) issued ahead of the poll
    // would put their HBM latency in front of the sweep.  Issued behind it they retire under the MFMA phase.
    f32x4 pend_s = {0.f, 0.f, 0.f, 0.f}, pend_u = pend_s, pend_w = pend_s;
    int pend_t = -1;
    // (Handing these stores to the four waves without pointwise state, through an LDS staging buffer, lost:
    // 0.76 -> 0.81 ms per launch.  Those waves poll too, with less lead over the stores, and the matrix phase waits
    // for its slowest wave.  DESIGN.md, "Retired experiment switches".)
    auto store_step = [&](int st_t, const f32x4& vs, const f32x4& vu, const f32x4& vw) {
        const int ptt = d ? (T - 1 - st_t) : st_t;
        const size_t o_s = (PK ? row0 + st_t : (size_t)b * T + ptt) * HO + (size_t)d * H + colc;
        if (a.s_out) st4(a.s_out + o_s, vs);  // the fp32 copy: only for callers that read the layer's output tensor
        if (a.s16_out) {  // the same spikes as a bf16 plane (0 / 1.0) for the GEMMs that consume them
            st2(a.s16_out + o_s, spike_quad16(vs));
        }
        if constexpr (!STREAM) {
            st4_saved<true>(a.u_save, (PK ? row0 + st_t : (size_t)bp * T + st_t) * H + col, vu, a.save16, a.theta);
            if (ADAPT) st4_saved<false>(a.w_save, (PK ? row0 + st_t : (size_t)bp * T + st_t) * H + col, vw, a.save16, a.theta);
        }
    };
    auto flush_pending = [&]() {
        if (pend_t >= 0 && valid && (!PK || pend_t < len)) store_step(pend_t, pend_s, pend_u, pend_w);
        pend_t = -1;
    };
    PROF_DECL

    for (int t = a.t_begin; t < (PK ? min(a.t_end, t_tile) : a.t_end); ++t) {
        PROF_STAMP(-1);
        // this step's projection row.  (The take-over copy of the prefetch register ends up at the loop latch with
        // an `s_waitcnt vmcnt(0)` in front of the next poll's issue.  Measured against it in one call, 40 launches
        // each: the prefetch by LDS-DMA — no register destination, no wait anywhere but the poll's own — 0.679 vs
        // 0.669 ms per launch, its LDS read hoisted in front of the matrix phase 0.69; 256-1024 cycles of s_sleep
        // ahead of the first poll sweep +0.02 ms per 256.  The round-2 code, with a FLAT flag read and a
        // conditional load in the loop body, waited vmcnt(0) behind the reduction barrier instead: 0.699.)
        f32x4 xv;
        float rec[4] = {0.f, 0.f, 0.f, 0.f};

        if (t == 0 || EXT) {
            rec[0] = rec_first.x; rec[1] = rec_first.y; rec[2] = rec_first.z; rec[3] = rec_first.w;
            xv = x_next;
            x_next = x_second;
        } else {
            // ---- gather the 32 x H spike bits of step t-1 (tag == t) for this wave's k-groups
            const gu64* base = (const gu64*)a.chan + ((size_t)(t - 1) * a.n_rt_total + rt) * a.n_ct * 32;
            u64 gran[KGW];
            const u64 t_start = __builtin_amdgcn_s_memrealtime();
            for (unsigned spins = 0;; ++spins) {
                // all loads of the sweep are issued back to back (clamped index, no control flow between
                // them) and only then compared: ONE round trip per sweep.  (A short-circuit `ok && tag==t`
                // inside a per-k-group `if` made hipcc wait vmcnt(0) after every load: 8 serialized round
                // trips, ~5.5k cycles per step — the largest single cost of the first versions.)
#pragma unroll
                for (int kk = 0; kk < KGW; ++kk) {
                    const int kgc = min(wave + NW * kk, a.n_ct - 1);
                    gran[kk] = __hip_atomic_load(base + (size_t)kgc * 32 + li, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                unsigned bad = 0;
#pragma unroll
                for (int kk = 0; kk < KGW; ++kk) {
                    const unsigned m = (wave + NW * kk < a.n_ct) ? 0xFFFFFFFFu : 0u;
                    bad |= ((unsigned)(gran[kk] >> 32) ^ (unsigned)t) & m;
                }
                if (__all(bad == 0)) break;
                if ((spins & 63u) == 63u &&
                    __builtin_amdgcn_s_memrealtime() - t_start > TIMEOUT_TICKS) {
                    raise_timeout(a.status, &abort_flag[t & 1], SPARCH_STATUS_REC_FWD, t);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            PROF_STAMP(0);  // poll wait
            // (the empty asm makes the take-over a use of the prefetch register AT THIS POINT: as a plain copy the
            // register allocator placed it at the loop latch, with a `vmcnt(0)` in front of the next poll)
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[e] = x_next[e];
            if (pw && t + 1 < a.t_end) x_next = ld4s(wx_ptr(t + 1));
            flush_pending();
            // ---- s_{t-1} @ V on the bf16 MFMA: spikes expanded through the LDS table (lane
            //      (row li, k-half hh) takes byte 2*ks + hh of its row's 32-bit word)
            u32x4 af[KGW][2];
#pragma unroll
            for (int kk = 0; kk < KGW; ++kk) {
                // k-groups beyond H (padding of the register layout) contribute zero spikes; keeping the whole
                // section free of branches lets the scheduler interleave LUT reads with the MFMA chain
                const unsigned wbits = (wave + NW * kk < a.n_ct) ? (unsigned)gran[kk] : 0u;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    af[kk][ks] = lut[(wbits >> (16 * ks + 8 * hh)) & 0xFFu];
            }
            f32x16 acc[CW];
#pragma unroll
            for (int c = 0; c < CW; ++c)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KGW; ++kk)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int p = NP - 1; p >= 0; --p)
#pragma unroll
                        for (int c = 0; c < CW; ++c) acc[c] = mfma_bf16(af[kk][ks], vb[c][kk][ks][p], acc[c]);
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                float* rd = red[t & 1][wave][c];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
                    rd[row * RED_LD4 + li] = acc[c][i];
                }
            }
            PROF_STAMP(1);  // expand + MFMA + LDS write
        }
        if (xcd_local && xcc_id() != my_xcc) raise_timeout(a.status, &abort_flag[t & 1], SPARCH_STATUS_REC_FWD, t);  // moved to another XCD
        lds_barrier();
        PROF_STAMP(2);  // barrier
        if (lds_flag_read(&abort_flag[t & 1])) break;
        // Everything from here to the end of the step belongs to the waves that own pointwise state.  A WAVE-UNIFORM
        // branch (round 3): until then the upper four waves of an 8-wave workgroup ran the whole update on dead
        // values — per-thread `valid` only masked its stores — and took every other vector issue slot of the
        // pointwise waves they share a SIMD with (stamped: 1.44 k cycles of "pointwise" on wave 4 beside 1.54 k on
        // wave 0).  They now go straight on to the next step's poll.
        if (pw_wave) {
        if (t > 0 && !EXT) {
            // unpadded 128-byte rows: a thread's four columns are one aligned ds_read_b128 per partial tile, and the
            // b128 lane groups (rows r, r+1 of column quads 0-3 / 4-7) fall on all 64 banks (conflict-free, like the
            // MFMA lanes' ds_write_b32 of 32 consecutive floats) — 8 LDS instructions instead of 32 on this chain
            const int cj = CW == 2 ? tid >> 8 : 0;
            f32x4 sum = *reinterpret_cast<const f32x4*>(&red[t & 1][0][cj][r * RED_LD4 + cq * 4]);
#pragma unroll
            for (int w_ = 1; w_ < NW; ++w_) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&red[t & 1][w_][cj][r * RED_LD4 + cq * 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[e] = sum[e] + v[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) rec[e] = sum[e];
        }

        // ---- pointwise membrane update for this thread's 4 neurons
        // (Hoisting the rec-independent part of this update in front of the poll was measured: 0.75 -> 0.81 ms
        // per launch — its use of x_t there waits, in order, for the previous step's bulk stores.)
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        f32x4 uo, wo;
        unsigned nib = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xn = neuron_input(xs[e], false, 0.f, has_norm, sc[e], sh[e]);
            neuron_step<ADAPT, true>(u[e], w[e], s[e], xn, rec[e], p[e], a.theta);
            uo[e] = u[e];
            wo[e] = w[e];
            if (valid) nib |= (s[e] != 0.0f ? 1u : 0u) << e;
        }
        // ---- publish this tile's spikes first (it is on every consumer's critical path): one
        //      tagged granule per row; dropout and the bulk stores then overlap the peers' step
        // OR over the 8 lanes of a row with DPP moves (quad xor 1, quad xor 2, then the mirrored half row
        // brings in the other quad) — __shfl_xor would go through the LDS crossbar three times in a row
        unsigned word = nib << (cq * 4);
        word |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)word, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
        word |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)word, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
        word |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)word, 0x141, 0xF, 0xF, true);  // row_half_mirror
        if (EXT) {
            if (valid) {  // the step's raw (pre-dropout) spikes: operand of the caller's s_t @ V product
                *reinterpret_cast<u32x2*>(a.s_step16 + (size_t)bp * H + col) = spike_quad16(s);
            }
        } else if (pw && cq == 0 && t + 1 < (PK ? t_tile : T)) {
            gu64* slot = (gu64*)a.chan + (((size_t)t * a.n_rt_total + rt) * a.n_ct + ct) * 32 + r;
            const u64 granule = ((u64)(unsigned)(t + 1) << 32) | (u64)word;
            if (xcd_local) __hip_atomic_store(slot, granule, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_store(slot, granule, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (NW == 8 && CW == 1) lds_barrier();  // releases the upper waves into the next step's poll (see the else branch)
        PROF_STAMP(3);  // pointwise + publish
        if (valid) {
            const int tt = d ? (T - 1 - t) : t;
            const size_t o_out = (PK ? row0 + t : (size_t)b * T + tt) * HO + (size_t)d * H + colc;
            f32x4 so;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float k = drop ? keep_scale(seed, o_out + e, a.p_drop, a.inv_keep) : 1.0f;
                so[e] = s[e] * k;
                if constexpr (LEN) so[e] = t < len ? so[e] : 0.0f;
                cnt[e] += (so[e] != 0.0f) ? 1u : 0u;
            }
            pend_s = so; pend_u = uo; pend_w = wo;
        }
        } else {
            // ... but not at once: the peers' granules of this step cannot exist before their pointwise phase is
            // over, and sweeps that must fail load the one L2 channel that holds the row tile's granule lines
            // (measured, 40 launches each in one call: polling at once 0.70 ms per launch; 1024 / 1536 / 2048 cycles
            // of s_sleep first 0.665 / 0.646 / 0.72 — past the pointwise phase the upper waves are late themselves;
            // spinning on an LDS word the first wave sets when it has published 0.68: the spin takes issue slots
            // and LDS cycles from the pointwise waves).  So they park in a second barrier that the pointwise waves
            // join right behind their publish store: no instruction issues while a wave waits there, and the
            // wait adapts to the cell kind and the clock.
            lds_barrier();
        }
        pend_t = t;
        PROF_STAMP(4);  // dropout
    }
    flush_pending();
    PROF_FLUSH(0)
    if constexpr (STREAM) {
        if (valid) {  // the state this launch ended in, in place (nobody else reads or writes these elements)
            const size_t o = (size_t)bp * H + col;
            *reinterpret_cast<f32x4*>(const_cast<float*>(a.u0) + o) = f32x4{u[0], u[1], u[2], u[3]};
            *reinterpret_cast<f32x4*>(const_cast<float*>(a.s0) + o) = f32x4{s[0], s[1], s[2], s[3]};
            if (ADAPT) *reinterpret_cast<f32x4*>(const_cast<float*>(a.w0) + o) = f32x4{w[0], w[1], w[2], w[3]};
            if (!EXT) {  // (the step variant has written the plane already)
                *reinterpret_cast<u32x2*>(a.s_step16 + o) = spike_quad16(s);
            }
        }
    }

    // ---- spike counts (post-dropout) -> one integer atomic per (direction, column) per workgroup
    if (a.spike_count) {
        if (valid) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (cnt[e]) atomicAdd(&cnt_lds[d][(CW == 2 ? (tid >> 8) * CT : 0) + cq * 4 + e], cnt[e]);
        }
        __syncthreads();
        if (tid < 2 * CW * CT) {
            const int dd = tid / (CW * CT), c = tid % (CW * CT);
            const unsigned v = cnt_lds[dd][c];
            if (v && dd < a.dirs && ctw * CW * CT + c < H) atomicAdd(a.spike_count + (size_t)dd * H + ctw * CW * CT + c, v);
        }
    }
}

// ------------------------------------------------------------------------------ backward
// NW waves per workgroup, each contracting over its own k-groups (kg = wave + NW*kk) into a partial
// 32 x 32 tile that is summed through LDS.  NW = 8 (two waves per SIMD) whenever there are enough k-groups:
// per step a SIMD has 112 MFMAs, ~770 VALU instructions of splitting and 32 tile loads to issue, and with
// a single wave those queue behind each other (and behind the first load's latency); two waves fill each
// other's stalls.  The pointwise reverse step and the stores stay on the first 256 threads.
// NP: planes of the hand-off tiles and of V^T — 3 = exact split, six cross terms (default); 1 = the bf16 operand
// mode: the producer rounds its dWx once, 2 KB tiles, ONE MFMA per k16-step.
// S16: the saved states u / w are bf16 (common.h save_u16) — a template parameter so that every global load of the
// time loop is ONE unconditional instruction (see `load_step`).
// CW: 32-column groups per workgroup (see rec_fwd_kernel): 2 = the bf16 operand mode's 64-column workgroups, all 512
// threads own pointwise state, the workgroup publishes the tiles of k-groups 2 ctw and 2 ctw + 1.
// The kernel exists as two families with ONE body (rec_bwd_body.inc): rec_bwd_kernel gates with the reference's
// box-car, rec_bwd_sg_kernel with one of the smooth surrogates, chosen by a wave-uniform switch on `sg` (fp32 saves
// only: S16 is never set there).
// ROW_LEN(b) / TAIL_ZERO(t, v): see cell_bwd_body.inc — the ragged family's row length and its select on the incoming
// gradient (a row's recurrent term is its own dWx_{t+1} row times V^T: zero over its tail like the carries).
// ST_PRE_LOAD / ST_POST_LOAD / ST_PLUS / ST_TAIL: the stateful family's (rec_bwd_st_kernel, behind the packed one); empty here.
#define ST_PRE_LOAD
#define ST_POST_LOAD
#define ST_PLUS(v, g) (v)
#define ST_TAIL
#define ROW_PK_INIT
#define T_HI a.t_end
#define T_RING T
#define RROW(r, t) ((size_t)(r) * T + (t))
#define ROW_STORE(t) true
#define ROW_LEN(b) T
#define TAIL_ZERO(t, v) (v)
template <bool ADAPT, int KGW, int NW, bool EXT = false, int NP = 3, bool S16 = false, int CW = 1>
__global__ __launch_bounds__(64 * NW, 1) void rec_bwd_kernel(RecArgs a)
#define SURROGATE_GATE(ds, x) boxcar_gate(ds, x)
#include "rec_bwd_body.inc"
#undef SURROGATE_GATE
template <bool ADAPT, int KGW, int NW, bool EXT = false, int NP = 3, int CW = 1, bool S16 = false>
__global__ __launch_bounds__(64 * NW, 1) void rec_bwd_sg_kernel(RecSgArgs a)
#define SURROGATE_GATE(ds, x) smooth_gate(a.sg.id, a.sg.k, ds, x)
#include "rec_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_LEN
#undef TAIL_ZERO
// the ragged family (sparch_rec_cell_bwd_len): any surrogate, the box-car included, fp32 or bf16 saves
#define ROW_LEN(b) a.lengths[b]
#define TAIL_ZERO(t, v) ((t) < row_len ? (v) : 0.0f)
template <bool ADAPT, int KGW, int NW, bool EXT = false, int NP = 3, bool S16 = false, int CW = 1>
__global__ __launch_bounds__(64 * NW, 1) void rec_bwd_len_kernel(RecLenArgs a)
#define SURROGATE_GATE(ds, x) any_gate(a.sg.id, a.sg.k, ds, x)
#include "rec_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_PK_INIT
#undef T_HI
#undef T_RING
#undef RROW
#undef ROW_STORE
// the packed family (sparch_rec_cell_bwd_pk): the ragged one's length and gradient select, on packed rows
#define ROW_PK_INIT                                   \
    const size_t row0 = (size_t)a.offsets[b];         \
    const int t_tile = __builtin_amdgcn_readfirstlane(a.lengths[min(rt * RT, a.Bp - 1)]);
#define T_HI min(a.t_end, t_tile)
#define T_RING t_tile
#define RROW(r, t) (row0 + (size_t)min((int)(t), row_len - 1))
#define ROW_STORE(t) ((t) < row_len)
template <bool ADAPT, int KGW, int NW, bool EXT = false, int NP = 3, bool S16 = false, int CW = 1>
__global__ __launch_bounds__(64 * NW, 1) void rec_bwd_pk_kernel(RecPkArgs a)
#define SURROGATE_GATE(ds, x) any_gate(a.sg.id, a.sg.k, ds, x)
#include "rec_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_PK_INIT
#undef T_HI
#undef T_RING
#undef RROW
#undef ROW_STORE
#undef ROW_LEN
#undef TAIL_ZERO
#undef ST_PRE_LOAD
#undef ST_POST_LOAD
#undef ST_PLUS
#undef ST_TAIL
// the stateful family (sparch_rec_cell_bwd_st; DESIGN.md section 6, "Stateful training"): the plain family's rows, any
// surrogate, whole-sequence launches, fp32 operands and saves.  The gradient arriving on the final state enters at the
// reverse pass's first step only (two wave-uniform branches with their own loads: the kernel's registers have no room to
// hold twelve values through the loop), the initial state's goes out from the last carries.
#define ROW_PK_INIT
#define T_HI a.t_end
#define T_RING T
#define RROW(r, t) ((size_t)(r) * T + (t))
#define ROW_STORE(t) true
#define ROW_LEN(b) T
#define TAIL_ZERO(t, v) (v)
#define ST_PRE_LOAD                                                                      \
    f32x4 st_s = {0.f, 0.f, 0.f, 0.f}, st_u = st_s;                                      \
    if (t == T - 1) {                                                                    \
        if (a.g_sT) st_s = ld4(a.g_sT + (size_t)bpc * H + colc);                         \
        if (a.g_uT) st_u = ld4(a.g_uT + (size_t)bpc * H + colc);                         \
    }
#define ST_POST_LOAD                                                                     \
    f32x4 st_w = {0.f, 0.f, 0.f, 0.f};                                                   \
    if (ADAPT && t == T - 1 && a.g_wT) st_w = ld4(a.g_wT + (size_t)bpc * H + colc);
#define ST_PLUS(v, g) ((v) + (g))
#define ST_TAIL                                                                          \
    if (a.t_begin == 0) {                                                                \
        const f32x4 t_al = pcol[0][d][cqx], t_be = pcol[1][d][cqx], t_a = pcol[2][d][cqx], t_b = pcol[3][d][cqx]; \
        f32x4 o_u, o_w, o_s;                                                             \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                  \
            o_u[e] = t_al[e] * du_n[e];                                                  \
            o_s[e] = -o_u[e];                                                            \
            o_w[e] = 0.f;                                                                \
            if (ADAPT) {                                                                 \
                o_u[e] = o_u[e] + t_a[e] * dw_n[e];                                      \
                o_s[e] = o_s[e] + t_b[e] * dw_n[e];                                      \
                o_w[e] = t_be[e] * dw_n[e];                                              \
            }                                                                            \
        }                                                                                \
        if (a.g_u0) st4(a.g_u0 + (size_t)bp * H + col, o_u);                             \
        if (ADAPT && a.g_w0) st4(a.g_w0 + (size_t)bp * H + col, o_w);                    \
        if (a.g_s0) st4(a.g_s0 + (size_t)bp * H + col, o_s);                             \
    }
template <bool ADAPT, int KGW, int NW, bool EXT = false, int NP = 3, bool S16 = false, int CW = 1>
__global__ __launch_bounds__(64 * NW, 1) void rec_bwd_st_kernel(RecStArgs a)
#define SURROGATE_GATE(ds, x) any_gate(a.sg.id, a.sg.k, ds, x)
#include "rec_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_PK_INIT
#undef T_HI
#undef T_RING
#undef RROW
#undef ROW_STORE
#undef ROW_LEN
#undef TAIL_ZERO
#undef ST_PRE_LOAD
#undef ST_POST_LOAD
#undef ST_PLUS
#undef ST_TAIL


// ------------------------------------------------------------------ dense recurrent cell (ANN baselines, f-4)
// RNNLayer._rnn_cell (anns.py:328-339): y_t = act(Wx_t + y_{t-1} V^T), y_{-1} = 0, and its reverse pass
//     dpre_t = (g_t + dpre_{t+1} V) * act'(y_t).
// Both directions are the same machine as the spiking backward above: per step a workgroup contracts the
// PREVIOUS step's dense fp32 row tile (handed over through the tagged ring, split exactly into three bf16
// planes by the consumer) with its resident slice of V (six cross terms), then applies a pointwise rule and
// publishes its own 32 x 32 tile.  `s` counts steps in processing order (forward: t = s, backward:
// t = T-1-s); the tile of step s goes to ring slot s % RING (sentinel protocol of the spiking backward).
struct AnnArgs {
    int B, dirs, T, H, Bp;
    int n_ct, nkg, n_rt_total;
    int rt_base, n_rt_launch;
    int s_begin, s_end;
    const float* Wx; const float* scale; const float* shift;
    const u32x4* vpack;
    float p_drop, inv_keep; uint64_t seed;
    float* y_state; float* y_out;                  // forward outputs
    const float* g_out; const float* y_in;         // backward inputs (y_in = the forward's y_state)
    float* dpre; float* y_prev;                    // backward outputs
    char* ring; unsigned* status;
    unsigned* xcd_tab;  // agreement table of the XCD-local stores (whole-sequence launches), or null
    // step variant (EXT): this ONE step's recurrent product comes from the caller (Bp,H); the step's y / dpre
    // also goes to a contiguous (Bp,H) buffer, the operand of the caller's next product
    const float* rec_ext; float* step_out;
};

__device__ __forceinline__ float ann_act(int kind, float v) {
    if (kind == SPARCH_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    if (kind == SPARCH_ACT_RELU) return v <= 0.0f ? 0.0f : v;  // a NaN stays a NaN (torch.relu); fmaxf would return 0
    return tanhf(v);
}
__device__ __forceinline__ float ann_dact(int kind, float a) {  // through the activation's output
    if (kind == SPARCH_ACT_SIGMOID) return a * (1.0f - a);
    if (kind == SPARCH_ACT_RELU) return a > 0.0f ? 1.0f : 0.0f;
    return 1.0f - a * a;
}

template <int ACT, bool BWD, int KGW, int NW, bool EXT = false>
__global__ __launch_bounds__(64 * NW, 1) void ann_rec_kernel(AnnArgs a) {
    __shared__ __attribute__((aligned(16))) float red[2][NW][RT * RED_LD];
    __shared__ __attribute__((aligned(16))) u32x4 vlo[NW][KGW][2][64];
    __shared__ int abort_flag[2];
    __shared__ int xcd_local_flag;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rt = a.rt_base + (int)(blockIdx.x % a.n_rt_launch);
    const int ct = (int)(blockIdx.x / a.n_rt_launch);
    const int T = a.T, H = a.H, HO = a.H * a.dirs;

    const bool pw = tid < 256;
    const int r = (tid & 255) >> 3, cq = tid & 7;
    const int bp = rt * RT + r, col = ct * CT + cq * 4;
    const bool valid = pw && bp < a.Bp && col < H;
    const int bpc = min(bp, a.Bp - 1), colc = min(col, H - 4);
    const int d = bpc / a.B, b = bpc - d * a.B;

    u32x4 vb[KGW][2][2];
    if (!EXT) load_slice32<KGW, NW>(vb, vlo[wave], a.vpack, ct, a.nkg, wave, lane);
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (!BWD && a.scale) { sc = ld4(a.scale + colc); sh = ld4(a.shift + colc); }
    if (tid < 2) abort_flag[tid] = 0;
    const unsigned my_xcc = xcc_id();
    xcd_agree((EXT || !a.xcd_tab) ? nullptr : (gu32*)a.xcd_tab + (size_t)rt * a.n_ct, SENTINEL, a.n_ct, ct, my_xcc, tid, &xcd_local_flag);
    __syncthreads();
    const bool xcd_local = xcd_local_flag != 0;  // this row tile's workgroups share an XCD: plain hand-off stores

    // hand-off tiles as pre-split bf16 planes (6 KB), as in the spiking backward
    const unsigned slot_bytes = (unsigned)((size_t)a.n_rt_total * a.n_ct * PTILE_BYTES);
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(a.ring, 0, (int)(RING * slot_bytes), 0x00020000);
    const unsigned rt_off = (unsigned)((size_t)rt * a.n_ct * PTILE_BYTES);
    const bool drop = a.p_drop > 0.0f;
    const uint64_t seed = drop ? resolve_seed(a.seed) : 0;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // per-step operands of the pointwise rule: forward x = Wx[b, tt]; backward g = g_out[b, tt, d*H..],
    // y_t and y_{t-1} of this row in cell time
    auto load_step = [&](int s, f32x4& v0, f32x4& v1, f32x4& v2) {
        const int t = BWD ? (T - 1 - s) : s;
        const int tt = d ? (T - 1 - t) : t;
        if (!BWD) {
            v0 = ld4(a.Wx + ((size_t)b * T + tt) * H + colc);
        } else {
            v0 = ld4(a.g_out + ((size_t)b * T + tt) * HO + (size_t)d * H + colc);
            v1 = ld4(a.y_in + ((size_t)bpc * T + t) * H + colc);
            v2 = t > 0 ? ld4(a.y_in + ((size_t)bpc * T + (t - 1)) * H + colc) : zero4;
        }
    };
    f32x4 n0 = zero4, n1 = zero4, n2 = zero4;
    if (pw) load_step(a.s_begin, n0, n1, n2);

    for (int s = a.s_begin; s < a.s_end; ++s) {
        const f32x4 c0 = n0, c1 = n1, c2 = n2;
        float rec[4] = {0.f, 0.f, 0.f, 0.f};
        const int par = s & 1;
        if (pw && s + 1 < a.s_end) load_step(s + 1, n0, n1, n2);

        if (s > 0 && !EXT)
            ring_product32<KGW, NW, 3>(vb, vlo[wave], rsrc, (unsigned)((s - 1) % RING) * slot_bytes + rt_off + (unsigned)lane * 16u,
                                       a.n_ct, wave, lane, &abort_flag[par], red[par][wave]);
        lds_barrier();
        vm_settled();
        if (lds_flag_read(&abort_flag[par])) break;
        if (s > 0 && EXT) {
            const f32x4 v = ld4(a.rec_ext + (size_t)bpc * H + colc);
            rec[0] = v.x; rec[1] = v.y; rec[2] = v.z; rec[3] = v.w;
        } else if (s > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) rec[e] = wave_sum(red[par], r * RED_LD + cq * 4 + e);
        }

        // ---- pointwise rule
        const int t = BWD ? (T - 1 - s) : s;
        const int tt = d ? (T - 1 - t) : t;
        const size_t o_out = ((size_t)b * T + tt) * HO + (size_t)d * H + colc;
        f32x4 val, aux;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float k = drop ? keep_scale(seed, o_out + e, a.p_drop, a.inv_keep) : 1.0f;
            if (!BWD) {
                float xn = c0[e];
                if (a.scale) xn = bn_affine(xn, sc[e], sh[e]);
                const float y = ann_act(ACT, xn + rec[e]);                      // anns.py:336
                val[e] = valid ? y : 0.0f;
                aux[e] = y * k;                                                 // dropout after the cell (323-324)
            } else {
                const float dp = (c0[e] * k + rec[e]) * ann_dact(ACT, c1[e]);
                val[e] = valid ? dp : 0.0f;
                aux[e] = c2[e];
            }
        }
        // ---- publish this step's tile as planes (fragment order; the last step's has no reader): a thread's 4
        //      columns are half a 16-byte piece per plane
        if (EXT) {
            if (valid) st4(a.step_out + (size_t)bp * H + col, val);
        } else if (pw) {
            const unsigned piece = (unsigned)(((cq >> 2) * 3 * 64 + ((cq >> 1) & 1) * 32 + r) * 16 + (cq & 1) * 8);
            publish_planes(rsrc, slot_bytes, rt_off + (unsigned)ct * PTILE_BYTES + piece, s, s + 1 < T, val, xcd_local);
        }
        lds_barrier();
        // ---- off the critical path: outputs
        if (valid) {
            if (!BWD) {
                st4(a.y_state + ((size_t)bp * T + t) * H + col, val);
                st4(a.y_out + ((size_t)b * T + tt) * HO + (size_t)d * H + col, aux);
            } else {
                st4(a.dpre + ((size_t)bp * T + tt) * H + col, val);
                st4(a.y_prev + ((size_t)bp * T + tt) * H + col, aux);
            }
        }
    }
    raise_if_aborted(abort_flag, a.status, BWD ? SPARCH_STATUS_ANN_REC_BWD : SPARCH_STATUS_ANN_REC_FWD, tid);
}

// ------------------------------------------------------------------------------ V prepack
// vpack[ct][kg][ks][p][lane] = 8 bf16 (16 B): plane p (0 hi, 1 mid, 2 lo) of Vm[k][col] (forward) or
// Vm[col][k] (backward) for k = kg*32 + 16*ks + 8*(lane>>5) + j, j = 0..7, col = ct*32 + (lane&31);
// Vm = V with a zero diagonal, zero padded.  This is the B-operand fragment of v_mfma_f32_32x32x16_bf16.
__global__ void vpack_kernel(int H, int n_ct, int nkg, int transpose, int rne, const float* __restrict__ V,
                             u32x4* __restrict__ vpack) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)n_ct * nkg * 2 * 64;
    if (idx >= total) return;
    const int lane = (int)(idx & 63), ks = (int)((idx >> 6) & 1);
    const int kg = (int)((idx >> 7) % nkg), ct = (int)((idx >> 7) / nkg);
    const int col = ct * 32 + (lane & 31);
    const bool tr = transpose & 1, keep_diag = transpose & 2;  // bit 1: dense matrix of an ANN cell, no mask
    unsigned short pl[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = kg * 32 + 16 * ks + 8 * (lane >> 5) + j;
        float v = 0.f;
        if (k < H && col < H && (keep_diag || k != col)) v = tr ? V[(size_t)col * H + k] : V[(size_t)k * H + col];
        vsplit(v, rne, pl[0][j], pl[1][j], pl[2][j]);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (unsigned)pl[p][2 * q] | ((unsigned)pl[p][2 * q + 1] << 16);
        vpack[((((size_t)ct * nkg + kg) * 2 + ks) * 3 + p) * 64 + lane] = o;
    }
}
// forward fragments, backward (transposed) fragments and the masked copy of a spiking layer's V in ONE launch (a
// training step needs all three; three launches were ~25 us of launch + queue gaps per layer)
__global__ void vpack_both_kernel(int H, int n_ct, int nkg, int rne, const float* __restrict__ V, u32x4* __restrict__ vpack_f,
                                  u32x4* __restrict__ vpack_b, float* __restrict__ Vm) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)n_ct * nkg * 2 * 64;
    if (idx < total) {
        const int lane = (int)(idx & 63), ks = (int)((idx >> 6) & 1);
        const int kg = (int)((idx >> 7) % nkg), ct = (int)((idx >> 7) / nkg);
        const int col = ct * 32 + (lane & 31);
        unsigned short pf[3][8], pb[3][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = kg * 32 + 16 * ks + 8 * (lane >> 5) + j;
            const bool in = k < H && col < H && k != col;
            vsplit(in ? V[(size_t)k * H + col] : 0.f, rne, pf[0][j], pf[1][j], pf[2][j]);
            vsplit(in ? V[(size_t)col * H + k] : 0.f, rne, pb[0][j], pb[1][j], pb[2][j]);
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            u32x4 of, ob;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                of[q] = (unsigned)pf[p][2 * q] | ((unsigned)pf[p][2 * q + 1] << 16);
                ob[q] = (unsigned)pb[p][2 * q] | ((unsigned)pb[p][2 * q + 1] << 16);
            }
            const size_t o = ((((size_t)ct * nkg + kg) * 2 + ks) * 3 + p) * 64 + lane;
            vpack_f[o] = of;
            vpack_b[o] = ob;
        }
    }
    if (Vm) {
        const size_t n = (size_t)H * H, stride = (size_t)gridDim.x * blockDim.x;
        for (size_t e = idx; e < n; e += stride) {
            const int i = (int)(e / H), j = (int)(e % H);
            Vm[e] = (i == j) ? 0.f : V[e];
        }
    }
}
__global__ void vmask_kernel(int H, const float* __restrict__ V, float* __restrict__ Vm) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)H * H) return;
    const int i = (int)(idx / H), j = (int)(idx % H);
    Vm[idx] = (i == j) ? 0.f : V[idx];
}

int pick_kgw(int H) {
    const int need = cdiv(cdiv(H, 32), 4);
    for (int k : {1, 2, 4, 8})
        if (need <= k) return k;
    return 0;  // H > 1024: V slice no longer fits the register file in this layout
}

size_t fwd_chan_bytes(int Bp, int T, int H) {
    return (size_t)T * cdiv(Bp, RT) * cdiv(H, CT) * 32 * sizeof(u64);
}
size_t bwd_ring_bytes(int Bp, int H) {  // dense fp32 tiles (the RNN cell)
    return (size_t)RING * cdiv(Bp, RT) * cdiv(H, CT) * TILE_BYTES;
}
size_t bwd_pring_bytes(int Bp, int H) {  // pre-split plane tiles (the spiking backward)
    return (size_t)RING * cdiv(Bp, RT) * cdiv(H, CT) * PTILE_BYTES;
}
// agreement table of the XCD-local stores: one word per workgroup, behind the granules / the ring
size_t xcd_tab_bytes(int Bp, int H) { return (size_t)cdiv(Bp, RT) * cdiv(H, CT) * sizeof(unsigned); }
int g_xcd_local = -1;  // -1: SPARCH_XCD_LOCAL (default on); 0 / 1: set by sparch_set_xcd_local
bool xcd_local_enabled() {
    static const bool env_on = [] { const char* e = getenv("SPARCH_XCD_LOCAL"); return !e || atoi(e) != 0; }();
    return g_xcd_local < 0 ? env_on : g_xcd_local != 0;
}

// ---- the kernel tables: the ONE mapping from what a call asks for to the instantiation that runs it.  Launching and
// the co-residency question both go through it, so the question is asked of the kernel that is launched.
using RecKernel = KernelRef<RecArgs>;
using AnnKernel = KernelRef<AnnArgs>;
using rec_plan::rec_kb;
using rec_plan::rec_nw;

// NP = 1: the bf16 operand mode (sparch_set_operand_precision) — the V pack then holds one rounded plane
// STREAM: the streaming forward's instantiations (state in / out, no saves; 32-column workgroups only)
// CW = 2: 64-column workgroups (bf16 operand mode, not streaming, the 8-wave kernels: kgw >= 2)
// S16: the backward that reads bf16 saved states (the forward takes a.save16 at run time)
// SG: the backward with a smooth surrogate (rec_bwd_sg_kernel, RecSgArgs): one row per fp32-save backward row
using RecSgKernel = KernelRef<RecSgArgs>;
template <bool SG> using RecKernelOf = std::conditional_t<SG, RecSgKernel, RecKernel>;
template <bool BWD, bool ADAPT, int NP, bool STREAM, int K, int CW, bool S16, bool SG>
constexpr RecKernelOf<SG> rec_kernel_of() {
    constexpr int KB = rec_kb(K), NW = rec_nw(K);
    if constexpr (SG) return kernel_with_occupancy<RecSgArgs, rec_bwd_sg_kernel<ADAPT, KB, NW, false, NP, CW>, 64 * NW>();
    else if constexpr (BWD) return kernel_with_occupancy<RecArgs, rec_bwd_kernel<ADAPT, KB, NW, false, NP, S16, CW>, 64 * NW>();
    else return kernel_with_occupancy<RecArgs, rec_fwd_kernel<ADAPT, KB, NW, false, NP, CW, STREAM>, 64 * NW>();
}
template <bool BWD, bool STREAM = false, bool SG = false>
RecKernelOf<SG> rec_kernel(bool adapt, bool low, int kgw, int cw, bool save16) {
    static_assert(!(BWD && STREAM), "streaming is forward-only");
    static_assert(!SG || BWD, "the surrogate is the backward's");
    return rec_plan::with_kgw(kgw, [&](auto k) {
        return rec_plan::with_bool(adapt, [&](auto ad) {
            return rec_plan::with_bool(BWD && !SG && save16, [&](auto s16) -> RecKernelOf<SG> {
                constexpr int K = decltype(k)::value;
                constexpr bool A = decltype(ad)::value, S16 = BWD && !SG && decltype(s16)::value;
                if (!low) return rec_kernel_of<BWD, A, 3, STREAM, K, 1, S16, SG>();
                if constexpr (!STREAM && K >= 2)
                    if (cw == 2) return rec_kernel_of<BWD, A, 1, false, K, 2, S16, SG>();
                return rec_kernel_of<BWD, A, 1, STREAM, K, 1, S16, SG>();
            });
        });
    });
}
// the ragged kernels (RecLenArgs): the persistent forward with LEN, and the one backward family of every surrogate;
// PK: their packed forms (RecPkArgs)
template <bool PK> using RecLenArgsOf = std::conditional_t<PK, RecPkArgs, RecLenArgs>;
template <bool PK> using RecLenKernelOf = KernelRef<RecLenArgsOf<PK>>;
using RecLenKernel = RecLenKernelOf<false>;
template <bool BWD, bool PK = false>
RecLenKernelOf<PK> rec_len_kernel(bool adapt, bool low, int kgw, int cw, bool save16) {
    return rec_plan::with_kgw(kgw, [&](auto k) {
        return rec_plan::with_bool(adapt, [&](auto ad) {
            return rec_plan::with_bool(BWD && save16, [&](auto s16) -> RecLenKernelOf<PK> {
                constexpr int K = decltype(k)::value, KB = rec_kb(K), NW = rec_nw(K);
                constexpr bool A = decltype(ad)::value, S16 = decltype(s16)::value;
                auto of = [](auto np, auto cwc) -> RecLenKernelOf<PK> {
                    constexpr int NP = decltype(np)::value, CW = decltype(cwc)::value;
                    if constexpr (BWD && PK) return kernel_with_occupancy<RecPkArgs, rec_bwd_pk_kernel<A, KB, NW, false, NP, S16, CW>, 64 * NW>();
                    else if constexpr (PK) return kernel_with_occupancy<RecPkArgs, rec_fwd_kernel<A, KB, NW, false, NP, CW, false, true, true>, 64 * NW>();
                    else if constexpr (BWD) return kernel_with_occupancy<RecLenArgs, rec_bwd_len_kernel<A, KB, NW, false, NP, S16, CW>, 64 * NW>();
                    else return kernel_with_occupancy<RecLenArgs, rec_fwd_kernel<A, KB, NW, false, NP, CW, false, true>, 64 * NW>();
                };
                using rec_plan::kgw_c;
                if (!low) return of(kgw_c<3>{}, kgw_c<1>{});
                if constexpr (K >= 2)
                    if (cw == 2) return of(kgw_c<1>{}, kgw_c<2>{});
                return of(kgw_c<1>{}, kgw_c<1>{});
            });
        });
    });
}
template <bool PK = false>
RecLenArgsOf<PK> with_lengths(const RecArgs& a, const SurrogateArgs sg, const int* lengths, const int* offsets = nullptr) {
    RecLenArgsOf<PK> g;
    static_cast<RecArgs&>(g) = a;
    g.sg = sg;
    g.lengths = lengths;
    if constexpr (PK) g.offsets = offsets;
    return g;
}
// the stateful backward kernels (RecStArgs): fp32 operands, fp32 saves, 32-column workgroups, any surrogate
using RecStKernel = KernelRef<RecStArgs>;
RecStKernel rec_st_kernel(bool adapt, int kgw) {
    return rec_plan::with_kgw(kgw, [&](auto k) {
        return rec_plan::with_bool(adapt, [&](auto ad) -> RecStKernel {
            constexpr int K = decltype(k)::value, KB = rec_kb(K), NW = rec_nw(K);
            return kernel_with_occupancy<RecStArgs, rec_bwd_st_kernel<decltype(ad)::value, KB, NW, false, 3, false, 1>, 64 * NW>();
        });
    });
}
// the step variants (EXT): the recurrent product comes from the caller, one k-group class, no hand-off
template <bool BWD, bool STREAM = false>
RecKernel rec_step_kernel(bool adapt) {
    constexpr int KB = rec_kb(1), NW = rec_nw(1);
    return rec_plan::with_bool(adapt, [](auto ad) -> RecKernel {
        constexpr bool A = decltype(ad)::value;
        if constexpr (BWD) return {rec_bwd_kernel<A, KB, NW, true>, 64 * NW};
        else return {rec_fwd_kernel<A, KB, NW, true, 3, 1, STREAM>, 64 * NW};
    });
}
RecSgKernel rec_step_sg_kernel(bool adapt) {
    constexpr int KB = rec_kb(1), NW = rec_nw(1);
    return rec_plan::with_bool(adapt, [](auto ad) -> RecSgKernel {
        return {rec_bwd_sg_kernel<decltype(ad)::value, KB, NW, true>, 64 * NW};
    });
}
RecSgArgs with_surrogate(const RecArgs& a, const SurrogateArgs sg) {
    RecSgArgs g;
    static_cast<RecArgs&>(g) = a;
    g.sg = sg;
    return g;
}
// dense cell; EXT: its step variant (kgw = 1 only).  An unknown activation or kgw has no kernel.
template <bool BWD, bool EXT = false>
AnnKernel ann_kernel(int act, int kgw) {
    return rec_plan::with_kgw(kgw, [&](auto k) -> AnnKernel {
        constexpr int K = decltype(k)::value, KB = rec_kb(K), NW = rec_nw(K);
        if constexpr (EXT && K != 1) return {};
        else switch (act) {
            case SPARCH_ACT_SIGMOID: return {ann_rec_kernel<SPARCH_ACT_SIGMOID, BWD, KB, NW, EXT>, 64 * NW};
            case SPARCH_ACT_RELU: return {ann_rec_kernel<SPARCH_ACT_RELU, BWD, KB, NW, EXT>, 64 * NW};
            case SPARCH_ACT_TANH: return {ann_rec_kernel<SPARCH_ACT_TANH, BWD, KB, NW, EXT>, 64 * NW};
            default: return {};
        }
    });
}

// ---- one pass of the persistent kernels: size and check the workspace, clear it, plan and walk (rec_plan.h)
// SG (backward): `sg` names a smooth surrogate and the pass runs on the rec_bwd_sg_kernel rows of the table
// lengths (not null): the ragged pass, on the rec_len_kernel table (`sg` is then any surrogate); PK: its packed form
// (offsets not null), whole-sequence launches only
// ST (backward): the stateful pass, on the rec_st_kernel table (`sg` is any surrogate, `stx` the six state-gradient
// pointers), whole-sequence launches only
template <bool BWD, bool STREAM = false, bool SG = false, bool LEN = false, bool PK = false, bool ST = false>
int run_rec(int kind, RecArgs& a, size_t chan_bytes, int steps_per_launch, hipStream_t st, const SurrogateArgs sg = {},
            const int* lengths = nullptr, const int* offsets = nullptr, const RecStArgs* stx = nullptr) {
    static_assert(!LEN || (!STREAM && !SG), "the ragged pass has its own table");
    static_assert(!PK || LEN, "the packed pass is a ragged one");
    static_assert(!ST || (BWD && !STREAM && !SG && !LEN), "the stateful pass has its own table");
    if ((PK || ST) && steps_per_launch < a.T) return SPARCH_EINVAL;
    const bool adapt = kind == SPARCH_KIND_RADLIF;
    const bool low = sparch_operand_bf16() != 0;  // the V pack must have been made in the same mode
    const int kgw = pick_kgw(a.H);
    if (kgw == 0) return SPARCH_EINVAL;
    a.n_ct = cdiv(a.H, CT);
    a.nkg = 4 * kgw;
    a.n_rt_total = cdiv(a.Bp, RT);
    if (!a.chan || chan_bytes < sparch_rec_chan_bytes(a.Bp, a.T, a.H)) return SPARCH_EWORKSPACE;
    // forward: zeroed granules; backward: every ring piece reads "not written yet" until its producer's store lands.
    // The agreement table of the XCD-local stores sits behind either and is cleared with it.
    const size_t hb = BWD ? bwd_pring_bytes(a.Bp, a.H) : fwd_chan_bytes(a.Bp, a.T, a.H);
    if (int rc = clear_handoff(a.chan, BWD ? SENTINEL : 0u, hb + xcd_tab_bytes(a.Bp, a.H), st)) return rc;
    if (BWD) a.ring = reinterpret_cast<char*>(a.chan);

    static const int cw_env = [] { const char* e = getenv("SPARCH_REC_CW"); return e ? atoi(e) : 0; }();
    rec_plan::Policy pol;
    pol.ask_occupancy = true;
    pol.refuse_degrade = (a.save16 && !BWD) || PK || ST;  // bf16 saves need the whole-sequence forward launch; so do packed rows and the stateful pass
    pol.has_cw2 = !STREAM && low && kgw >= 2;
    pol.cw_override = cw_env;
    const int cus = sparch_device_cus();
    const rec_plan::Plan q = rec_plan::make_plan(a.n_rt_total, a.T, a.n_ct, steps_per_launch, cus, pol, [&](unsigned grid, int cw) {
        if constexpr (ST) return co_resident(rec_st_kernel(adapt, kgw), grid, cus);
        else if constexpr (LEN) return co_resident(rec_len_kernel<BWD, PK>(adapt, low, kgw, cw, a.save16 != 0), grid, cus);
        else return co_resident(rec_kernel<BWD, STREAM, SG>(adapt, low, kgw, cw, a.save16 != 0), grid, cus);
    });
    if (!q.ok) return SPARCH_EINVAL;
    // whole-sequence launches only (one agreement per launch)
    a.xcd_tab = q.whole && xcd_local_enabled() ? reinterpret_cast<unsigned*>(reinterpret_cast<char*>(a.chan) + hb) : nullptr;
    if constexpr (ST) {
        if (!q.whole || q.cw != 1 || low) return SPARCH_EINVAL;
        const RecStKernel k = rec_st_kernel(adapt, kgw);
        return rec_plan::walk(q, true, [&](int rt0, int n_rt, int t0, int t1) {
            a.rt_base = rt0; a.n_rt_launch = n_rt; a.t_begin = t0; a.t_end = t1;
            RecStArgs g = *stx;
            static_cast<RecArgs&>(g) = a;
            g.sg = sg;
            return launch_kernel(k, (unsigned)(q.wg_per_rt * n_rt), g, st);
        });
    }
    if constexpr (LEN) {
        if (PK && !q.whole) return SPARCH_EINVAL;
        const RecLenKernelOf<PK> k = rec_len_kernel<BWD, PK>(adapt, low, kgw, q.cw, a.save16 != 0);
        return rec_plan::walk(q, BWD, [&](int rt0, int n_rt, int t0, int t1) {
            a.rt_base = rt0; a.n_rt_launch = n_rt; a.t_begin = t0; a.t_end = t1;
            return launch_kernel(k, (unsigned)(q.wg_per_rt * n_rt), with_lengths<PK>(a, sg, lengths, offsets), st);
        });
    }
    const RecKernelOf<SG> k = rec_kernel<BWD, STREAM, SG>(adapt, low, kgw, q.cw, a.save16 != 0);
    return rec_plan::walk(q, BWD, [&](int rt0, int n_rt, int t0, int t1) {
        a.rt_base = rt0; a.n_rt_launch = n_rt; a.t_begin = t0; a.t_end = t1;
        if constexpr (SG) return launch_kernel(k, (unsigned)(q.wg_per_rt * n_rt), with_surrogate(a, sg), st);
        else return launch_kernel(k, (unsigned)(q.wg_per_rt * n_rt), a, st);
    });
}

template <bool BWD>
int run_ann(int act, AnnArgs& a, void* chan, size_t chan_bytes, int steps_per_launch, hipStream_t st) {
    const int kgw = pick_kgw(a.H);
    const AnnKernel k = ann_kernel<BWD>(act, kgw);
    if (!k.fn) return SPARCH_EINVAL;
    a.n_ct = cdiv(a.H, CT);
    a.nkg = 4 * kgw;
    a.n_rt_total = cdiv(a.Bp, RT);
    if (!chan || chan_bytes < sparch_rec_chan_bytes(a.Bp, a.T, a.H)) return SPARCH_EWORKSPACE;
    const size_t rb = bwd_pring_bytes(a.Bp, a.H);  // plane tiles, the agreement table behind them
    if (int rc = clear_handoff(chan, SENTINEL, rb + xcd_tab_bytes(a.Bp, a.H), st)) return rc;
    a.ring = reinterpret_cast<char*>(chan);
    rec_plan::Policy pol;
    pol.whole_before_degrade = true;
    const rec_plan::Plan q = rec_plan::make_plan(a.n_rt_total, a.T, a.n_ct, steps_per_launch, sparch_device_cus(), pol);
    a.xcd_tab = q.whole && xcd_local_enabled() ? reinterpret_cast<unsigned*>(a.ring + rb) : nullptr;  // whole-sequence launches only
    return rec_plan::walk(q, false, [&](int rt0, int n_rt, int s0, int s1) {
        a.rt_base = rt0; a.n_rt_launch = n_rt; a.s_begin = s0; a.s_end = s1;
        return launch_kernel(k, (unsigned)(q.wg_per_rt * n_rt), a, st);
    });
}

// ---- what the entry points share.  Every SPARCH_EINVAL check of an entry comes before its SPARCH_EALIGN check.
bool rec_shape_ok(int kind, int B, int dirs, int T, int H, int t = 0) {  // H % 4: the kernels move four columns at a time
    return (kind == SPARCH_KIND_RLIF || kind == SPARCH_KIND_RADLIF) && shape_ok(B, dirs, T, H, 4) && t >= 0 && t < T;
}
// a stream is causal (one direction) and runs in eval (no dropout)
bool stream_ok(int dirs, float p_drop) { return dirs == 1 && p_drop == 0.0f; }
// what only the adaptive kind reads
bool adapt_set(int kind, std::initializer_list<const void*> ps) { return kind != SPARCH_KIND_RADLIF || all_set(ps); }
// BatchNorm backward folded in: all three or none, and 16-byte aligned (a misaligned one is refused like a missing one)
bool bn_ok(const float* bn_x, const float* bn_mean, const float* bn_invstd) {
    return !bn_x || (bn_mean && bn_invstd && al16({bn_x, bn_mean, bn_invstd}));
}
bool act_ok(int act) { return act == SPARCH_ACT_SIGMOID || act == SPARCH_ACT_RELU || act == SPARCH_ACT_TANH; }

// shape, neuron parameters and the state a pass starts from
RecArgs rec_args(int B, int dirs, int T, int H, const float* alpha, const float* beta, const float* a, const float* b,
                 const float* u0, const float* w0, const float* s0, float theta, float p_drop, uint64_t seed) {
    RecArgs r = base_args<RecArgs>(B, dirs, T, H, p_drop, seed);
    r.alpha = alpha; r.beta = beta; r.a = a; r.b = b; r.u0 = u0; r.w0 = w0; r.s0 = s0; r.theta = theta;
    return r;
}
void rec_fwd_io(RecArgs& r, const float* Wx, const float* scale, const float* shift, const float* rec0, float* s_out,
                uint16_t* s16_out, uint32_t* spike_count) {
    r.Wx = Wx; r.scale = scale; r.shift = shift; r.rec0 = rec0;
    r.s_out = s_out; r.s16_out = s16_out; r.spike_count = spike_count;
}
void rec_bwd_io(RecArgs& r, const float* g_out, const float* g_rate, const void* u_save, const void* w_save, float* dWx,
                uint16_t* s_prev16, float* dparam_ws, const float* bn_x, const float* bn_mean, const float* bn_invstd) {
    r.g_out = g_out; r.g_rate = g_rate; r.g_rate_scale = 1.0f / ((float)r.B * (float)r.T);
    r.u_save = (float*)const_cast<void*>(u_save); r.w_save = (float*)const_cast<void*>(w_save);
    r.dWx = dWx; r.s_prev16 = s_prev16; r.dparam_ws = dparam_ws;
    r.bn_x = bn_x; r.bn_mean = bn_mean; r.bn_invstd = bn_invstd; r.bn_src = bn_x ? bn_x : g_out;
}
// one step [t, t + 1) over all row tiles
int rec_step_launch(const RecKernel& k, RecArgs& r, int t, void* stream) {
    const unsigned grid = step_geometry(r);
    r.t_begin = t; r.t_end = t + 1;
    return launch_kernel(k, grid, r, (hipStream_t)stream);
}
int rec_step_launch(const RecSgKernel& k, RecArgs& r, const SurrogateArgs sg, int t, void* stream) {
    const unsigned grid = step_geometry(r);
    r.t_begin = t; r.t_end = t + 1;
    return launch_kernel(k, grid, with_surrogate(r, sg), (hipStream_t)stream);
}
int ann_step_launch(const AnnKernel& k, AnnArgs& a, int s, const float* rec, float* step_out, void* stream) {
    const unsigned grid = step_geometry(a);
    a.s_begin = s; a.s_end = s + 1; a.rec_ext = rec; a.step_out = step_out;
    return launch_kernel(k, grid, a, (hipStream_t)stream);
}

}  // namespace

#ifdef SPARCH_REC_PROF
extern "C" int sparch_rec_prof_read(unsigned long long* host_out, int reset) {
    static unsigned long long zero[2 * 512 * 12];
    if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_rec_prof), sizeof(zero)) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_rec_prof), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#endif

extern "C" size_t sparch_vpack_bytes(int H) {
    const int kgw = pick_kgw(H);
    if (H <= 0 || kgw == 0) return 0;
    return (size_t)cdiv(H, CT) * (4 * kgw) * 2 * 3 * 64 * sizeof(u32x4);
}

extern "C" int sparch_vpack(int H, const float* V, int transpose, float* vpack, float* vmasked, void* stream, int precision) {
    SPARCH_ENTER();
    PrecisionScope prec_scope_(precision);
    if (!prec_scope_.ok) return SPARCH_EINVAL;
    const int kgw = pick_kgw(H);
    if (H <= 0 || kgw == 0 || !V || !vpack) return SPARCH_EINVAL;
    if (!aligned16(vpack)) return SPARCH_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int n_ct = cdiv(H, CT), nkg = 4 * kgw;
    const size_t total = (size_t)n_ct * nkg * 2 * 64;
    hipLaunchKernelGGL(vpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, H, n_ct, nkg,
                       transpose, sparch_operand_bf16(), V, reinterpret_cast<u32x4*>(vpack));
    SPARCH_CHECK_LAUNCH();
    if (vmasked) {
        const size_t n = (size_t)H * H;
        hipLaunchKernelGGL(vmask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, H, V, vmasked);
        SPARCH_CHECK_LAUNCH();
    }
    return SPARCH_OK;
}

extern "C" int sparch_vpack_both(int H, const float* V, float* vpack_fwd, float* vpack_bwd, float* vmasked, void* stream, int precision) {
    SPARCH_ENTER();
    PrecisionScope prec_scope_(precision);
    if (!prec_scope_.ok) return SPARCH_EINVAL;
    const int kgw = pick_kgw(H);
    if (H <= 0 || kgw == 0 || !V || !vpack_fwd || !vpack_bwd) return SPARCH_EINVAL;
    if (!aligned16(vpack_fwd) || !aligned16(vpack_bwd)) return SPARCH_EALIGN;
    const int n_ct = cdiv(H, CT), nkg = 4 * kgw;
    const size_t total = (size_t)n_ct * nkg * 2 * 64;
    hipLaunchKernelGGL(vpack_both_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, H, n_ct,
                       nkg, sparch_operand_bf16(), V, reinterpret_cast<u32x4*>(vpack_fwd), reinterpret_cast<u32x4*>(vpack_bwd), vmasked);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_set_xcd_local(int on) {
    const int was = xcd_local_enabled() ? 1 : 0;
    g_xcd_local = on < 0 ? -1 : (on != 0);
    return was;
}

extern "C" int sparch_vmask(int H, const float* V, float* vmasked, void* stream) {
    SPARCH_ENTER();
    if (H <= 0 || !V || !vmasked) return SPARCH_EINVAL;
    const size_t n = (size_t)H * H;
    hipLaunchKernelGGL(vmask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, H, V, vmasked);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" size_t sparch_rec_chan_bytes(int Bp, int T, int H) {
    if (Bp <= 0 || T <= 0 || H <= 0) return 0;
    // forward: T x row tiles x column tiles x 32 granules of 8 B; backward: fp32 tile ring
    const size_t f = fwd_chan_bytes(Bp, T, H), b = bwd_pring_bytes(Bp, H);
    // rounded up to 16 bytes: the agreement table is 4 bytes per workgroup, and a caller that sizes its buffer in
    // 8-byte words (round 2: `nbytes // 8` in the Python host) must not come out 4 bytes short of the table's
    // last word when the number of workgroups is odd
    return ((f > b ? f : b) + xcd_tab_bytes(Bp, H) + 15) & ~(size_t)15;
}

namespace {
// sparch_rec_cell_fwd and sparch_rec_cell_fwd_len (lengths not null, checked by the caller)
int rec_cell_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                                   const float* scale, const float* shift, const float* alpha,
                                   const float* beta, const float* a, const float* b,
                                   const float* vpack, const float* rec0, const float* u0,
                                   const float* w0, const float* s0, float theta, float p_drop,
                                   uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                                   int save_bf16, uint32_t* spike_count, void* chan, size_t chan_bytes,
                                   uint32_t* status, int steps_per_launch, void* stream, int precision,
                                   const int* lengths, const int* offsets = nullptr) {
    PrecisionScope prec_scope_(precision);
    if (!prec_scope_.ok) return SPARCH_EINVAL;
    // bf16 saved states cannot carry the exact state from one launch of a chunked forward to the next
    if (save_bf16 && steps_per_launch < T) return SPARCH_EINVAL;
    if (!rec_shape_ok(kind, B, dirs, T, H) || !all_set({Wx, alpha, vpack, rec0, u0, s0, u_save, status}) ||
        (!s_out && !s16_out) || !adapt_set(kind, {beta, a, b, w0, w_save}) || !paired(scale, shift) || !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({Wx, vpack, rec0, u0, w0, s0, s_out, s16_out, u_save, w_save, chan})) return SPARCH_EALIGN;
    RecArgs r = rec_args(B, dirs, T, H, alpha, beta, a, b, u0, w0, s0, theta, p_drop, seed);
    rec_fwd_io(r, Wx, scale, shift, rec0, s_out, s16_out, spike_count);
    r.vpack = reinterpret_cast<const u32x4*>(vpack);
    r.u_save = (float*)u_save; r.w_save = (float*)w_save; r.save16 = save_bf16 != 0;
    r.chan = (u64*)chan; r.status = status;
    if (offsets)
        return run_rec<false, false, false, true, true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream, {}, lengths, offsets);
    if (lengths) return run_rec<false, false, false, true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream, {}, lengths);
    return run_rec<false>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream);
}
}  // namespace

extern "C" int sparch_rec_cell_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                                   const float* scale, const float* shift, const float* alpha,
                                   const float* beta, const float* a, const float* b,
                                   const float* vpack, const float* rec0, const float* u0,
                                   const float* w0, const float* s0, float theta, float p_drop,
                                   uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                                   int save_bf16, uint32_t* spike_count, void* chan, size_t chan_bytes,
                                   uint32_t* status, int steps_per_launch, void* stream, int precision) {
    SPARCH_ENTER();
    return rec_cell_fwd(kind, B, dirs, T, H, Wx, scale, shift, alpha, beta, a, b, vpack, rec0, u0, w0, s0, theta, p_drop,
                        seed, s_out, s16_out, u_save, w_save, save_bf16, spike_count, chan, chan_bytes, status,
                        steps_per_launch, stream, precision, nullptr);
}

extern "C" int sparch_rec_cell_fwd_len(int kind, int B, int dirs, int T, int H, const float* Wx,
                                       const float* scale, const float* shift, const float* alpha,
                                       const float* beta, const float* a, const float* b,
                                       const float* vpack, const float* rec0, const float* u0,
                                       const float* w0, const float* s0, float theta, float p_drop,
                                       uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                                       int save_bf16, uint32_t* spike_count, const int* lengths, long long n_valid,
                                       void* chan, size_t chan_bytes, uint32_t* status, int steps_per_launch,
                                       void* stream, int precision) {
    SPARCH_ENTER();
    if (!ragged_ok(dirs, lengths, n_valid)) return SPARCH_EINVAL;
    return rec_cell_fwd(kind, B, dirs, T, H, Wx, scale, shift, alpha, beta, a, b, vpack, rec0, u0, w0, s0, theta, p_drop,
                        seed, s_out, s16_out, u_save, w_save, save_bf16, spike_count, chan, chan_bytes, status,
                        steps_per_launch, stream, precision, lengths);
}

extern "C" int sparch_rec_cell_fwd_pk(int kind, int B, int dirs, int T, int H, const float* Wx,
                                      const float* scale, const float* shift, const float* alpha,
                                      const float* beta, const float* a, const float* b,
                                      const float* vpack, const float* rec0, const float* u0,
                                      const float* w0, const float* s0, float theta, float p_drop,
                                      uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                                      int save_bf16, uint32_t* spike_count, const int* lengths, const int* offsets,
                                      long long n_valid, void* chan, size_t chan_bytes, uint32_t* status,
                                      int steps_per_launch, void* stream, int precision) {
    SPARCH_ENTER();
    if (!packed_ok(dirs, lengths, offsets, n_valid) || steps_per_launch < T) return SPARCH_EINVAL;
    return rec_cell_fwd(kind, B, dirs, T, H, Wx, scale, shift, alpha, beta, a, b, vpack, rec0, u0, w0, s0, theta, p_drop,
                        seed, s_out, s16_out, u_save, w_save, save_bf16, spike_count, chan, chan_bytes, status,
                        steps_per_launch, stream, precision, lengths, offsets);
}

extern "C" int sparch_rec_cell_stream_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                                          const float* scale, const float* shift, const float* alpha,
                                          const float* beta, const float* a, const float* b,
                                          const float* vpack, const float* rec0, float* u, float* w, float* s,
                                          uint16_t* s16_state, float theta, float p_drop, float* s_out,
                                          uint16_t* s16_out, uint32_t* spike_count, void* chan, size_t chan_bytes,
                                          uint32_t* status, int steps_per_launch, void* stream, int precision) {
    SPARCH_ENTER();
    PrecisionScope prec_scope_(precision);
    if (!prec_scope_.ok) return SPARCH_EINVAL;
    // the state is mandatory
    if (!rec_shape_ok(kind, B, dirs, T, H) || !stream_ok(dirs, p_drop) || !all_set({u, s, s16_state, Wx, alpha, vpack, rec0, status}) ||
        (!s_out && !s16_out) || !adapt_set(kind, {w, beta, a, b}) || !paired(scale, shift))
        return SPARCH_EINVAL;
    if (!al16({Wx, vpack, rec0, u, w, s, s16_state, s_out, s16_out, chan})) return SPARCH_EALIGN;
    RecArgs r = rec_args(B, 1, T, H, alpha, beta, a, b, u, w, s, theta, 0.0f, 0);
    rec_fwd_io(r, Wx, scale, shift, rec0, s_out, s16_out, spike_count);
    r.vpack = reinterpret_cast<const u32x4*>(vpack);
    r.s_step16 = s16_state;
    r.chan = (u64*)chan; r.status = status;
    return run_rec<false, true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream);
}

namespace {
// sparch_rec_cell_bwd_sg and sparch_rec_cell_bwd_len (lengths not null: n_valid is the rate gradient's sample count)
int rec_cell_bwd(int kind, int B, int dirs, int T, int H, const float* g_out,
                                      const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                      const float* alpha, const float* beta, const float* a,
                                      const float* b, const float* vpack_t, const float* u0,
                                      const float* w0, const float* s0, float theta, float p_drop,
                                      uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                                      const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                      void* chan, size_t chan_bytes, uint32_t* status,
                                      int steps_per_launch, int surrogate, float surrogate_scale, void* stream,
                                      int precision, const int* lengths, long long n_valid,
                                      const int* offsets = nullptr, const RecStArgs* stx = nullptr) {
    if (!surrogate_ok(surrogate, surrogate_scale, save_bf16)) return SPARCH_EINVAL;
    PrecisionScope prec_scope_(precision);
    if (!prec_scope_.ok) return SPARCH_EINVAL;
    if (!bn_ok(bn_x, bn_mean, bn_invstd) || !rec_shape_ok(kind, B, dirs, T, H) ||
        !all_set({g_out, u_save, alpha, vpack_t, u0, s0, dWx, s_prev16, dparam_ws, status}) ||
        !adapt_set(kind, {beta, a, b, w0, w_save}) || !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({g_out, u_save, w_save, vpack_t, u0, w0, s0, dWx, s_prev16, dparam_ws, chan})) return SPARCH_EALIGN;
    if (bwd_pring_bytes(B * dirs, H) >= ((size_t)1 << 31)) return SPARCH_EINVAL;  // 32-bit buffer offsets
    RecArgs r = rec_args(B, dirs, T, H, alpha, beta, a, b, u0, w0, s0, theta, p_drop, seed);
    rec_bwd_io(r, g_out, g_rate, u_save, w_save, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd);
    r.vpack = reinterpret_cast<const u32x4*>(vpack_t);
    r.save16 = save_bf16 != 0;
    r.chan = (u64*)chan; r.status = status;
    if (stx)
        return run_rec<true, false, false, false, false, true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream,
                                                               SurrogateArgs{surrogate, surrogate_scale}, nullptr, nullptr, stx);
    if (lengths) {
        r.g_rate_scale = 1.0f / (float)n_valid;
        if (offsets)
            return run_rec<true, false, false, true, true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream,
                                                           SurrogateArgs{surrogate, surrogate_scale}, lengths, offsets);
        return run_rec<true, false, false, true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream,
                                                 SurrogateArgs{surrogate, surrogate_scale}, lengths);
    }
    if (surrogate == SPARCH_SURROGATE_BOXCAR) return run_rec<true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream);
    return run_rec<true, false, true>(kind, r, chan_bytes, steps_per_launch, (hipStream_t)stream,
                                      SurrogateArgs{surrogate, surrogate_scale});
}
}  // namespace

extern "C" int sparch_rec_cell_bwd_sg(int kind, int B, int dirs, int T, int H, const float* g_out,
                                      const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                      const float* alpha, const float* beta, const float* a,
                                      const float* b, const float* vpack_t, const float* u0,
                                      const float* w0, const float* s0, float theta, float p_drop,
                                      uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                                      const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                      void* chan, size_t chan_bytes, uint32_t* status,
                                      int steps_per_launch, int surrogate, float surrogate_scale, void* stream,
                                      int precision) {
    SPARCH_ENTER();
    return rec_cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, vpack_t, u0, w0,
                        s0, theta, p_drop, seed, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd, chan, chan_bytes, status,
                        steps_per_launch, surrogate, surrogate_scale, stream, precision, nullptr, 0);
}

extern "C" int sparch_rec_cell_bwd_len(int kind, int B, int dirs, int T, int H, const float* g_out,
                                       const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                       const float* alpha, const float* beta, const float* a,
                                       const float* b, const float* vpack_t, const float* u0,
                                       const float* w0, const float* s0, float theta, float p_drop,
                                       uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                                       const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                       const int* lengths, long long n_valid, void* chan, size_t chan_bytes,
                                       uint32_t* status, int steps_per_launch, int surrogate, float surrogate_scale,
                                       void* stream, int precision) {
    SPARCH_ENTER();
    if (!ragged_ok(dirs, lengths, n_valid)) return SPARCH_EINVAL;
    return rec_cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, vpack_t, u0, w0,
                        s0, theta, p_drop, seed, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd, chan, chan_bytes, status,
                        steps_per_launch, surrogate, surrogate_scale, stream, precision, lengths, n_valid);
}
extern "C" int sparch_rec_cell_bwd_pk(int kind, int B, int dirs, int T, int H, const float* g_out,
                                      const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                      const float* alpha, const float* beta, const float* a,
                                      const float* b, const float* vpack_t, const float* u0,
                                      const float* w0, const float* s0, float theta, float p_drop,
                                      uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                                      const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                      const int* lengths, const int* offsets, long long n_valid, void* chan,
                                      size_t chan_bytes, uint32_t* status, int steps_per_launch, int surrogate,
                                      float surrogate_scale, void* stream, int precision) {
    SPARCH_ENTER();
    if (!packed_ok(dirs, lengths, offsets, n_valid) || steps_per_launch < T) return SPARCH_EINVAL;
    return rec_cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, vpack_t, u0, w0,
                        s0, theta, p_drop, seed, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd, chan, chan_bytes, status,
                        steps_per_launch, surrogate, surrogate_scale, stream, precision, lengths, n_valid, offsets);
}
extern "C" int sparch_rec_cell_bwd_st(int kind, int B, int dirs, int T, int H, const float* g_out,
                                      const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                      const float* alpha, const float* beta, const float* a,
                                      const float* b, const float* vpack_t, const float* u0,
                                      const float* w0, const float* s0, float theta, float p_drop,
                                      uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                                      const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                      void* chan, size_t chan_bytes, uint32_t* status,
                                      int steps_per_launch, int surrogate, float surrogate_scale,
                                      const float* g_uT, const float* g_wT, const float* g_sT, float* g_u0,
                                      float* g_w0, float* g_s0, void* stream, int precision) {
    SPARCH_ENTER();
    // a carried state is causal, the final state is read from fp32 saves, whole-sequence launches, fp32 operands, H <= 1024
    if (dirs != 1 || save_bf16 != 0 || steps_per_launch < T || precision != 0 || H > 1024) return SPARCH_EINVAL;
    if (!al16({g_uT, g_wT, g_sT, g_u0, g_w0, g_s0})) {
        // (behind the sibling's SPARCH_EINVAL checks, like every SPARCH_EALIGN: run them first on the plain arguments)
        const int rc = rec_cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, vpack_t,
                                    u0, w0, s0, theta, p_drop, seed, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd,
                                    nullptr, 0, status, steps_per_launch, surrogate, surrogate_scale, stream, precision,
                                    nullptr, 0);
        return rc == SPARCH_EINVAL ? rc : SPARCH_EALIGN;
    }
    RecStArgs stx{};
    stx.g_uT = g_uT; stx.g_wT = g_wT; stx.g_sT = g_sT; stx.g_u0 = g_u0; stx.g_w0 = g_w0; stx.g_s0 = g_s0;
    return rec_cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, vpack_t, u0, w0,
                        s0, theta, p_drop, seed, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd, chan, chan_bytes, status,
                        steps_per_launch, surrogate, surrogate_scale, stream, precision, nullptr, 0, nullptr, &stx);
}
extern "C" int sparch_rec_cell_bwd(int kind, int B, int dirs, int T, int H, const float* g_out,
                                   const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                   const float* alpha, const float* beta, const float* a,
                                   const float* b, const float* vpack_t, const float* u0,
                                   const float* w0, const float* s0, float theta, float p_drop,
                                   uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                                   const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                   void* chan, size_t chan_bytes, uint32_t* status,
                                   int steps_per_launch, void* stream, int precision) {
    return sparch_rec_cell_bwd_sg(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, vpack_t,
                                  u0, w0, s0, theta, p_drop, seed, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd, chan,
                                  chan_bytes, status, steps_per_launch, SPARCH_SURROGATE_BOXCAR, 0.0f, stream, precision);
}

// ---- f-4: dense recurrent cell of the RNN baseline (anns.py:328-339)
extern "C" int sparch_ann_rec_fwd(int act, int B, int dirs, int T, int H, const float* Wx, const float* scale,
                                  const float* shift, const float* vpack, float p_drop, uint64_t seed,
                                  float* y_out, float* y_state, void* chan, size_t chan_bytes, uint32_t* status,
                                  int steps_per_launch, void* stream) {
    SPARCH_ENTER();
    // (an unknown act is refused here, before chan is touched)
    if (!shape_ok(B, dirs, T, H, 4) || !act_ok(act) || !all_set({Wx, vpack, y_out, y_state, status}) ||
        !paired(scale, shift) || !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({Wx, scale, shift, vpack, y_out, y_state, chan})) return SPARCH_EALIGN;
    AnnArgs a = base_args<AnnArgs>(B, dirs, T, H, p_drop, seed);
    a.Wx = Wx; a.scale = scale; a.shift = shift; a.vpack = reinterpret_cast<const u32x4*>(vpack);
    a.y_state = y_state; a.y_out = y_out; a.status = status;
    return run_ann<false>(act, a, chan, chan_bytes, steps_per_launch, (hipStream_t)stream);
}

extern "C" int sparch_ann_rec_bwd(int act, int B, int dirs, int T, int H, const float* g_out, const float* y_state,
                                  const float* vpack, float p_drop, uint64_t seed, float* dpre, float* y_prev,
                                  void* chan, size_t chan_bytes, uint32_t* status, int steps_per_launch,
                                  void* stream) {
    SPARCH_ENTER();
    // (an unknown act is refused here, before chan is touched)
    if (!shape_ok(B, dirs, T, H, 4) || !act_ok(act) || !all_set({g_out, y_state, vpack, dpre, y_prev, status}) ||
        !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({g_out, y_state, vpack, dpre, y_prev, chan})) return SPARCH_EALIGN;
    AnnArgs a = base_args<AnnArgs>(B, dirs, T, H, p_drop, seed);
    a.g_out = g_out; a.y_in = y_state; a.vpack = reinterpret_cast<const u32x4*>(vpack);
    a.dpre = dpre; a.y_prev = y_prev; a.status = status;
    return run_ann<true>(act, a, chan, chan_bytes, steps_per_launch, (hipStream_t)stream);
}

// ---- one time step with the recurrent product supplied by the caller: the path for hidden sizes whose V slice
//      does not fit the register-resident layout (H > 1024), any grid size, no inter-workgroup hand-off
extern "C" int sparch_rec_cell_step_fwd(int kind, int B, int dirs, int T, int H, int t, const float* Wx,
                                        const float* scale, const float* shift, const float* alpha,
                                        const float* beta, const float* a, const float* b, const float* rec,
                                        const float* u0, const float* w0, const float* s0, float theta,
                                        float p_drop, uint64_t seed, float* s_out, uint16_t* s16_out,
                                        float* u_save, float* w_save, uint32_t* spike_count,
                                        uint16_t* s_step16, void* stream) {
    SPARCH_ENTER();
    if (!rec_shape_ok(kind, B, dirs, T, H, t) || !all_set({Wx, alpha, rec, u0, s0, u_save, s_step16}) ||
        (!s_out && !s16_out) || !adapt_set(kind, {beta, a, b, w0, w_save}) || !paired(scale, shift) || !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({Wx, rec, u0, w0, s0, s_out, s16_out, u_save, w_save, s_step16})) return SPARCH_EALIGN;
    RecArgs r = rec_args(B, dirs, T, H, alpha, beta, a, b, u0, w0, s0, theta, p_drop, seed);
    rec_fwd_io(r, Wx, scale, shift, rec, s_out, s16_out, spike_count);
    r.u_save = u_save; r.w_save = w_save; r.s_step16 = s_step16;
    return rec_step_launch(rec_step_kernel<false>(kind == SPARCH_KIND_RADLIF), r, t, stream);
}

extern "C" int sparch_rec_cell_step_stream_fwd(int kind, int B, int dirs, int T, int H, int t, const float* Wx,
                                               const float* scale, const float* shift, const float* alpha,
                                               const float* beta, const float* a, const float* b,
                                               const float* rec, float* u, float* w, float* s,
                                               uint16_t* s16_state, float theta, float p_drop, float* s_out,
                                               uint16_t* s16_out, uint32_t* spike_count, void* stream) {
    SPARCH_ENTER();
    if (!rec_shape_ok(kind, B, dirs, T, H, t) || !stream_ok(dirs, p_drop) || !all_set({u, s, s16_state, Wx, alpha, rec}) ||
        (!s_out && !s16_out) || !adapt_set(kind, {w, beta, a, b}) || !paired(scale, shift))
        return SPARCH_EINVAL;
    if (!al16({Wx, rec, u, w, s, s16_state, s_out, s16_out})) return SPARCH_EALIGN;
    RecArgs r = rec_args(B, 1, T, H, alpha, beta, a, b, u, w, s, theta, 0.0f, 0);
    rec_fwd_io(r, Wx, scale, shift, rec, s_out, s16_out, spike_count);
    r.s_step16 = s16_state;
    return rec_step_launch(rec_step_kernel<false, true>(kind == SPARCH_KIND_RADLIF), r, t, stream);
}

extern "C" int sparch_rec_cell_step_bwd_sg(int kind, int B, int dirs, int T, int H, int t, const float* g_out,
                                           const float* g_rate, const float* u_save, const float* w_save,
                                           const float* alpha, const float* beta, const float* a, const float* b,
                                           const float* rec, const float* u0, const float* w0, const float* s0,
                                           float theta, float p_drop, uint64_t seed, float* dWx,
                                           uint16_t* s_prev16, float* dparam_ws, const float* bn_x,
                                           const float* bn_mean, const float* bn_invstd, float* dwx_step,
                                           int surrogate, float surrogate_scale, void* stream) {
    SPARCH_ENTER();
    if (!surrogate_ok(surrogate, surrogate_scale, 0)) return SPARCH_EINVAL;
    if (!bn_ok(bn_x, bn_mean, bn_invstd) || !rec_shape_ok(kind, B, dirs, T, H, t) ||
        !all_set({g_out, u_save, alpha, u0, s0, dWx, s_prev16, dparam_ws, dwx_step}) || (t + 1 < T && !rec) ||
        !adapt_set(kind, {beta, a, b, w0, w_save}) || !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({g_out, u_save, w_save, rec, u0, w0, s0, dWx, s_prev16, dparam_ws, dwx_step})) return SPARCH_EALIGN;
    RecArgs r = rec_args(B, dirs, T, H, alpha, beta, a, b, u0, w0, s0, theta, p_drop, seed);
    rec_bwd_io(r, g_out, g_rate, u_save, w_save, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd);
    r.rec0 = rec; r.dwx_step = dwx_step;
    if (surrogate == SPARCH_SURROGATE_BOXCAR) return rec_step_launch(rec_step_kernel<true>(kind == SPARCH_KIND_RADLIF), r, t, stream);
    return rec_step_launch(rec_step_sg_kernel(kind == SPARCH_KIND_RADLIF), r, SurrogateArgs{surrogate, surrogate_scale}, t, stream);
}
extern "C" int sparch_rec_cell_step_bwd(int kind, int B, int dirs, int T, int H, int t, const float* g_out,
                                        const float* g_rate, const float* u_save, const float* w_save,
                                        const float* alpha, const float* beta, const float* a, const float* b,
                                        const float* rec, const float* u0, const float* w0, const float* s0,
                                        float theta, float p_drop, uint64_t seed, float* dWx,
                                        uint16_t* s_prev16, float* dparam_ws, const float* bn_x,
                                        const float* bn_mean, const float* bn_invstd, float* dwx_step,
                                        void* stream) {
    return sparch_rec_cell_step_bwd_sg(kind, B, dirs, T, H, t, g_out, g_rate, u_save, w_save, alpha, beta, a, b, rec, u0, w0,
                                       s0, theta, p_drop, seed, dWx, s_prev16, dparam_ws, bn_x, bn_mean, bn_invstd, dwx_step,
                                       SPARCH_SURROGATE_BOXCAR, 0.0f, stream);
}

/* `s` counts steps in processing order (forward: t = s; backward: t = T-1-s); rec = y_{t-1} V^T (forward) /
 * dpre_{t+1} V (backward), ignored at s = 0.  (An unknown act is refused where the kernel is picked, behind the
 * alignment check.) */
extern "C" int sparch_ann_rec_step_fwd(int act, int B, int dirs, int T, int H, int s, const float* Wx,
                                       const float* scale, const float* shift, const float* rec, float p_drop,
                                       uint64_t seed, float* y_out, float* y_state, float* y_step, void* stream) {
    SPARCH_ENTER();
    if (!shape_ok(B, dirs, T, H, 4) || s < 0 || s >= T || !all_set({Wx, y_out, y_state, y_step}) || (s > 0 && !rec) ||
        !paired(scale, shift) || !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({Wx, scale, shift, rec, y_out, y_state, y_step})) return SPARCH_EALIGN;
    AnnArgs a = base_args<AnnArgs>(B, dirs, T, H, p_drop, seed);
    a.Wx = Wx; a.scale = scale; a.shift = shift; a.y_state = y_state; a.y_out = y_out;
    return ann_step_launch(ann_kernel<false, true>(act, 1), a, s, rec, y_step, stream);
}

extern "C" int sparch_ann_rec_step_bwd(int act, int B, int dirs, int T, int H, int s, const float* g_out,
                                       const float* y_state, const float* rec, float p_drop, uint64_t seed,
                                       float* dpre, float* y_prev, float* dpre_step, void* stream) {
    SPARCH_ENTER();
    if (!shape_ok(B, dirs, T, H, 4) || s < 0 || s >= T || !all_set({g_out, y_state, dpre, y_prev, dpre_step}) ||
        (s > 0 && !rec) || !p_drop_ok(p_drop))
        return SPARCH_EINVAL;
    if (!al16({g_out, y_state, rec, dpre, y_prev, dpre_step})) return SPARCH_EALIGN;
    AnnArgs a = base_args<AnnArgs>(B, dirs, T, H, p_drop, seed);
    a.g_out = g_out; a.y_in = y_state; a.dpre = dpre; a.y_prev = y_prev;
    return ann_step_launch(ann_kernel<true, true>(act, 1), a, s, rec, dpre_step, stream);
}

// G3/G4 (non-recurrent kinds), G5, G6, G7: fused spiking-cell kernels with the time
// loop inside the kernel.
//
// Forward replaces _lif_cell (snns.py:282-303) and _adlif_cell (419-445) together
// with SpikeFunctionBoxcar.forward (26-29), the bidirectional flip/cat glue
// (252-254, 272-275), nn.Dropout (278) and the firing-rate reduction (174).
// Backward replaces the autograd replay of those loops through
// SpikeFunctionBoxcar.backward (31-36); recurrences in SURVEY.md §8a.
//
// Mapping: one thread owns VEC (4 or 1) adjacent neurons of one virtual batch row and
// walks T in registers; lanes run along H so every global access of a wave is one
// contiguous segment (1 KiB at VEC=4).  Loads of the U next time steps are issued
// before the dependent arithmetic of the current ones (the inputs do not depend on the
// recurrence), which is what hides HBM latency at one or two waves per SIMD.
// Arithmetic keeps the reference's operation order with -ffp-contract=off, so given
// identical inputs the spikes are bit-identical to the eager CPU path.
// HBM-bound: 12H (LIF) / 16H (adLIF) bytes per sample-step forward, the same backward.
#include "neuron.h"
#include <type_traits>

namespace {

struct CellArgs {
    int B, dirs, T, H;
    const float* Wx; const float* scale; const float* shift;
    const float* alpha; const float* beta; const float* a; const float* b;
    const float* u0; const float* w0; const float* s0;
    float theta, p_drop, inv_keep; uint64_t seed;
    float* s_out; uint16_t* s16_out; float* u_save; float* w_save; uint32_t* spike_count;
    // backward
    const float* g_out; const float* g_rate; float g_rate_scale;
    float* dWx; float* dparam_ws;
    // BatchNorm backward folded in (nullable): the raw projection and its per-column statistics; the kernel
    // then also leaves sum_t dWx and sum_t dWx*xhat per (row, column) in two more planes of dparam_ws
    const float* bn_x; const float* bn_mean; const float* bn_invstd;
    int save16;  // u_save / w_save hold bf16 (common.h save_u16) instead of fp32
};

// The ragged entry points (`_len`): per-row sequence lengths (B,) behind CellArgs, which does not grow — only the
// `_len` instantiations take them.
struct CellLenArgs : CellArgs { const int* lengths; };
// The packed entry points (`_pk`): the batch's sequences sorted by length, sequence j in rows [offsets[j], offsets[j] +
// lengths[j]) of every (N,H) tensor (N = offsets[B]); B counts sequences and T is the longest length.
struct CellPkArgs : CellArgs { const int* lengths; const int* offsets; };
// The stateful entry point (`_st`, backward only): the gradient arriving on the final state (u_T, w_T, s_T) and the
// gradient of the initial state (u0, w0, s0) going out, each (B,H) and each nullable.
struct CellStArgs : CellArgs {
    const float* g_uT; const float* g_wT; const float* g_sT;
    float* g_u0; float* g_w0; float* g_s0;
};// The packed kernels give every sequence whole waves: a row of HQ threads is padded to the next multiple of 64 (the lanes
// behind HQ leave at once), so that no wave straddles two sequences and a wave's length and row offset are scalars.
__host__ __device__ constexpr int pk_row_threads(int HQ) { return (HQ + 63) / 64 * 64; }
template <class Args> constexpr int cell_mode = std::is_same_v<Args, CellPkArgs> ? 2 : std::is_same_v<Args, CellLenArgs> ? 1 : 0;
template <class Args> constexpr bool cell_stateful = std::is_same_v<Args, CellStArgs>;  // the stateful backward family

template <int VEC>
__device__ __forceinline__ void ldv(float (&d)[VEC], const float* p) {
    if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
        d[0] = p[0];
    }
}
// saved states (u, w): element index i of an fp32 or bf16 array
template <int VEC>
__device__ __forceinline__ void ld_saved(float (&d)[VEC], const float* base, size_t i, bool s16) {
    if (!s16) { ldv<VEC>(d, base + i); return; }
    const unsigned short* q = reinterpret_cast<const unsigned short*>(base) + i;
    if constexpr (VEC == 4) {
        const unsigned long long raw = *reinterpret_cast<const unsigned long long*>(q);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = bf16_to_f32((unsigned short)(raw >> (16 * e)));
    } else {
        d[0] = bf16_to_f32(q[0]);
    }
}
// Saved states (written by the forward, read once by the backward much later) are non-temporal accesses: they do not
// take the infinity cache's room from what the NEXT kernel reads (cfg2 step 0.956 -> 0.937 ms, one call).
template <int VEC, bool IS_U>
__device__ __forceinline__ void st_saved(float* base, size_t i, const float (&d)[VEC], bool s16, float theta) {
    if (!s16) {
        if constexpr (VEC == 4) __builtin_nontemporal_store(f32x4{d[0], d[1], d[2], d[3]}, reinterpret_cast<f32x4*>(base + i));
        else __builtin_nontemporal_store(d[0], base + i);
        return;
    }
    unsigned short* q = reinterpret_cast<unsigned short*>(base) + i;
    if constexpr (VEC == 4) {
        unsigned long long raw = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            raw |= (unsigned long long)(IS_U ? save_u16(d[e], theta) : f32_to_bf16_rne(d[e])) << (16 * e);
        *reinterpret_cast<unsigned long long*>(q) = raw;
    } else {
        q[0] = IS_U ? save_u16(d[0], theta) : f32_to_bf16_rne(d[0]);
    }
}
template <int VEC>
__device__ __forceinline__ void stv(float* p, const float (&d)[VEC]) {
    if constexpr (VEC == 4) {
        f32x4 v; v.x = d[0]; v.y = d[1]; v.z = d[2]; v.w = d[3];
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
        p[0] = d[0];
    }
}

// ------------------------------------------------------------------ the scan kernels: register-ring pipelines (round 3)
// Fetching a batch of steps, waiting for ALL of them (`s_waitcnt vmcnt(0)`), computing them and starting over leaves
// the HBM round trip of each batch uncovered at one wave per SIMD (65 k neurons at BASELINE configs[1] = 1024 waves on
// 1024 SIMDs), and nullable outputs put a scalar branch around every load and store (the first scan kernels, DESIGN.md
// section 6).  These kernels keep a register ring of the next D steps' inputs: every step issues ONE step's loads (D steps ahead,
// unconditional, clamped into range at the sequence end) and consumes the oldest slot, so the round trip sits behind
// D steps of arithmetic and stores; which outputs exist is a template parameter (no branch in the loop).  D is
// bounded by the wave's 6-bit vmcnt (in order, counts stores): with OPS vector-memory operations per step a load
// older than 63 / OPS steps is forced complete by any counted wait.  Same arithmetic, same order: bit-identical.
constexpr int pipe_depth(int vec, int ops) { return vec == 4 ? 8 : (63 / ops < 16 ? 63 / ops : 16); }

// one saved state (u or w) of VEC neurons as it comes off the wire: fp32, or bf16 words unpacked at the use
template <int VEC, bool S16> struct SavedVec;
template <int VEC> struct SavedVec<VEC, false> {
    float v[VEC];
    __device__ __forceinline__ void load(const float* base, size_t i) {
        if constexpr (VEC == 4) {
            const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + i));
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            v[0] = __builtin_nontemporal_load(base + i);
        }
    }
    __device__ __forceinline__ void expand(float (&d)[VEC]) const {
#pragma unroll
        for (int e = 0; e < VEC; ++e) d[e] = v[e];
    }
};
template <> struct SavedVec<4, true> {
    unsigned long long raw;
    __device__ __forceinline__ void load(const float* base, size_t i) {
        raw = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned short*>(base) + i);
    }
    __device__ __forceinline__ void expand(float (&d)[4]) const {
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = bf16_to_f32((unsigned short)(raw >> (16 * e)));
    }
};
template <> struct SavedVec<1, true> {
    unsigned short raw;
    __device__ __forceinline__ void load(const float* base, size_t i) { raw = reinterpret_cast<const unsigned short*>(base)[i]; }
    __device__ __forceinline__ void expand(float (&d)[1]) const { d[0] = bf16_to_f32(raw); }
};

// SAVE: 0 = no saved states (eval), 1 = fp32, 2 = bf16.  SOUT / S16OUT: the fp32 spike tensor / the bf16 plane.
// DROP: dropout is on (a template parameter: a scalar branch around the mask's hash inside the loop makes hipcc's
// wait-count pass fall back to `s_waitcnt vmcnt(0)` at the join, once per trip — the ring would drain every D steps)
// STATE (streaming, sparch_cell_stream_fwd): u0 / w0 / s0 are the stream's (Bp,H) state buffers — read here as ever,
// and written back from the registers behind the last step, so that the next chunk's launch continues the sequence.
// LEN (sparch_cell_fwd_len, one direction): the row's length is held by the thread, and the output spikes of steps at
// or past it are 0 — a select on the value, not a branch (see DROP).  The state still runs on over the padding.
// PK (sparch_cell_fwd_pk, one direction): the packed layout.  The thread's T is its sequence's own length and its rows
// start at offsets[b]: the loop, the ring's clamp and every index below are the plain kernel's on those two values, so
// there is no padded step to select away.
template <bool ADAPT, int VEC, int SAVE, bool SOUT, bool S16OUT, bool DROP, bool STATE = false, bool LEN = false, bool PK = false>
__global__ __launch_bounds__(256) void cell_fwd_pipe_kernel(
    std::conditional_t<PK, CellPkArgs, std::conditional_t<LEN, CellLenArgs, CellArgs>> c) {
    static_assert(!(PK && (LEN || STATE)), "packed: no lengths mask, no stream state");
    constexpr int D = pipe_depth(VEC, 1 + (SOUT ? 1 : 0) + (S16OUT ? 1 : 0) + (SAVE ? 1 + (ADAPT ? 1 : 0) : 0));
    // (PK is a constant: of `PK ? :` only the live arm is compiled, and without PK that is the expression it always was)
    const int HQ = PK ? pk_row_threads(c.H / VEC) : c.H / VEC;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Bp = c.B * c.dirs;
    if (idx >= (long long)Bp * HQ) return;
    const int bp = (int)(idx / HQ), h = (int)(idx % HQ) * VEC;
    if (PK && h >= c.H) return;
    const int d = bp / c.B, b = bp - d * c.B;
    // PK: a wave lies inside one sequence (pk_row_threads), so its length and first row are wave-uniform: scalars,
    // like c.T — the time loop keeps its scalar branches and the ring its counted waits
    [[maybe_unused]] int pk_len = 0, pk_row0 = 0;
    if constexpr (PK) {
        pk_len = __builtin_amdgcn_readfirstlane(c.lengths[b]);
        pk_row0 = __builtin_amdgcn_readfirstlane(c.offsets[b]);
    }
    const int T = PK ? pk_len : c.T, H = c.H, HO = c.H * c.dirs;

    Neuron<ADAPT> p[VEC];
    float sc[VEC], sh[VEC];
    float u[VEC], w[VEC], s[VEC];
    uint32_t cnt[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        p[e] = neuron_load<ADAPT>(c.alpha, c.beta, c.a, c.b, h + e);
        sc[e] = c.scale ? c.scale[h + e] : 1.0f;
        sh[e] = c.scale ? c.shift[h + e] : 0.0f;
        cnt[e] = 0;
    }
    ldv<VEC>(u, c.u0 + (size_t)bp * H + h);
    ldv<VEC>(s, c.s0 + (size_t)bp * H + h);
    if (ADAPT) ldv<VEC>(w, c.w0 + (size_t)bp * H + h);
    const bool has_norm = c.scale != nullptr;
    constexpr bool drop = DROP;
    const uint64_t seed = drop ? resolve_seed(c.seed) : 0;
    int len = T;
    if constexpr (LEN) len = c.lengths[b];

    const float* xrow = c.Wx + (PK ? (size_t)pk_row0 : (size_t)b * T) * H + h;
    auto fetch = [&](float (&x)[VEC], int t) __attribute__((always_inline)) {
        const int tc = min(t, T - 1);  // past the end: a step that is in range and never used
        ldv<VEC>(x, xrow + (size_t)(d ? (T - 1 - tc) : tc) * H);
    };
    auto step = [&](int t, const float (&x)[VEC]) __attribute__((always_inline)) {
        const int tt = d ? (T - 1 - t) : t;
        float so[VEC];
        const size_t o = ((PK ? (size_t)pk_row0 : (size_t)b * T) + tt) * HO + (size_t)d * H + h;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float xn = neuron_input(x[e], false, 0.f, has_norm, sc[e], sh[e]);
            neuron_step<ADAPT, false>(u[e], w[e], s[e], xn, 0.f, p[e], c.theta);
            const float k = drop ? keep_scale(seed, o + e, c.p_drop, c.inv_keep) : 1.0f;
            so[e] = s[e] * k;
            if constexpr (LEN) so[e] = t < len ? so[e] : 0.0f;
            cnt[e] += (so[e] != 0.0f) ? 1u : 0u;
        }
        if (SOUT) stv<VEC>(c.s_out + o, so);
        if (S16OUT) {
            if constexpr (VEC == 4) *reinterpret_cast<u32x2*>(c.s16_out + o) = spike_quad16(so);
            else c.s16_out[o] = spike_bf16(so[0] != 0.0f);
        }
        if (SAVE) {
            st_saved<VEC, true>(c.u_save, ((PK ? (size_t)pk_row0 : (size_t)bp * T) + t) * H + h, u, SAVE == 2, c.theta);
            if (ADAPT) st_saved<VEC, false>(c.w_save, ((PK ? (size_t)pk_row0 : (size_t)bp * T) + t) * H + h, w, SAVE == 2, c.theta);
        }
    };

    float ring[D][VEC];
#pragma unroll
    for (int j = 0; j < D; ++j) fetch(ring[j], j);
    // every prologue load is in before the loop is entered: hipcc's counted waits inside the loop are the merge of
    // this state and the back edge's — with the D fills still in flight here, slot 0 looks "14 operations old" on
    // every trip (`vmcnt(14)`, then 17, 19 ...) instead of a full ring old (`vmcnt(56)`)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    int t0 = 0;
    for (; t0 + D <= T; t0 += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            // consume, THEN refill the slot: issued ahead of the step's arithmetic the new value is live beside the
            // old one, the two cannot share a register, and hipcc's copies at the loop's back edge wait for every
            // load of the ring (`s_waitcnt vmcnt(4)` per trip: the pipeline drained every D steps)
            step(t0 + j, ring[j]);
            fetch(ring[j], t0 + j + D);
            // (the trip is one basic block: without this hipcc gathers the D refills at one end of it, and the first
            // slots are waited for a few operations after their issue)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (t0 + j >= T) break;
        step(t0 + j, ring[j]);
    }
    if (c.spike_count) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if (cnt[e]) atomicAdd(c.spike_count + (size_t)d * H + h + e, cnt[e]);
    }
    if constexpr (STATE) {  // each thread owns its elements of the state for the whole launch: in place
        const size_t o = (size_t)bp * H + h;
        stv<VEC>(const_cast<float*>(c.u0) + o, u);
        stv<VEC>(const_cast<float*>(c.s0) + o, s);
        if (ADAPT) stv<VEC>(const_cast<float*>(c.w0) + o, w);
    }
}

// The reverse pass exists as two kernel families with ONE body (cell_bwd_body.inc): cell_bwd_pipe_kernel gates with
// the reference's box-car, cell_bwd_pipe_sg_kernel with one of the smooth surrogates, chosen by a wave-uniform switch
// on its second argument (fp32 saves only: S16 is never set there).
// cell_bwd_pipe_len_kernel (sparch_cell_bwd_len) is the ragged one: ROW_LEN(b) is the row's length and TAIL_ZERO(t, v)
// takes the incoming gradient of step t as 0 at or past it; cell_bwd_pipe_len_sg_kernel is the same with a smooth gate
// (two kernels as above: with both gates behind one run-time switch the box-car's VEC = 4 kernels came out of hipcc
// with the smooth kernels' 256 VGPRs + AGPR copies at one wave per SIMD).
// cell_bwd_pipe_pk_kernel / cell_bwd_pipe_pk_sg_kernel (sparch_cell_bwd_pk) are the packed ones: ROW_T(b) is the
// sequence's own length and ROW0(r) its first packed row, and there is no tail to zero.
// cell_bwd_pipe_st_kernel / cell_bwd_pipe_st_sg_kernel (sparch_cell_bwd_st) are the stateful ones, behind the packed
// family below: ST_LOAD / ST_ADD / ST_TAIL take a gradient on the final state in and put the initial state's out; in
// every other family they are empty.
#define ST_LOAD
#define ST_DS(t, gs)                  \
    float ds = gs - al[e] * du_n[e]; \
    if (ADAPT) ds = ds + pb[e] * dw_n[e];
#define ST_DU(t, gate)                    \
    float du = gate + al[e] * du_n[e];   \
    if (ADAPT) du = du + pa[e] * dw_n[e];
#define ST_ADD(t, v, g) (v)
#define ST_TAIL
#define ROW_THREADS(HQ) (HQ)
#define ROW_GUARD(h)
#define ROW0_INIT(b) 0
#define ROW_T(b) c.T
#define ROW0(r) ((size_t)(r) * T)
#define ROW_LEN(b) T
#define TAIL_ZERO(t, v) (v)
template <bool ADAPT, int VEC, bool S16, bool BN, bool DROP>
__global__ __launch_bounds__(256) void cell_bwd_pipe_kernel(CellArgs c)
#define SURROGATE_GATE(ds, x) boxcar_gate(ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
template <bool ADAPT, int VEC, bool BN, bool DROP, bool S16 = false>
__global__ __launch_bounds__(256) void cell_bwd_pipe_sg_kernel(CellArgs c, SurrogateArgs sg)
#define SURROGATE_GATE(ds, x) smooth_gate(sg.id, sg.k, ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_LEN
#undef TAIL_ZERO
// (the select as a bit mask on the value: as `t < row_len ? v : 0.0f` hipcc gave the box-car kernels 167 VGPRs for 95 at one
// neuron per thread and 256 + 182 AGPR copies for 246 at four — one wave per SIMD less; as a mask 110 and 246)
#define ROW_LEN(b) c.lengths[b]
#define TAIL_ZERO(t, v) __uint_as_float(__float_as_uint(v) & ((t) < row_len ? 0xFFFFFFFFu : 0u))
template <bool ADAPT, int VEC, bool S16, bool BN, bool DROP>
__global__ __launch_bounds__(256) void cell_bwd_pipe_len_kernel(CellLenArgs c)
#define SURROGATE_GATE(ds, x) boxcar_gate(ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
template <bool ADAPT, int VEC, bool BN, bool DROP, bool S16 = false>
__global__ __launch_bounds__(256) void cell_bwd_pipe_len_sg_kernel(CellLenArgs c, SurrogateArgs sg)
#define SURROGATE_GATE(ds, x) smooth_gate(sg.id, sg.k, ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_LEN
#undef TAIL_ZERO
#undef ROW_T
#undef ROW0
#undef ROW_THREADS
#undef ROW_GUARD
#undef ROW0_INIT
// (whole waves per sequence, see pk_row_threads: the length and the row offset are wave-uniform, i.e. scalars like c.T)
#define ROW_THREADS(HQ) pk_row_threads(HQ)
#define ROW_GUARD(h) if ((h) >= c.H) return;
#define ROW0_INIT(b) __builtin_amdgcn_readfirstlane(c.offsets[b])
#define ROW_T(b) __builtin_amdgcn_readfirstlane(c.lengths[b])
#define ROW0(r) ((size_t)row0_pk)
#define ROW_LEN(b) T
#define TAIL_ZERO(t, v) (v)
template <bool ADAPT, int VEC, bool S16, bool BN, bool DROP>
__global__ __launch_bounds__(256) void cell_bwd_pipe_pk_kernel(CellPkArgs c)
#define SURROGATE_GATE(ds, x) boxcar_gate(ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
template <bool ADAPT, int VEC, bool BN, bool DROP, bool S16 = false>
__global__ __launch_bounds__(256) void cell_bwd_pipe_pk_sg_kernel(CellPkArgs c, SurrogateArgs sg)
#define SURROGATE_GATE(ds, x) smooth_gate(sg.id, sg.k, ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_LEN
#undef TAIL_ZERO
#undef ROW_T
#undef ROW0
#undef ROW_THREADS
#undef ROW_GUARD
#undef ROW0_INIT
#undef ST_LOAD
#undef ST_DS
#undef ST_DU
#undef ST_ADD
#undef ST_TAIL
// Stateful training ("Stateful training"): the plain family's rows, plus
//   into the chunk, at the reverse pass's first step only (du_{T+1} = dw_{T+1} = 0 there):
//     ds_T = (g_T + g_rate) k + g_sT,   du_T = gate(ds_T) + g_uT,   dw_T = g_wT - (1 - alpha) du_T
//   out of the chunk, from the carries the pass ends with:
//     g_u0 = alpha du_1 + a dw_1,   g_w0 = beta dw_1,   g_s0 = -alpha du_1 + b dw_1
#define ROW_THREADS(HQ) (HQ)
#define ROW_GUARD(h)
#define ROW0_INIT(b) 0
#define ROW_T(b) c.T
#define ROW0(r) ((size_t)(r) * T)
#define ROW_LEN(b) T
#define TAIL_ZERO(t, v) (v)
#define ST_LOAD                                                                                   \
    float st_gu[VEC], st_gw[VEC], st_gs[VEC];                                                     \
    _Pragma("unroll") for (int e = 0; e < VEC; ++e) st_gu[e] = st_gw[e] = st_gs[e] = 0.f;         \
    if (c.g_uT) ldv<VEC>(st_gu, c.g_uT + (size_t)bp * H + h);                                     \
    if (ADAPT && c.g_wT) ldv<VEC>(st_gw, c.g_wT + (size_t)bp * H + h);                            \
    if (c.g_sT) ldv<VEC>(st_gs, c.g_sT + (size_t)bp * H + h);
// (every step adds the carried terms as the sums S_t, U_t that ST_TAIL hands over at a boundary: a chained run's dWx is
// then the one-chunk run's bit for bit, adaptation included — fp32 addition does not reassociate)
#define ST_DS(t, gs)                                              \
    float st_s = -(al[e] * du_n[e]);                              \
    if (ADAPT) st_s = st_s + pb[e] * dw_n[e];                     \
    float ds = (gs) + ((t) == T - 1 ? st_gs[e] : st_s);
#define ST_DU(t, gate)                                            \
    float st_u = al[e] * du_n[e];                                 \
    if (ADAPT) st_u = st_u + pa[e] * dw_n[e];                     \
    float du = (gate) + ((t) == T - 1 ? st_gu[e] : st_u);
#define ST_ADD(t, v, g) ((t) == T - 1 ? (v) + (g) : (v))
#define ST_TAIL                                                                                  \
    {                                                                                             \
        float o_u[VEC], o_w[VEC], o_s[VEC];                                                       \
        _Pragma("unroll") for (int e = 0; e < VEC; ++e) {                                         \
            o_u[e] = al[e] * du_n[e];                                                             \
            o_s[e] = -o_u[e];                                                                     \
            o_w[e] = 0.f;                                                                         \
            if (ADAPT) {                                                                          \
                o_u[e] = o_u[e] + pa[e] * dw_n[e];                                                \
                o_s[e] = o_s[e] + pb[e] * dw_n[e];                                                \
                o_w[e] = be[e] * dw_n[e];                                                         \
            }                                                                                     \
        }                                                                                         \
        if (c.g_u0) stv<VEC>(c.g_u0 + (size_t)bp * H + h, o_u);                                   \
        if (ADAPT && c.g_w0) stv<VEC>(c.g_w0 + (size_t)bp * H + h, o_w);                          \
        if (c.g_s0) stv<VEC>(c.g_s0 + (size_t)bp * H + h, o_s);                                   \
    }
template <bool ADAPT, int VEC, bool BN, bool DROP, bool S16 = false>
__global__ __launch_bounds__(256) void cell_bwd_pipe_st_kernel(CellStArgs c)
#define SURROGATE_GATE(ds, x) boxcar_gate(ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
template <bool ADAPT, int VEC, bool BN, bool DROP, bool S16 = false>
__global__ __launch_bounds__(256) void cell_bwd_pipe_st_sg_kernel(CellStArgs c, SurrogateArgs sg)
#define SURROGATE_GATE(ds, x) smooth_gate(sg.id, sg.k, ds, x)
#include "cell_bwd_body.inc"
#undef SURROGATE_GATE
#undef ROW_LEN
#undef TAIL_ZERO
#undef ROW_T
#undef ROW0
#undef ROW_THREADS
#undef ROW_GUARD
#undef ROW0_INIT
#undef ST_LOAD
#undef ST_DS
#undef ST_DU
#undef ST_ADD
#undef ST_TAIL

// ------------------------------------------------------------------ readout cell
// Readout layer (snns.py:815-825): u_t = alpha u_{t-1} + (1-alpha) x_t, out = sum_t softmax_c(u_t).
// One workgroup of 256 threads per batch row; a chunk of up to 256 time steps (the whole sequence for the
// reference's shapes) is staged in LDS, and the thread's meaning changes per phase so that nothing needs a
// cross-lane reduction:
//   thread = element : the chunk's projection, one coalesced sweep with every load in flight at once -> LDS
//   thread = class   : the linear recurrence over t (one FMA per step, in place: x_t -> u_t)
//   thread = time    : softmax over the classes of "its" time step, sequentially over the C values in LDS
//                      (rows are CS floats apart: odd stride, conflict-free for thread = time)
//   thread = class   : out_c += p[t][c] in time order (the same summation order as the reference's loop)
// History (256 x 250 x 35): class-per-lane throughout with two butterfly reductions per step 137 / 194 us
// (forward / backward); one wave per row with these phases on 128-step chunks 65 / 103 us, of which most was
// global-load round trips (8 loads in flight per lane) and then the 64-rows-per-wave softmax phase running on one
// SIMD of the CU.
constexpr int RO_NT = 256;           // threads per batch row (and the most time steps per chunk)
constexpr int RO_LPT = 36;           // elements per thread and load batch of the staging sweep
constexpr int RO_FWD_FLOATS = 15872; // LDS floats of the forward kernel (62 KiB)
constexpr int RO_BWD_FLOATS = 39168; // of the backward kernel: three chunk images (153 KiB, dynamic)
constexpr unsigned RO_OOB = 0xFFFFFFF0u;
__host__ __device__ inline int ro_row_stride(int C) { return (C & 1) ? C + 2 : C + 1; }  // odd, > C: column C is a dump slot
inline int ro_chunk_steps(int T, int C, int lds_floats) {
    const int fit = lds_floats / ro_row_stride(C);
    return T < RO_NT ? (T < fit ? T : fit) : (RO_NT < fit ? RO_NT : fit);
}
// workgroup barrier for the LDS hand-offs between the phases: LDS-only fences (no vmcnt(0): the u_save / dWx
// stores of a phase stay in flight across it, which __syncthreads() would wait for)
__device__ __forceinline__ void ro_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// `n_rows` rows of `row_elems` floats from row `row` on (one row: a batch row's whole (T,C) image)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ro_row(const float* base, size_t row_elems, size_t row, int n_rows = 1) {
    // a null base gives an empty resource: loads return 0, stores are dropped
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base ? base + row * row_elems : nullptr), 0,
                                             base ? (int)(n_rows * row_elems * sizeof(float)) : 0, 0x00020000);
}
// bounds-checked fp32 accesses (the builtins move raw 32-bit words: bit casts, not conversions)
__device__ __forceinline__ float ro_load(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ void ro_store(float v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, off, 0, 0);
}
// (time, class) of the linear element index idx = first + 256 k of a chunk, advanced without divisions
struct RoCursor {
    int t, c, dq, dr, C;
    __device__ RoCursor(int first, int C_) : t(first / C_), c(first % C_), dq(RO_NT / C_), dr(RO_NT % C_), C(C_) {}
    __device__ __forceinline__ void next() {
        t += dq; c += dr;
        if (c >= C) { c -= C; ++t; }
    }
};
__device__ __forceinline__ const int* ro_offsets() { return nullptr; }
__device__ __forceinline__ const int* ro_offsets(const int* offsets) { return offsets; }
// Per-step readout (sparch_readout_*_seq): the trailing argument of the `_seq` kernels, in the place of the packed
// form's offsets.  mode: SPARCH_SEQ_PROB / SPARCH_SEQ_SUM.
struct RoSeq { float* seq; int mode; };          // forward: the per-step output (B,T,C)
struct RoGSeq { const float* g_seq; int mode; }; // backward: the per-step incoming gradient (B,T,C)
// Stateful training (sparch_readout_bwd_st): the backward's trailing argument, alone.  g_uT (B,C): the gradient arriving
// on the returned final membrane u_T, added to e_T; g_u0 (B,C), written: alpha du_1, the initial membrane's.  Each nullable.
struct RoSt { const float* g_uT; float* g_u0; };
template <class S> __device__ __forceinline__ const int* ro_offsets(S) { return nullptr; }
template <class S> __device__ __forceinline__ const int* ro_offsets(const int* offsets, S) { return offsets; }
// Selectable readout (sparch_readout_*_red): a trailing argument too, alone or behind the packed form's offsets.  The
// reduction over time M (SPARCH_RED_*) is a template argument — each mode is a kernel of its own, and the kernels without
// the argument are the softmax-sum.  arg (B,C): u_max's step of the maximum, written by the forward, read by the backward.
template <int M> struct RoRed { int* arg; };
template <class S> struct ro_red_of { static constexpr int value = -1; };
template <int M> struct ro_red_of<RoRed<M>> { static constexpr int value = M; };
template <class... A> constexpr int ro_red_mode() {
    int m = SPARCH_RED_SOFTMAX_SUM;
    ((m = ro_red_of<A>::value >= 0 ? ro_red_of<A>::value : m), ...);
    return m;
}
template <class S> __device__ __forceinline__ int* ro_arg1(S, int* r) { return r; }
template <int M> __device__ __forceinline__ int* ro_arg1(RoRed<M> red, int*) { return red.arg; }
template <class... A> __device__ __forceinline__ int* ro_red_arg([[maybe_unused]] A... a) {
    int* r = nullptr;
    ((r = ro_arg1(a, r)), ...);
    return r;
}
// the direct gradient e_t of a membrane mode at step t: gc is g (u_max, u_last) or g / T_b (u_mean)
template <int M> __device__ __forceinline__ float ro_red_e(float gc, int t, int arg_t, int t_last) {
    if constexpr (M == SPARCH_RED_U_MAX) return t == arg_t ? gc : 0.f;
    else if constexpr (M == SPARCH_RED_U_LAST) return t == t_last ? gc : 0.f;
    else return gc;
}
template <class S, class... A> constexpr bool ro_has = (std::is_same_v<S, A> || ...);
template <class S, class... A> __device__ __forceinline__ S ro_seq([[maybe_unused]] A... a) {
    if constexpr (ro_has<S, A...>) return (a, ...);
    else return S{nullptr, 0};
}
// (ro_softmax_row: common.h — the streaming step's readout kernel, streamstep.hip, shares it)

// STREAM (sparch_readout_stream_fwd): `u_io` (B,C) is the membrane state, read in place of u0 and written back behind
// the last step, and `out` comes in holding the running sum: the accumulator CONTINUES the one sequential sum over t
// (per-chunk sums added afterwards would round differently).
// LEN (sparch_readout_fwd_len): the row's own length bounds the recurrence, the softmax and the sum — out is the
// truncated sum over t < lengths[b], what the clip run alone gives; u_save is not written past it.
// Offsets (sparch_readout_fwd_pk, with LEN: one more argument, `const int* offsets`): the packed layout — the row's steps
// are rows [offsets[b], offsets[b] + lengths[b]) of Wx / u_save (N,C), and its buffer resources end at its own last step.
// RoSeq (sparch_readout_fwd_seq / _seq_len: one more argument, `RoSeq`, never with Offsets): the chunk image also goes
// out as seq[b, c0 + t, :] by a thread = element pass behind the sum — in PROB mode as the softmax phase left it, in SUM
// mode after the sum phase has put its accumulator back in place of every p_t it added (the accumulator of `out`
// itself: seq[b, t] is out after t + 1 steps).  With LEN the rows t >= lengths[b] of seq are written as 0.
// RoRed<M> (sparch_readout_fwd_red / _stream_fwd_red: one more argument, last; never with RoSeq): the reduction over time.
//   SOFTMAX_MEAN  the kernel above with one division of the accumulator by (float)T_b at the final store
//   U_MAX / U_MEAN / U_LAST  the membrane modes: no softmax phase, no sum phase and neither of their barriers; the
//       recurrence phase (thread = class) keeps the running maximum with its step (strict >: the earliest wins; u0 is no
//       candidate), or the sequential sum of u_t, in registers, and does not write u_t back to LDS — nobody reads it.
//   With STREAM the accumulator is carried in `out` as above: the running maximum (the caller starts it at -inf), the
//   un-normalised sum of u_t (the caller divides by its step count), or nothing (u_last: out = u); arg is not written.
// (A trailing parameter pack: the kernels without it keep the argument list they had.)
template <bool STREAM, bool LEN = false, class... Offsets>
__global__ __launch_bounds__(RO_NT) void readout_fwd_kernel(int B, int T, int C, int rows, const float* __restrict__ Wx,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ shift,
                                                            const float* __restrict__ alpha,
                                                            const float* __restrict__ u0, float* __restrict__ out,
                                                            float* __restrict__ u_save, float* u_io,
                                                            const int* __restrict__ lengths, Offsets... pk) {
    constexpr bool PK = ro_has<const int*, Offsets...>, SEQ = ro_has<RoSeq, Offsets...>;
    constexpr int RED = ro_red_mode<Offsets...>();
    constexpr bool MEMB = RED >= SPARCH_RED_U_MAX;  // a reduction of the membrane itself
    static_assert(sizeof...(Offsets) <= 1 + (PK && RED != 0) && (!PK || LEN), "packed rows carry their lengths");
    static_assert(!(SEQ && STREAM), "the per-step output belongs to the whole-sequence forms");
    static_assert(!(SEQ && RED != 0), "the per-step output is the softmax-sum's");
    [[maybe_unused]] const int* offsets = ro_offsets(pk...);
    [[maybe_unused]] const RoSeq sq = ro_seq<RoSeq>(pk...);
    [[maybe_unused]] int* const arg = ro_red_arg(pk...);
    __shared__ float us[RO_FWD_FLOATS];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int Tb = LEN ? min(max(lengths[b], 0), T) : T;  // the steps this row has
    const int CS = ro_row_stride(C);
    const bool act = tid < C;
    const bool wave_has_class = (tid & ~63) < C;  // wave-uniform: waves past the classes skip the class phases
    const int cc = act ? tid : C;
    const int cp = act ? tid : 0;
    const Neuron<false> p = neuron_load<false>(alpha, nullptr, nullptr, nullptr, cp);
    const bool has_bn = scale != nullptr;
    const float sc = has_bn ? scale[cp] : 1.0f, sh = has_bn ? shift[cp] : 0.0f;
    float u = STREAM ? u_io[(size_t)b * C + cp] : u0[(size_t)b * C + cp];
    float acc = STREAM ? out[(size_t)b * C + cp] : RED == SPARCH_RED_U_MAX ? -INFINITY : 0.f;
    [[maybe_unused]] int amax = 0;  // U_MAX: the step of acc
    const __amdgpu_buffer_rsrc_t rx = PK ? ro_row(Wx, (size_t)C, offsets[b], Tb) : ro_row(Wx, (size_t)T * C, b),
                                 ru = PK ? ro_row(u_save, (size_t)C, offsets[b], Tb) : ro_row(u_save, (size_t)T * C, b);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rs = ro_row(sq.seq, (size_t)T * C, b);
    if constexpr (SEQ && LEN) {  // thread = element: the padded tail of seq
        for (int idx = Tb * C + tid; idx < T * C; idx += RO_NT) ro_store(0.f, rs, (unsigned)((size_t)idx * sizeof(float)));
    }
    for (int c0 = 0; c0 < Tb; c0 += rows) {
        const int len = min(rows, Tb - c0), n = len * C;
        // thread = element: the chunk's projection -> LDS
        {
            RoCursor cur(tid, C);
            for (int base = 0; base < n; base += RO_NT * RO_LPT) {
                float v[RO_LPT];
#pragma unroll
                for (int k = 0; k < RO_LPT; ++k) {
                    const int idx = base + tid + RO_NT * k;
                    v[k] = ro_load(rx, idx < n ? (unsigned)(((size_t)c0 * C + idx) * sizeof(float)) : RO_OOB);
                }
#pragma unroll
                for (int k = 0; k < RO_LPT; ++k) {
                    const int idx = base + tid + RO_NT * k;
                    us[idx < n ? cur.t * CS + cur.c : C] = v[k];
                    cur.next();
                }
            }
        }
        ro_barrier();
        // thread = class: recurrence, in place (x_t -> u_t).  Whole groups of 8 steps run without predicates on
        // running LDS / row offsets (the step is a handful of instructions: its issue time is the phase);
        // the ragged tail goes step by step.
        if (wave_has_class) {
            float* q = us + cc;                                                      // -> us[t][cc]
            unsigned go = act ? (unsigned)(((size_t)c0 * C + tid) * sizeof(float)) : RO_OOB;  // -> u_save[c0 + t][tid]
            const unsigned gstep = act ? (unsigned)(C * sizeof(float)) : 0u;
            int t0 = 0;
            for (; t0 + 8 <= len; t0 += 8) {
                float x[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = q[j * CS];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    u = readout_step(u, neuron_input(x[j], false, 0.f, has_bn, sc, sh), p.al, p.oma);
                    if constexpr (!MEMB) q[j * CS] = u;
                    ro_store(u, ru, go + j * gstep);
                    if constexpr (RED == SPARCH_RED_U_MAX) { if (u > acc) { acc = u; amax = c0 + t0 + j; } }
                    if constexpr (RED == SPARCH_RED_U_MEAN) acc = acc + u;
                }
                q += 8 * CS;
                go += 8 * gstep;
            }
            for (; t0 < len; ++t0) {
                u = readout_step(u, neuron_input(*q, false, 0.f, has_bn, sc, sh), p.al, p.oma);
                if constexpr (!MEMB) *q = u;
                ro_store(u, ru, go);
                if constexpr (RED == SPARCH_RED_U_MAX) { if (u > acc) { acc = u; amax = c0 + t0; } }
                if constexpr (RED == SPARCH_RED_U_MEAN) acc = acc + u;
                q += CS;
                go += gstep;
            }
        }
        ro_barrier();  // (membrane modes: the chunk's only other barrier — the next staging sweep overwrites the image)
        if constexpr (!MEMB) {
        // thread = time: softmax over classes, in place
        for (int tl = tid; tl < len; tl += RO_NT) {
            float* row = us + tl * CS;
            const float den = ro_softmax_row(row, C);
            for (int c = 0; c < C; ++c) row[c] = row[c] / den;
        }
        ro_barrier();
        // thread = class: out += softmax(u_t) in time order             // snns.py:823
        if (wave_has_class) {
            std::conditional_t<SEQ, float, const float>* p = us + cc;
            [[maybe_unused]] const bool put = SEQ && sq.mode == SPARCH_SEQ_SUM;  // the running sum replaces p_t
            int t0 = 0;
            for (; t0 + 8 <= len; t0 += 8) {
                float pv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) pv[j] = p[j * CS];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    acc = acc + pv[j];
                    if constexpr (SEQ) { if (put) p[j * CS] = acc; }
                }
                p += 8 * CS;
            }
            for (; t0 < len; ++t0, p += CS) {
                acc = acc + *p;
                if constexpr (SEQ) { if (put) *p = acc; }
            }
        }
        ro_barrier();
        }
        if constexpr (SEQ) {
            // thread = element: the chunk image -> seq[b, c0 ..], the staging sweep run backwards
            RoCursor cur(tid, C);
            for (int base = 0; base < n; base += RO_NT * RO_LPT) {
                float v[RO_LPT];
#pragma unroll
                for (int k = 0; k < RO_LPT; ++k) {
                    const int idx = base + tid + RO_NT * k;
                    v[k] = us[idx < n ? cur.t * CS + cur.c : C];
                    cur.next();
                }
#pragma unroll
                for (int k = 0; k < RO_LPT; ++k) {
                    const int idx = base + tid + RO_NT * k;
                    ro_store(v[k], rs, idx < n ? (unsigned)(((size_t)c0 * C + idx) * sizeof(float)) : RO_OOB);
                }
            }
            ro_barrier();  // (the next chunk's staging sweep overwrites the image)
        }
    }
    if constexpr (RED == SPARCH_RED_U_LAST) acc = u;
    if constexpr (!STREAM && (RED == SPARCH_RED_SOFTMAX_MEAN || RED == SPARCH_RED_U_MEAN)) acc = acc / (float)Tb;
    if (act) out[(size_t)b * C + cc] = acc;
    if constexpr (!STREAM && RED == SPARCH_RED_U_MAX) { if (act) arg[(size_t)b * C + cc] = amax; }
    if (STREAM && act) u_io[(size_t)b * C + cc] = u;
}

// Backward of the above.  With p_t = softmax(u_t) and g = dL/dout:
//   e_t = p_t * (g - <p_t, g>)            (thread = time; independent over t)
//   du_t = alpha du_{t+1} + e_t,  dWx_t = (1-alpha) du_t,  dalpha += du_t (u_{t-1} - u_t) / (1-alpha)
//                                          (thread = class; reverse time)
// Three chunk images in LDS: u (overwritten by e), u_{t-1} - u_t, and BatchNorm's xhat of the raw projection.
// LEN (sparch_readout_bwd_len): the reverse recurrence starts at the row's last valid step; dWx past it is written as 0.
// Offsets (sparch_readout_bwd_pk, with LEN): packed rows as in the forward; there is no tail of dWx to write.
// RoGSeq (sparch_readout_bwd_seq / _seq_len: one more argument, `RoGSeq`, never with Offsets): the gradient of p_t is per
// step, G_t = g + A_t, with a fourth chunk image for A: g_seq[t] as staged (PROB), or the reverse running sum
// S_t = S_{t+1} + g_seq[t] (SUM), which a thread = class reverse pass in front of the thread = time phase puts in place of
// g_seq[t]; S lives in a register across the chunks, which already run in reverse, and starts from 0 at the row's last
// step — g_seq behind it is never read.  g_out may be null (g = 0).
// RoRed<M> (sparch_readout_bwd_red: one more argument, last; never with RoGSeq): SOFTMAX_MEAN is the kernel above with
// g / (float)T_b in place of g.  The membrane modes have no thread = time phase: e_t is a select on the step (u_max: g at
// t = arg[b,c]; u_last: g at t = T_b - 1) or the constant g / (float)T_b (u_mean), formed in the reverse recurrence from
// registers.  The u image has no reader then and is not staged (its LDS stays allotted: the chunks are the plain
// kernel's); u_{t-1} - u_t and xhat are staged as above, for dalpha and BatchNorm's sums.
extern __shared__ __attribute__((aligned(16))) float ro_dyn_lds[];
template <bool LEN, class... Offsets>
__global__ __launch_bounds__(RO_NT) void readout_bwd_kernel(int B, int T, int C, int rows, const float* __restrict__ g_out,
                                                            const float* __restrict__ u_save,
                                                            const float* __restrict__ alpha,
                                                            const float* __restrict__ u0, float* __restrict__ dWx,
                                                            float* __restrict__ dalpha_ws,
                                                            const float* __restrict__ bn_x,
                                                            const float* __restrict__ bn_mean,
                                                            const float* __restrict__ bn_invstd,
                                                            const int* __restrict__ lengths, Offsets... pk) {
    constexpr bool PK = ro_has<const int*, Offsets...>, SEQ = ro_has<RoGSeq, Offsets...>;
    constexpr int RED = ro_red_mode<Offsets...>();
    constexpr bool MEMB = RED >= SPARCH_RED_U_MAX;
    constexpr bool ST = ro_has<RoSt, Offsets...>;
    static_assert(sizeof...(Offsets) <= 1 + (PK && RED != 0) && (!PK || LEN), "packed rows carry their lengths");
    static_assert(!(SEQ && RED != 0), "the per-step gradient is the softmax-sum's");
    static_assert(!ST || (sizeof...(Offsets) == 1 && !LEN), "the stateful form is the plain softmax-sum's");
    [[maybe_unused]] const int* offsets = ro_offsets(pk...);
    [[maybe_unused]] const RoGSeq sq = ro_seq<RoGSeq>(pk...);
    [[maybe_unused]] const int* const arg = ro_red_arg(pk...);
    __shared__ float gs[RO_NT];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int Tb = LEN ? min(max(lengths[b], 0), T) : T;  // the steps this row has
    const int CS = ro_row_stride(C);
    float* const ue = ro_dyn_lds;            // [rows][CS] u_t, then e_t
    float* const dl = ue + rows * CS;        // [rows][CS] u_{t-1} - u_t
    float* const xh = dl + rows * CS;        // [rows][CS] xhat_t
    [[maybe_unused]] float* const ga = xh + rows * CS;  // SEQ: [rows][CS] g_seq[t], then S_t (SUM), then G_t
    const bool act = tid < C;
    const bool wave_has_class = (tid & ~63) < C;
    const int cc = act ? tid : C;
    const int cp = act ? tid : 0;
    const float al = clampf(alpha[cp], SP_ALPHA_LO, SP_ALPHA_HI), oma = 1.0f - al;  // (neuron.h: this copy stays)
    [[maybe_unused]] float gc = 0.f;   // RED: this class's g, over (float)T_b in the mean modes
    [[maybe_unused]] int arg_t = 0;    // U_MAX: the step that takes it
    if constexpr (RED != 0) {
        gc = act ? g_out[(size_t)b * C + cp] : 0.f;
        if constexpr (RED == SPARCH_RED_SOFTMAX_MEAN || RED == SPARCH_RED_U_MEAN) gc = gc / (float)Tb;
        // (through a buffer resource like the rows: with a flat load of arg, hipcc held dWx's resource in VGPRs in the
        // <false, RoRed<U_MAX>> instantiation and wrapped every dWx store in a waterfall loop, 35 us for 22 — seen in the
        // ISA, the reason not established; lanes past the classes read 0 and carry gc = 0)
        if constexpr (RED == SPARCH_RED_U_MAX)
            arg_t = (int)__builtin_amdgcn_raw_buffer_load_b32(ro_row(reinterpret_cast<const float*>(arg), (size_t)C, b),
                                                              act ? (unsigned)(tid * sizeof(int)) : RO_OOB, 0, 0);
        if constexpr (!MEMB) gs[tid] = gc;
    } else
    if constexpr (SEQ) gs[tid] = (act && g_out) ? g_out[(size_t)b * C + cp] : 0.f;
    else
    gs[tid] = act ? g_out[(size_t)b * C + cp] : 0.f;
    float du = 0.f, acc = 0.f;
    [[maybe_unused]] float S = 0.f;  // SEQ, SUM mode: sum of g_seq[t'] over the steps t' behind the current one
    // BatchNorm backward's column sums folded in (nullable): sum_t dWx and sum_t dWx*xhat per (row, class)
    const bool bn = bn_x != nullptr;
    float acc_dy = 0.f, acc_dyx = 0.f;
    const __amdgpu_buffer_rsrc_t ru = PK ? ro_row(u_save, (size_t)C, offsets[b], Tb) : ro_row(u_save, (size_t)T * C, b),
                                 rb = PK ? ro_row(bn_x, (size_t)C, offsets[b], Tb) : ro_row(bn_x, (size_t)T * C, b),
                                 rd = PK ? ro_row(dWx, (size_t)C, offsets[b], Tb) : ro_row(dWx, (size_t)T * C, b),
                                 r0 = ro_row(u0, (size_t)C, b);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t rg = ro_row(sq.g_seq, (size_t)T * C, b);
    if constexpr (LEN && !PK) {  // thread = element: the padded tail of dWx
        for (int idx = Tb * C + tid; idx < T * C; idx += RO_NT) ro_store(0.f, rd, (unsigned)((size_t)idx * sizeof(float)));
    }
    const int nchunk = (Tb + rows - 1) / rows;
    for (int ch = nchunk - 1; ch >= 0; --ch) {
        const int c0 = ch * rows, len = min(rows, Tb - c0), n = len * C;
        // thread = element: u_t, u_{t-1} - u_t (u_{-1} = u0) and xhat_t of the chunk -> LDS
        {
            RoCursor cur(tid, C);
            constexpr int LPT = RO_LPT / 2;
            for (int base = 0; base < n; base += RO_NT * LPT) {
                float vu[LPT], vx[LPT];
                [[maybe_unused]] float vg[LPT];
                unsigned vp[LPT], v0[LPT];
#pragma unroll
                for (int k = 0; k < LPT; ++k) {
                    const int idx = base + tid + RO_NT * k;
                    const bool in = idx < n;
                    const size_t e = (size_t)c0 * C + idx;           // element of the batch row
                    const bool first = in && e < (size_t)C;          // time step 0: the step before is u0
                    vu[k] = ro_load(ru, in ? (unsigned)(e * sizeof(float)) : RO_OOB);
                    vx[k] = ro_load(rb, in ? (unsigned)(e * sizeof(float)) : RO_OOB);
                    vp[k] = __builtin_amdgcn_raw_buffer_load_b32(ru, (in && !first) ? (unsigned)((e - C) * sizeof(float)) : RO_OOB, 0, 0);
                    v0[k] = __builtin_amdgcn_raw_buffer_load_b32(r0, first ? (unsigned)(e * sizeof(float)) : RO_OOB, 0, 0);
                    if constexpr (SEQ) vg[k] = ro_load(rg, in ? (unsigned)(e * sizeof(float)) : RO_OOB);
                }
#pragma unroll
                for (int k = 0; k < LPT; ++k) {
                    const int idx = base + tid + RO_NT * k;
                    const int at = idx < n ? cur.t * CS + cur.c : C;
                    const int cl = idx < n ? cur.c : 0;
                    if constexpr (!MEMB) ue[at] = vu[k];
                    dl[at] = __uint_as_float(vp[k] | v0[k]) - vu[k];   // exactly one of the two loads was in range
                    xh[at] = bn ? (vx[k] - bn_mean[cl]) * bn_invstd[cl] : 0.f;
                    if constexpr (SEQ) ga[at] = vg[k];
                    cur.next();
                }
            }
        }
        ro_barrier();
        if constexpr (SEQ) {
            // thread = class: g_seq[t] -> S_t in place, in reverse time order (one sequential fp32 sum per class)
            if (sq.mode == SPARCH_SEQ_SUM) {
                if (wave_has_class) {
                    float* q = ga + (len - 1) * CS + cc;
                    int left = len;
                    for (; left >= 8; left -= 8) {
                        float gv[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) gv[j] = q[-j * CS];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            S = S + gv[j];
                            q[-j * CS] = S;
                        }
                        q -= 8 * CS;
                    }
                    for (; left > 0; --left, q -= CS) {
                        S = S + *q;
                        *q = S;
                    }
                }
                ro_barrier();
            }
        }
        // thread = time: e_t in place
        if constexpr (!MEMB) {
        for (int tl = tid; tl < len; tl += RO_NT) {
            float* row = ue + tl * CS;
            const float den = ro_softmax_row(row, C);
            float dot = 0.f;
            if constexpr (SEQ) {
                float* grow = ga + tl * CS;
                for (int c = 0; c < C; ++c) {
                    const float pc = row[c] / den;
                    const float G = gs[c] + grow[c];
                    row[c] = pc;
                    grow[c] = G;
                    dot += pc * G;
                }
                for (int c = 0; c < C; ++c) row[c] = row[c] * (grow[c] - dot);
            } else {
            for (int c = 0; c < C; ++c) {
                const float pc = row[c] / den;
                row[c] = pc;
                dot += pc * gs[c];
            }
            for (int c = 0; c < C; ++c) row[c] = row[c] * (gs[c] - dot);
            }
        }
        ro_barrier();
        }
        // thread = class: reverse recurrence (groups of 8 steps without predicates, then the ragged rest)
        if (wave_has_class) {
            if constexpr (ST) {  // the gradient on u_T joins e_T (this thread's own element of the image, written by it)
                const float* g_uT = ro_seq<RoSt>(pk...).g_uT;
                if (ch == nchunk - 1 && act && g_uT) ue[(len - 1) * CS + cc] += g_uT[(size_t)b * C + cp];
            }
            int at = (len - 1) * CS + cc;                                            // -> [t][cc] of the three images
            unsigned go = act ? (unsigned)(((size_t)(c0 + len - 1) * C + tid) * sizeof(float)) : RO_OOB;  // -> dWx[c0 + t][tid]
            const unsigned gstep = act ? (unsigned)(C * sizeof(float)) : 0u;
            int left = len;
            [[maybe_unused]] int tt = c0 + len - 1;  // membrane modes: the step `at` stands on
            for (; left >= 8; left -= 8) {
                float ev[8], dv[8], xv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if constexpr (MEMB) ev[j] = ro_red_e<RED>(gc, tt - j, arg_t, Tb - 1);
                    else
                    ev[j] = ue[at - j * CS];
                    dv[j] = dl[at - j * CS]; xv[j] = xh[at - j * CS];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    du = al * du + ev[j];
                    const float dwx = oma * du;
                    ro_store(dwx, rd, go - j * gstep);
                    acc = acc + du * dv[j];
                    acc_dy = acc_dy + dwx;
                    acc_dyx = acc_dyx + dwx * xv[j];
                }
                at -= 8 * CS;
                go -= 8 * gstep;
                tt -= 8;
            }
            for (; left > 0; --left) {
                if constexpr (MEMB) du = al * du + ro_red_e<RED>(gc, tt--, arg_t, Tb - 1);
                else
                du = al * du + ue[at];
                const float dwx = oma * du;
                ro_store(dwx, rd, go);
                acc = acc + du * dl[at];
                acc_dy = acc_dy + dwx;
                acc_dyx = acc_dyx + dwx * xh[at];
                at -= CS;
                go -= gstep;
            }
        }
        ro_barrier();
    }
    if (act) {
        dalpha_ws[(size_t)b * C + cc] = acc / oma;
        if (bn) {
            dalpha_ws[((size_t)B + b) * C + cc] = acc_dy;
            dalpha_ws[((size_t)2 * B + b) * C + cc] = acc_dyx;
        }
        if constexpr (ST) {  // du holds du_1: the initial membrane's gradient
            float* g_u0 = ro_seq<RoSt>(pk...).g_u0;
            if (g_u0) g_u0[(size_t)b * C + cc] = al * du;
        }
    }
}

// Args = CellLenArgs / CellPkArgs: the ragged / packed instantiations (the forward's LEN / PK, and their backward families)
template <bool ADAPT, int VEC, bool DROP, class Args>
void launch_cell_pipe(bool bwd, const Args& c, const SurrogateArgs& sg, unsigned blocks, hipStream_t st) {
    constexpr bool LEN = cell_mode<Args> == 1, PK = cell_mode<Args> == 2;
    if constexpr (cell_stateful<Args>) {  // the stateful backward (fp32 saves: the entry point has refused bf16 ones)
        auto go = [&](auto bn) {
            constexpr bool BN = decltype(bn)::value;
            if (sg.id == SPARCH_SURROGATE_BOXCAR)
                hipLaunchKernelGGL((cell_bwd_pipe_st_kernel<ADAPT, VEC, BN, DROP>), dim3(blocks), dim3(256), 0, st, c);
            else
                hipLaunchKernelGGL((cell_bwd_pipe_st_sg_kernel<ADAPT, VEC, BN, DROP>), dim3(blocks), dim3(256), 0, st, c, sg);
        };
        if (c.bn_x) go(std::true_type{}); else go(std::false_type{});
        return;
    } else
    if constexpr (LEN || PK) {
        if (bwd) {
            auto go = [&](auto s16, auto bn) {  // (bf16 saves: the box-car only — the entry point has refused the rest)
                constexpr bool S16 = decltype(s16)::value, BN = decltype(bn)::value;
                if constexpr (PK) {
                    if (S16 || sg.id == SPARCH_SURROGATE_BOXCAR)
                        hipLaunchKernelGGL((cell_bwd_pipe_pk_kernel<ADAPT, VEC, S16, BN, DROP>), dim3(blocks), dim3(256), 0, st, c);
                    else
                        hipLaunchKernelGGL((cell_bwd_pipe_pk_sg_kernel<ADAPT, VEC, BN, DROP>), dim3(blocks), dim3(256), 0, st, c, sg);
                } else
                if (S16 || sg.id == SPARCH_SURROGATE_BOXCAR)
                    hipLaunchKernelGGL((cell_bwd_pipe_len_kernel<ADAPT, VEC, S16, BN, DROP>), dim3(blocks), dim3(256), 0, st, c);
                else
                    hipLaunchKernelGGL((cell_bwd_pipe_len_sg_kernel<ADAPT, VEC, BN, DROP>), dim3(blocks), dim3(256), 0, st, c, sg);
            };
            if (c.save16) { if (c.bn_x) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{}); }
            else          { if (c.bn_x) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{}); }
            return;
        }
    } else {
    if (bwd && sg.id != SPARCH_SURROGATE_BOXCAR) {  // (fp32 saves: the entry point has refused bf16 ones)
        auto go = [&](auto bn) {
            hipLaunchKernelGGL((cell_bwd_pipe_sg_kernel<ADAPT, VEC, decltype(bn)::value, DROP>), dim3(blocks), dim3(256), 0,
                               st, c, sg);
        };
        if (c.bn_x) go(std::true_type{}); else go(std::false_type{});
        return;
    }
    if (bwd) {
        auto go = [&](auto s16, auto bn) {
            hipLaunchKernelGGL((cell_bwd_pipe_kernel<ADAPT, VEC, decltype(s16)::value, decltype(bn)::value, DROP>),
                               dim3(blocks), dim3(256), 0, st, c);
        };
        if (c.save16) { if (c.bn_x) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{}); }
        else          { if (c.bn_x) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{}); }
        return;
    }
    }
    auto go = [&](auto save, auto sout, auto s16out) {
        hipLaunchKernelGGL((cell_fwd_pipe_kernel<ADAPT, VEC, decltype(save)::value, decltype(sout)::value,
                                                 decltype(s16out)::value, DROP, false, LEN, PK>),
                           dim3(blocks), dim3(256), 0, st, c);
    };
    auto outs = [&](auto save) {
        if (c.s_out && c.s16_out) go(save, std::true_type{}, std::true_type{});
        else if (c.s_out) go(save, std::true_type{}, std::false_type{});
        else go(save, std::false_type{}, std::true_type{});
    };
    if (!c.u_save) outs(std::integral_constant<int, 0>{});
    else if (c.save16) outs(std::integral_constant<int, 2>{});
    else outs(std::integral_constant<int, 1>{});
}

template <bool ADAPT, class Args>
int launch_cell(bool bwd, Args& c, hipStream_t st, const SurrogateArgs sg = {}) {
    const long long work = (long long)c.B * c.dirs * c.H;
    const bool vec_ok = (c.H % 4 == 0);
    // VEC=4 only when it still leaves >= 8 waves per CU; small problems favour more threads
    const bool vec4 = vec_ok && work >= (long long)256 * 8 * 64 * 4;
    long long threads = vec4 ? work / 4 : work;
    if constexpr (cell_mode<Args> == 2) threads = (long long)c.B * pk_row_threads(vec4 ? c.H / 4 : c.H);  // whole waves per sequence
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    const bool drop = c.p_drop > 0.0f;
    if (vec4) { if (drop) launch_cell_pipe<ADAPT, 4, true, Args>(bwd, c, sg, blocks, st); else launch_cell_pipe<ADAPT, 4, false, Args>(bwd, c, sg, blocks, st); }
    else      { if (drop) launch_cell_pipe<ADAPT, 1, true, Args>(bwd, c, sg, blocks, st); else launch_cell_pipe<ADAPT, 1, false, Args>(bwd, c, sg, blocks, st); }
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// the streaming forward: no saved states, no dropout, the end state written back (same thread mapping as launch_cell)
template <bool ADAPT>
int launch_cell_stream(const CellArgs& c, hipStream_t st) {
    const long long work = (long long)c.B * c.H;
    const bool vec4 = (c.H % 4 == 0) && work >= (long long)256 * 8 * 64 * 4;
    const long long threads = vec4 ? work / 4 : work;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    auto go = [&](auto vec, auto sout, auto s16out) {
        hipLaunchKernelGGL((cell_fwd_pipe_kernel<ADAPT, decltype(vec)::value, 0, decltype(sout)::value,
                                                 decltype(s16out)::value, false, true>),
                           dim3(blocks), dim3(256), 0, st, c);
    };
    auto outs = [&](auto vec) {
        if (c.s_out && c.s16_out) go(vec, std::true_type{}, std::true_type{});
        else if (c.s_out) go(vec, std::true_type{}, std::false_type{});
        else go(vec, std::false_type{}, std::true_type{});
    };
    if (vec4) outs(std::integral_constant<int, 4>{});
    else outs(std::integral_constant<int, 1>{});
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

bool ptrs_aligned(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (p && !aligned16(p)) return false;
    return true;
}

// sparch_cell_fwd and sparch_cell_fwd_len (ragged: the row lengths, checked by the caller)
int cell_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                               const float* scale, const float* shift, const float* alpha,
                               const float* beta, const float* a, const float* b, const float* u0,
                               const float* w0, const float* s0, float theta, float p_drop,
                               uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                               int save_bf16, uint32_t* spike_count, void* stream, const int* lengths,
                               const int* offsets = nullptr) {
    if (kind != SPARCH_KIND_LIF && kind != SPARCH_KIND_ADLIF) return SPARCH_EINVAL;
    const bool adapt = kind == SPARCH_KIND_ADLIF;
    if (B <= 0 || T <= 0 || H <= 0 || (dirs != 1 && dirs != 2) || !Wx || !alpha || !u0 || !s0 || (!s_out && !s16_out))
        return SPARCH_EINVAL;
    if (adapt && (!beta || !a || !b || !w0)) return SPARCH_EINVAL;
    if (adapt && ((u_save == nullptr) != (w_save == nullptr))) return SPARCH_EINVAL;  // saved together or not at all
    if ((scale == nullptr) != (shift == nullptr)) return SPARCH_EINVAL;
    if (!(p_drop >= 0.0f && p_drop < 1.0f)) return SPARCH_EINVAL;
    if (!ptrs_aligned({Wx, u0, w0, s0, s_out, u_save, w_save})) return SPARCH_EALIGN;
    CellArgs c{};
    c.B = B; c.dirs = dirs; c.T = T; c.H = H;
    c.Wx = Wx; c.scale = scale; c.shift = shift;
    c.alpha = alpha; c.beta = beta; c.a = a; c.b = b;
    c.u0 = u0; c.w0 = w0; c.s0 = s0;
    c.theta = theta; c.p_drop = p_drop; c.inv_keep = 1.0f / (1.0f - p_drop); c.seed = seed;
    c.s_out = s_out; c.s16_out = s16_out; c.u_save = (float*)u_save; c.w_save = (float*)w_save;
    c.save16 = save_bf16 != 0; c.spike_count = spike_count;
    if (offsets) {
        CellPkArgs cp{c, lengths, offsets};
        return adapt ? launch_cell<true>(false, cp, (hipStream_t)stream) : launch_cell<false>(false, cp, (hipStream_t)stream);
    }
    if (lengths) {
        CellLenArgs cl{c, lengths};
        return adapt ? launch_cell<true>(false, cl, (hipStream_t)stream) : launch_cell<false>(false, cl, (hipStream_t)stream);
    }
    return adapt ? launch_cell<true>(false, c, (hipStream_t)stream)
                 : launch_cell<false>(false, c, (hipStream_t)stream);
}

// sparch_cell_bwd_sg and sparch_cell_bwd_len (ragged: n_valid is the rate gradient's sample count)
int cell_bwd(int kind, int B, int dirs, int T, int H, const float* g_out,
                                  const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                  const float* alpha, const float* beta, const float* a, const float* b,
                                  const float* u0, const float* w0, const float* s0, float theta,
                                  float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                                  const float* bn_mean, const float* bn_invstd, int surrogate, float surrogate_scale,
                                  void* stream, const int* lengths, long long n_valid, const int* offsets = nullptr) {
    if (!surrogate_ok(surrogate, surrogate_scale, save_bf16)) return SPARCH_EINVAL;
    if (kind != SPARCH_KIND_LIF && kind != SPARCH_KIND_ADLIF) return SPARCH_EINVAL;
    if (bn_x && (!bn_mean || !bn_invstd || !aligned16(bn_x))) return SPARCH_EINVAL;
    const bool adapt = kind == SPARCH_KIND_ADLIF;
    if (B <= 0 || T <= 0 || H <= 0 || (dirs != 1 && dirs != 2) || !g_out || !u_save || !alpha || !u0 ||
        !s0 || !dWx || !dparam_ws)
        return SPARCH_EINVAL;
    if (adapt && (!beta || !a || !b || !w0 || !w_save)) return SPARCH_EINVAL;
    if (!(p_drop >= 0.0f && p_drop < 1.0f)) return SPARCH_EINVAL;
    if (!ptrs_aligned({g_out, u_save, w_save, u0, w0, s0, dWx, dparam_ws})) return SPARCH_EALIGN;
    CellArgs c{};
    c.B = B; c.dirs = dirs; c.T = T; c.H = H;
    c.alpha = alpha; c.beta = beta; c.a = a; c.b = b;
    c.u0 = u0; c.w0 = w0; c.s0 = s0;
    c.theta = theta; c.p_drop = p_drop; c.inv_keep = 1.0f / (1.0f - p_drop); c.seed = seed;
    c.u_save = (float*)const_cast<void*>(u_save); c.w_save = (float*)const_cast<void*>(w_save);
    c.save16 = save_bf16 != 0;
    c.g_out = g_out; c.g_rate = g_rate;
    c.g_rate_scale = lengths ? 1.0f / (float)n_valid : 1.0f / ((float)B * (float)T);
    c.dWx = dWx; c.dparam_ws = dparam_ws;
    c.bn_x = bn_x; c.bn_mean = bn_mean; c.bn_invstd = bn_invstd;
    const SurrogateArgs sg{surrogate, surrogate_scale};
    if (offsets) {
        CellPkArgs cp{c, lengths, offsets};
        return adapt ? launch_cell<true>(true, cp, (hipStream_t)stream, sg) : launch_cell<false>(true, cp, (hipStream_t)stream, sg);
    }
    if (lengths) {
        CellLenArgs cl{c, lengths};
        return adapt ? launch_cell<true>(true, cl, (hipStream_t)stream, sg) : launch_cell<false>(true, cl, (hipStream_t)stream, sg);
    }
    return adapt ? launch_cell<true>(true, c, (hipStream_t)stream, sg)
                 : launch_cell<false>(true, c, (hipStream_t)stream, sg);
}

}  // namespace

extern "C" int sparch_cell_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                               const float* scale, const float* shift, const float* alpha,
                               const float* beta, const float* a, const float* b, const float* u0,
                               const float* w0, const float* s0, float theta, float p_drop,
                               uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                               int save_bf16, uint32_t* spike_count, void* stream) {
    SPARCH_ENTER();
    return cell_fwd(kind, B, dirs, T, H, Wx, scale, shift, alpha, beta, a, b, u0, w0, s0, theta, p_drop, seed, s_out,
                    s16_out, u_save, w_save, save_bf16, spike_count, stream, nullptr);
}

extern "C" int sparch_cell_fwd_len(int kind, int B, int dirs, int T, int H, const float* Wx,
                                   const float* scale, const float* shift, const float* alpha,
                                   const float* beta, const float* a, const float* b, const float* u0,
                                   const float* w0, const float* s0, float theta, float p_drop,
                                   uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                                   int save_bf16, uint32_t* spike_count, const int* lengths, long long n_valid,
                                   void* stream) {
    SPARCH_ENTER();
    if (!ragged_ok(dirs, lengths, n_valid)) return SPARCH_EINVAL;
    return cell_fwd(kind, B, dirs, T, H, Wx, scale, shift, alpha, beta, a, b, u0, w0, s0, theta, p_drop, seed, s_out,
                    s16_out, u_save, w_save, save_bf16, spike_count, stream, lengths);
}

extern "C" int sparch_cell_fwd_pk(int kind, int B, int dirs, int T, int H, const float* Wx,
                                  const float* scale, const float* shift, const float* alpha,
                                  const float* beta, const float* a, const float* b, const float* u0,
                                  const float* w0, const float* s0, float theta, float p_drop,
                                  uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                                  int save_bf16, uint32_t* spike_count, const int* lengths, const int* offsets,
                                  long long n_valid, void* stream) {
    SPARCH_ENTER();
    if (!packed_ok(dirs, lengths, offsets, n_valid)) return SPARCH_EINVAL;
    return cell_fwd(kind, B, dirs, T, H, Wx, scale, shift, alpha, beta, a, b, u0, w0, s0, theta, p_drop, seed, s_out,
                    s16_out, u_save, w_save, save_bf16, spike_count, stream, lengths, offsets);
}

extern "C" int sparch_cell_stream_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                                      const float* scale, const float* shift, const float* alpha,
                                      const float* beta, const float* a, const float* b, float* u, float* w,
                                      float* s, float theta, float p_drop, float* s_out, uint16_t* s16_out,
                                      uint32_t* spike_count, void* stream) {
    SPARCH_ENTER();
    if (kind != SPARCH_KIND_LIF && kind != SPARCH_KIND_ADLIF) return SPARCH_EINVAL;
    const bool adapt = kind == SPARCH_KIND_ADLIF;
    // a stream is causal (one direction) and runs in eval (no dropout); the state is mandatory
    if (dirs != 1 || p_drop != 0.0f || !u || !s || (adapt && !w)) return SPARCH_EINVAL;
    if (B <= 0 || T <= 0 || H <= 0 || !Wx || !alpha || (!s_out && !s16_out)) return SPARCH_EINVAL;
    if (adapt && (!beta || !a || !b)) return SPARCH_EINVAL;
    if ((scale == nullptr) != (shift == nullptr)) return SPARCH_EINVAL;
    if (!ptrs_aligned({Wx, u, w, s, s_out})) return SPARCH_EALIGN;
    CellArgs c{};
    c.B = B; c.dirs = 1; c.T = T; c.H = H;
    c.Wx = Wx; c.scale = scale; c.shift = shift;
    c.alpha = alpha; c.beta = beta; c.a = a; c.b = b;
    c.u0 = u; c.w0 = w; c.s0 = s;
    c.theta = theta; c.p_drop = 0.0f; c.inv_keep = 1.0f;
    c.s_out = s_out; c.s16_out = s16_out; c.spike_count = spike_count;
    return adapt ? launch_cell_stream<true>(c, (hipStream_t)stream) : launch_cell_stream<false>(c, (hipStream_t)stream);
}

extern "C" int sparch_cell_bwd_sg(int kind, int B, int dirs, int T, int H, const float* g_out,
                                  const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                  const float* alpha, const float* beta, const float* a, const float* b,
                                  const float* u0, const float* w0, const float* s0, float theta,
                                  float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                                  const float* bn_mean, const float* bn_invstd, int surrogate, float surrogate_scale,
                                  void* stream) {
    SPARCH_ENTER();
    return cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, u0, w0, s0, theta,
                    p_drop, seed, dWx, dparam_ws, bn_x, bn_mean, bn_invstd, surrogate, surrogate_scale, stream, nullptr, 0);
}

extern "C" int sparch_cell_bwd_len(int kind, int B, int dirs, int T, int H, const float* g_out,
                                   const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                   const float* alpha, const float* beta, const float* a, const float* b,
                                   const float* u0, const float* w0, const float* s0, float theta,
                                   float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                                   const float* bn_mean, const float* bn_invstd, const int* lengths, long long n_valid,
                                   int surrogate, float surrogate_scale, void* stream) {
    SPARCH_ENTER();
    if (!ragged_ok(dirs, lengths, n_valid)) return SPARCH_EINVAL;
    return cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, u0, w0, s0, theta,
                    p_drop, seed, dWx, dparam_ws, bn_x, bn_mean, bn_invstd, surrogate, surrogate_scale, stream, lengths,
                    n_valid);
}

extern "C" int sparch_cell_bwd_pk(int kind, int B, int dirs, int T, int H, const float* g_out,
                                  const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                  const float* alpha, const float* beta, const float* a, const float* b,
                                  const float* u0, const float* w0, const float* s0, float theta,
                                  float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                                  const float* bn_mean, const float* bn_invstd, const int* lengths, const int* offsets,
                                  long long n_valid, int surrogate, float surrogate_scale, void* stream) {
    SPARCH_ENTER();
    if (!packed_ok(dirs, lengths, offsets, n_valid)) return SPARCH_EINVAL;
    return cell_bwd(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, u0, w0, s0, theta,
                    p_drop, seed, dWx, dparam_ws, bn_x, bn_mean, bn_invstd, surrogate, surrogate_scale, stream, lengths,
                    n_valid, offsets);
}

extern "C" int sparch_cell_bwd(int kind, int B, int dirs, int T, int H, const float* g_out,
                               const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                               const float* alpha, const float* beta, const float* a, const float* b,
                               const float* u0, const float* w0, const float* s0, float theta,
                               float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                               const float* bn_mean, const float* bn_invstd, void* stream) {
    return sparch_cell_bwd_sg(kind, B, dirs, T, H, g_out, g_rate, u_save, w_save, save_bf16, alpha, beta, a, b, u0, w0,
                              s0, theta, p_drop, seed, dWx, dparam_ws, bn_x, bn_mean, bn_invstd,
                              SPARCH_SURROGATE_BOXCAR, 0.0f, stream);
}

namespace {
bool seq_mode_ok(int mode) { return mode == SPARCH_SEQ_PROB || mode == SPARCH_SEQ_SUM; }

// seq: the `_seq` forms' per-step output with its mode (never with offsets), else null
int readout_fwd(int B, int T, int C, const float* Wx, const float* scale, const float* shift, const float* alpha,
                const float* u0, float* out, float* u_save, const int* lengths, const int* offsets, void* stream,
                const RoSeq* seq = nullptr) {
    if (B <= 0 || T <= 0 || C <= 0 || C > 256 || !Wx || !alpha || !u0 || !out) return SPARCH_EINVAL;
    if ((scale == nullptr) != (shift == nullptr)) return SPARCH_EINVAL;
    if (seq && (!seq->seq || !seq_mode_ok(seq->mode) || offsets)) return SPARCH_EINVAL;
    const int rows = ro_chunk_steps(T, C, RO_FWD_FLOATS);
    if (seq && lengths)
        hipLaunchKernelGGL((readout_fwd_kernel<false, true, RoSeq>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C, rows,
                           Wx, scale, shift, alpha, u0, out, u_save, (float*)nullptr, lengths, *seq);
    else if (seq)
        hipLaunchKernelGGL((readout_fwd_kernel<false, false, RoSeq>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C, rows,
                           Wx, scale, shift, alpha, u0, out, u_save, (float*)nullptr, (const int*)nullptr, *seq);
    else if (offsets)
        hipLaunchKernelGGL((readout_fwd_kernel<false, true, const int*>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C,
                           rows, Wx, scale, shift, alpha, u0, out, u_save, (float*)nullptr, lengths, offsets);
    else if (lengths)
        hipLaunchKernelGGL((readout_fwd_kernel<false, true>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C, rows, Wx,
                           scale, shift, alpha, u0, out, u_save, (float*)nullptr, lengths);
    else
        hipLaunchKernelGGL((readout_fwd_kernel<false>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C, rows, Wx,
                           scale, shift, alpha, u0, out, u_save, (float*)nullptr, (const int*)nullptr);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// offsets: none, the packed form's `const int* offsets`, or the per-step form's `RoGSeq` (one chunk image more)
template <bool LEN, class... Offsets>
int readout_bwd(int B, int T, int C, const float* g_out, const float* bn_x, const float* bn_mean, const float* bn_invstd,
                const float* u_save, const float* alpha, const float* u0, float* dWx, float* dalpha_ws, const int* lengths,
                void* stream, Offsets... offsets) {
    // (dalpha uses u_{t-1}-x_t = (u_{t-1}-u_t)/(1-alpha): the projection is re-read only for BatchNorm's sums)
    constexpr bool SEQ = ro_has<RoGSeq, Offsets...>;
    constexpr int images = SEQ ? 4 : 3;
    if (B <= 0 || T <= 0 || C <= 0 || C > 256 || (!g_out && !SEQ) || !u_save || !alpha || !u0 || !dWx || !dalpha_ws)
        return SPARCH_EINVAL;
    if (bn_x && (!bn_mean || !bn_invstd)) return SPARCH_EINVAL;
    if constexpr (SEQ) {
        const RoGSeq sq = (offsets, ...);
        if (!sq.g_seq || !seq_mode_ok(sq.mode)) return SPARCH_EINVAL;
    }
    const int rows = ro_chunk_steps(T, C, RO_BWD_FLOATS / images);
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(readout_bwd_kernel<LEN, Offsets...>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)(RO_BWD_FLOATS * sizeof(float)));
    if (attr != hipSuccess) { sparch_note_hip_error((int)attr); return SPARCH_ELAUNCH; }
    hipLaunchKernelGGL((readout_bwd_kernel<LEN, Offsets...>), dim3(B), dim3(RO_NT),
                       (size_t)images * rows * ro_row_stride(C) * sizeof(float), (hipStream_t)stream, B, T, C, rows, g_out, u_save,
                       alpha, u0, dWx, dalpha_ws, bn_x, bn_mean, bn_invstd, lengths, offsets...);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}
}  // namespace

extern "C" int sparch_readout_fwd(int B, int T, int C, const float* Wx, const float* scale,
                                  const float* shift, const float* alpha, const float* u0, float* out,
                                  float* u_save, void* stream) {
    SPARCH_ENTER();
    return readout_fwd(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, nullptr, nullptr, stream);
}

extern "C" int sparch_readout_fwd_len(int B, int T, int C, const float* Wx, const float* scale,
                                      const float* shift, const float* alpha, const float* u0, float* out,
                                      float* u_save, const int* lengths, long long n_valid, void* stream) {
    SPARCH_ENTER();
    if (!ragged_ok(1, lengths, n_valid)) return SPARCH_EINVAL;
    return readout_fwd(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, lengths, nullptr, stream);
}

extern "C" int sparch_readout_fwd_pk(int B, int T, int C, const float* Wx, const float* scale,
                                     const float* shift, const float* alpha, const float* u0, float* out,
                                     float* u_save, const int* lengths, const int* offsets, long long n_valid,
                                     void* stream) {
    SPARCH_ENTER();
    if (!packed_ok(1, lengths, offsets, n_valid)) return SPARCH_EINVAL;
    return readout_fwd(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, lengths, offsets, stream);
}

extern "C" int sparch_readout_stream_fwd(int B, int T, int C, const float* Wx, const float* scale,
                                         const float* shift, const float* alpha, float* u, float* out,
                                         void* stream) {
    SPARCH_ENTER();
    if (B <= 0 || T <= 0 || C <= 0 || C > 256 || !Wx || !alpha || !u || !out) return SPARCH_EINVAL;
    if ((scale == nullptr) != (shift == nullptr)) return SPARCH_EINVAL;
    hipLaunchKernelGGL(readout_fwd_kernel<true>, dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C,
                       ro_chunk_steps(T, C, RO_FWD_FLOATS), Wx, scale, shift, alpha, (const float*)nullptr, out,
                       (float*)nullptr, u, (const int*)nullptr);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_readout_bwd(int B, int T, int C, const float* g_out, const float* bn_x,
                                  const float* bn_mean, const float* bn_invstd, const float* u_save,
                                  const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                                  void* stream) {
    SPARCH_ENTER();
    return readout_bwd<false>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, nullptr, stream);
}

extern "C" int sparch_readout_bwd_len(int B, int T, int C, const float* g_out, const float* bn_x,
                                      const float* bn_mean, const float* bn_invstd, const float* u_save,
                                      const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                                      const int* lengths, long long n_valid, void* stream) {
    SPARCH_ENTER();
    if (!ragged_ok(1, lengths, n_valid)) return SPARCH_EINVAL;
    return readout_bwd<true>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, lengths, stream);
}

// The per-step forms (include/sparch_hip.h).  They stand in front of sparch_readout_bwd_pk so that its kernel stays the
// last one this file emits: the per-symbol device-code digest sees the padding behind a kernel.
extern "C" int sparch_readout_fwd_seq(int B, int T, int C, const float* Wx, const float* scale,
                                      const float* shift, const float* alpha, const float* u0, float* out,
                                      float* u_save, float* seq, int seq_mode, void* stream) {
    SPARCH_ENTER();
    const RoSeq sq{seq, seq_mode};
    return readout_fwd(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, nullptr, nullptr, stream, &sq);
}

extern "C" int sparch_readout_fwd_seq_len(int B, int T, int C, const float* Wx, const float* scale,
                                          const float* shift, const float* alpha, const float* u0, float* out,
                                          float* u_save, float* seq, int seq_mode, const int* lengths,
                                          long long n_valid, void* stream) {
    SPARCH_ENTER();
    if (!ragged_ok(1, lengths, n_valid)) return SPARCH_EINVAL;
    const RoSeq sq{seq, seq_mode};
    return readout_fwd(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, lengths, nullptr, stream, &sq);
}

extern "C" int sparch_readout_bwd_seq(int B, int T, int C, const float* g_out, const float* g_seq, int seq_mode,
                                      const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                      const float* u_save, const float* alpha, const float* u0, float* dWx,
                                      float* dalpha_ws, void* stream) {
    SPARCH_ENTER();
    return readout_bwd<false>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, nullptr, stream,
                              RoGSeq{g_seq, seq_mode});
}

extern "C" int sparch_readout_bwd_seq_len(int B, int T, int C, const float* g_out, const float* g_seq, int seq_mode,
                                          const float* bn_x, const float* bn_mean, const float* bn_invstd,
                                          const float* u_save, const float* alpha, const float* u0, float* dWx,
                                          float* dalpha_ws, const int* lengths, long long n_valid, void* stream) {
    SPARCH_ENTER();
    if (!ragged_ok(1, lengths, n_valid)) return SPARCH_EINVAL;
    return readout_bwd<true>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, lengths, stream,
                             RoGSeq{g_seq, seq_mode});
}

extern "C" int sparch_readout_chunk_steps(int T, int C, int bwd, int seq) {
    if (T <= 0 || C <= 0 || C > 256) return 0;
    return ro_chunk_steps(T, C, bwd ? RO_BWD_FLOATS / (seq ? 4 : 3) : RO_FWD_FLOATS);
}

// Stateful training (include/sparch_hip.h), in front of sparch_readout_bwd_pk for the same reason.
// (launch_cell / launch_cell_pipe with Args = CellStArgs: the one thread-mapping rule and dispatch of every family)
extern "C" int sparch_cell_bwd_st(int kind, int B, int dirs, int T, int H, const float* g_out,
                                  const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                                  const float* alpha, const float* beta, const float* a, const float* b,
                                  const float* u0, const float* w0, const float* s0, float theta,
                                  float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                                  const float* bn_mean, const float* bn_invstd, int surrogate, float surrogate_scale,
                                  const float* g_uT, const float* g_wT, const float* g_sT, float* g_u0, float* g_w0,
                                  float* g_s0, void* stream) {
    SPARCH_ENTER();
    if (dirs != 1 || save_bf16 != 0) return SPARCH_EINVAL;  // a carried state is causal; the final state is read from fp32 saves
    if (!surrogate_ok(surrogate, surrogate_scale, 0)) return SPARCH_EINVAL;
    if (kind != SPARCH_KIND_LIF && kind != SPARCH_KIND_ADLIF) return SPARCH_EINVAL;
    if (bn_x && (!bn_mean || !bn_invstd || !aligned16(bn_x))) return SPARCH_EINVAL;
    const bool adapt = kind == SPARCH_KIND_ADLIF;
    if (B <= 0 || T <= 0 || H <= 0 || !g_out || !u_save || !alpha || !u0 || !s0 || !dWx || !dparam_ws) return SPARCH_EINVAL;
    if (adapt && (!beta || !a || !b || !w0 || !w_save)) return SPARCH_EINVAL;
    if (!(p_drop >= 0.0f && p_drop < 1.0f)) return SPARCH_EINVAL;
    if (!ptrs_aligned({g_out, u_save, w_save, u0, w0, s0, dWx, dparam_ws, g_uT, g_wT, g_sT, g_u0, g_w0, g_s0}))
        return SPARCH_EALIGN;
    CellStArgs c{};
    c.B = B; c.dirs = 1; c.T = T; c.H = H;
    c.alpha = alpha; c.beta = beta; c.a = a; c.b = b;
    c.u0 = u0; c.w0 = w0; c.s0 = s0;
    c.theta = theta; c.p_drop = p_drop; c.inv_keep = 1.0f / (1.0f - p_drop); c.seed = seed;
    c.u_save = (float*)const_cast<void*>(u_save); c.w_save = (float*)const_cast<void*>(w_save);
    c.save16 = 0;
    c.g_out = g_out; c.g_rate = g_rate;
    c.g_rate_scale = 1.0f / ((float)B * (float)T);
    c.dWx = dWx; c.dparam_ws = dparam_ws;
    c.bn_x = bn_x; c.bn_mean = bn_mean; c.bn_invstd = bn_invstd;
    c.g_uT = g_uT; c.g_wT = g_wT; c.g_sT = g_sT;
    c.g_u0 = g_u0; c.g_w0 = g_w0; c.g_s0 = g_s0;
    const SurrogateArgs sg{surrogate, surrogate_scale};
    return adapt ? launch_cell<true>(true, c, (hipStream_t)stream, sg) : launch_cell<false>(true, c, (hipStream_t)stream, sg);
}

extern "C" int sparch_readout_bwd_st(int B, int T, int C, const float* g_out, const float* bn_x,
                                     const float* bn_mean, const float* bn_invstd, const float* u_save,
                                     const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                                     const float* g_uT, float* g_u0, void* stream) {
    SPARCH_ENTER();
    return readout_bwd<false>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, nullptr, stream,
                              RoSt{g_uT, g_u0});
}

// The selectable readout (include/sparch_hip.h), in front of sparch_readout_bwd_pk for the same reason.
namespace {
// the `_red` entry points' refusals, in front of everything else
bool red_ok(int C, int red, const void* arg, const int* lengths, const int* offsets, long long n_valid) {
    if (red < SPARCH_RED_SOFTMAX_SUM || red > SPARCH_RED_U_LAST) return false;
    if (red == SPARCH_RED_U_MAX && !arg) return false;
    if (offsets && !lengths) return false;
    if (lengths && n_valid < 1) return false;
    return C <= 256;
}

template <int M>
int readout_fwd_red(int B, int T, int C, const float* Wx, const float* scale, const float* shift, const float* alpha,
                    const float* u0, float* out, float* u_save, int* arg, const int* lengths, const int* offsets,
                    void* stream) {
    const int rows = ro_chunk_steps(T, C, RO_FWD_FLOATS);
    const RoRed<M> red{arg};
    if (offsets)
        hipLaunchKernelGGL((readout_fwd_kernel<false, true, const int*, RoRed<M>>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream,
                           B, T, C, rows, Wx, scale, shift, alpha, u0, out, u_save, (float*)nullptr, lengths, offsets, red);
    else if (lengths)
        hipLaunchKernelGGL((readout_fwd_kernel<false, true, RoRed<M>>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C,
                           rows, Wx, scale, shift, alpha, u0, out, u_save, (float*)nullptr, lengths, red);
    else
        hipLaunchKernelGGL((readout_fwd_kernel<false, false, RoRed<M>>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C,
                           rows, Wx, scale, shift, alpha, u0, out, u_save, (float*)nullptr, (const int*)nullptr, red);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

template <int M>
int readout_bwd_red(int B, int T, int C, const float* g_out, const float* bn_x, const float* bn_mean,
                    const float* bn_invstd, const float* u_save, const float* alpha, const float* u0, float* dWx,
                    float* dalpha_ws, const int* arg, const int* lengths, const int* offsets, void* stream) {
    const RoRed<M> red{const_cast<int*>(arg)};  // (the backward only reads it)
    if (offsets)
        return readout_bwd<true>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, lengths, stream,
                                 offsets, red);
    if (lengths)
        return readout_bwd<true>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, lengths, stream,
                                 red);
    return readout_bwd<false>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, nullptr, stream,
                              red);
}

template <int M>
int readout_stream_fwd_red(int B, int T, int C, const float* Wx, const float* scale, const float* shift,
                           const float* alpha, float* u, float* out, void* stream) {
    hipLaunchKernelGGL((readout_fwd_kernel<true, false, RoRed<M>>), dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, B, T, C,
                       ro_chunk_steps(T, C, RO_FWD_FLOATS), Wx, scale, shift, alpha, (const float*)nullptr, out,
                       (float*)nullptr, u, (const int*)nullptr, RoRed<M>{nullptr});
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}
}  // namespace

extern "C" int sparch_readout_fwd_red(int B, int T, int C, const float* Wx, const float* scale,
                                      const float* shift, const float* alpha, const float* u0, float* out,
                                      float* u_save, int red, int* arg, const int* lengths, const int* offsets,
                                      long long n_valid, void* stream) {
    SPARCH_ENTER();
    if (!red_ok(C, red, arg, lengths, offsets, n_valid)) return SPARCH_EINVAL;
    if (red == SPARCH_RED_SOFTMAX_SUM)  // the softmax-sum's own entry points
        return offsets   ? sparch_readout_fwd_pk(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, lengths, offsets, n_valid, stream)
               : lengths ? sparch_readout_fwd_len(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, lengths, n_valid, stream)
                         : sparch_readout_fwd(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, stream);
    if (B <= 0 || T <= 0 || C <= 0 || !Wx || !alpha || !u0 || !out) return SPARCH_EINVAL;
    if ((scale == nullptr) != (shift == nullptr)) return SPARCH_EINVAL;
    switch (red) {
        case SPARCH_RED_SOFTMAX_MEAN:
            return readout_fwd_red<SPARCH_RED_SOFTMAX_MEAN>(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, arg, lengths, offsets, stream);
        case SPARCH_RED_U_MAX:
            return readout_fwd_red<SPARCH_RED_U_MAX>(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, arg, lengths, offsets, stream);
        case SPARCH_RED_U_MEAN:
            return readout_fwd_red<SPARCH_RED_U_MEAN>(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, arg, lengths, offsets, stream);
        default:
            return readout_fwd_red<SPARCH_RED_U_LAST>(B, T, C, Wx, scale, shift, alpha, u0, out, u_save, arg, lengths, offsets, stream);
    }
}

extern "C" int sparch_readout_stream_fwd_red(int B, int T, int C, const float* Wx, const float* scale,
                                             const float* shift, const float* alpha, float* u, float* out, int red,
                                             void* stream) {
    SPARCH_ENTER();
    if (red < SPARCH_RED_SOFTMAX_SUM || red > SPARCH_RED_U_LAST || C > 256) return SPARCH_EINVAL;
    if (red == SPARCH_RED_SOFTMAX_SUM || red == SPARCH_RED_SOFTMAX_MEAN)  // (the mean's division is the caller's)
        return sparch_readout_stream_fwd(B, T, C, Wx, scale, shift, alpha, u, out, stream);
    if (B <= 0 || T <= 0 || C <= 0 || !Wx || !alpha || !u || !out) return SPARCH_EINVAL;
    if ((scale == nullptr) != (shift == nullptr)) return SPARCH_EINVAL;
    switch (red) {
        case SPARCH_RED_U_MAX: return readout_stream_fwd_red<SPARCH_RED_U_MAX>(B, T, C, Wx, scale, shift, alpha, u, out, stream);
        case SPARCH_RED_U_MEAN: return readout_stream_fwd_red<SPARCH_RED_U_MEAN>(B, T, C, Wx, scale, shift, alpha, u, out, stream);
        default: return readout_stream_fwd_red<SPARCH_RED_U_LAST>(B, T, C, Wx, scale, shift, alpha, u, out, stream);
    }
}

extern "C" int sparch_readout_bwd_pk(int B, int T, int C, const float* g_out, const float* bn_x,
                                     const float* bn_mean, const float* bn_invstd, const float* u_save,
                                     const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                                     const int* lengths, const int* offsets, long long n_valid, void* stream);

extern "C" int sparch_readout_bwd_red(int B, int T, int C, const float* g_out, const float* bn_x,
                                      const float* bn_mean, const float* bn_invstd, const float* u_save,
                                      const float* alpha, const float* u0, float* dWx, float* dalpha_ws, int red,
                                      const int* arg, const int* lengths, const int* offsets, long long n_valid,
                                      void* stream) {
    SPARCH_ENTER();
    if (!red_ok(C, red, arg, lengths, offsets, n_valid)) return SPARCH_EINVAL;
    if (red == SPARCH_RED_SOFTMAX_SUM)
        return offsets   ? sparch_readout_bwd_pk(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, lengths, offsets, n_valid, stream)
               : lengths ? sparch_readout_bwd_len(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, lengths, n_valid, stream)
                         : sparch_readout_bwd(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, stream);
    switch (red) {
        case SPARCH_RED_SOFTMAX_MEAN:
            return readout_bwd_red<SPARCH_RED_SOFTMAX_MEAN>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, arg, lengths, offsets, stream);
        case SPARCH_RED_U_MAX:
            return readout_bwd_red<SPARCH_RED_U_MAX>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, arg, lengths, offsets, stream);
        case SPARCH_RED_U_MEAN:
            return readout_bwd_red<SPARCH_RED_U_MEAN>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, arg, lengths, offsets, stream);
        default:
            return readout_bwd_red<SPARCH_RED_U_LAST>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, arg, lengths, offsets, stream);
    }
}

extern "C" int sparch_readout_bwd_pk(int B, int T, int C, const float* g_out, const float* bn_x,
                                     const float* bn_mean, const float* bn_invstd, const float* u_save,
                                     const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                                     const int* lengths, const int* offsets, long long n_valid, void* stream) {
    SPARCH_ENTER();
    if (!packed_ok(1, lengths, offsets, n_valid)) return SPARCH_EINVAL;
    return readout_bwd<true>(B, T, C, g_out, bn_x, bn_mean, bn_invstd, u_save, alpha, u0, dWx, dalpha_ws, lengths, stream,
                                   offsets);
}

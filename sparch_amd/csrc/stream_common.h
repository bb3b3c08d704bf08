// What the streaming steps share.  The two fused spiking steps (streamstep.hip: dense; streamsparse.hip: event-driven)
// share all but how x_t W^T and s V are summed: the argument struct, the entries' checks, the kernel dispatch, the device
// tails.  The dense spiking step and the baselines' step (streamann.hip) share the row-tile rule and switch, the geometry
// of a workgroup, the staged dense dot product stream_dot and the wave sum.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "neuron.h"

namespace {

// W / V: the dense step's W (H,K) and vmask_t (H,ld); the event-driven step's Wt (K,ldw) and vmask (H,ld)
struct StreamArgs {
    int B, K, H, ld, ldx, ldw, in_u8;  // (ldw: the event-driven step only)
    const void* x;
    const float *W, *bias, *scale, *shift, *alpha, *beta, *a, *b, *V;
    float *u, *w;
    const float* s_in;
    float* s_out;
    uint16_t* s16_out;
    float theta;
    uint32_t* spike_count;
};

bool all16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (p && !aligned16(p)) return false;
    return true;
}

// the smallest row tile that holds the batch: fewer accumulators and LDS reads for the few-row stream
int stream_row_tile(int B) { return B >= 9 ? 16 : B >= 5 ? 8 : B >= 3 ? 4 : B; }

// The hidden-layer entries' checks (every SPARCH_EINVAL before SPARCH_EALIGN).  transposed: the weights are Wt (K,ldw).
int stream_step_check(int kind, int in_dtype, const StreamArgs& g, bool transposed) {
    if (kind != SPARCH_KIND_LIF && kind != SPARCH_KIND_ADLIF && kind != SPARCH_KIND_RLIF && kind != SPARCH_KIND_RADLIF)
        return SPARCH_EINVAL;
    const bool adapt = kind == SPARCH_KIND_ADLIF || kind == SPARCH_KIND_RADLIF;
    const bool rec = kind == SPARCH_KIND_RLIF || kind == SPARCH_KIND_RADLIF;
    if (in_dtype != 0 && in_dtype != 1) return SPARCH_EINVAL;
    if (g.B <= 0 || g.K <= 0 || g.H <= 0 || g.ld < g.H || g.ldx < g.K) return SPARCH_EINVAL;
    if (transposed && (g.ldw < g.H || (g.ldw & 3) != 0)) return SPARCH_EINVAL;
    if (!g.x || !g.W || !g.alpha || !g.u || !g.s_in || !g.s_out) return SPARCH_EINVAL;
    if (adapt && (!g.beta || !g.a || !g.b || !g.w)) return SPARCH_EINVAL;
    if (rec && (!g.V || g.s_in == g.s_out)) return SPARCH_EINVAL;  // every workgroup reads all of s_in
    if ((g.scale == nullptr) != (g.shift == nullptr)) return SPARCH_EINVAL;
    if (!all16({g.W, g.V, g.u, g.w, g.s_in, g.s_out, g.s16_out})) return SPARCH_EALIGN;
    if (cdiv(g.B, stream_row_tile(g.B)) > 65535) return SPARCH_EINVAL;  // grid.y walks the row tiles
    return SPARCH_OK;
}

// The readout entries' checks.  transposed: the weights are Wt (K,ldc).
int stream_readout_check(int B, int K, int C, const float* x, int ldx, const float* W, bool transposed, int ldc,
                         const float* scale, const float* shift, const float* alpha, const float* u, const float* out) {
    if (B <= 0 || K <= 0 || C <= 0 || C > 256 || ldx < K) return SPARCH_EINVAL;
    if (transposed && (ldc < C || (ldc & 3) != 0)) return SPARCH_EINVAL;
    if (!x || !W || !alpha || !u || !out) return SPARCH_EINVAL;
    if ((scale == nullptr) != (shift == nullptr)) return SPARCH_EINVAL;
    if (!aligned16(W)) return SPARCH_EALIGN;
    return SPARCH_OK;
}

// f(row tile) as a compile-time constant, for a row tile of stream_row_tile()
template <class F>
void stream_row_tiles(int RT, F&& f) {
    switch (RT) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}

// f(row tile, ADAPT, REC) as compile-time constants, for a checked kind and a row tile of stream_row_tile()
template <class F>
void stream_dispatch(int RT, int kind, F&& f) {
    stream_row_tiles(RT, [&](auto rt) {
        switch (kind) {
            case SPARCH_KIND_LIF: f(rt, std::false_type{}, std::false_type{}); break;
            case SPARCH_KIND_ADLIF: f(rt, std::true_type{}, std::false_type{}); break;
            case SPARCH_KIND_RLIF: f(rt, std::false_type{}, std::true_type{}); break;
            default: f(rt, std::true_type{}, std::true_type{}); break;
        }
    });
}

// ---- device side.  The operands of the pointwise phase are asked for at kernel entry, unclamped, so that they arrive
//      while the dot products run; the tails clamp and use them.
template <bool ADAPT>
struct StreamColumn {  // what one column (hidden unit, or class of the readout) brings
    Neuron<ADAPT> raw;
    float bias, sc, sh;
};
template <bool ADAPT>
__device__ __forceinline__ StreamColumn<ADAPT> stream_column(const float* alpha, const float* beta, const float* a,
                                                             const float* b, const float* bias, const float* scale,
                                                             const float* shift, int i) {
    return {neuron_load_raw<ADAPT>(alpha, beta, a, b, i), bias ? bias[i] : 0.f, scale ? scale[i] : 1.f,
            scale ? shift[i] : 0.f};
}

// One (row, column) of a hidden layer behind its two sums sx = x_t W^T and sr = s V: the membrane step on the
// prefetched state (u, w, s), the new state and the spike plane at offset o, the spike count of column h.
template <bool ADAPT, bool REC>
__device__ __forceinline__ void stream_pointwise(const StreamArgs& a, const StreamColumn<ADAPT>& col, float sx,
                                                 float sr, float u, float w, float s, size_t o, int h) {
    const Neuron<ADAPT> p = neuron_clamp(col.raw);
    const float xn = neuron_input(sx, a.bias != nullptr, col.bias, a.scale != nullptr, col.sc, col.sh);
    neuron_step<ADAPT, REC>(u, w, s, xn, sr, p, a.theta);
    const bool spike = s != 0.0f;
    if (ADAPT) a.w[o] = w;
    a.u[o] = u;
    a.s_out[o] = s;
    if (a.s16_out) a.s16_out[o] = spike_bf16(spike);
    if (spike && a.spike_count) atomicAdd(a.spike_count + h, 1u);
}

// The readout's step behind its sum wx (thread = class tid < C of batch row b; all threads of the workgroup call): the
// recurrence of readout_fwd_kernel (cell.hip), then the softmax by one thread in the arithmetic (and the order) of that
// kernel's thread = time phase, then out += softmax(u).  `row`: >= C floats of LDS.
__device__ __forceinline__ void stream_readout_tail(float* row, bool act, int b, int C, float wx,
                                                    const StreamColumn<false>& col, bool has_bias, bool has_scale,
                                                    float u_prev, float out_prev, float* u_io, float* out) {
    // (the element's offset is formed HERE, from tid: formed from the clamped class index of the callers' prefetch it
    // is the prefetch's own address, kept live across their loops — stream_step_readout_kernel<false> then spills)
    const int tid = threadIdx.x;
    const size_t o = (size_t)b * C + tid;
    if (act) {
        const Neuron<false> p = neuron_clamp(col.raw);
        const float xn = neuron_input(wx, has_bias, col.bias, has_scale, col.sc, col.sh);
        const float u = readout_step(u_prev, xn, p.al, p.oma);
        u_io[o] = u;
        row[tid] = u;
    }
    __syncthreads();
    if (tid == 0) {
        const float den = ro_softmax_row(row, C);
        for (int c = 0; c < C; ++c) row[c] = row[c] / den;
    }
    __syncthreads();
    if (act) out[o] = out_prev + row[tid];                   // snns.py:823
}

// ---- the dense steps' dot products (streamstep.hip, streamann.hip): a workgroup is 4 waves and owns 4 adjacent columns
//      (one per wave) for one tile of RT <= 16 batch rows
constexpr int STREAM_NT = 256;   // 4 waves
constexpr int STREAM_COLS = 4;   // columns per workgroup: one per wave
// floats of one staged row piece: the tile is RT x KP floats of LDS (<= 32 KB)
__host__ __device__ constexpr int stream_piece(int RT) { return RT <= 8 ? 1024 : 512; }

// acc[g][r] += sum_k src[r0 + r][k] * wrow[g][k], k < K.  All 256 threads stage the tile's piece once for the G gates;
// the calling wave's lanes stride over k.  A wave without a column is given any valid rows (it stages, keeps the
// barriers, and its sums are never read).  U8: src holds uint8 counts, not floats.
// VEC: rows of the weight matrices are 16-byte aligned (base aligned, row stride a multiple of 4) — 16-byte loads;
// otherwise scalar loads throughout (a compile-time choice: as a run-time one hipcc issues the loads of both forms).
// TAIL: K itself need not be a multiple of 4 (the spiking step's V, K = H in rows of ld floats): 16-byte loads up to
// K & ~3, the <= 3 left over by the first lanes.  Without it VEC says that K is a multiple of 4.
// Every global load is UNCONDITIONAL on a clamped address and masked where it is used: a load under a branch makes
// hipcc wait for it at the join, one round trip per load instead of one per piece.
template <int RT, int G, bool U8, bool VEC, bool TAIL>
__device__ __forceinline__ void stream_dot(float* xs, const void* src, int ld_src, const float* const (&wrow)[G], int K,
                                           int r0, int B, float (&acc)[G][RT]) {
    constexpr int KP = stream_piece(RT), NV = KP / 256, NS = KP / 64, NI = KP / STREAM_NT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int Kv = VEC ? (TAIL ? (K & ~3) : K) : 0;
    for (int k0 = 0; k0 < K; k0 += KP) {
        const int klen = min(KP, K - k0);
        // ---- this wave's weights of the piece -> registers (in flight while the tile is staged)
        f32x4 wv[G][VEC ? NV : 1];
        float ws[G][VEC ? 1 : NS];
        float wt[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            wt[g] = 0.f;
            if (VEC) {
#pragma unroll
                for (int i = 0; i < NV; ++i)  // (a row of a vec matrix holds (K + 3) & ~3 floats: the clamp stays inside)
                    wv[g][i] = *reinterpret_cast<const f32x4*>(
                        wrow[g] + min(k0 + (i * 64 + lane) * 4, TAIL ? max(Kv - 4, 0) : K - 4));
                if (TAIL) wt[g] = wrow[g][min(Kv + lane, K - 1)];
            } else {
#pragma unroll
                for (int i = 0; i < NS; ++i) ws[g][i] = wrow[g][min(k0 + i * 64 + lane, K - 1)];
            }
        }
        // ---- the row tile's piece -> LDS (rows past B as zeros): all loads first, then the stores
        float xv[RT][NI];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const size_t o = (size_t)min(r0 + r, B - 1) * ld_src;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const size_t oo = o + min(k0 + tid + i * STREAM_NT, K - 1);
                xv[r][i] = U8 ? (float)static_cast<const uint8_t*>(src)[oo] : static_cast<const float*>(src)[oo];
            }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int kk = tid + i * STREAM_NT;
                if (kk < klen) xs[r * KP + kk] = (r0 + r < B) ? xv[r][i] : 0.f;
            }
        }
        __syncthreads();
        if (VEC) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int kk = (i * 64 + lane) * 4;
                if (TAIL ? k0 + kk < Kv : kk < klen) {
#pragma unroll
                    for (int r = 0; r < RT; ++r) {
                        const f32x4 x4 = *reinterpret_cast<const f32x4*>(&xs[r * KP + kk]);
#pragma unroll
                        for (int g = 0; g < G; ++g) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[g][r] = __builtin_fmaf(wv[g][i][e], x4[e], acc[g][r]);
                        }
                    }
                }
            }
            if (TAIL) {
                // the <= 3 columns behind the last 16 bytes (the lane's term joined by &: both sides are plain
                // compares, and hipcc then forms the mask as it does for one gate without a gate loop around wt)
                if ((Kv >= k0 && Kv < k0 + KP) & (Kv + lane < K)) {
#pragma unroll
                    for (int r = 0; r < RT; ++r) {
                        const float xk = xs[r * KP + (Kv - k0) + lane];
#pragma unroll
                        for (int g = 0; g < G; ++g) acc[g][r] = __builtin_fmaf(wt[g], xk, acc[g][r]);
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int kk = i * 64 + lane;
                if (kk < klen) {
#pragma unroll
                    for (int r = 0; r < RT; ++r) {
                        const float xk = xs[r * KP + kk];
#pragma unroll
                        for (int g = 0; g < G; ++g) acc[g][r] = __builtin_fmaf(ws[g][i], xk, acc[g][r]);
                    }
                }
            }
        }
        __syncthreads();  // the piece is consumed: the next one (or the next operand) may be staged
    }
}

// the 64 lane partials of a wave, added by a butterfly: every lane holds the sum
__device__ __forceinline__ float stream_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

}  // namespace

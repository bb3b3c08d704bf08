// Streaming inference for the non-spiking baselines (MLP, RNN, LiGRU, GRU; sparch_amd/anns.py), ONE time step per call.
//
// sparch_ann_stream_step     one hidden layer, one step, all rows: the projection(s) x_t W?^T (+ bias, eval BatchNorm
//                            affine), the recurrent product(s) y V?^T and the cell, in one launch (GRU: two launches,
//                            phase 1 = gates z, r and r * y, phase 2 = candidate and new state).
// sparch_ann_stream_readout  the readout's step: acc += softmax(y_t), out = norm(acc W^T + bias).
//
// The whole-sequence entry points (sparch_ann_rec_fwd, sparch_ligru_fwd, sparch_gru_fwd, sparch_softmax_sum_fwd) start
// from y = 0 and return no state; here the state goes in and comes out, so a live stream costs one kernel boundary per
// layer and step instead of a forward over the whole prefix.  Nothing waits inside a launch: every workgroup of a
// recurrent phase reads the WHOLE previous state (GRU phase 2: all of r * y) and writes its own columns of another
// buffer, so the only ordering is the kernel boundary.
//
// Shape (hidden layer), that of stream_step_kernel (streamstep.hip): a workgroup is 4 waves and owns 4 adjacent columns
// (one per wave) for one tile of RT <= 16 batch rows (grid.y walks the row tiles: no batch cap).  A wave's column is one
// row of every weight matrix of the phase — W? (H,K) and V? (H,H) as stored: row h of V is what y V^T needs, no
// transpose, no mask —, streamed once per row tile straight into registers (16-byte loads where K and H are multiples
// of 4, scalar loads otherwise; issued before the tile is staged); the row tile of x_t, then of y, sits in LDS in
// K-pieces, staged ONCE for all gates of the phase and read by all four waves.  Dot products are fp32 FMA chains, 64
// lane partials per (row, column, gate) added by a butterfly.  The dot product is stream_dot of stream_common.h, the one
// of the spiking step, here with the phase's gates, fp32 input and the column tail off; the workgroup's geometry and
// the row-tile switch are that header's too.
//
// The arithmetic is the expression trees of annstep.hip / gatedcell.hip / act.hip (this file is built with
// -ffp-contract=off): sigm(v) = 1 / (1 + expf(-v)), ReLU keeps a NaN, tanhf, the projection through neuron_input.
#include "stream_common.h"

namespace {

// what a launch computes; the gate slots of AnnArgs it uses
enum { SA_MLP = 0, SA_RNN = 1, SA_LIGRU = 2, SA_GRU1 = 3, SA_GRU2 = 4 };
//   SA_MLP / SA_RNN / SA_GRU2   slot 0 = the candidate (W, V)
//   SA_LIGRU                    slot 0 = the candidate, slot 1 = the update gate z
//   SA_GRU1                     slot 0 = the update gate z, slot 1 = the reset gate r
__host__ __device__ constexpr int sa_gates(int mode) { return (mode == SA_LIGRU || mode == SA_GRU1) ? 2 : 1; }

struct AnnArgs {
    int B, K, H, ld, ldx, act;
    const float* x;                                       // (B,K) row stride ldx, or NULL: the projections are `pre`
    const float *W[2], *bias[2], *scale[2], *shift[2], *pre[2], *V[2];
    const float* y_in;                                    // (B,H) row stride ld: the previous state
    const float* rec;                                     // what V multiplies: y_in, in GRU phase 2 r * y
    float *y_out, *z, *ry;                                // (B,H) row stride ld
};

__device__ __forceinline__ float sa_sigm(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ float sa_act(int kind, float v) {
    if (kind == SPARCH_ACT_SIGMOID) return sa_sigm(v);
    if (kind == SPARCH_ACT_RELU) return v <= 0.0f ? 0.0f : v;  // a NaN stays a NaN
    return tanhf(v);
}

template <int RT, int MODE, bool VEC>
__global__ __launch_bounds__(STREAM_NT) void ann_stream_step_kernel(AnnArgs a) {
    constexpr int G = sa_gates(MODE), KP = stream_piece(RT);
    constexpr bool REC = MODE != SA_MLP;
    __shared__ __attribute__((aligned(16))) float xs[RT * KP];
    __shared__ float red[2][G][RT][STREAM_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h0 = blockIdx.x * STREAM_COLS, r0 = blockIdx.y * RT;
    const int hw = min(h0 + wave, a.H - 1);  // this wave's column (a wave past H: any valid one, never read)
    // ---- the pointwise phase's operands, asked for now (thread = (row, column)): they arrive while the dot products run
    const int r = tid >> 2, c = tid & 3;
    const int row = r0 + r, h = h0 + c;
    const bool valid = r < RT && row < a.B && h < a.H;
    const int hc = min(h, a.H - 1), rc = min(row, a.B - 1);
    const size_t o = (size_t)rc * a.ld + hc;
    const bool proj = a.x != nullptr;
    const float yp = REC ? a.y_in[o] : 0.f;
    const float zp = MODE == SA_GRU2 ? a.z[o] : 0.f;
    float pb[G], psc[G], psh[G], ppre[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        pb[g] = a.bias[g] ? a.bias[g][hc] : 0.f;
        psc[g] = a.scale[g] ? a.scale[g][hc] : 1.f;
        psh[g] = a.scale[g] ? a.shift[g][hc] : 0.f;
        ppre[g] = proj ? 0.f : a.pre[g][(size_t)rc * a.H + hc];
    }

    float accx[G][RT], accr[G][RT];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int i = 0; i < RT; ++i) accx[g][i] = accr[g][i] = 0.f;
    }
    if (proj) {
        const float* wr[G];
#pragma unroll
        for (int g = 0; g < G; ++g) wr[g] = a.W[g] + (size_t)hw * a.K;
        stream_dot<RT, G, false, VEC, false>(xs, a.x, a.ldx, wr, a.K, r0, a.B, accx);
    }
    if (REC) {
        const float* vr[G];
#pragma unroll
        for (int g = 0; g < G; ++g) vr[g] = a.V[g] + (size_t)hw * a.H;
        stream_dot<RT, G, false, VEC, false>(xs, a.rec, a.ld, vr, a.H, r0, a.B, accr);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const float sx = stream_wave_sum(accx[g][i]);
            const float sr = REC ? stream_wave_sum(accr[g][i]) : 0.f;
            if (lane == 0) {
                red[0][g][i][wave] = sx;
                red[1][g][i][wave] = sr;
            }
        }
    }
    __syncthreads();
    if (!valid) return;
    float p[G], s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        p[g] = proj ? neuron_input(red[0][g][r][c], a.bias[g] != nullptr, pb[g], a.scale[g] != nullptr, psc[g], psh[g])
                    : ppre[g];
        s[g] = red[1][g][r][c];
    }
    if (MODE == SA_MLP) {
        a.y_out[o] = sa_act(a.act, p[0]);                          // anns.py:226
    } else if (MODE == SA_RNN) {
        a.y_out[o] = sa_act(a.act, p[0] + s[0]);                   // anns.py:336
    } else if (MODE == SA_LIGRU) {
        const float z = sa_sigm(p[1] + s[1]);                      // anns.py:457
        const float pc = p[0] + s[0];
        const float cand = pc <= 0.0f ? 0.0f : pc;                 // anns.py:458
        a.y_out[o] = z * yp + (1.0f - z) * cand;                   // anns.py:459
    } else if (MODE == SA_GRU1) {
        const float z = sa_sigm(p[0] + s[0]);                      // anns.py:589
        const float rg = sa_sigm(p[1] + s[1]);                     // anns.py:590
        a.z[o] = z;
        a.ry[o] = rg * yp;
    } else {
        const float cand = tanhf(p[0] + s[0]);                     // anns.py:591
        a.y_out[o] = zp * yp + (1.0f - zp) * cand;                 // anns.py:592
    }
}

// ---- readout: one workgroup per batch row, 16 waves.  acc (K floats) is updated by its owners (thread = features
//      tid, tid + 1024, ..), kept in LDS for the product; a wave takes classes wave, wave + 16, .., lanes stride over K.
constexpr int AR_NT = 1024;
constexpr int AR_KMAX = 4096;
constexpr int AR_CMAX = 256;

// max or sum over the workgroup: butterfly per wave, then the 16 wave values in a fixed order by every thread
__device__ __forceinline__ float ar_reduce(float v, bool is_max, float* red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float w = __shfl_xor(v, off, 64);
        v = is_max ? fmaxf(v, w) : v + w;
    }
    __syncthreads();  // protects `red` from the previous use
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int i = 1; i < AR_NT / 64; ++i) t = is_max ? fmaxf(t, red[i]) : t + red[i];
    return t;
}

template <bool VEC>  // 16-byte weight loads (K a multiple of 4) or scalar ones
__global__ __launch_bounds__(AR_NT) void ann_stream_readout_kernel(int K, int C, const float* __restrict__ y, int ldy,
                                                                   float* acc, const float* __restrict__ W,
                                                                   const float* __restrict__ bias, int norm,
                                                                   const float* __restrict__ p0,
                                                                   const float* __restrict__ p1, float eps,
                                                                   float* __restrict__ out) {
    constexpr int NI = AR_KMAX / AR_NT;
    __shared__ __attribute__((aligned(16))) float as[AR_KMAX];
    __shared__ float row[AR_CMAX];
    __shared__ float red[AR_NT / 64];
    __shared__ float stat[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const float* yr = y + (size_t)b * ldy;
    float* ar = acc + (size_t)b * K;
    // the class operands, asked for now
    const bool cls = tid < C;
    const int cc = cls ? tid : 0;
    const float cb = bias ? bias[cc] : 0.f;
    const float c0 = norm != SPARCH_RO_NORM_NONE ? p0[cc] : 1.f, c1 = norm != SPARCH_RO_NORM_NONE ? p1[cc] : 0.f;
    // ---- acc += softmax(y_t): anns.py:658-663, in the arithmetic of softmax_sum_kernel (act.hip)
    float v[NI], a0[NI];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int k = tid + i * AR_NT, kc = min(k, K - 1);
        v[i] = yr[kc];
        a0[i] = ar[kc];
        if (k < K) m = fmaxf(m, v[i]);
    }
    m = ar_reduce(m, true, red, tid);
    float den = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (tid + i * AR_NT < K) {
            v[i] = expf(v[i] - m);
            den += v[i];
        }
    }
    den = ar_reduce(den, false, red, tid);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int k = tid + i * AR_NT;
        if (k < K) {
            const float sum = a0[i] + v[i] / den;                  // anns.py:663
            ar[k] = sum;
            as[k] = sum;
        }
    }
    __syncthreads();
    // ---- row[c] = acc W[c]^T
    for (int c = wave; c < C; c += AR_NT / 64) {
        const float* wr = W + (size_t)c * K;
        float d = 0.f;
        if (VEC) {
            for (int k = lane * 4; k < K; k += 256) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + k);
                const f32x4 x4 = *reinterpret_cast<const f32x4*>(&as[k]);
#pragma unroll
                for (int e = 0; e < 4; ++e) d = __builtin_fmaf(w4[e], x4[e], d);
            }
        } else {
            for (int k = lane; k < K; k += 64) d = __builtin_fmaf(wr[k], as[k], d);
        }
        d = stream_wave_sum(d);
        if (lane == 0) row[c] = d;
    }
    __syncthreads();
    // ---- out = norm(row + bias): anns.py:650-654
    const float wy = bias ? row[cc] + cb : row[cc];
    if (norm == SPARCH_RO_NORM_LAYERNORM) {  // over the C outputs, in the arithmetic of layernorm_fwd_kernel (norm.hip)
        __syncthreads();
        if (cls) row[tid] = wy;
        __syncthreads();
        if (wave == 0) {
            float sm = 0.f;
            for (int c = lane; c < C; c += 64) sm += row[c];
            const float mean = stream_wave_sum(sm) / (float)C;
            float sq = 0.f;
            for (int c = lane; c < C; c += 64) {
                const float dv = row[c] - mean;
                sq += dv * dv;
            }
            const float var = stream_wave_sum(sq) / (float)C;
            if (lane == 0) {
                stat[0] = mean;
                stat[1] = 1.0f / sqrtf(var + eps);
            }
        }
        __syncthreads();
        if (cls) out[(size_t)b * C + tid] = (wy - stat[0]) * stat[1] * c0 + c1;
    } else if (cls) {
        out[(size_t)b * C + tid] = norm == SPARCH_RO_NORM_AFFINE ? bn_affine(wy, c0, c1) : wy;
    }
}

template <bool VEC>
void launch_ann(int mode, int RT, const AnnArgs& a, dim3 grid, hipStream_t st) {
    auto tiles = [&](auto m) {
        stream_row_tiles(RT, [&](auto rt) {
            hipLaunchKernelGGL((ann_stream_step_kernel<decltype(rt)::value, decltype(m)::value, VEC>), grid,
                               dim3(STREAM_NT), 0, st, a);
        });
    };
    switch (mode) {
        case SA_MLP: tiles(std::integral_constant<int, SA_MLP>{}); break;
        case SA_RNN: tiles(std::integral_constant<int, SA_RNN>{}); break;
        case SA_LIGRU: tiles(std::integral_constant<int, SA_LIGRU>{}); break;
        case SA_GRU1: tiles(std::integral_constant<int, SA_GRU1>{}); break;
        default: tiles(std::integral_constant<int, SA_GRU2>{}); break;
    }
}

}  // namespace

extern "C" int sparch_ann_stream_step(int cell, int phase, int act, int B, int K, int H, int ld, const float* x,
                                      int ldx, const float* const* W, const float* const* bias,
                                      const float* const* scale, const float* const* shift, const float* const* pre,
                                      const float* const* V, const float* y_in, float* y_out, float* z, float* ry,
                                      void* stream) {
    SPARCH_ENTER();
    int mode;
    switch (cell) {
        case SPARCH_CELL_MLP: mode = SA_MLP; break;
        case SPARCH_CELL_RNN: mode = SA_RNN; break;
        case SPARCH_CELL_LIGRU: mode = SA_LIGRU; break;
        case SPARCH_CELL_GRU: mode = phase == 1 ? SA_GRU1 : SA_GRU2; break;
        default: return SPARCH_EINVAL;
    }
    if (cell == SPARCH_CELL_GRU ? (phase != 1 && phase != 2) : phase != 0) return SPARCH_EINVAL;
    if ((mode == SA_MLP || mode == SA_RNN) && (act < SPARCH_ACT_SIGMOID || act > SPARCH_ACT_TANH)) return SPARCH_EINVAL;
    if (B <= 0 || K <= 0 || H <= 0 || ld < H || (x && ldx < K)) return SPARCH_EINVAL;
    // the gate slots (0 candidate, 1 update z, 2 reset r) this launch reads, in the kernel's order
    const int slot[2] = {mode == SA_GRU1 ? 1 : 0, mode == SA_GRU1 ? 2 : 1};
    const int G = sa_gates(mode);
    const bool rec = mode != SA_MLP;
    AnnArgs a{};
    a.B = B; a.K = K; a.H = H; a.ld = ld; a.ldx = ldx; a.act = act; a.x = x;
    for (int g = 0; g < G; ++g) {
        const int s = slot[g];
        a.W[g] = W ? W[s] : nullptr;
        a.bias[g] = bias ? bias[s] : nullptr;
        a.scale[g] = scale ? scale[s] : nullptr;
        a.shift[g] = shift ? shift[s] : nullptr;
        a.pre[g] = pre ? pre[s] : nullptr;
        a.V[g] = V ? V[s] : nullptr;
        if (x ? !a.W[g] : !a.pre[g]) return SPARCH_EINVAL;
        if ((a.scale[g] == nullptr) != (a.shift[g] == nullptr)) return SPARCH_EINVAL;
        if (rec && !a.V[g]) return SPARCH_EINVAL;
    }
    a.y_in = y_in; a.y_out = y_out; a.z = z; a.ry = ry;
    a.rec = mode == SA_GRU2 ? ry : y_in;
    if (rec && !y_in) return SPARCH_EINVAL;
    if (mode == SA_GRU1 ? (!z || !ry) : !y_out) return SPARCH_EINVAL;
    if (mode == SA_GRU2 && (!z || !ry)) return SPARCH_EINVAL;
    // every workgroup reads all of the operand of V: what the launch writes is another buffer
    if ((mode == SA_RNN || mode == SA_LIGRU) && y_out == y_in) return SPARCH_EINVAL;
    if (mode == SA_GRU1 && (z == y_in || ry == y_in || z == ry)) return SPARCH_EINVAL;
    if (mode == SA_GRU2 && (y_out == ry || y_out == z)) return SPARCH_EINVAL;
    const int RT = stream_row_tile(B);
    if (cdiv(B, RT) > 65535) return SPARCH_EINVAL;  // grid.y walks the row tiles
    const bool gru = cell == SPARCH_CELL_GRU;
    if (!all16({a.W[0], a.W[1], a.V[0], a.V[1], y_in, y_out, gru ? z : nullptr, gru ? ry : nullptr})) return SPARCH_EALIGN;
    const dim3 grid(cdiv(H, STREAM_COLS), cdiv(B, RT));
    // 16-byte weight loads where every row of every weight matrix read is aligned, scalar ones otherwise
    if ((!x || (K & 3) == 0) && (!rec || (H & 3) == 0)) launch_ann<true>(mode, RT, a, grid, (hipStream_t)stream);
    else launch_ann<false>(mode, RT, a, grid, (hipStream_t)stream);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_ann_stream_readout(int B, int K, int C, const float* y, int ldy, float* acc, const float* W,
                                         const float* bias, int norm, const float* p0, const float* p1, float eps,
                                         float* out, void* stream) {
    SPARCH_ENTER();
    if (B <= 0 || K <= 0 || C <= 0 || K > AR_KMAX || C > AR_CMAX || ldy < K) return SPARCH_EINVAL;
    if (!y || !acc || !W || !out) return SPARCH_EINVAL;
    if (norm != SPARCH_RO_NORM_NONE && norm != SPARCH_RO_NORM_AFFINE && norm != SPARCH_RO_NORM_LAYERNORM)
        return SPARCH_EINVAL;
    if (norm != SPARCH_RO_NORM_NONE && (!p0 || !p1)) return SPARCH_EINVAL;
    if (!aligned16(W) || !aligned16(acc)) return SPARCH_EALIGN;
    if ((K & 3) == 0)
        hipLaunchKernelGGL(ann_stream_readout_kernel<true>, dim3(B), dim3(AR_NT), 0, (hipStream_t)stream, K, C, y, ldy,
                           acc, W, bias, norm, p0, p1, eps, out);
    else
        hipLaunchKernelGGL(ann_stream_readout_kernel<false>, dim3(B), dim3(AR_NT), 0, (hipStream_t)stream, K, C, y, ldy,
                           acc, W, bias, norm, p0, p1, eps, out);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// Streaming inference, chunks of ONE time step: projection + cell in one launch per layer.
//
// sparch_stream_step_fwd   one hidden layer, one step, all rows:  Wx = x_t W^T (+ bias), the eval BatchNorm affine,
//                          rec = s_in Vmasked for the recurrent kinds, the membrane update, the new state.
// sparch_stream_step_readout  the readout layer's step: Wx, affine, u = alpha u + (1 - alpha) Wx, out += softmax(u).
//
// A chunk of one step is 1 .. a few hundred rows: the MFMA projection kernels (built for 64 000 rows) and the
// boundary product run a dozen dependent launches on it, and the step costs the length of that chain.  Here a step
// costs one kernel boundary per layer.  Nothing waits inside a launch: every workgroup reads the WHOLE previous spike
// state s_in and writes its own columns of s_out, a different buffer, so the only ordering is the kernel boundary.
//
// Shape (hidden layer): a workgroup is 4 waves and owns 4 adjacent columns of the layer (one per wave) for one tile
// of RT <= 16 batch rows (grid.y walks the row tiles: no batch cap).  A wave's column is one row of W (H,K) and one
// row of vmask_t: both are streamed ONCE per row tile, straight into registers (16-byte loads issued before the tile
// of x_t is staged, so their latency overlaps the staging), lanes striding over K; the row tile of x_t / s_in sits
// in LDS in K-pieces and is read by all four waves.  The weights of a layer (<= 8 MB) are read again every step and a
// column always lands on the same workgroup index, so they are loaded with the default cache policy and stay in L2.
// The dot products are fp32 FMA chains, 64 lane partials per (row, column) added by a butterfly: exact wherever the
// sums are exact in any order (dyadic weights on 0/1 spikes), otherwise within a few ulp of any other fp32 order.
// The pointwise update is the one of rec_fwd_kernel (reccell.hip) and cell_fwd_pipe_kernel (cell.hip): neuron.h, through
// the tails of stream_common.h.  The dot product is stream_dot of stream_common.h (one gate, the column tail on), which
// the baselines' step shares.  What is here: the two kernels and the readout's geometry, the entry points.
#include "stream_common.h"

namespace {

template <int RT, bool ADAPT, bool REC, bool VEC>
__global__ __launch_bounds__(STREAM_NT) void stream_step_kernel(StreamArgs a) {
    constexpr int KP = stream_piece(RT);
    __shared__ __attribute__((aligned(16))) float xs[RT * KP];
    __shared__ float red[2][RT][STREAM_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h0 = blockIdx.x * STREAM_COLS, r0 = blockIdx.y * RT;
    const int hw = min(h0 + wave, a.H - 1);  // this wave's column (a wave past H: any valid one, never read)
    // ---- the pointwise phase's operands, asked for now (thread = (row, column), the tile's 4 columns of a row
    //      adjacent in memory): they arrive while the dot products run
    const int r = tid >> 2, c = tid & 3;
    const int row = r0 + r, h = h0 + c;
    const bool valid = r < RT && row < a.B && h < a.H;
    const int hc = min(h, a.H - 1);
    const size_t o = (size_t)min(row, a.B - 1) * a.ld + hc;
    const StreamColumn<ADAPT> pc = stream_column<ADAPT>(a.alpha, a.beta, a.a, a.b, a.bias, a.scale, a.shift, hc);
    const float u = a.u[o], w = ADAPT ? a.w[o] : 0.f, s = a.s_in[o];

    float accx[1][RT], accr[1][RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) accx[0][i] = accr[0][i] = 0.f;
    // (one gate; the tail switch on: V has H columns in rows of ld floats)
    if (a.in_u8)
        stream_dot<RT, 1, true, VEC, true>(xs, a.x, a.ldx, {a.W + (size_t)hw * a.K}, a.K, r0, a.B, accx);
    else
        stream_dot<RT, 1, false, VEC, true>(xs, a.x, a.ldx, {a.W + (size_t)hw * a.K}, a.K, r0, a.B, accx);
    if (REC) stream_dot<RT, 1, false, VEC, true>(xs, a.s_in, a.ld, {a.V + (size_t)hw * a.ld}, a.H, r0, a.B, accr);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const float sx = stream_wave_sum(accx[0][i]);
        const float sr = REC ? stream_wave_sum(accr[0][i]) : 0.f;
        if (lane == 0) {
            red[0][i][wave] = sx;
            red[1][i][wave] = sr;
        }
    }
    __syncthreads();
    if (valid) stream_pointwise<ADAPT, REC>(a, pc, red[0][r][c], red[1][r][c], u, w, s, o, h);
}

// ---- readout: one workgroup per batch row, 16 waves; a wave takes groups of RO_CG classes, lanes stride over K
constexpr int RO_NT = 1024;
constexpr int RO_KP = 1024;  // floats of x_t staged per piece: 16 weight floats per lane, class and piece
// classes whose weight loads are in flight together: 3 with 16-byte loads (35 classes: one group per wave), 1 with
// scalar ones (16 loads and their addresses per class: more would spill)
__host__ __device__ constexpr int ro_group(bool VEC) { return VEC ? 3 : 1; }

template <bool VEC>
struct RoWeights {
    f32x4 v[ro_group(VEC)][VEC ? RO_KP / 256 : 1];
    float s[ro_group(VEC)][VEC ? 1 : RO_KP / 64];
};
// the weights of classes c0 .. c0 + ro_group(VEC) - 1 for the piece at k0: loads on clamped addresses, masked at their use
// (see stream_dot, stream_common.h)
template <bool VEC>
__device__ __forceinline__ void ro_load_group(RoWeights<VEC>& w, const float* __restrict__ W, int K, int C, int c0,
                                              int k0, int lane) {
#pragma unroll
    for (int j = 0; j < ro_group(VEC); ++j) {
        const float* wr = W + (size_t)min(c0 + j, C - 1) * K;
        if (VEC) {
#pragma unroll
            for (int i = 0; i < RO_KP / 256; ++i)
                w.v[j][i] = *reinterpret_cast<const f32x4*>(wr + min(k0 + (i * 64 + lane) * 4, K - 4));
        } else {
#pragma unroll
            for (int i = 0; i < RO_KP / 64; ++i) w.s[j][i] = wr[min(k0 + i * 64 + lane, K - 1)];
        }
    }
}

template <bool VEC>  // 16-byte weight loads (K a multiple of 4) or scalar ones
__global__ __launch_bounds__(RO_NT) void stream_step_readout_kernel(int K, int C, const float* __restrict__ x, int ldx,
                                                                    const float* __restrict__ W,
                                                                    const float* __restrict__ bias,
                                                                    const float* __restrict__ scale,
                                                                    const float* __restrict__ shift,
                                                                    const float* __restrict__ alpha, float* u_io,
                                                                    float* out) {
    __shared__ __attribute__((aligned(16))) float xs[RO_KP];
    __shared__ float row[256];  // Wx, then u, then softmax(u) of the classes
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const float* xr = x + (size_t)b * ldx;
    // thread = class operands, asked for now
    const bool act = tid < C;
    const int cc = act ? tid : 0;
    const StreamColumn<false> pc = stream_column<false>(alpha, nullptr, nullptr, nullptr, bias, scale, shift, cc);
    const float u_prev = u_io[(size_t)b * C + cc], out_prev = out[(size_t)b * C + cc];
    if (act) row[tid] = 0.f;
    constexpr int RO_CG = ro_group(VEC), C_STEP = (RO_NT / 64) * RO_CG;
    for (int k0 = 0; k0 < K; k0 += RO_KP) {
        const int klen = min(RO_KP, K - k0);
        const float xv = xr[min(k0 + tid, K - 1)];
        RoWeights<VEC> w;
        ro_load_group<VEC>(w, W, K, C, wave * RO_CG, k0, lane);  // the first group, in flight while x_t is staged
        if (tid < klen) xs[tid] = xv;
        __syncthreads();
        for (int c0 = wave * RO_CG; c0 < C; c0 += C_STEP) {  // (a class belongs to one wave: no race on row[c])
            if (c0 != wave * RO_CG) ro_load_group<VEC>(w, W, K, C, c0, k0, lane);
#pragma unroll
            for (int j = 0; j < RO_CG; ++j) {
                float acc = 0.f;
                if (VEC) {
#pragma unroll
                    for (int i = 0; i < RO_KP / 256; ++i) {
                        const int kk = (i * 64 + lane) * 4;
                        if (kk < klen) {
                            const f32x4 x4 = *reinterpret_cast<const f32x4*>(&xs[kk]);
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(w.v[j][i][e], x4[e], acc);
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < RO_KP / 64; ++i)
                        if (i * 64 + lane < klen) acc = __builtin_fmaf(w.s[j][i], xs[i * 64 + lane], acc);
                }
                acc = stream_wave_sum(acc);
                if (lane == 0 && c0 + j < C) row[c0 + j] = row[c0 + j] + acc;
            }
        }
        __syncthreads();
    }
    stream_readout_tail(row, act, b, C, row[cc], pc, bias != nullptr, scale != nullptr, u_prev, out_prev,
                        u_io, out);
}

template <bool VEC>
void launch_step(int RT, int kind, const StreamArgs& a, dim3 grid, hipStream_t st) {
    stream_dispatch(RT, kind, [&](auto rt, auto adapt, auto rec) {
        hipLaunchKernelGGL((stream_step_kernel<decltype(rt)::value, decltype(adapt)::value, decltype(rec)::value, VEC>), grid,
                           dim3(STREAM_NT), 0, st, a);
    });
}

}  // namespace

extern "C" int sparch_stream_step_fwd(int kind, int B, int K, int H, int ld, int in_dtype, const void* x, int ldx,
                                      const float* W, const float* bias, const float* scale, const float* shift,
                                      const float* alpha, const float* beta, const float* a, const float* b,
                                      const float* vmask_t, float* u, float* w, const float* s_in, float* s_out,
                                      uint16_t* s16_out, float theta, uint32_t* spike_count, void* stream) {
    SPARCH_ENTER();
    StreamArgs g{};
    g.B = B; g.K = K; g.H = H; g.ld = ld; g.ldx = ldx; g.in_u8 = in_dtype;
    g.x = x; g.W = W; g.bias = bias; g.scale = scale; g.shift = shift;
    g.alpha = alpha; g.beta = beta; g.a = a; g.b = b; g.V = vmask_t;
    g.u = u; g.w = w; g.s_in = s_in; g.s_out = s_out; g.s16_out = s16_out; g.theta = theta; g.spike_count = spike_count;
    if (const int rc = stream_step_check(kind, in_dtype, g, false)) return rc;
    const int RT = stream_row_tile(B);
    const dim3 grid(cdiv(H, STREAM_COLS), cdiv(B, RT));
    // 16-byte weight loads where every row of W and of vmask_t is aligned, scalar ones otherwise
    const bool rec = kind == SPARCH_KIND_RLIF || kind == SPARCH_KIND_RADLIF;
    if ((K & 3) == 0 && (!rec || (ld & 3) == 0)) launch_step<true>(RT, kind, g, grid, (hipStream_t)stream);
    else launch_step<false>(RT, kind, g, grid, (hipStream_t)stream);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_stream_step_readout(int B, int K, int C, const float* x, int ldx, const float* W,
                                          const float* bias, const float* scale, const float* shift,
                                          const float* alpha, float* u, float* out, void* stream) {
    SPARCH_ENTER();
    if (const int rc = stream_readout_check(B, K, C, x, ldx, W, false, 0, scale, shift, alpha, u, out)) return rc;
    if ((K & 3) == 0)
        hipLaunchKernelGGL(stream_step_readout_kernel<true>, dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, K, C, x, ldx,
                           W, bias, scale, shift, alpha, u, out);
    else
        hipLaunchKernelGGL(stream_step_readout_kernel<false>, dim3(B), dim3(RO_NT), 0, (hipStream_t)stream, K, C, x,
                           ldx, W, bias, scale, shift, alpha, u, out);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// Streaming inference, chunks of ONE time step, EVENT-DRIVEN: only the weights of active inputs are read.
//
// sparch_stream_step_sparse_fwd      one hidden layer, one step, all rows: the contract of sparch_stream_step_fwd
//                                    (streamstep.hip) on transposed weight operands.
// sparch_stream_step_sparse_readout  the readout layer's step: the contract of sparch_stream_step_readout.
//
// The dense fused step streams all of W (H,K) and vmask_t (H,H) through the CUs each step, and multiplies more than
// nine tenths of them by zero: the operands are spikes (5 - 9 % active).  Here the weights are stored so that everything
// one active input k contributes is ONE contiguous row — Wt (K, ldw) = W transposed, vmask (H_in, ld) = the masked V as
// it is — and a step reads nnz rows of them instead of all.
//
// Shape (hidden layer): a workgroup is 4 waves and owns SP_COLS = 64 adjacent columns (lane = column) for one tile of
// RT <= 16 batch rows (grid.y walks the row tiles: no batch cap).  Per operand (x_t, then s_in), in pieces of
// sp_piece(RT) input positions:
//   1. compaction   the 256 threads load the row tile's piece (uint8 converted on the way, rows past B and positions
//                   past K as zeros) into registers; per row the (k, value) pairs with value != 0 go to a list in LDS in
//                   ascending k: a wave ballot and the count of set lower lanes give the place inside the wave's 64
//                   positions, the waves' counts meet in LDS and one thread per row scans them.  No atomics.  Values are
//                   kept (counts above 1, mel features, a drawn real-valued s0: one code path).
//   2. accumulation entry p of a row's list (p counted from the start of the ROW, across pieces) belongs to wave p & 3;
//                   a wave load is 64 adjacent floats of weight row k (two 128-byte lines), SP_U of them in flight (the
//                   addresses come from LDS and are known ahead), acc = fma(value, wt, acc) in ascending p.
// then the four waves' partial sums of a (row, column) meet in LDS and are added as (p0 + p1) + (p2 + p3), Wx and s V
// apart, and the pointwise update — stream_pointwise (stream_common.h), the dense step's own — writes the new state.
// The readout is one workgroup per batch row: the same compaction, thread = class runs over the whole list in
// ascending k (one chain), then stream_readout_tail, the dense readout step's own.  What is here: sp_compact, sp_dot,
// the geometry of the two kernels, the entry points.
//
// Why it is exact: leaving out a term whose input is 0 removes an exact +-0 from an fp32 sum that starts at +0; for
// finite weights no partial sum changes.  What differs from the dense fused kernel is only the ORDER and grouping of the
// non-zero terms, which depends on nothing but the row's own list (not on B, the tile or the piece): bit-equal wherever
// the sums are exact in any order (dyadic weights on 0/1 spikes, counts or dyadic states), within the last bits of
// any other fp32 order on real-valued weights.  No float atomics, no list split across workgroups: a pure function of
// the inputs.  Built with -ffp-contract=off like streamstep.hip, so the same pointwise expressions give the same bits.
//
// Weight loads keep the default cache policy: a column tile always lands on the same workgroup index, hence on the same
// XCD's L2, and the weights are read again every step.
#include "stream_common.h"

namespace {

constexpr int SP_NT = 256;   // 4 waves
constexpr int SP_WAVES = 4;  // ways a row's list is dealt
constexpr int SP_COLS = 64;  // columns per workgroup: one per lane
constexpr int SP_U = 8;      // weight rows in flight per wave
// input positions compacted per piece: the lists are RT x piece (position, value) pairs of LDS, 6 bytes each (<= 24 KB)
__host__ __device__ constexpr int sp_piece(int RT) { return RT <= 2 ? 1024 : RT <= 8 ? 512 : 256; }

// One piece [k0, k0 + KP) of the row tile of src -> per row the ascending list of its non-zero (k - k0, value) pairs:
// lk / lv [r * KP + j], j < pcnt[r]; pbase[r] = the number of entries the row's earlier pieces held.  `tot` is the
// running length of row tid's list (threads tid < RT; carried by the caller from piece to piece).  All SP_NT threads
// call; the lists may be read behind the call (it ends in a barrier) and must be consumed before the next one.
// Every global load is UNCONDITIONAL on a clamped address and masked where it is used (see stream_dot, stream_common.h).
template <int RT, bool U8>
__device__ __forceinline__ void sp_compact(float* lv, uint16_t* lk, int* wcnt, int* pcnt, int* pbase, int& tot,
                                           const void* src, int ld_src, int K, int k0, int r0, int B) {
    constexpr int KP = sp_piece(RT), NI = KP / SP_NT, NW = NI * SP_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (r0 made opaque: hoisted out of the callers' piece loops, the rows' offsets and in-batch masks are 4 SGPRs per
    // row for the whole kernel)
    asm volatile("" : "+s"(r0));
    float xv[RT][NI];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const size_t o = (size_t)min(r0 + r, B - 1) * ld_src;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const size_t oo = o + min(k0 + i * SP_NT + tid, K - 1);
            xv[r][i] = U8 ? (float)static_cast<const uint8_t*>(src)[oo] : static_cast<const float*>(src)[oo];
        }
    }
    int below[RT][NI];  // active lanes below this one in its wave, -1: this one is not active
#pragma unroll
    for (int r = 0; r < RT; ++r) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const bool on = (r0 + r < B) && (k0 + i * SP_NT + tid < K) && (xv[r][i] != 0.0f);
            const unsigned long long m = __ballot(on);
            below[r][i] = on ? __popcll(m & ((1ull << lane) - 1ull)) : -1;
            // (made a VGPR value HERE: left alone, hipcc keeps the two 64-bit masks of every (r, i) in SGPRs across
            // the barriers and forms this behind them — 4 SGPRs each, which spill at RT >= 8)
            asm volatile("" : "+v"(below[r][i]));
            if (lane == 0) wcnt[(r * NI + i) * SP_WAVES + wave] = __popcll(m);
        }
    }
    __syncthreads();
    if (tid < RT) {  // thread = row: the waves' counts -> their offsets (k ascends with i, then wave, then lane)
        int off = 0;
        for (int j = 0; j < NW; ++j) {
            const int c = wcnt[tid * NW + j];
            wcnt[tid * NW + j] = off;
            off += c;
        }
        pcnt[tid] = off;
        pbase[tid] = tot;
        tot += off;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (below[r][i] >= 0) {
                const int pos = wcnt[(r * NI + i) * SP_WAVES + wave] + below[r][i];  // < KP: a piece has KP positions
                lv[r * KP + pos] = xv[r][i];
                lk[r * KP + pos] = (uint16_t)(i * SP_NT + tid);  // the position inside the piece
            }
        }
    }
    __syncthreads();
}

// part[r][lane] = fma(value, wt[k][col], part[r][lane]) over the entries p = wave, wave + 4, ... of row r's list, p
// counted from the start of the row's list; wrow (K, ldw) holds one contiguous row per input position.  `part` is the
// calling wave's own plane of partial sums in LDS (a thread reads and writes its own slots only; they start at 0): a
// row's sum lives in a register while its entries of one piece are added and waits there for the next piece, so the
// loop over the rows stays rolled (unrolled over 16 rows, its loop bounds and addresses overflow the scalar registers).
template <int RT, bool U8>
__device__ __forceinline__ void sp_dot(float* lv, uint16_t* lk, int* wcnt, int* pcnt, int* pbase, const void* src,
                                       int ld_src, const float* wrow, int ldw, int K, int r0, int B, int col,
                                       float (*part)[SP_COLS]) {
    constexpr int KP = sp_piece(RT);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int tot = 0;
    for (int k0 = 0; k0 < K; k0 += KP) {
        sp_compact<RT, U8>(lv, lk, wcnt, pcnt, pbase, tot, src, ld_src, K, k0, r0, B);
#pragma unroll 1
        for (int r = 0; r < RT; ++r) {
            const int n = pcnt[r];
            int j = (wave - pbase[r]) & (SP_WAVES - 1);
            if (j >= n) continue;
            float acc = part[r][lane];
            for (; j < n; j += SP_WAVES * SP_U) {
                float v[SP_U], wt[SP_U];
                int k[SP_U];
#pragma unroll
                for (int e = 0; e < SP_U; ++e) {  // (behind the list's end: its last entry again, not used)
                    const int jj = min(j + e * SP_WAVES, n - 1);
                    k[e] = k0 + lk[r * KP + jj];
                    v[e] = lv[r * KP + jj];
                }
#pragma unroll
                for (int e = 0; e < SP_U; ++e) wt[e] = wrow[(size_t)k[e] * ldw + col];
#pragma unroll
                for (int e = 0; e < SP_U; ++e)
                    if (j + e * SP_WAVES < n) acc = __builtin_fmaf(v[e], wt[e], acc);
            }
            part[r][lane] = acc;
        }
        __syncthreads();  // the piece is consumed: the next one (or the next operand) may be compacted
    }
}

template <int RT, bool ADAPT, bool REC>
__global__ __launch_bounds__(SP_NT) void stream_step_sparse_kernel(StreamArgs a) {
    constexpr int RPT = (RT + SP_WAVES - 1) / SP_WAVES;  // rows of the pointwise phase per thread
    __shared__ float lv[RT * sp_piece(RT)];
    __shared__ uint16_t lk[RT * sp_piece(RT)];
    __shared__ float red[2][SP_WAVES][RT][SP_COLS];  // partial sums [operand][wave][row][column] (<= 32 KB)
    __shared__ int wcnt[RT * sp_piece(RT) / 64];
    __shared__ int pcnt[RT], pbase[RT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h0 = blockIdx.x * SP_COLS, r0 = blockIdx.y * RT;
    const int h = h0 + lane, hc = min(h, a.H - 1);  // (a lane past H: any valid column, never written)
    // ---- the pointwise phase's operands, asked for now (thread = column, rows wave, wave + 4, ...): they arrive
    //      while the lists are made
    const StreamColumn<ADAPT> pc = stream_column<ADAPT>(a.alpha, a.beta, a.a, a.b, a.bias, a.scale, a.shift, hc);
    float u_prev[RPT], w_prev[RPT], s_prev[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const size_t o = (size_t)min(r0 + wave + i * SP_WAVES, a.B - 1) * a.ld + hc;
        u_prev[i] = a.u[o];
        w_prev[i] = ADAPT ? a.w[o] : 0.f;
        s_prev[i] = a.s_in[o];
    }

#pragma unroll
    for (int r = 0; r < RT; ++r) red[0][wave][r][lane] = red[1][wave][r][lane] = 0.f;  // (this thread's own slots)
    if (a.in_u8)
        sp_dot<RT, true>(lv, lk, wcnt, pcnt, pbase, a.x, a.ldx, a.W, a.ldw, a.K, r0, a.B, hc, red[0][wave]);
    else
        sp_dot<RT, false>(lv, lk, wcnt, pcnt, pbase, a.x, a.ldx, a.W, a.ldw, a.K, r0, a.B, hc, red[0][wave]);
    if (REC) sp_dot<RT, false>(lv, lk, wcnt, pcnt, pbase, a.s_in, a.ld, a.V, a.ld, a.H, r0, a.B, hc, red[1][wave]);
    // ---- the four waves' partial sums of a (row, column) in one fixed tree (sp_dot ends in a barrier)
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = wave + i * SP_WAVES, row = r0 + r;
        if (r >= RT || row >= a.B || h >= a.H) continue;
        const size_t o = (size_t)row * a.ld + h;
        const float sx = (red[0][0][r][lane] + red[0][1][r][lane]) + (red[0][2][r][lane] + red[0][3][r][lane]);
        const float sr = REC ? (red[1][0][r][lane] + red[1][1][r][lane]) + (red[1][2][r][lane] + red[1][3][r][lane]) : 0.f;
        stream_pointwise<ADAPT, REC>(a, pc, sx, sr, u_prev[i], w_prev[i], s_prev[i], o, h);
    }
}

// ---- readout: one workgroup per batch row, thread = class over the row's whole list
constexpr int SR_RT = 1;

__global__ __launch_bounds__(SP_NT) void stream_step_sparse_readout_kernel(int K, int C, const float* __restrict__ x,
                                                                           int ldx, const float* __restrict__ Wt, int ldc,
                                                                           const float* __restrict__ bias,
                                                                           const float* __restrict__ scale,
                                                                           const float* __restrict__ shift,
                                                                           const float* __restrict__ alpha, float* u_io,
                                                                           float* out) {
    constexpr int KP = sp_piece(SR_RT);
    __shared__ float lv[KP];
    __shared__ uint16_t lk[KP];
    __shared__ int wcnt[KP / 64];
    __shared__ int pcnt[SR_RT], pbase[SR_RT];
    __shared__ float row[256];  // u, then softmax(u) of the classes
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    // thread = class operands, asked for now
    const bool act = tid < C;
    const int cc = act ? tid : C - 1;
    const StreamColumn<false> pc = stream_column<false>(alpha, nullptr, nullptr, nullptr, bias, scale, shift, cc);
    const float u_prev = u_io[(size_t)b * C + cc], out_prev = out[(size_t)b * C + cc];
    float acc = 0.f;
    int tot = 0;
    for (int k0 = 0; k0 < K; k0 += KP) {
        sp_compact<SR_RT, false>(lv, lk, wcnt, pcnt, pbase, tot, x + (size_t)b * ldx, ldx, K, k0, 0, 1);
        const int n = pcnt[0];
        for (int j = 0; j < n; j += SP_U) {
            float v[SP_U], wt[SP_U];
            int k[SP_U];
#pragma unroll
            for (int e = 0; e < SP_U; ++e) {
                const int jj = min(j + e, n - 1);
                k[e] = k0 + lk[jj];
                v[e] = lv[jj];
            }
#pragma unroll
            for (int e = 0; e < SP_U; ++e) wt[e] = Wt[(size_t)k[e] * ldc + cc];
#pragma unroll
            for (int e = 0; e < SP_U; ++e)
                if (j + e < n) acc = __builtin_fmaf(v[e], wt[e], acc);
        }
        __syncthreads();
    }
    stream_readout_tail(row, act, b, C, acc, pc, bias != nullptr, scale != nullptr, u_prev, out_prev, u_io,
                        out);
}

}  // namespace

extern "C" int sparch_stream_step_sparse_fwd(int kind, int B, int K, int H, int ld, int in_dtype, const void* x, int ldx,
                                             const float* Wt, int ldw, const float* bias, const float* scale,
                                             const float* shift, const float* alpha, const float* beta, const float* a,
                                             const float* b, const float* vmask, float* u, float* w, const float* s_in,
                                             float* s_out, uint16_t* s16_out, float theta, uint32_t* spike_count,
                                             void* stream) {
    SPARCH_ENTER();
    StreamArgs g{};
    g.B = B; g.K = K; g.H = H; g.ld = ld; g.ldx = ldx; g.ldw = ldw; g.in_u8 = in_dtype;
    g.x = x; g.W = Wt; g.bias = bias; g.scale = scale; g.shift = shift;
    g.alpha = alpha; g.beta = beta; g.a = a; g.b = b; g.V = vmask;
    g.u = u; g.w = w; g.s_in = s_in; g.s_out = s_out; g.s16_out = s16_out; g.theta = theta; g.spike_count = spike_count;
    if (const int rc = stream_step_check(kind, in_dtype, g, true)) return rc;
    const int RT = stream_row_tile(B);  // the smallest row tile that holds the batch, as the dense step chooses it
    const dim3 grid(cdiv(H, SP_COLS), cdiv(B, RT));
    stream_dispatch(RT, kind, [&](auto rt, auto adapt, auto rec) {
        hipLaunchKernelGGL((stream_step_sparse_kernel<decltype(rt)::value, decltype(adapt)::value, decltype(rec)::value>), grid,
                           dim3(SP_NT), 0, (hipStream_t)stream, g);
    });
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_stream_step_sparse_readout(int B, int K, int C, const float* x, int ldx, const float* Wt, int ldc,
                                                 const float* bias, const float* scale, const float* shift,
                                                 const float* alpha, float* u, float* out, void* stream) {
    SPARCH_ENTER();
    if (const int rc = stream_readout_check(B, K, C, x, ldx, Wt, true, ldc, scale, shift, alpha, u, out)) return rc;
    hipLaunchKernelGGL(stream_step_sparse_readout_kernel, dim3(B), dim3(SP_NT), 0, (hipStream_t)stream, K, C, x, ldx, Wt,
                       ldc, bias, scale, shift, alpha, u, out);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// Axonal delays: a learnable time shift per input feature of a layer ("Axonal delays").
//
// delay (K,) fp32 is the parameter theta; every kernel derives the integer shift d_i = rint(clamp(theta_i, 0, D)) on
// the device (round half to even: 2.5 -> 2, 3.5 -> 4; a NaN gives 0), so the host never reads theta.  With len_b the
// row's own length (T without lengths):
//     y[b,t,i]   = x[b, t - d_i, i]    if d_i <= t < len_b, else 0                       (sparch_delay_fwd)
//     g_x[b,t,i] = g_y[b, t + d_i, i]  if t + d_i < len_b,  else 0                       (sparch_delay_bwd)
//     g_theta[i] = gate_i * sum_b sum_{t = d_i}^{len_b - 1} g_y[b,t,i] * (x[b,t-d_i-1,i] - x[b,t-d_i,i]),  x[b,-1,i] = 0
//     gate_i     = 1 if 0 <= theta_i <= D else 0  (torch.clamp's backward)
// Both directions are one gather over rows of the same sequence, so the elements move as raw 2- or 4-byte patterns
// (the bf16 spike plane, fp32 tensors) and the results are copies.  Where the row size and every base address allow
// 16-byte pieces, a workgroup stages the source rows of its tile in LDS with whole 16-byte loads and every thread picks
// the 16 bytes it stores out of LDS (delay_gather_tile_kernel: 1.1 - 1.35 x the time of a plain row copy of the same
// bytes, against 3.2 - 3.7 x for per-element loads out of L2; profiles/delay_bench.jsonl); other shapes move one element
// per thread (delay_gather_kernel).
// g_theta: every workgroup sums a slice of rows for 64 columns into a workspace slab, a second launch adds the slabs in
// their fixed order — no atomics, the same bits on every run.
// Layouts: dense (B,T,K) with a row stride; lengths (B,) as the `_len` kernels take them; offsets non-NULL: the packed
// layout of a PackPlan — sequence j owns rows [offsets[j], offsets[j] + lengths[j]) and the shift stays inside them (T
// is then the longest length; rows t >= lengths[j] do not exist and are not written).
// sparch_delay_stream: the same shift on a chunk (B,Tc,K) of a stream, with the last D input steps carried in `hist`
// (B,D,K) (row D - 1 is the newest) and advanced in place; a thread owns its columns of one batch row through the
// whole call, so the gather and the advance of the history need no ordering between threads.
#include "common.h"

namespace {

typedef unsigned dl_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int delay_steps(float theta, int D) {
    return (int)rintf(fminf(fmaxf(theta, 0.0f), (float)D));
}

// N elements of type E as one value that is stored at once
template <class E, int N> struct DlVec { E v[N]; };
template <> struct alignas(16) DlVec<uint16_t, 8> { uint16_t v[8]; };
template <> struct alignas(16) DlVec<uint32_t, 4> { uint32_t v[4]; };

struct DelayArgs {
    int B, T, K, D;
    unsigned groups;  // pieces per row: of 16 bytes in the tile kernel, single elements otherwise
    const float* delay;
    const void* src; void* dst;
    long long lds, ldd;  // row strides, in elements
    const int* lengths; const int* offsets;
};

// One thread per element of the index space (sequence j, step t, column), for rows that do not move in 16-byte pieces.
// BWD: the source row is t + d (g_x from g_y), else t - d (y from x).  The load is issued from an address inside the
// sequence and selected afterwards.
template <class E, bool BWD>
__global__ __launch_bounds__(256) void delay_gather_kernel(DelayArgs a) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long row = idx / a.groups;
    const int col = (int)(idx - row * a.groups);
    if (row >= (unsigned long long)a.B * a.T) return;
    const int j = (int)(row / a.T), t = (int)(row - (unsigned long long)j * a.T);
    const int len = a.lengths ? min(max(a.lengths[j], 0), a.T) : a.T;
    if (a.offsets && t >= len) return;  // packed: the row does not exist
    const long long base = a.offsets ? (long long)a.offsets[j] : (long long)j * a.T;
    const int d = delay_steps(a.delay[col], a.D);
    const int ts = BWD ? t + d : t - d;
    const bool ok = t < len && (BWD ? ts < len : ts >= 0);
    const E v = static_cast<const E*>(a.src)[(base + (ok ? ts : t)) * a.lds + col];
    static_cast<E*>(a.dst)[(base + t) * a.ldd + col] = ok ? v : (E)0;
}

// The same gather for rows that move in 16-byte pieces, through LDS: a workgroup owns TILE_ROWS steps x TILE_PIECES
// pieces (128 bytes of every row) of one sequence, stages the TILE_ROWS + D source rows it can reach with whole 16-byte
// loads (rows outside the sequence as zeros), and every thread then picks its 16 output bytes element by element out of
// LDS.  A form with per-element global loads (2 or 4 bytes per lane and instruction) and one 16-byte store per thread
// ran at 1.6 - 1.8 TB/s at the cfg3 / cfg2 shapes (profiles/delay_bench_l2_gather.jsonl); the staged form reads
// (TILE_ROWS + D) / TILE_ROWS of the bytes at the width of a copy (profiles/delay_bench.jsonl).  LDS rows are padded
// by one piece against bank conflicts between the rows of a wave.
constexpr int TILE_ROWS = 64, TILE_PIECES = 8, TILE_LD = (TILE_PIECES + 1) * 16;  // bytes per LDS row

template <class E, bool BWD>
__global__ __launch_bounds__(256) void delay_gather_tile_kernel(DelayArgs a, unsigned tiles_t, unsigned tiles_c) {
    constexpr int N = 16 / (int)sizeof(E);
    extern __shared__ __attribute__((aligned(16))) unsigned char tile[];
    const unsigned tc = blockIdx.x % tiles_c;
    const unsigned tt = (blockIdx.x / tiles_c) % tiles_t;
    const int j = (int)(blockIdx.x / tiles_c / tiles_t);
    const int len = a.lengths ? min(max(a.lengths[j], 0), a.T) : a.T;
    const int t0 = (int)tt * TILE_ROWS;
    if (a.offsets && t0 >= len) return;  // packed: none of the tile's rows exists (the whole workgroup leaves)
    const long long base = a.offsets ? (long long)a.offsets[j] : (long long)j * a.T;
    const int first = BWD ? t0 : t0 - a.D;  // the step staged in LDS row 0
    const int staged = TILE_ROWS + a.D;
    const int piece0 = (int)tc * TILE_PIECES;
    const int pieces = min(TILE_PIECES, (int)a.groups - piece0);  // (>= 1: the grid has no empty column tile)
    const E* src = static_cast<const E*>(a.src);
    for (int p = threadIdx.x; p < staged * TILE_PIECES; p += 256) {
        const int r = p / TILE_PIECES, c = p % TILE_PIECES;
        const int ts = first + r;
        dl_u32x4 v = {0u, 0u, 0u, 0u};
        if (c < pieces && ts >= 0 && ts < len)
            v = *reinterpret_cast<const dl_u32x4*>(src + (base + ts) * a.lds + (long long)(piece0 + c) * N);
        *reinterpret_cast<dl_u32x4*>(tile + r * TILE_LD + c * 16) = v;
    }
    __syncthreads();
    const int c = threadIdx.x % TILE_PIECES;
    if (c >= pieces) return;
    const int col = (piece0 + c) * N;
    int d[N];
#pragma unroll
    for (int e = 0; e < N; ++e) d[e] = delay_steps(a.delay[col + e], a.D);
    for (int r = threadIdx.x / TILE_PIECES; r < TILE_ROWS; r += 256 / TILE_PIECES) {
        const int t = t0 + r;
        if (t >= a.T || (a.offsets && t >= len)) break;
        DlVec<E, N> out;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int ts = BWD ? t + d[e] : t - d[e];
            const bool ok = t < len && (BWD ? ts < len : ts >= 0);
            const int rs = ok ? ts - first : 0;  // 0 <= rs < TILE_ROWS + D
            const E v = *reinterpret_cast<const E*>(tile + rs * TILE_LD + c * 16 + e * (int)sizeof(E));
            out.v[e] = ok ? v : (E)0;
        }
        *reinterpret_cast<DlVec<E, N>*>(static_cast<E*>(a.dst) + (base + t) * a.ldd + col) = out;
    }
}

template <class E> __device__ __forceinline__ float dl_value(E v);
template <> __device__ __forceinline__ float dl_value<uint16_t>(uint16_t v) { return bf16_to_f32(v); }
template <> __device__ __forceinline__ float dl_value<uint32_t>(uint32_t v) { return __uint_as_float(v); }

struct DelayGradArgs {
    int B, T, K, D;
    long long chunk_rows;  // rows of the (B,T) index space per workgroup, a multiple of 4
    const float* delay;
    const float* gy; long long ldg;
    const void* x; long long ldx;
    float scale;
    float* ws;  // (chunks, K)
    const int* lengths; const int* offsets;
};

// grid (column tiles of 64, chunks): thread (c, r) of 64 x 4 sums rows r, r + 4, ... of its chunk for column c, the
// four partial sums are added in the order r = 0..3 and written to slab `chunk` of the workspace.
template <class E>
__global__ __launch_bounds__(256) void delay_grad_partial_kernel(DelayGradArgs a) {
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + c;
    const long long rows = (long long)a.B * a.T;
    const long long row0 = (long long)blockIdx.y * a.chunk_rows;
    const long long row1 = min(row0 + a.chunk_rows, rows);
    float acc = 0.0f;
    if (i < a.K) {
        const E* x = static_cast<const E*>(a.x);
        const int d = delay_steps(a.delay[i], a.D);
#pragma unroll 4
        for (long long row = row0 + r; row < row1; row += 4) {
            const int j = (int)(row / a.T), t = (int)(row - (long long)j * a.T);
            const int len = a.lengths ? min(max(a.lengths[j], 0), a.T) : a.T;
            const long long base = a.offsets ? (long long)a.offsets[j] : (long long)j * a.T;
            const bool ok = t >= d && t < len;
            const int tg = ok ? t : 0;        // (row 0 of a sequence always exists)
            const int tb = ok ? t - d : 0;    // x[t - d]
            const int ta = tb > 0 ? tb - 1 : 0;  // x[t - d - 1], 0 before the first step
            const float g = a.gy[(base + tg) * a.ldg + i];
            const float xb = dl_value<E>(x[(base + tb) * a.ldx + i]);
            const float xa = dl_value<E>(x[(base + ta) * a.ldx + i]);
            const float dx = ((tb > 0 ? xa : 0.0f) - xb) * a.scale;
            acc += ok ? g * dx : 0.0f;
        }
    }
    part[r][c] = acc;
    __syncthreads();
    if (r == 0 && i < a.K)
        a.ws[(size_t)blockIdx.y * a.K + i] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

// g_theta[i] = gate_i * (slab 0 + slab 1 + ... in this order)
__global__ __launch_bounds__(256) void delay_grad_finish_kernel(int K, int D, int chunks, const float* delay,
                                                                 const float* ws, float* g_delay) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    float s = 0.0f;
    for (int c = 0; c < chunks; ++c) s += ws[(size_t)c * K + i];
    const float th = delay[i];
    g_delay[i] = (th >= 0.0f && th <= (float)D) ? s : 0.0f;
}

struct DelayStreamArgs {
    int B, Tc, K, D;
    unsigned groups;
    const float* delay;
    const void* x; void* y; void* hist;
    long long ldx, ldy;
};

// One thread per (batch row, piece of N columns): the chunk's Tc delayed steps, then the history moved on by Tc steps.
// hist[h] <- (hist ++ x)[h + Tc] walks h upwards and reads ahead of what it writes, inside the thread's own columns.
template <class E, int N>
__global__ __launch_bounds__(256) void delay_stream_kernel(DelayStreamArgs a) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long b = idx / a.groups;
    const unsigned piece = (unsigned)(idx - b * a.groups);
    if (b >= (unsigned long long)a.B) return;
    const int col = (int)piece * N;
    const E* x = static_cast<const E*>(a.x) + (long long)b * a.Tc * a.ldx + col;
    E* y = static_cast<E*>(a.y) + (long long)b * a.Tc * a.ldy + col;
    E* hist = static_cast<E*>(a.hist) + (long long)b * a.D * a.K + col;
    int d[N];
#pragma unroll
    for (int e = 0; e < N; ++e) d[e] = delay_steps(a.delay[col + e], a.D);
    for (int t = 0; t < a.Tc; ++t) {
        DlVec<E, N> out;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int ts = t - d[e];  // >= -D
            out.v[e] = ts >= 0 ? x[(long long)ts * a.ldx + e] : hist[(long long)(a.D + ts) * a.K + e];
        }
        *reinterpret_cast<DlVec<E, N>*>(y + (long long)t * a.ldy) = out;
    }
    for (int h = 0; h < a.D; ++h) {
        const int s = h + a.Tc;
        const DlVec<E, N> v = s < a.D ? *reinterpret_cast<const DlVec<E, N>*>(hist + (long long)s * a.K)
                                      : *reinterpret_cast<const DlVec<E, N>*>(x + (long long)(s - a.D) * a.ldx);
        *reinterpret_cast<DlVec<E, N>*>(hist + (long long)h * a.K) = v;
    }
}

// the pieces a row is moved in: 16 bytes where K, every row stride and every base address allow, else one element
static int piece_elems(int K, int elem_size, long long ld0, long long ld1, const void* p0, const void* p1,
                       const void* p2 = nullptr) {
    const int n = 16 / elem_size;
    const bool rows_ok = K % n == 0 && ld0 % n == 0 && ld1 % n == 0;
    return (rows_ok && aligned16(p0) && aligned16(p1) && aligned16(p2)) ? n : 1;
}

static bool shape_ok(int B, int T, int K, int max_delay) {
    return B > 0 && T > 0 && K > 0 && max_delay >= 1 && max_delay <= 255;
}

template <bool BWD>
int launch_gather(int B, int T, int K, int elem_size, int max_delay, const float* delay, const void* src, long long lds,
                  void* dst, long long ldd, const int* lengths, const int* offsets, hipStream_t st) {
    const int n = piece_elems(K, elem_size, lds, ldd, src, dst);
    DelayArgs a{B, T, K, max_delay, (unsigned)(K / n), delay, src, dst, lds, ldd, lengths, offsets};
    const dim3 block(256);
    if (n > 1) {  // 16-byte pieces: staged through LDS
        const unsigned long long tiles_t = (unsigned long long)cdiv(T, TILE_ROWS), tiles_c = cdiv((int)a.groups, TILE_PIECES);
        const unsigned long long blocks = (unsigned long long)B * tiles_t * tiles_c;
        if (blocks > 0x7FFFFFFFull) return SPARCH_EINVAL;
        const dim3 grid((unsigned)blocks);
        const size_t lds_bytes = (size_t)(TILE_ROWS + max_delay) * TILE_LD;  // at most 319 rows of 144 bytes
        if (elem_size == 2)
            hipLaunchKernelGGL((delay_gather_tile_kernel<uint16_t, BWD>), grid, block, lds_bytes, st, a, (unsigned)tiles_t,
                               (unsigned)tiles_c);
        else
            hipLaunchKernelGGL((delay_gather_tile_kernel<uint32_t, BWD>), grid, block, lds_bytes, st, a, (unsigned)tiles_t,
                               (unsigned)tiles_c);
    } else {
        const unsigned long long blocks = ((unsigned long long)B * T * a.groups + 255) / 256;
        if (blocks > 0x7FFFFFFFull) return SPARCH_EINVAL;
        const dim3 grid((unsigned)blocks);
        if (elem_size == 2) hipLaunchKernelGGL((delay_gather_kernel<uint16_t, BWD>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((delay_gather_kernel<uint32_t, BWD>), grid, block, 0, st, a);
    }
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// rows of the (B,T) index space per workgroup of the g_theta sum: at most 128 slabs, at least 32 rows each
static long long grad_chunk_rows(long long rows) {
    long long r = (rows + 127) / 128;
    if (r < 32) r = 32;
    return (r + 3) / 4 * 4;
}

}  // namespace

extern "C" int sparch_delay_fwd(int B, int T, int K, int elem_size, int max_delay, const float* delay, const void* x,
                                long long ldx, void* y, long long ldy, const int* lengths, const int* offsets,
                                void* stream) {
    SPARCH_ENTER();
    if (!shape_ok(B, T, K, max_delay) || !delay || !x || !y || ldx < K || ldy < K) return SPARCH_EINVAL;
    if ((elem_size != 2 && elem_size != 4) || (offsets && !lengths)) return SPARCH_EINVAL;
    return launch_gather<false>(B, T, K, elem_size, max_delay, delay, x, ldx, y, ldy, lengths, offsets,
                                (hipStream_t)stream);
}

extern "C" size_t sparch_delay_bwd_workspace_bytes(int B, int T, int K) {
    if (B <= 0 || T <= 0 || K <= 0) return 0;
    const long long rows = (long long)B * T;
    const long long chunk = grad_chunk_rows(rows);
    return (size_t)((rows + chunk - 1) / chunk) * (size_t)K * sizeof(float);
}

extern "C" int sparch_delay_bwd(int B, int T, int K, int x_elem_size, int max_delay, const float* delay,
                                const float* g_y, long long ldg, const void* x, long long ldx, float x_scale,
                                float* g_x, long long ldgx, float* g_delay, void* ws, size_t ws_bytes,
                                const int* lengths, const int* offsets, void* stream) {
    SPARCH_ENTER();
    if (!shape_ok(B, T, K, max_delay) || !delay || !g_y || ldg < K || (!g_x && !g_delay)) return SPARCH_EINVAL;
    if (offsets && !lengths) return SPARCH_EINVAL;
    if (g_x && ldgx < K) return SPARCH_EINVAL;
    if (g_delay && (!x || ldx < K || (x_elem_size != 2 && x_elem_size != 4) || !ws)) return SPARCH_EINVAL;
    if (g_delay && ws_bytes < sparch_delay_bwd_workspace_bytes(B, T, K)) return SPARCH_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (g_x) {
        const int rc = launch_gather<true>(B, T, K, 4, max_delay, delay, g_y, ldg, g_x, ldgx, lengths, offsets, st);
        if (rc != SPARCH_OK) return rc;
    }
    if (g_delay) {
        const long long rows = (long long)B * T;
        const long long chunk = grad_chunk_rows(rows);
        const int chunks = (int)((rows + chunk - 1) / chunk);
        DelayGradArgs a{B, T, K, max_delay, chunk, delay, g_y, ldg, x, ldx, x_scale, (float*)ws, lengths, offsets};
        const dim3 grid((unsigned)cdiv(K, 64), (unsigned)chunks), block(256);
        if (x_elem_size == 2) hipLaunchKernelGGL((delay_grad_partial_kernel<uint16_t>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((delay_grad_partial_kernel<uint32_t>), grid, block, 0, st, a);
        SPARCH_CHECK_LAUNCH();
        hipLaunchKernelGGL(delay_grad_finish_kernel, dim3((unsigned)cdiv(K, 256)), dim3(256), 0, st, K, max_delay,
                           chunks, delay, (const float*)ws, g_delay);
        SPARCH_CHECK_LAUNCH();
    }
    return SPARCH_OK;
}

extern "C" int sparch_delay_stream(int B, int Tc, int K, int elem_size, int max_delay, const float* delay,
                                   const void* x, long long ldx, void* y, long long ldy, void* hist, void* stream) {
    SPARCH_ENTER();
    if (!shape_ok(B, Tc, K, max_delay) || !delay || !x || !y || !hist || ldx < K || ldy < K) return SPARCH_EINVAL;
    if (elem_size != 2 && elem_size != 4) return SPARCH_EINVAL;
    const int n = piece_elems(K, elem_size, ldx, ldy, x, y, hist);
    DelayStreamArgs a{B, Tc, K, max_delay, (unsigned)(K / n), delay, x, y, hist, ldx, ldy};
    const unsigned long long blocks = ((unsigned long long)B * a.groups + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return SPARCH_EINVAL;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 2 && n == 8) hipLaunchKernelGGL((delay_stream_kernel<uint16_t, 8>), grid, block, 0, st, a);
    else if (elem_size == 2) hipLaunchKernelGGL((delay_stream_kernel<uint16_t, 1>), grid, block, 0, st, a);
    else if (n == 4) hipLaunchKernelGGL((delay_stream_kernel<uint32_t, 4>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((delay_stream_kernel<uint32_t, 1>), grid, block, 0, st, a);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

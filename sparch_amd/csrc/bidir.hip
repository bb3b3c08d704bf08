// Bidirectional layers on ragged batches: the data movements in front of and behind the one-direction `_len` / `_pk`
// cell kernels ("Bidirectional ragged batches").
//
// A bidirectional layer on B clips of lengths L[b] runs the one-direction cell on 2B sequences: sequence b is clip b,
// sequence B + b is clip b read backwards INSIDE ITS OWN LENGTH (step t of it is the clip's step L[b] - 1 - t).
//   split      (B,T,C) -> (2B,T,C): rows [0,B) a copy, row B + b the flipped clip, zeros on every tail
//   split_bwd  its adjoint: g_src[b,t] = g[b,t] + g[B+b, L[b]-1-t], zero on the tails
//   join       (2B,T,H) bf16 0/1 plane -> (B,T,2H): y[b,t,:H] = s[b,t], y[b,t,H:] = s[B+b, L[b]-1-t], zero tails; also the
//              fp32 tensor (plane * scale) when asked for, and the spikes counted per output column (integer atomics)
//   join_bwd   its adjoint, a gather (B,T,2H) -> (2B,T,H), plus the firing rate's gradient on the valid steps
// Every kernel indexes the PADDED space (sequence j, step t, piece): no search in offsets, as pack_rows_kernel.  The
// packed (`_pk`) forms take the single batch's plan (lengths sorted descending, offsets their exclusive prefix sum) and,
// per sequence, the first row of its forward and of its reverse twin in the doubled packed tensor (fwd, rev): where
// the doubled plan puts them is the host's business.  There are no tails in a packed tensor.
#include "common.h"

namespace {

typedef unsigned bd_u32x4 __attribute__((ext_vector_type(4)));

struct BidirMap {
    int B, T;            // sequences; steps of the index space (packed: the longest length)
    const int* lengths;  // (B,)
    const int* offsets;  // packed: (B + 1,) rows of the single batch; nullptr: the padded layout
    const int* fwd;      // packed: (B,) first doubled row of sequence j ...
    const int* rev;      // ... and of its reversed twin
};

// rows of step t of sequence j: in the single tensor (one), in the doubled one forward (f) and reversed (r).  For a
// tail step (t >= L, padded layout only) f and r are the two tail rows to clear.
struct BidirRows { size_t one, f, r; bool in; };
__device__ __forceinline__ BidirRows bidir_rows(const BidirMap& m, int j, int t) {
    const int L = m.lengths[j];
    BidirRows q;
    q.in = t < L;
    if (m.offsets) {
        q.one = (size_t)m.offsets[j] + t;
        q.f = (size_t)m.fwd[j] + t;
        q.r = (size_t)m.rev[j] + (q.in ? L - 1 - t : 0);
    } else {
        q.one = (size_t)j * m.T + t;
        q.f = q.one;
        q.r = ((size_t)m.B + j) * m.T + (q.in ? L - 1 - t : t);
    }
    return q;
}

// ---------------------------------------------------------------------------------------------- split and its adjoint
struct SplitArgs {
    BidirMap m;
    unsigned row_pieces;  // pieces (of sizeof(V) bytes) per row
    const void* src; void* dst;
};

// BWD: dst is the single tensor, src the doubled one (fp32 pieces): dst = src[f] + src[r].
template <class V, bool BWD>
__global__ __launch_bounds__(256) void bidir_split_kernel(SplitArgs a) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long row = idx / a.row_pieces;
    const unsigned piece = (unsigned)(idx - row * a.row_pieces);
    if (row >= (unsigned long long)a.m.B * a.m.T) return;
    const int j = (int)(row / a.m.T), t = (int)(row - (unsigned long long)j * a.m.T);
    const BidirRows q = bidir_rows(a.m, j, t);
    if (!q.in && a.m.offsets) return;  // packed: no tails
    const size_t one = q.one * a.row_pieces + piece, f = q.f * a.row_pieces + piece, r = q.r * a.row_pieces + piece;
    if constexpr (BWD) {
        V v{};
        if (q.in) v = static_cast<const V*>(a.src)[f] + static_cast<const V*>(a.src)[r];
        static_cast<V*>(a.dst)[one] = v;
    } else {
        V v{};
        if (q.in) v = static_cast<const V*>(a.src)[one];
        static_cast<V*>(a.dst)[f] = v;
        static_cast<V*>(a.dst)[r] = v;
    }
}

bool map_ok(int B, int T, int C, const int* lengths, long long n_valid, bool pk, const int* offsets, const int* fwd,
            const int* rev) {
    if (B <= 0 || T <= 0 || C <= 0 || !lengths || n_valid < 1 || n_valid > (long long)B * T) return false;
    if (B > 0x3FFFFFFF) return false;  // (2B sequences)
    return !pk || (offsets && fwd && rev);
}

// blocks of 256 threads for `threads` threads, or 0 where the grid would not fit
unsigned blocks_for(unsigned long long threads) {
    const unsigned long long blocks = (threads + 255) / 256;
    return blocks > 0x7FFFFFFFull ? 0u : (unsigned)blocks;
}

int split_fwd(int B, int T, int C, int elem_size, const void* src, void* dst, const int* lengths, const int* offsets,
              const int* fwd, const int* rev, long long n_valid, bool pk, void* stream) {
    if (!map_ok(B, T, C, lengths, n_valid, pk, offsets, fwd, rev) || !src || !dst) return SPARCH_EINVAL;
    if (elem_size != 1 && elem_size != 2 && elem_size != 4) return SPARCH_EINVAL;
    const uintptr_t both = (uintptr_t)src | (uintptr_t)dst;
    if (both % elem_size != 0) return SPARCH_EALIGN;
    const size_t row_bytes = (size_t)C * elem_size;
    const int w = (row_bytes % 16 == 0 && both % 16 == 0) ? 16 : (row_bytes % 4 == 0 && both % 4 == 0) ? 4
                  : (row_bytes % 2 == 0 && both % 2 == 0) ? 2 : 1;
    if (row_bytes / w > 0xFFFFFFFFull) return SPARCH_EINVAL;
    SplitArgs a{{B, T, lengths, pk ? offsets : nullptr, fwd, rev}, (unsigned)(row_bytes / w), src, dst};
    const unsigned blocks = blocks_for((unsigned long long)B * T * a.row_pieces);
    if (!blocks) return SPARCH_EINVAL;
    const dim3 grid(blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (w) {
        case 16: hipLaunchKernelGGL((bidir_split_kernel<bd_u32x4, false>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((bidir_split_kernel<uint32_t, false>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((bidir_split_kernel<uint16_t, false>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((bidir_split_kernel<uint8_t, false>), grid, block, 0, st, a); break;
    }
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

int split_bwd(int B, int T, int C, const float* g, float* g_src, const int* lengths, const int* offsets, const int* fwd,
              const int* rev, long long n_valid, bool pk, void* stream) {
    if (!map_ok(B, T, C, lengths, n_valid, pk, offsets, fwd, rev) || !g || !g_src) return SPARCH_EINVAL;
    const uintptr_t both = (uintptr_t)g | (uintptr_t)g_src;
    if (both % 4 != 0) return SPARCH_EALIGN;
    const bool wide = C % 4 == 0 && both % 16 == 0;
    SplitArgs a{{B, T, lengths, pk ? offsets : nullptr, fwd, rev}, (unsigned)(wide ? C / 4 : C), g, g_src};
    const unsigned blocks = blocks_for((unsigned long long)B * T * a.row_pieces);
    if (!blocks) return SPARCH_EINVAL;
    const dim3 grid(blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL((bidir_split_kernel<f32x4, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bidir_split_kernel<float, true>), grid, block, 0, st, a);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// ---------------------------------------------------------------------------------------------------------------- join
struct JoinArgs {
    BidirMap m;
    unsigned half_pieces;  // pieces (of sizeof(V) bytes) per H bf16 values: an output row has twice as many
    int rows_per_block;    // steps of the index space one block walks through
    const void* s16; void* y16;
    float* y32; float scale;
    unsigned* count;
};

constexpr int JOIN_WAVES = 4;  // a block is 4 waves of 64 lanes: lane = output piece, wave = step

// Lane p of a wave owns output piece p of every step the wave visits, so the spikes it sees belong to the same E
// columns throughout: they are counted in registers, summed over the block's waves in LDS, and one integer atomic per
// column and block reaches memory.
template <class V>
__global__ __launch_bounds__(64 * JOIN_WAVES) void bidir_join_kernel(JoinArgs a) {
    constexpr int E = sizeof(V) / 2;
    __shared__ unsigned red[JOIN_WAVES][64 * E];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned p = blockIdx.x * 64u + lane, out_pieces = 2u * a.half_pieces;
    const bool mine = p < out_pieces;
    const unsigned d = (mine && p >= a.half_pieces) ? 1u : 0u, q = p - d * a.half_pieces;
    unsigned cnt[E];
#pragma unroll
    for (int e = 0; e < E; ++e) cnt[e] = 0u;
    const unsigned long long rows = (unsigned long long)a.m.B * a.m.T;
    const unsigned long long row0 = (unsigned long long)blockIdx.y * a.rows_per_block;
    for (int i = (int)wave; i < a.rows_per_block && mine; i += JOIN_WAVES) {
        const unsigned long long row = row0 + i;
        if (row >= rows) break;
        const int j = (int)(row / a.m.T), t = (int)(row - (unsigned long long)j * a.m.T);
        const BidirRows k = bidir_rows(a.m, j, t);
        if (!k.in && a.m.offsets) continue;  // packed: no tails
        V v{};
        if (k.in) v = static_cast<const V*>(a.s16)[(d ? k.r : k.f) * a.half_pieces + q];
        static_cast<V*>(a.y16)[k.one * out_pieces + p] = v;
        uint16_t h[E];
        __builtin_memcpy(h, &v, sizeof(V));
#pragma unroll
        for (int e = 0; e < E; ++e) cnt[e] += (h[e] & 0x7FFFu) ? 1u : 0u;
        if (a.y32) {
            float f[E];
#pragma unroll
            for (int e = 0; e < E; ++e) f[e] = bf16_to_f32(h[e]) * a.scale;
            float* o = a.y32 + (k.one * out_pieces + p) * E;
            if constexpr (E == 8) {  // (the 16-byte form is chosen only where y32 is 16-byte aligned too)
                reinterpret_cast<f32x4*>(o)[0] = f32x4{f[0], f[1], f[2], f[3]};
                reinterpret_cast<f32x4*>(o)[1] = f32x4{f[4], f[5], f[6], f[7]};
            } else {
#pragma unroll
                for (int e = 0; e < E; ++e) o[e] = f[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) red[wave][lane * E + e] = cnt[e];
    __syncthreads();
    if (wave == 0 && mine) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            unsigned n = 0;
            for (int w = 0; w < JOIN_WAVES; ++w) n += red[w][lane * E + e];
            if (n) atomicAdd(a.count + (size_t)p * E + e, n);
        }
    }
}

int join_fwd(int B, int T, int H, const uint16_t* s16, uint16_t* y16, float* y32, float scale, uint32_t* count,
             const int* lengths, const int* offsets, const int* fwd, const int* rev, long long n_valid, bool pk,
             void* stream) {
    if (!map_ok(B, T, H, lengths, n_valid, pk, offsets, fwd, rev) || !s16 || !y16 || !count) return SPARCH_EINVAL;
    if (H > 0x3FFFFFFF) return SPARCH_EINVAL;
    const uintptr_t both = (uintptr_t)s16 | (uintptr_t)y16;
    if (both % 2 != 0 || (uintptr_t)y32 % 4 != 0 || (uintptr_t)count % 4 != 0) return SPARCH_EALIGN;
    const size_t half_bytes = (size_t)H * 2;
    const int w = (half_bytes % 16 == 0 && (both | (uintptr_t)y32) % 16 == 0) ? 16
                  : (half_bytes % 4 == 0 && both % 4 == 0) ? 4 : 2;
    JoinArgs a{{B, T, lengths, pk ? offsets : nullptr, fwd, rev}, (unsigned)(half_bytes / w), 32, s16, y16, y32, scale, count};
    const unsigned long long rows = (unsigned long long)B * T;
    unsigned long long gy = (rows + a.rows_per_block - 1) / a.rows_per_block;
    if (gy > 65535ull) {  // (the grid's y extent: longer walks per block instead)
        const unsigned long long per = (rows + 65534ull) / 65535ull;
        if (per > 0x7FFFFFFFull) return SPARCH_EINVAL;
        a.rows_per_block = (int)per;
        gy = (rows + per - 1) / per;
    }
    const dim3 grid((2u * a.half_pieces + 63u) / 64u, (unsigned)gy), block(64 * JOIN_WAVES);
    hipStream_t st = (hipStream_t)stream;
    switch (w) {
        case 16: hipLaunchKernelGGL((bidir_join_kernel<bd_u32x4>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((bidir_join_kernel<uint32_t>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((bidir_join_kernel<uint16_t>), grid, block, 0, st, a); break;
    }
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// ------------------------------------------------------------------------------------------------ the join's adjoint
struct JoinBwdArgs {
    BidirMap m;
    unsigned half_pieces;  // pieces (of sizeof(V) bytes) per H fp32 values
    const float* g; const float* g_rate; float rate_scale;
    float* g2;
};

// One thread per piece of the (B,T,2H) gradient: it goes to the row of the doubled tensor its spikes came from, with
// the firing rate's gradient g_rate[column] * rate_scale added (one fp32 product, one fp32 sum); the doubled tensor's
// tail rows are cleared by the tail steps' threads.
template <class V>
__global__ __launch_bounds__(256) void bidir_join_bwd_kernel(JoinBwdArgs a) {
    constexpr int E = sizeof(V) / 4;
    const unsigned out_pieces = 2u * a.half_pieces;
    const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long row = idx / out_pieces;
    const unsigned p = (unsigned)(idx - row * out_pieces);
    if (row >= (unsigned long long)a.m.B * a.m.T) return;
    const int j = (int)(row / a.m.T), t = (int)(row - (unsigned long long)j * a.m.T);
    const BidirRows k = bidir_rows(a.m, j, t);
    if (!k.in && a.m.offsets) return;  // packed: no tails
    const unsigned d = p >= a.half_pieces ? 1u : 0u, q = p - d * a.half_pieces;
    float v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = 0.0f;
    if (k.in) {
        const V in = reinterpret_cast<const V*>(a.g)[k.one * out_pieces + p];
        __builtin_memcpy(v, &in, sizeof(V));
        if (a.g_rate) {
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = v[e] + a.g_rate[(size_t)p * E + e] * a.rate_scale;
        }
    }
    V out;
    __builtin_memcpy(&out, v, sizeof(V));
    reinterpret_cast<V*>(a.g2)[(d ? k.r : k.f) * a.half_pieces + q] = out;
}

int join_bwd(int B, int T, int H, const float* g, const float* g_rate, float rate_scale, float* g2, const int* lengths,
             const int* offsets, const int* fwd, const int* rev, long long n_valid, bool pk, void* stream) {
    if (!map_ok(B, T, H, lengths, n_valid, pk, offsets, fwd, rev) || !g || !g2) return SPARCH_EINVAL;
    if (H > 0x3FFFFFFF) return SPARCH_EINVAL;
    const uintptr_t both = (uintptr_t)g | (uintptr_t)g2;
    if (both % 4 != 0 || (uintptr_t)g_rate % 4 != 0) return SPARCH_EALIGN;
    const bool wide = H % 4 == 0 && both % 16 == 0;
    JoinBwdArgs a{{B, T, lengths, pk ? offsets : nullptr, fwd, rev}, (unsigned)(wide ? H / 4 : H), g, g_rate, rate_scale, g2};
    const unsigned blocks = blocks_for((unsigned long long)B * T * 2ull * a.half_pieces);
    if (!blocks) return SPARCH_EINVAL;
    const dim3 grid(blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL((bidir_join_bwd_kernel<f32x4>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((bidir_join_bwd_kernel<float>), grid, block, 0, st, a);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

}  // namespace

extern "C" int sparch_bidir_split_len(int B, int T, int C, int elem_size, const void* src, void* dst, const int* lengths,
                                      long long n_valid, void* stream) {
    SPARCH_ENTER();
    return split_fwd(B, T, C, elem_size, src, dst, lengths, nullptr, nullptr, nullptr, n_valid, false, stream);
}

extern "C" int sparch_bidir_split_pk(int B, int T, int C, int elem_size, const void* src, void* dst, const int* lengths,
                                     const int* offsets, const int* fwd, const int* rev, long long n_valid, void* stream) {
    SPARCH_ENTER();
    return split_fwd(B, T, C, elem_size, src, dst, lengths, offsets, fwd, rev, n_valid, true, stream);
}

extern "C" int sparch_bidir_split_bwd_len(int B, int T, int C, const float* g, float* g_src, const int* lengths,
                                          long long n_valid, void* stream) {
    SPARCH_ENTER();
    return split_bwd(B, T, C, g, g_src, lengths, nullptr, nullptr, nullptr, n_valid, false, stream);
}

extern "C" int sparch_bidir_split_bwd_pk(int B, int T, int C, const float* g, float* g_src, const int* lengths,
                                         const int* offsets, const int* fwd, const int* rev, long long n_valid,
                                         void* stream) {
    SPARCH_ENTER();
    return split_bwd(B, T, C, g, g_src, lengths, offsets, fwd, rev, n_valid, true, stream);
}

extern "C" int sparch_bidir_join_len(int B, int T, int H, const uint16_t* s16, uint16_t* y16, float* y32, float scale,
                                     uint32_t* spike_count, const int* lengths, long long n_valid, void* stream) {
    SPARCH_ENTER();
    return join_fwd(B, T, H, s16, y16, y32, scale, spike_count, lengths, nullptr, nullptr, nullptr, n_valid, false, stream);
}

extern "C" int sparch_bidir_join_pk(int B, int T, int H, const uint16_t* s16, uint16_t* y16, float* y32, float scale,
                                    uint32_t* spike_count, const int* lengths, const int* offsets, const int* fwd,
                                    const int* rev, long long n_valid, void* stream) {
    SPARCH_ENTER();
    return join_fwd(B, T, H, s16, y16, y32, scale, spike_count, lengths, offsets, fwd, rev, n_valid, true, stream);
}

extern "C" int sparch_bidir_join_bwd_len(int B, int T, int H, const float* g, const float* g_rate, float rate_scale,
                                         float* g2, const int* lengths, long long n_valid, void* stream) {
    SPARCH_ENTER();
    return join_bwd(B, T, H, g, g_rate, rate_scale, g2, lengths, nullptr, nullptr, nullptr, n_valid, false, stream);
}

extern "C" int sparch_bidir_join_bwd_pk(int B, int T, int H, const float* g, const float* g_rate, float rate_scale,
                                        float* g2, const int* lengths, const int* offsets, const int* fwd, const int* rev,
                                        long long n_valid, void* stream) {
    SPARCH_ENTER();
    return join_bwd(B, T, H, g, g_rate, rate_scale, g2, lengths, offsets, fwd, rev, n_valid, true, stream);
}

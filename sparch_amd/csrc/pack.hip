// Packed ragged batches: the row gather / scatter between a padded (B,T,C) tensor and the packed (N,C) one.
//
// The batch's sequences are sorted by length, descending and stable: sequence j of that order is batch row order[j],
// has lengths[j] steps and occupies packed rows [offsets[j], offsets[j] + lengths[j]) — offsets is the exclusive prefix
// sum, offsets[B] = N.  sparch_pack_rows copies step t < lengths[j] of batch row order[j] to packed row offsets[j] + t;
// sparch_unpack_rows copies it back and writes zeros on every row's tail, so that its target needs no clearing.
// Rows are moved as raw bytes (elements of 1, 2 or 4 bytes: uint8 counts, bf16 planes, fp32 tensors) in the widest
// pieces the row size and the two base addresses allow: 16 bytes where C * size is a multiple of 16.
#include "common.h"

namespace {

typedef unsigned pk_u32x4 __attribute__((ext_vector_type(4)));

struct PackArgs {
    int B, T;
    unsigned row_pieces;  // pieces (of sizeof(V) bytes) per row
    const void* src; void* dst;
    const int* order; const int* lengths; const int* offsets;
};

// One thread per piece of the PADDED index space (j, t, piece): a packed row's sequence would otherwise have to be
// searched for in offsets.  UNPACK: packed -> padded with zero tails; else padded -> packed (tail threads do nothing).
template <class V, bool UNPACK>
__global__ __launch_bounds__(256) void pack_rows_kernel(PackArgs a) {
    const unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long row = idx / a.row_pieces;
    const unsigned piece = (unsigned)(idx - row * a.row_pieces);
    if (row >= (unsigned long long)a.B * a.T) return;
    const int j = (int)(row / a.T), t = (int)(row - (unsigned long long)j * a.T);
    const bool in = t < a.lengths[j];
    const size_t padded = ((size_t)a.order[j] * a.T + t) * a.row_pieces + piece;
    const size_t packed = ((size_t)a.offsets[j] + t) * a.row_pieces + piece;  // (used only where `in`)
    if constexpr (UNPACK) {
        V v{};
        if (in) v = static_cast<const V*>(a.src)[packed];
        static_cast<V*>(a.dst)[padded] = v;
    } else {
        if (in) static_cast<V*>(a.dst)[packed] = static_cast<const V*>(a.src)[padded];
    }
}

template <bool UNPACK>
int pack_rows(int B, int T, int C, int elem_size, const void* src, void* dst, const int* order, const int* lengths,
              const int* offsets, long long n_valid, void* stream) {
    if (B <= 0 || T <= 0 || C <= 0 || !src || !dst || !order || !lengths || !offsets || n_valid < 1) return SPARCH_EINVAL;
    if (elem_size != 1 && elem_size != 2 && elem_size != 4) return SPARCH_EINVAL;
    if (n_valid > (long long)B * T) return SPARCH_EINVAL;
    const size_t row_bytes = (size_t)C * elem_size;
    const uintptr_t both = (uintptr_t)src | (uintptr_t)dst;
    const int w = (row_bytes % 16 == 0 && both % 16 == 0) ? 16 : (row_bytes % 4 == 0 && both % 4 == 0) ? 4
                  : (row_bytes % 2 == 0 && both % 2 == 0) ? 2 : 1;
    if (row_bytes / w > 0xFFFFFFFFull) return SPARCH_EINVAL;
    PackArgs a{B, T, (unsigned)(row_bytes / w), src, dst, order, lengths, offsets};
    const unsigned long long threads = (unsigned long long)B * T * a.row_pieces;
    const unsigned long long blocks = (threads + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return SPARCH_EINVAL;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (w) {
        case 16: hipLaunchKernelGGL((pack_rows_kernel<pk_u32x4, UNPACK>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((pack_rows_kernel<uint32_t, UNPACK>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((pack_rows_kernel<uint16_t, UNPACK>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((pack_rows_kernel<uint8_t, UNPACK>), grid, block, 0, st, a); break;
    }
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

}  // namespace

extern "C" int sparch_pack_rows(int B, int T, int C, int elem_size, const void* src, void* dst, const int* order,
                                const int* lengths, const int* offsets, long long n_valid, void* stream) {
    SPARCH_ENTER();
    return pack_rows<false>(B, T, C, elem_size, src, dst, order, lengths, offsets, n_valid, stream);
}

extern "C" int sparch_unpack_rows(int B, int T, int C, int elem_size, const void* src, void* dst, const int* order,
                                  const int* lengths, const int* offsets, long long n_valid, void* stream) {
    SPARCH_ENTER();
    return pack_rows<true>(B, T, C, elem_size, src, dst, order, lengths, offsets, n_valid, stream);
}

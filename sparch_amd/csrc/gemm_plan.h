// Host-side arithmetic of the matrix products (gemm_spike.hip, gemm.hip), in one place: which leading dimensions a
// product form accepts, into how many K ranges a product is cut, how long a range is and how many bytes its slabs
// take.  Plain C++17, no HIP types: a host compiler builds it alone (a sweep over the whole input grid needs no GPU).
#pragma once
#include <cstddef>

namespace gemm_plan {

// C[M,N] = A * B with A given as [M,K] (NT, NN) or [K,M] (TN) and B as [N,K] (NT) or [K,N] (NN, TN), row-major
enum class Form { NT, NN, TN };

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// positive sizes, and every leading dimension at least its row's width
constexpr bool dims_ok(Form f, int M, int N, int K, int lda, int ldb, int ldc) {
    return M > 0 && N > 0 && K > 0 && lda >= (f == Form::TN ? M : K) && ldb >= (f == Form::NT ? K : N) && ldc >= N;
}

// K ranges of a product on BM x BN tiles that runs one workgroup per CU: one full round of co-resident workgroups (a
// partial second round costs more than the shorter K range per workgroup gains), at least 8 K tiles per range (the
// pipelined kernel's minimum).
constexpr int splits_for(int M, int N, int K, int BM, int BN, int BK, int target_wgs) {
    const int tiles = cdiv(M, BM) * cdiv(N, BN), kt = cdiv(K, BK);
    int s = target_wgs / tiles;
    if (s > kt / 8) s = kt / 8;
    return s < 1 ? 1 : s;
}

// gemm.hip's rule: doubled until there are about 1024 workgroups (4 per CU), at least 8 K tiles per range
constexpr int splits_doubling(int M, int N, int K, int BM, int BN, int BK) {
    const int tiles = cdiv(M, BM) * cdiv(N, BN), kt = cdiv(K, BK);
    int s = 1;
    while (tiles * s < 1024 && kt / (s * 2) >= 8) s *= 2;
    return s;
}

// length of a K range, whole K tiles: of a direct product (one range) and of one cut into `splits`
constexpr int k_per_split(int K, int BK, int splits = 1) { return cdiv(cdiv(K, splits), BK) * BK; }

// `splits` slabs of M rows, `width` floats each
constexpr size_t slab_bytes(int splits, int M, int width) { return (size_t)splits * M * width * sizeof(float); }

}  // namespace gemm_plan

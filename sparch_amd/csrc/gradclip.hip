// Gradient clipping by global norm, on the device and in a fixed reduction order ("Gradient
// clipping"): the norm of a whole gradient list, the clip coefficient and the decision to skip a non-finite step are
// made by two kinds of launch and left in an 8-word clip state that sparch_adam_step_clip (optim.hip) and
// sparch_scale_grads read.  Nothing comes back to the host.
//
//   grad_sumsq    the tensor table travels in the kernel argument as in adam_kernel (24 tensors per launch, 4096
//                 elements per workgroup, empty tensors passed over).  Thread t of a workgroup owns the elements
//                 base + 1024 j + 4 t + {0..3}, j = 0..3, and adds (double)g * g over them in that order; a fixed
//                 256-lane tree in double follows.  ONE double per workgroup goes to the workspace.  No atomics and no
//                 "last block" ticket: the result does not depend on the order in which workgroups run, nor on
//                 whether a tensor could be read with 16-byte loads (the ownership of elements is the same either
//                 way), so every replica of a data-parallel run gets the same bits.
//   clip_finish   one workgroup.  A wave per tensor sums that tensor's partials (lane l takes every 64th, then a
//                 butterfly), wave 0 sums the tensors' sums the same way; all in double, then ONE rounding to fp32.
//
// Workspace: P doubles (one per workgroup, in table order), n_tensors doubles (per-tensor sums) and n_tensors
// {first partial, number of partials} pairs, which grad_sumsq writes from its kernel argument (no host copy: the call
// can be captured in a HIP graph).
#include "common.h"

#include <cmath>

namespace {

constexpr int CLIP_MAX = 24;       // tensors per launch (kernel-argument budget), as ADAM_MAX
constexpr int CLIP_CHUNK = 4096;   // elements per workgroup, as ADAM_CHUNK

struct Span { long long first, count; };

struct SumsqBatch {
    const float* g[CLIP_MAX];
    long long first_blk[CLIP_MAX + 1];  // prefix sum of ceil(n / CLIP_CHUNK) within the launch
    long long n[CLIP_MAX];
    int slot[CLIP_MAX];                 // the tensor's index in the caller's table
    int count;
    int slot_lo, slot_hi;               // the table slots this launch answers for (the empty ones among them: count 0)
    long long pbase;                    // index of this launch's first partial
    double* partials;
    Span* spans;
};

__global__ __launch_bounds__(256) void grad_sumsq_kernel(SumsqBatch a) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {  // the spans of this launch's slots, for clip_finish
        for (int s = a.slot_lo + tid; s < a.slot_hi; s += 256) a.spans[s] = Span{0, 0};
        __syncthreads();
        if (tid < a.count) a.spans[a.slot[tid]] = Span{a.pbase + a.first_blk[tid], a.first_blk[tid + 1] - a.first_blk[tid]};
    }
    int ti = 0;
    while (ti + 1 < a.count && (long long)blockIdx.x >= a.first_blk[ti + 1]) ++ti;  // uniform, <= 24 steps
    const long long base = ((long long)blockIdx.x - a.first_blk[ti]) * CLIP_CHUNK;
    const long long n = a.n[ti];
    const float* __restrict__ g = a.g[ti];
    const bool vec = (reinterpret_cast<uintptr_t>(g) & 15u) == 0;  // base is a multiple of 4096 elements
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < CLIP_CHUNK / 1024; ++j) {
        const long long i = base + (long long)j * 1024 + tid * 4;
        if (i >= n) break;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec && i + 3 < n) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(g + i);
            x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i + k < n) x[k] = g[i + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)x[k] * (double)x[k];  // (+0 for the elements behind n)
    }
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.partials[a.pbase + blockIdx.x] = red[0];
}

// sum over the 64 lanes of a wave, the same bits in every lane (fp addition is commutative: both partners of an
// exchange form the same sum)
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

__global__ __launch_bounds__(256) void clip_finish_kernel(const double* __restrict__ partials, const Span* __restrict__ spans,
                                                          double* __restrict__ tsum, int n_tensors, int have_spans,
                                                          float max_norm, uint32_t* __restrict__ clip,
                                                          float* __restrict__ tensor_norms,
                                                          const uint32_t* __restrict__ skip_if_nonzero) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < n_tensors; t += 4) {
        const Span sp = have_spans ? spans[t] : Span{0, 0};
        double acc = 0.0;
        for (long long k = lane; k < sp.count; k += 64) acc += partials[sp.first + k];
        acc = wave_sum(acc);
        if (lane == 0) {
            tsum[t] = acc;
            if (tensor_norms) tensor_norms[t] = (float)sqrt(acc);
        }
    }
    __syncthreads();  // (tsum: written and read by this workgroup only)
    if (wave != 0) return;
    double total = 0.0;
    for (int t = lane; t < n_tensors; t += 64) total += tsum[t];
    total = wave_sum(total);
    if (lane != 0) return;
    const float norm = (float)sqrt(total);
    clip[0] = __float_as_uint(norm);
    clip[7] = 0u;
    if (skip_if_nonzero && *skip_if_nonzero != 0u) {  // a timed-out step: the optimizer skips on the word itself
        clip[1] = __float_as_uint(1.0f);
        clip[2] = 0u;
        return;
    }
    // torch.nn.utils.clip_grad_norm_'s formula and epsilon: three fp32 operations
    const float coef = fminf(max_norm / (norm + 1e-6f), 1.0f);
    clip[1] = __float_as_uint(coef);
    if (!(fabsf(norm) <= 3.402823466e38f)) {  // NaN or inf (a sum of squares above fp32's range counts as inf)
        clip[2] = 1u;
        clip[3] += 1u;
        return;
    }
    clip[2] = 0u;
    clip[4] += 1u;
    if (coef < 1.0f) clip[5] += 1u;
    if (norm > __uint_as_float(clip[6])) clip[6] = __float_as_uint(norm);
}

struct ScaleBatch {
    float* g[CLIP_MAX];
    long long first_blk[CLIP_MAX + 1];
    long long n[CLIP_MAX];
    int count;
    const uint32_t* clip;
};

__global__ __launch_bounds__(256) void scale_grads_kernel(ScaleBatch a) {
    if (a.clip[2] != 0u) return;  // a non-finite norm: the gradients stay as they are (torch would write NaNs)
    const float coef = __uint_as_float(a.clip[1]);
    int ti = 0;
    while (ti + 1 < a.count && (long long)blockIdx.x >= a.first_blk[ti + 1]) ++ti;  // uniform, <= 24 steps
    const long long base = ((long long)blockIdx.x - a.first_blk[ti]) * CLIP_CHUNK;
    const long long n = a.n[ti];
    float* __restrict__ g = a.g[ti];
#pragma unroll 4
    for (int j = 0; j < CLIP_CHUNK / 256; ++j) {
        const long long i = base + (long long)j * 256 + threadIdx.x;
        if (i >= n) break;
        g[i] = g[i] * coef;
    }
}

// the table checks every entry of this file makes before any device work; returns the number of partials (>= 0)
long long table_partials(int n_tensors, const void* const* ptrs, const int64_t* numel) {
    if (n_tensors < 0 || (n_tensors > 0 && (!numel || !ptrs))) return -1;
    long long blocks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numel[t] < 0 || (numel[t] > 0 && !ptrs[t])) return -1;
        blocks += (numel[t] + CLIP_CHUNK - 1) / CLIP_CHUNK;
        if (blocks > 0x7fffffffLL) return -1;  // (a grid's x extent)
    }
    return blocks;
}

size_t ws_bytes_for(long long partials, int n_tensors) {
    return (size_t)partials * sizeof(double) + (size_t)n_tensors * (sizeof(double) + sizeof(Span));
}

}  // namespace

extern "C" size_t sparch_grad_norm_ws_bytes(int n_tensors, const int64_t* numel) {
    if (n_tensors <= 0 || !numel) return 0;
    long long blocks = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numel[t] < 0) return 0;
        blocks += (numel[t] + CLIP_CHUNK - 1) / CLIP_CHUNK;
    }
    return ws_bytes_for(blocks, n_tensors);
}

extern "C" int sparch_grad_norm(int n_tensors, const float* const* grads, const int64_t* numel, float max_norm,
                                void* ws, size_t ws_bytes, uint32_t* clip, float* tensor_norms,
                                const uint32_t* skip_if_nonzero, void* stream) {
    SPARCH_ENTER();
    const long long total = table_partials(n_tensors, reinterpret_cast<const void* const*>(grads), numel);
    if (total < 0) return SPARCH_EINVAL;
    if (!(max_norm > 0.0f)) return SPARCH_EINVAL;  // NaN, zero or negative
    if (!clip) return SPARCH_EINVAL;
    const size_t need = ws_bytes_for(total, n_tensors);
    if (need > 0 && (!ws || ws_bytes < need)) return SPARCH_EWORKSPACE;
    double* partials = static_cast<double*>(ws);
    double* tsum = partials + total;
    Span* spans = reinterpret_cast<Span*>(tsum + n_tensors);
    long long pbase = 0;
    int launches = 0;
    for (int t = 0; t < n_tensors;) {  // ONE running index, as sparch_adam_step
        SumsqBatch a{};
        a.slot_lo = t;
        long long blk = 0;
        for (; t < n_tensors && a.count < CLIP_MAX; ++t) {
            if (numel[t] == 0) continue;
            const int c = a.count++;
            a.g[c] = grads[t];
            a.n[c] = numel[t];
            a.slot[c] = t;
            a.first_blk[c] = blk;
            blk += (numel[t] + CLIP_CHUNK - 1) / CLIP_CHUNK;
        }
        a.first_blk[a.count] = blk;
        while (t < n_tensors && numel[t] == 0) ++t;  // the empty slots behind its last tensor are this launch's too
        a.slot_hi = t;
        if (a.count == 0) break;  // every tensor is empty: nothing to launch, clip_finish is told so
        a.pbase = pbase;
        a.partials = partials;
        a.spans = spans;
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, a);
        SPARCH_CHECK_LAUNCH();
        pbase += blk;
        ++launches;
    }
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, spans, tsum, n_tensors,
                       launches > 0 ? 1 : 0, max_norm, clip, tensor_norms, skip_if_nonzero);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_scale_grads(int n_tensors, float* const* grads, const int64_t* numel, const uint32_t* clip,
                                  void* stream) {
    SPARCH_ENTER();
    if (table_partials(n_tensors, reinterpret_cast<const void* const*>(grads), numel) < 0) return SPARCH_EINVAL;
    if (!clip) return SPARCH_EINVAL;
    for (int t = 0; t < n_tensors;) {
        ScaleBatch a{};
        long long blk = 0;
        for (; t < n_tensors && a.count < CLIP_MAX; ++t) {
            if (numel[t] == 0) continue;
            const int c = a.count++;
            a.g[c] = grads[t];
            a.n[c] = numel[t];
            a.first_blk[c] = blk;
            blk += (numel[t] + CLIP_CHUNK - 1) / CLIP_CHUNK;
        }
        a.first_blk[a.count] = blk;
        if (a.count == 0) continue;
        a.clip = clip;
        hipLaunchKernelGGL(scale_grads_kernel, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, a);
        SPARCH_CHECK_LAUNCH();
    }
    return SPARCH_OK;
}

// f-3  Batches of HD / SC from a device-resident audio store (functional.AudioStore: every clip of a split in one flat
// sample array, uploaded once) and a device list of clip indices.  Nothing here has arithmetic of its own:
//   * audio_gather_fbank_kernel is fbank_padded_kernel (fbank.hip) with the clip found through idx -> starts / lengths
//     instead of a row of a batch buffer; tables and frames come from the same device functions (fbank_frame.h), so a
//     frame has the bits sparch_fbank_padded_fwd gives it;
//   * audio_gather_augment_kernel is augment_kernel (augment.hip) with the clip found the same way (augment_clip.h);
//     it also writes the rows' lengths for the sparch_fbank_padded_fwd launch behind it.
// An index outside the store is an empty clip with label -1.  Plain vector loads and stores only.
#include <climits>

#include "common.h"
#include "augment_clip.h"
#include "fbank_frame.h"

namespace {

// Clip idx[row] of the store: its length (0 for an index outside [0, n_store)) and first sample; the label goes to
// y[row] from one thread of the workgroups for which `writes_y` holds.  One value per workgroup.
template <typename T>
__device__ __forceinline__ const T* store_clip(const T* __restrict__ samples, const long long* __restrict__ starts,
                                               const int* __restrict__ lengths, const long long* __restrict__ labels,
                                               long long n_store, const long long* __restrict__ idx, int row,
                                               bool writes_y, long long* __restrict__ y, int& n) {
    const long long i = idx[row];
    const bool inside = i >= 0 && i < n_store;
    n = inside ? max(lengths[i], 0) : 0;
    if (writes_y && y && threadIdx.x == 0) y[row] = inside ? labels[i] : -1;
    return samples + (inside ? starts[i] : 0);
}

template <typename T>
__global__ __launch_bounds__(256) void audio_gather_fbank_kernel(
    const T* __restrict__ samples, const long long* __restrict__ starts, const int* __restrict__ lengths,
    const long long* __restrict__ labels, long long n_store, const long long* __restrict__ idx, int n_frames,
    int n_mels, float* __restrict__ out, long long* __restrict__ y) {
    using namespace fbank_dev;
    __shared__ FbankLds s;
    const int tid = threadIdx.x;
    const int chunks = (n_frames + FPW - 1) / FPW;
    const int row = blockIdx.x / chunks, frame0 = (blockIdx.x % chunks) * FPW;
    const int frame_end = min(frame0 + FPW, n_frames);
    int n;
    const T* src = store_clip(samples, starts, lengths, labels, n_store, idx, row, frame0 == 0, y, n);
    // as in fbank_padded_kernel: the branch, with the barriers inside it, is taken by the whole workgroup or not at
    // all; a frame is computed only when all its samples lie inside the clip
    const int live_end = min(frames_of(n), frame_end);
    float* dst = out + (size_t)row * n_frames * n_mels;
    if (frame0 < live_end) {
        const MelEdges m = fbank_tables(s, n_mels);
        for (int frame = frame0; frame < live_end; ++frame)
            fbank_frame(s, m, n_mels, src + (size_t)frame * SHIFT, dst + (size_t)frame * n_mels);
    }
    const int zero0 = max(frame0, live_end);
    for (size_t i = (size_t)zero0 * n_mels + tid; i < (size_t)frame_end * n_mels; i += 256) dst[i] = 0.f;
}

template <typename T>
__global__ __launch_bounds__(augment_dev::NT) void audio_gather_augment_kernel(
    const T* __restrict__ samples, const long long* __restrict__ starts, const int* __restrict__ lengths,
    const long long* __restrict__ labels, long long n_store, const long long* __restrict__ idx, int ld,
    const float* __restrict__ params, float min_snr, float max_snr, uint64_t seed, int rate, int ring_floats,
    float* __restrict__ out, int* __restrict__ out_lengths, long long* __restrict__ y) {
    const int row = blockIdx.x;
    int n;
    const T* src = store_clip(samples, starts, lengths, labels, n_store, idx, row, true, y, n);
    n = min(n, ld);
    if (threadIdx.x == 0) out_lengths[row] = n;
    augment_dev::augment_clip(n, src, out + (size_t)row * ld, params + (size_t)row * SPARCH_AUGM_FIELDS, row, min_snr,
                              max_snr, seed, rate, ring_floats);
}

bool store_args_ok(const void* samples, int dtype, const long long* starts, const int* lengths,
                   const long long* labels, long long n_store, const long long* idx, int batch, const long long* y) {
    return samples && (dtype == 0 || dtype == 1) && starts && lengths && (labels || !y) && n_store > 0 && idx
           && batch > 0;
}

}  // namespace

extern "C" int sparch_audio_gather_fbank(const void* samples, int dtype, const long long* starts, const int* lengths,
                                         const long long* labels, long long n_store, const long long* idx, int batch,
                                         int n_frames_out, int n_mels, float* out, long long* y, void* stream) {
    SPARCH_ENTER();
    if (!store_args_ok(samples, dtype, starts, lengths, labels, n_store, idx, batch, y) || n_frames_out <= 0
        || n_mels <= 0 || n_mels > 256 || !out)
        return SPARCH_EINVAL;
    const int chunks = cdiv(n_frames_out, fbank_dev::FPW);
    if ((long long)batch * chunks > INT_MAX) return SPARCH_EINVAL;
    const dim3 grid((unsigned)(batch * chunks)), block(256);
    if (dtype == 0)
        hipLaunchKernelGGL(audio_gather_fbank_kernel<float>, grid, block, 0, (hipStream_t)stream,
                           static_cast<const float*>(samples), starts, lengths, labels, n_store, idx, n_frames_out,
                           n_mels, out, y);
    else
        hipLaunchKernelGGL(audio_gather_fbank_kernel<int16_t>, grid, block, 0, (hipStream_t)stream,
                           static_cast<const int16_t*>(samples), starts, lengths, labels, n_store, idx, n_frames_out,
                           n_mels, out, y);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_audio_gather_augment(const void* samples, int dtype, const long long* starts, const int* lengths,
                                           const long long* labels, long long n_store, const long long* idx,
                                           int batch, int ld, const float* params, float min_snr, float max_snr,
                                           unsigned long long noise_seed, int sample_rate, float* out,
                                           int* out_lengths, long long* y, void* stream) {
    SPARCH_ENTER();
    if (!store_args_ok(samples, dtype, starts, lengths, labels, n_store, idx, batch, y) || ld <= 0 || !params || !out
        || !out_lengths || sample_rate < 8000 || sample_rate > 48000)
        return SPARCH_EINVAL;
    using namespace augment_dev;
    const int ring_floats = rings_max(sample_rate);
    const size_t lds_bytes = (size_t)sparch_augment_lds_bytes(sample_rate);
    const size_t lds_max = (size_t)sparch_augment_lds_bytes(48000);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 0) {
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void*>(audio_gather_augment_kernel<float>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        if (attr != hipSuccess) { sparch_note_hip_error((int)attr); return SPARCH_ELAUNCH; }
        hipLaunchKernelGGL(audio_gather_augment_kernel<float>, dim3((unsigned)batch), dim3(NT), lds_bytes, st,
                           static_cast<const float*>(samples), starts, lengths, labels, n_store, idx, ld, params,
                           min_snr, max_snr, (uint64_t)noise_seed, sample_rate, ring_floats, out, out_lengths, y);
    } else {
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void*>(audio_gather_augment_kernel<int16_t>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        if (attr != hipSuccess) { sparch_note_hip_error((int)attr); return SPARCH_ELAUNCH; }
        hipLaunchKernelGGL(audio_gather_augment_kernel<int16_t>, dim3((unsigned)batch), dim3(NT), lds_bytes, st,
                           static_cast<const int16_t*>(samples), starts, lengths, labels, n_store, idx, ld, params,
                           min_snr, max_snr, (uint64_t)noise_seed, sample_rate, ring_floats, out, out_lengths, y);
    }
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

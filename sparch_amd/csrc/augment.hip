// f-3  Waveform augmentation of the HD / SC training clips, on the padded batch buffer of the collate function.
//
// Replaces the reference's per-clip ComposeMany([RandomApply(PolarityInversion, 0.8), RandomApply(Noise, p_noise),
// RandomApply(Gain, 0.3), RandomApply(Reverb(16000), 0.6)]) (nonspiking_datasets.py:71-78, 170-177, applied at :93,
// :191).  The arithmetic is third-party (torchaudio_augmentations 0.2.4 and sox 14.4's `reverb` effect, neither part
// of the reference's own code): what follows restates them ("augment"), PARITY UNPINNED against the
// real libraries; pinned bit for bit against the NumPy restatement in tests/augment_numpy.py (noise off).
//
// The host draws the per-clip decisions and values (dataloaders/augment.py: one row of SPARCH_AUGM_FIELDS floats per
// clip); the kernel applies them.  One 256-thread workgroup per clip:
//   * stages 1-3 are elementwise (polarity, + noise * noise_std, gain with its clamp), the noise drawn from a
//     Philox4x32-10 stream keyed by (seed, row, sample) (Box-Muller); noise_std needs the clip's unbiased standard
//     deviation first (two passes over the clip, in double, only for rows with noise);
//   * a row without reverb writes v and is done;
//   * reverb: two filter arrays (sox's stereo depth of 100 % makes two wet channels of the mono input), each eight
//     feedback combs in parallel then four all-passes in series, on x = clamp(v, -1, 1).  Every ring lives in LDS.
//     The only sequential recurrence is the comb's one-pole `store`: wave 0 runs it, one lane per (array, comb), over
//     a chunk of CH samples, and writes each comb's delayed output y into a chunk buffer.  One chunk behind it, wave 1
//     sums the combs, runs the all-passes and mixes, one lane per sample, in blocks no longer than the shortest
//     all-pass delay (inside a block every delayed read refers to an earlier block).  Waves 2-3 make x for the chunk
//     ahead of the combs.  One barrier per chunk.  Every operation is the restatement's, in its order, one fp32
//     rounding each (-ffp-contract=off), so the output is the restatement's bit for bit.
#include <climits>

#include "common.h"
#include "augment_clip.h"

namespace {

using namespace augment_dev;

template <typename T>
__global__ __launch_bounds__(NT) void augment_kernel(int ld, const int* __restrict__ lengths,
                                                     const T* __restrict__ wave, const float* __restrict__ params,
                                                     float min_snr, float max_snr, uint64_t seed, int rate,
                                                     int ring_floats, float* __restrict__ out) {
    const int row = blockIdx.x;
    // the same in all threads (one row of the table), as augment_clip asks
    const int n = min(max(lengths[row], 0), ld);
    augment_clip(n, wave + (size_t)row * ld, out + (size_t)row * ld, params + (size_t)row * SPARCH_AUGM_FIELDS, row,
                 min_snr, max_snr, seed, rate, ring_floats);
}

}  // namespace

extern "C" int sparch_augment_lds_bytes(int sample_rate) {
    SPARCH_ENTER();
    if (sample_rate < 8000 || sample_rate > 48000) return 0;
    return (rings_max(sample_rate) + Y_FLOATS + X_FLOATS) * (int)sizeof(float);
}

extern "C" int sparch_augment_padded(int n_clips, int ld, const int* lengths, int in_dtype, const void* wave,
                                     const float* params, float min_snr, float max_snr,
                                     unsigned long long noise_seed, int sample_rate, float* out, void* stream) {
    SPARCH_ENTER();
    if (n_clips < 0 || ld < 0 || (in_dtype != 0 && in_dtype != 1) || sample_rate < 8000 || sample_rate > 48000)
        return SPARCH_EINVAL;
    if (n_clips > 0 && (!lengths || !wave || !params || !out)) return SPARCH_EINVAL;
    if (n_clips == 0 || ld == 0) return SPARCH_OK;
    const int ring_floats = rings_max(sample_rate);
    const size_t lds_bytes = (size_t)sparch_augment_lds_bytes(sample_rate);
    const size_t lds_max = (size_t)sparch_augment_lds_bytes(48000);
    hipStream_t st = (hipStream_t)stream;
    if (in_dtype == 0) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(augment_kernel<float>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        if (attr != hipSuccess) { sparch_note_hip_error((int)attr); return SPARCH_ELAUNCH; }
        hipLaunchKernelGGL(augment_kernel<float>, dim3((unsigned)n_clips), dim3(NT), lds_bytes, st, ld, lengths,
                           static_cast<const float*>(wave), params, min_snr, max_snr, (uint64_t)noise_seed,
                           sample_rate, ring_floats, out);
    } else {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(augment_kernel<int16_t>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        if (attr != hipSuccess) { sparch_note_hip_error((int)attr); return SPARCH_ELAUNCH; }
        hipLaunchKernelGGL(augment_kernel<int16_t>, dim3((unsigned)n_clips), dim3(NT), lds_bytes, st, ld, lengths,
                           static_cast<const int16_t*>(wave), params, min_snr, max_snr, (uint64_t)noise_seed,
                           sample_rate, ring_floats, out);
    }
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

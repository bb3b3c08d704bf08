// G9: Kaldi-compatible log-mel filterbank front-end, fused into one kernel.
//
// Replaces `torchaudio.compliance.kaldi.fbank(x, num_mel_bins=40)` at
// nonspiking_datasets.py:96, 194.  The arithmetic lives in third-party torchaudio 0.12.0
// (requirements.txt:14), which is NOT in /root/reference and not installed: the algorithm
// below restates torchaudio's published defaults from memory —
//   16 kHz, 25 ms frames (400) every 10 ms (160), snip_edges (frames = 1 + (N-400)/160),
//   dither 0, per-frame DC removal, pre-emphasis 0.97 with replicated first sample,
//   povey window hann(400, periodic=False)^0.85, zero-pad to 512, |rFFT|^2,
//   triangular mel bins between 20 Hz and Nyquist on mel = 1127 ln(1 + f/700),
//   log(max(e, FLT_EPSILON)), no energy row, no mean subtraction.
// PARITY UNPINNED against torchaudio itself; pinned against an independent NumPy
// restatement and analytic known-answer signals in tests/.
//
// One 256-thread workgroup per FPW consecutive frames of a clip: the per-launch tables (FFT twiddles, povey
// window, mel value of every bin, first / last bin of every triangular filter) are built ONCE per workgroup
// in LDS; per frame: samples -> LDS, block mean, pre-emphasis + window, 512-point radix-2 FFT entirely in
// LDS (one butterfly per thread per stage), power spectrum, and the 40 triangular sums over each filter's
// own bin range only (ascending bin order: the same partial sums as a loop over all 256 bins, whose other
// terms are exact zeros).  (First version: one frame per workgroup, tables and window recomputed per frame —
// sincospif / powf / logf for every frame — and 40 threads x 256 bins for the mel stage: 0.45 ms for
// 256 x 16000 samples; this one: see DESIGN.md.)
//
// Two kernels share the tables and the per-frame code: fbank_kernel (sparch_fbank_fwd) for a batch of clips of one
// length, and fbank_padded_kernel (sparch_fbank_padded_fwd) for clips of different lengths packed into rows of one
// buffer, whose output is what pad_sequence makes of the per-clip features (the reference's HD / SC collate,
// nonspiking_datasets.py:104-111): each clip's frames, then exact zeros up to the longest clip's frame count.  A
// frame inside a clip has the same bits in both kernels; a workgroup whose frames are all padding only writes zeros.
#include <climits>

#include "common.h"
#include "fbank_frame.h"

namespace {

using namespace fbank_dev;

// Fixed length: every clip has n_samples samples and n_frames = frames_of(n_samples) frames.
__global__ __launch_bounds__(256) void fbank_kernel(int n_clips, int n_samples, int n_frames, int n_mels,
                                                    const float* __restrict__ wave, float* __restrict__ out) {
    __shared__ FbankLds s;
    const int chunks = (n_frames + FPW - 1) / FPW;
    const int clip = blockIdx.x / chunks, frame0 = (blockIdx.x % chunks) * FPW;
    const MelEdges m = fbank_tables(s, n_mels);
    for (int f = 0; f < FPW; ++f) {
        const int frame = frame0 + f;
        if (frame >= n_frames) break;  // uniform
        fbank_frame(s, m, n_mels, wave + (size_t)clip * n_samples + (size_t)frame * SHIFT,
                    out + ((size_t)clip * n_frames + frame) * n_mels);
    }
}

// Variable length, padded as pad_sequence pads per-clip features: clip i (row i of a (n_clips, ld) buffer) has
// frames_of(min(max(lengths[i], 0), ld)) frames; its frames from there up to n_frames are exact zeros.  A frame is
// computed only when all its samples lie inside the clip, so nothing past ld or past lengths[i] is read.
template <typename T>
__global__ __launch_bounds__(256) void fbank_padded_kernel(int ld, const int* __restrict__ lengths, int n_frames,
                                                           int n_mels, const T* __restrict__ wave,
                                                           float* __restrict__ out) {
    __shared__ FbankLds s;
    const int tid = threadIdx.x;
    const int chunks = (n_frames + FPW - 1) / FPW;
    const int clip = blockIdx.x / chunks, frame0 = (blockIdx.x % chunks) * FPW;
    const int frame_end = min(frame0 + FPW, n_frames);
    // one value per workgroup (every thread reads the same word): the branch below, with the barriers inside it,
    // is taken by all threads of the workgroup or by none
    const int live_end = min(frames_of(min(max(lengths[clip], 0), ld)), frame_end);
    float* dst = out + (size_t)clip * n_frames * n_mels;
    if (frame0 < live_end) {
        const MelEdges m = fbank_tables(s, n_mels);
        for (int frame = frame0; frame < live_end; ++frame)
            fbank_frame(s, m, n_mels, wave + (size_t)clip * ld + (size_t)frame * SHIFT, dst + (size_t)frame * n_mels);
    }
    const int zero0 = max(frame0, live_end);  // padding frames of this workgroup: zeros, no tables needed
    for (size_t i = (size_t)zero0 * n_mels + tid; i < (size_t)frame_end * n_mels; i += 256) dst[i] = 0.f;
}

}  // namespace

extern "C" int sparch_fbank_frames(int n_samples) {
    SPARCH_ENTER();
    return frames_of(n_samples);
}

extern "C" int sparch_fbank_fwd(int n_clips, int n_samples, int n_mels, const float* wave, float* out,
                                void* stream) {
    SPARCH_ENTER();
    const int n_frames = sparch_fbank_frames(n_samples);
    if (n_clips <= 0 || n_frames <= 0 || n_mels <= 0 || n_mels > 256 || !wave || !out) return SPARCH_EINVAL;
    const int chunks = (n_frames + FPW - 1) / FPW;
    hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)(n_clips * chunks)), dim3(256), 0, (hipStream_t)stream,
                       n_clips, n_samples, n_frames, n_mels, wave, out);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_fbank_padded_fwd(int n_clips, int ld, const int* lengths, int n_frames_out, int n_mels,
                                       int in_dtype, const void* wave, float* out, void* stream) {
    SPARCH_ENTER();
    if (n_clips <= 0 || ld <= 0 || n_frames_out <= 0 || n_mels <= 0 || n_mels > 256 || (in_dtype != 0 && in_dtype != 1)
        || !lengths || !wave || !out)
        return SPARCH_EINVAL;
    const int chunks = cdiv(n_frames_out, FPW);
    if ((long long)n_clips * chunks > INT_MAX) return SPARCH_EINVAL;
    const dim3 grid((unsigned)(n_clips * chunks)), block(256);
    if (in_dtype == 0)
        hipLaunchKernelGGL(fbank_padded_kernel<float>, grid, block, 0, (hipStream_t)stream, ld, lengths,
                           n_frames_out, n_mels, static_cast<const float*>(wave), out);
    else
        hipLaunchKernelGGL(fbank_padded_kernel<int16_t>, grid, block, 0, (hipStream_t)stream, ld, lengths,
                           n_frames_out, n_mels, static_cast<const int16_t*>(wave), out);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

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

namespace {

constexpr int FRAME = 400, SHIFT = 160, NFFT = 512, NBIN = NFFT / 2;  // 256 usable bins (+Nyquist, weight 0)
constexpr float SAMPLE_RATE = 16000.0f, LOW_HZ = 20.0f, PREEMPH = 0.97f;

__device__ __forceinline__ float mel_of(float hz) { return 1127.0f * logf(1.0f + hz / 700.0f); }

constexpr int FPW = 7;  // frames per workgroup (98 frames of a 1 s clip = 14 x 7)

__host__ __device__ constexpr int frames_of(int n_samples) {
    return n_samples < FRAME ? 0 : 1 + (n_samples - FRAME) / SHIFT;
}

// LDS of one workgroup: the per-launch tables and the frame being transformed.
struct FbankLds {
    float re[NFFT], im[NFFT];
    float tw_c[NBIN], tw_s[NBIN];
    float melpt[NBIN];
    float win[NFFT];
    int f_lo[256], f_hi[256];
    float part[4];
};

struct MelEdges { float left, center, right; };  // thread tid's triangular filter (tid < n_mels)

// Tables, once per workgroup: twiddles e^{-2 pi i k / 512}, mel value of every FFT bin centre, povey window, and per
// mel filter the bins with a non-zero weight.  Every thread of the workgroup calls it (two __syncthreads).
__device__ __forceinline__ MelEdges fbank_tables(FbankLds& s, int n_mels) {
    const int tid = threadIdx.x;
    {
        float sn, c;
        sincospif(-2.0f * (float)tid / (float)NFFT, &sn, &c);
        s.tw_c[tid] = c; s.tw_s[tid] = sn;
        s.melpt[tid] = mel_of((float)tid * (SAMPLE_RATE / (float)NFFT));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + 256 * j;
            const float hann = 0.5f - 0.5f * cospif(2.0f * (float)i / (float)(FRAME - 1));
            s.win[i] = i < FRAME ? powf(hann, 0.85f) : 0.f;
        }
    }
    __syncthreads();
    const float mel_lo = mel_of(LOW_HZ), mel_hi = mel_of(0.5f * SAMPLE_RATE);
    const float delta = (mel_hi - mel_lo) / (float)(n_mels + 1);
    MelEdges m;
    m.left = mel_lo + (float)tid * delta; m.center = m.left + delta; m.right = m.center + delta;
    if (tid < n_mels) {  // melpt is increasing: the bins strictly inside (left, right) form one range
        int lo = 0, hi = NBIN;  // lo = first bin with melpt > left (binary search, 8 steps)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (s.melpt[mid] > m.left) hi = mid; else lo = mid + 1; }
        int a = lo, b = NBIN;   // a = first bin with melpt >= right
        while (a < b) { const int mid = (a + b) >> 1; if (s.melpt[mid] < m.right) a = mid + 1; else b = mid; }
        s.f_lo[tid] = lo; s.f_hi[tid] = a;
    }
    __syncthreads();
    return m;
}

// Samples are fp32 in [-1, 1], or 16-bit PCM scaled by 2^-15 as they are loaded (exact: the same bits as the fp32
// path on pcm / 32768).
__device__ __forceinline__ float load_sample(const float* __restrict__ p, int i) { return p[i]; }
__device__ __forceinline__ float load_sample(const int16_t* __restrict__ p, int i) {
    return (float)p[i] * 0x1p-15f;
}

// One frame: src -> n_mels log-mel energies at dst.  src[0, FRAME) must be samples of the clip.  Every thread of the
// workgroup calls it (the frame is uniform); it ends with a barrier, so LDS is free for the next frame.
template <typename T>
__device__ __forceinline__ void fbank_frame(FbankLds& s, const MelEdges& m, int n_mels, const T* __restrict__ src,
                                            float* __restrict__ dst) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // frame -> registers (2 samples per thread), block mean
    float x0 = (tid < FRAME) ? load_sample(src, tid) : 0.f;
    float x1 = (tid + 256 < FRAME) ? load_sample(src, tid + 256) : 0.f;
    float sum = x0 + x1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) s.part[wv] = sum;
    __syncthreads();
    const float mean = ((s.part[0] + s.part[1]) + (s.part[2] + s.part[3])) / (float)FRAME;
    if (tid < FRAME) s.re[tid] = x0 - mean;
    if (tid + 256 < FRAME) s.re[tid + 256] = x1 - mean;
    __syncthreads();
    // pre-emphasis (x[i] - 0.97 x[i-1], first sample replicated) and povey window
    float y[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = tid + 256 * j;
        float v = 0.f;
        if (i < FRAME) {
            const float prev = s.re[i > 0 ? i - 1 : 0];
            v = (s.re[i] - PREEMPH * prev) * s.win[i];
        }
        y[j] = v;
    }
    __syncthreads();
    // bit-reversed scatter for the decimation-in-time FFT
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = tid + 256 * j;
        const int rev = (int)(__brev((unsigned)i) >> (32 - 9));
        s.re[rev] = y[j];
        s.im[rev] = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int stage = 0; stage < 9; ++stage) {
        const int half = 1 << stage;
        const int k = tid & (half - 1);
        const int i0 = ((tid >> stage) << (stage + 1)) + k, i1 = i0 + half;
        const int tw = k << (8 - stage);
        const float c = s.tw_c[tw], sn = s.tw_s[tw];
        const float ar = s.re[i0], ai = s.im[i0], br = s.re[i1], bi = s.im[i1];
        const float tr = br * c - bi * sn, ti = br * sn + bi * c;
        s.re[i0] = ar + tr; s.im[i0] = ai + ti;
        s.re[i1] = ar - tr; s.im[i1] = ai - ti;
        __syncthreads();
    }
    // power spectrum of bins 0..255 (the Nyquist bin carries zero mel weight)
    const float pw = s.re[tid] * s.re[tid] + s.im[tid] * s.im[tid];
    __syncthreads();
    s.re[tid] = pw;
    __syncthreads();
    if (tid < n_mels) {
        float e = 0.f;
        for (int i = s.f_lo[tid]; i < s.f_hi[tid]; ++i) {
            const float mp = s.melpt[i];
            const float up = (mp - m.left) / (m.center - m.left), down = (m.right - mp) / (m.right - m.center);
            const float wgt = fmaxf(0.f, fminf(up, down));
            e += wgt * s.re[i];
        }
        dst[tid] = logf(fmaxf(e, 1.1920928955078125e-07f));
    }
    __syncthreads();  // re / im / part are reused by the next frame
}

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

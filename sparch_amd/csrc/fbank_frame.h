// G9 (the mel front-end; labelled as fbank.hip, whose code this is): the per-frame device code of the log-mel
// front-end (see fbank.hip for the algorithm), shared by the kernels of
// fbank.hip (clips in rows of a batch buffer) and audio_store.hip (clips gathered from a device-resident split):
// one definition, so a frame has the same bits whichever kernel computes it.
#pragma once
#include "common.h"

namespace fbank_dev {

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

}  // namespace fbank_dev

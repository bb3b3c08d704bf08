// f-3: the per-clip device code of the waveform augmentation (see augment.hip for the algorithm), shared by
// augment_kernel (clips in rows of a batch buffer) and the gather kernel of audio_store.hip (clips of a
// device-resident split): one definition, so a clip is augmented to the same bits by either.
#pragma once
#include "common.h"

namespace augment_dev {

constexpr int NT = 256;          // threads: wave 0 combs, wave 1 all-passes and mix, waves 2-3 stage the input
constexpr int CH = 256;          // samples per chunk
constexpr int YS = CH + 1;       // stride of a comb's row in the chunk buffer (16 comb lanes write without conflict)
constexpr int NF = 12;           // filters per array: 8 combs, then 4 all-passes
constexpr int Y_FLOATS = 2 * 16 * YS, X_FLOATS = 3 * CH;
// sox reverb: a = -1 / ln(0.7), b = 100 / (ln(0.02) a + 1) (minimum / maximum feedback), in double
constexpr double FB_A = 0x1.66dec3df20aebp+1, FB_B = -0x1.4106b3fce35d8p+3;
constexpr float WET_GAIN = 0.015f;

// Filter lengths at 44.1 kHz (Freeverb's), m = 0..7 combs, 8..11 all-passes.
__host__ __device__ inline int base_len(int m) {
    return m == 0 ? 1116 : m == 1 ? 1188 : m == 2 ? 1277 : m == 3 ? 1356 : m == 4 ? 1422 : m == 5 ? 1491
         : m == 6 ? 1557 : m == 7 ? 1617 : m == 8 ? 225 : m == 9 ? 341 : m == 10 ? 441 : 556;
}

// Delay of filter m of array k: the stereo offset k * (-1)^m (12 samples at 44.1 kHz) alternates over all twelve
// filters; the combs scale with the room size, the all-passes do not.
__host__ __device__ inline int filter_size(int m, int k, double scale, double r) {
    const double len = (double)base_len(m) + 12.0 * (double)((m & 1) ? -k : k);
    return (int)floor((m < 8 ? scale * r * len : r * len) + 0.5);
}

// LDS floats of every ring of both arrays at room size 100 (the largest; sizes grow with it).
inline int rings_max(int rate) {
    const double r = (double)rate / 44100.0;
    int total = 0;
    for (int k = 0; k < 2; ++k)
        for (int m = 0; m < NF; ++m) total += filter_size(m, k, 1.0, r);
    return (total + 3) & ~3;
}

__device__ __forceinline__ float load_sample(const float* __restrict__ p, int i) { return p[i]; }
__device__ __forceinline__ float load_sample(const int16_t* __restrict__ p, int i) {
    return (float)p[i] * 0x1p-15f;
}

// Philox4x32-10 (Salmon et al., SC'11) of counter (t, row, 0, 0) under the 64-bit key; one standard normal from the
// first two words (Box-Muller, u1 in (0, 1] so the logarithm is finite).
__device__ __forceinline__ float normal_at(uint64_t seed, int row, int t) {
    uint32_t c0 = (uint32_t)t, c1 = (uint32_t)row, c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const float u1 = (float)((c0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(c1 >> 8) * 0x1p-24f;
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

// Stages 1-3 of one sample.  The gain's clamp belongs to that stage (torchaudio's Vol): without it v may leave [-1, 1].
struct Dry {
    bool pol, noise, gain;
    float nstd, ratio;
    uint64_t seed;
    int row;
    __device__ __forceinline__ float operator()(float s, int t) const {
        if (pol) s = -s;
        if (noise) s = s + normal_at(seed, row, t) * nstd;
        if (gain) s = clampf(s * ratio, -1.0f, 1.0f);
        return s;
    }
};

__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();  // red may still be read by a previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One clip: src[0, n) -> dst[0, n) under the table row prm (SPARCH_AUGM_FIELDS floats); `row` keys the noise stream.
// Every thread of the NT-thread workgroup calls it with the same arguments (they decide branches around barriers).
// Uses the workgroup's dynamic LDS (sparch_augment_lds_bytes) from its start.
template <typename T>
__device__ __forceinline__ void augment_clip(int n, const T* __restrict__ src, float* __restrict__ dst,
                                             const float* __restrict__ prm, int row, float min_snr, float max_snr,
                                             uint64_t seed, int rate, int ring_floats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[NT / 64];
    __shared__ int fsize[2 * NF], fbase[2 * NF];
    const int tid = threadIdx.x;
    Dry dry{prm[0] != 0.0f, prm[1] != 0.0f && n >= 2, prm[2] != 0.0f, 0.0f, prm[5], seed, row};

    if (dry.noise) {  // unbiased std of the clip (its polarity does not change it), then random.uniform(a, b) in fp32
        double s = 0.0;
        for (int t = tid; t < n; t += NT) s += (double)load_sample(src, t);
        const double mean = block_sum(s, red) / (double)n;
        double q = 0.0;
        for (int t = tid; t < n; t += NT) {
            const double d = (double)load_sample(src, t) - mean;
            q += d * d;
        }
        const float sd = (float)sqrt(block_sum(q, red) / (double)(n - 1));
        const float a = min_snr * sd, b = max_snr * sd;
        dry.nstd = a + (b - a) * prm[4];
    }
    if (prm[3] == 0.0f) {
        for (int t = tid; t < n; t += NT) dst[t] = dry(load_sample(src, t), t);
        return;
    }
    const int n_chunks = (n + CH - 1) / CH;
    if (n_chunks == 0) return;

    // ---- reverb (sox: reverberance R, HF damping D, room scale S in percent; wet gain 0 dB, no pre-delay)
    const float R = clampf(prm[6], 0.0f, 100.0f), D = clampf(prm[7], 0.0f, 100.0f), S = clampf(prm[8], 0.0f, 100.0f);
    const float fb = (float)(1.0 - exp(((double)R - FB_B) / (FB_A * FB_B)));
    const float damp = (float)((double)D / 100.0 * 0.3 + 0.2);
    if (tid < 2 * NF)
        fsize[tid] = filter_size(tid % NF, tid / NF, (double)S / 100.0 * 0.9 + 0.1, (double)rate / 44100.0);
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int f = 0; f < 2 * NF; ++f) { fbase[f] = b; b += fsize[f]; }
    }
    for (int i = tid; i < ring_floats; i += NT) lds[i] = 0.0f;  // every ring and store starts at 0
    float* ybuf = lds + ring_floats;                            // [2 chunks][16 combs][YS]
    float* xbuf = ybuf + Y_FLOATS;                              // [3 chunks][CH]: x = clamp(v, -1, 1), 0 past n
    for (int i = tid; i < CH; i += NT) xbuf[i] = i < n ? clampf(dry(load_sample(src, i), i), -1.0f, 1.0f) : 0.0f;
    __syncthreads();

    const int wave_id = tid >> 6, lane = tid & 63;
    if (wave_id == 0) {
        // comb j of array k (lanes 0-15): y = ring[t - N]; store = y + (store - y) damp; ring[t] = x + store fb.
        // (The barriers stay outside the lane branch: a barrier is taken by the whole wave.)
        const int f = (lane >> 3) * NF + (lane & 7), N = lane < 16 ? fsize[f] : 0;
        float* ring = lds + (lane < 16 ? fbase[f] : 0);
        float store = 0.0f;
        int p = 0;  // slot of t (and of t - N: the ring holds exactly the last N values)
        for (int c = 0; c < n_chunks; ++c) {
            if (lane < 16) {
                const float* xc = xbuf + (c % 3) * CH;
                float* yrow = ybuf + (c & 1) * 16 * YS + lane * YS;
                for (int i = 0; i < CH; i += 8) {
                    float y[8];
                    int q[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {  // N >= 20: the eight slots are distinct
                        q[u] = p + u >= N ? p + u - N : p + u;
                        y[u] = ring[q[u]];
                    }
                    const f32x4 xa = *reinterpret_cast<const f32x4*>(xc + i);
                    const f32x4 xb = *reinterpret_cast<const f32x4*>(xc + i + 4);
                    const float xv[8] = {xa[0], xa[1], xa[2], xa[3], xb[0], xb[1], xb[2], xb[3]};
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        store = y[u] + (store - y[u]) * damp;
                        ring[q[u]] = xv[u] + store * fb;
                        yrow[i + u] = y[u];
                    }
                    p = p + 8 >= N ? p + 8 - N : p + 8;
                }
            }
            __syncthreads();
        }
        __syncthreads();  // the all-pass wave's last chunk
    } else if (wave_id == 1) {
        // all-pass j of array k: y = ring[t - M]; ring[t] = out + y / 2; out = y - out
        int M[8], base[8], pos[8];  // filter 8 + j of array k at index 4k + j; pos: slot of the block's first sample
        int blk = 64;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int f = (a >> 2) * NF + 8 + (a & 3);
            M[a] = fsize[f]; base[a] = fbase[f]; pos[a] = 0;
            blk = min(blk, M[a]);  // >= 41 at 8 kHz
        }
        __syncthreads();  // chunk 0's combs
        for (int c = 0; c < n_chunks; ++c) {
            const float* xc = xbuf + (c % 3) * CH;
            const float* yc = ybuf + (c & 1) * 16 * YS;
            for (int b0 = 0; b0 < CH; b0 += blk) {
                const int len = min(blk, CH - b0), i = b0 + lane;
                if (lane < len) {
                    float wet[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        float o = 0.0f;
#pragma unroll
                        for (int j = 7; j >= 0; --j) o = o + yc[(k * 8 + j) * YS + i];
#pragma unroll
                        for (int j = 3; j >= 0; --j) {
                            const int a = 4 * k + j;
                            const int s = pos[a] + lane >= M[a] ? pos[a] + lane - M[a] : pos[a] + lane;
                            float* slot = lds + base[a] + s;
                            const float y = *slot;
                            *slot = o + y * 0.5f;
                            o = y - o;
                        }
                        wet[k] = o * WET_GAIN;
                    }
                    const float x = xc[i];
                    const int t = c * CH + i;
                    if (t < n) dst[t] = 0.5f * (clampf(x + wet[0], -1.0f, 1.0f) + clampf(x + wet[1], -1.0f, 1.0f));
                }
#pragma unroll
                for (int a = 0; a < 8; ++a) pos[a] = pos[a] + len >= M[a] ? pos[a] + len - M[a] : pos[a] + len;
            }
            __syncthreads();
        }
    } else {
        for (int c = 0; c < n_chunks; ++c) {  // x of chunk c + 1 while the combs run chunk c
            if (c + 1 < n_chunks) {
                float* xn = xbuf + ((c + 1) % 3) * CH;
                for (int i = tid - 128; i < CH; i += 128) {
                    const int t = (c + 1) * CH + i;
                    xn[i] = t < n ? clampf(dry(load_sample(src, t), t), -1.0f, 1.0f) : 0.0f;
                }
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

}  // namespace augment_dev

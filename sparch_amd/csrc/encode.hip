// Spike encoders (include/sparch_hip.h, "Spike encoders"): real-valued features (B,T,K) -> spike
// counts, as the bf16 plane the first layer's GEMMs read, as bytes and / or as fp32 — the output trio of
// sparch_events_gather_bin.  Three codes behind one entry point:
//   RATE  : one Bernoulli draw per element from the dropout hash of common.h; stateless, one flat pass.
//   IF    : a non-leaky integrator per (b, k) that emits floor(v) and keeps the fraction; a scan over time.
//   DELTA : send-on-delta against a reference per (b, k), ON / OFF columns; a scan over time.
// Everything is plain fp32 with one rounding per operation (the library is built with -ffp-contract=off), so the tests
// restate it in numpy bit for bit.
#include "common.h"

namespace {

constexpr int ENC_NT = 256;
constexpr int ENC_D = SPARCH_ENCODE_PREFETCH;   // steps of x in flight per thread of a scan kernel

struct EncArgs {
    int B, T, K, KW, ldp;        // KW = K' (the output width)
    const float *x, *lo, *scale;
    float* state;
    int fresh;
    long long t0;
    uint64_t seed;
    const int* lengths;
    uint16_t* plane;
    uint8_t* counts;
    float* dense;
    uint32_t* totals;
};

// the 24-bit uniform of keep_scale (common.h) itself: the same hash of (seed, idx), the same conversion
__device__ __forceinline__ float enc_uniform(uint64_t seed, uint64_t idx) {
    const uint32_t a = mix32((uint32_t)idx ^ (uint32_t)seed);
    const uint32_t b = mix32(a + (uint32_t)(idx >> 32) * 0x9E3779B9U + (uint32_t)(seed >> 32));
    return (float)(b >> 8) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float enc_z(float x, float lo, float scale) { return __fmul_rn(__fsub_rn(x, lo), scale); }
__device__ __forceinline__ bool enc_finite(float z) { return fabsf(z) <= 3.402823466e38f; }   // false for a NaN
__device__ __forceinline__ uint16_t enc_bf16(unsigned n) { return (uint16_t)(__float_as_uint((float)n) >> 16); }  // n <= 255: exact

// ---- RATE: thread (r, g) owns the 8 plane columns [8g, 8g + 8) of the rows r, r + R, r + 2R, ... — consecutive
// threads take consecutive 16-byte pieces of a plane row, then the next row; a thread keeps its columns, so the
// totals are eight registers, added up per workgroup in LDS (a workgroup of a narrow input holds each column group
// many times) and then once per column and workgroup in memory.
__global__ __launch_bounds__(ENC_NT) void encode_rate_kernel(EncArgs a, int G, long long R) {
    __shared__ unsigned tot[ENC_NT * 8];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * ENC_NT + tid;
    const long long M = (long long)a.B * a.T;
    const bool active = i < R * G;
    const int g = (int)(i % G);
    const int c0 = g * 8;
    unsigned cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
        float lo[8], sc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = c0 + j < a.K;
            lo[j] = in ? a.lo[c0 + j] : 0.0f;
            sc[j] = in ? a.scale[c0 + j] : 0.0f;
        }
        const bool wide = (a.K % 4) == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15u) == 0 && c0 + 8 <= a.K;
        for (long long m = i / G; m < M; m += R) {
            const int b = (int)(m / a.T), t = (int)(m - (long long)b * a.T);
            const bool valid = !a.lengths || t < a.lengths[b];
            float xv[8];
            if (wide) {   // K % 4 == 0 and x 16-byte aligned: the row piece is two aligned quads
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(a.x + m * a.K + c0);
                const f32x4 q1 = *reinterpret_cast<const f32x4*>(a.x + m * a.K + c0 + 4);
                xv[0] = q0.x; xv[1] = q0.y; xv[2] = q0.z; xv[3] = q0.w;
                xv[4] = q1.x; xv[5] = q1.y; xv[6] = q1.z; xv[7] = q1.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[j] = c0 + j < a.K ? a.x[m * a.K + c0 + j] : 0.0f;   // all loads before the first use
            }
            const uint64_t base = ((uint64_t)(a.t0 + t) * (uint64_t)a.B + (uint64_t)b) * (uint64_t)a.K + (uint64_t)c0;
            unsigned n[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float z = enc_z(xv[j], lo[j], sc[j]);
                const float p = z > 0.0f ? (z < 1.0f ? z : 1.0f) : 0.0f;      // a NaN: 0
                n[j] = (valid && c0 + j < a.K && enc_uniform(a.seed, base + j) < p) ? 1u : 0u;
                cnt[j] += n[j];
            }
            if (a.plane) {
                const uint4 v = make_uint4(enc_bf16(n[0]) | (unsigned)enc_bf16(n[1]) << 16, enc_bf16(n[2]) | (unsigned)enc_bf16(n[3]) << 16,
                                           enc_bf16(n[4]) | (unsigned)enc_bf16(n[5]) << 16, enc_bf16(n[6]) | (unsigned)enc_bf16(n[7]) << 16);
                *reinterpret_cast<uint4*>(a.plane + m * a.ldp + c0) = v;      // c0 + 8 <= ldp: the pad columns too
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (c0 + j >= a.K) continue;
                if (a.counts) a.counts[m * a.K + c0 + j] = (uint8_t)n[j];
                if (a.dense) a.dense[m * a.K + c0 + j] = (float)n[j];
            }
        }
    }
    if (!a.totals) return;   // (uniform)
    // slot of a thread: its column group where the workgroup holds every group (G < ENC_NT), else its own
    const bool shared = G < ENC_NT;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot[tid * 8 + j] = 0;
    __syncthreads();
    if (active) {
        const int slot = shared ? g : tid;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (cnt[j]) atomicAdd(&tot[slot * 8 + j], cnt[j]);   // LDS
    }
    __syncthreads();
    if (shared) {
        // tot[c] is column c: consecutive lanes add to consecutive words, one atomic instruction per 64 columns.  (The
        // adds of all workgroups meet on the same few cache lines: with a lane per column group and eight adds 32
        // bytes apart the call took 60 us instead of 11 at (256, 98, 40) and 158 instead of 84 at (256, 250, 700).)
        for (int c = tid; c < a.K; c += ENC_NT)
            if (tot[c]) atomicAdd(a.totals + c, tot[c]);
    } else if (active) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned v = tot[tid * 8 + j];
            if (v && c0 + j < a.K) atomicAdd(a.totals + c0 + j, v);
        }
    }
}

// ---- IF / DELTA: thread (b, j).  j < K is feature k = j: a register ring of the next ENC_D steps of x (the loads do
// not depend on the carried state; one load is issued per step, ENC_D steps ahead, clamped into range at the end, as in
// the LIF scan of cell.hip), the state in a register from the first step to the last.  j >= K writes the zeros of plane
// column K' + (j - K) — the columns behind K' that the GEMMs read as part of the row.  Which outputs exist is a template
// parameter: no branch around a store inside the loop.  At most 1 + 6 vector-memory operations per step (DELTA with
// all outputs): 8 steps stay inside the 6-bit vmcnt.
template <int CODE, bool PLANE, bool COUNTS, bool DENSE>
__global__ __launch_bounds__(ENC_NT) void encode_scan_kernel(EncArgs a) {
    constexpr int D = ENC_D;
    const int npad = PLANE ? a.ldp - a.KW : 0;
    const int NTB = a.K + npad;                       // threads per batch row
    const long long idx = (long long)blockIdx.x * ENC_NT + threadIdx.x;
    if (idx >= (long long)a.B * NTB) return;
    const int b = (int)(idx / NTB), j = (int)(idx - (long long)b * NTB);
    const int T = a.T, K = a.K, KW = a.KW;
    const size_t row0 = (size_t)b * T;
    if (j >= K) {
        if constexpr (PLANE) {
            uint16_t* p = a.plane + row0 * a.ldp + KW + (j - K);
            for (int t = 0; t < T; ++t) p[(size_t)t * a.ldp] = 0;
        }
        return;
    }
    const int k = j;
    const float lo = a.lo[k], sc = a.scale[k];
    const int len = a.lengths ? a.lengths[b] : T;
    float st = a.fresh ? 0.0f : a.state[(size_t)b * K + k];
    unsigned tot_on = 0, tot_off = 0;
    const bool fresh = a.fresh != 0;

    const float* xcol = a.x + row0 * K + k;
    auto fetch = [&](float& x, int t) __attribute__((always_inline)) {
        const int tc = min(t, T - 1);   // past the end: a step that is in range and never used
        x = xcol[(size_t)tc * K];
    };
    auto step = [&](int t, float x) __attribute__((always_inline)) {
        const float z = enc_z(x, lo, sc);
        const bool valid = t < len;
        unsigned on = 0, off = 0;
        if constexpr (CODE == SPARCH_ENCODE_IF) {
            const float drive = z > 0.0f ? (z < 255.0f ? z : 255.0f) : 0.0f;
            const float v = __fadd_rn(st, drive);
            const float n = floorf(v);
            on = valid ? (unsigned)n : 0u;
            st = valid ? __fsub_rn(v, n) : st;
        } else {
            const bool fin = enc_finite(z);
            const bool first = fresh && t == 0;
            const float e = __fsub_rn(z, st);
            const float mag = fabsf(e);
            const float n = (fin && e == e) ? (mag < 255.0f ? floorf(mag) : 255.0f) : 0.0f;   // an inf difference: 255
            const float moved = __fadd_rn(st, copysignf(n, e));
            const float next = first ? (fin ? z : 0.0f) : (fin ? moved : st);
            const unsigned ni = (valid && !first) ? (unsigned)n : 0u;
            on = e > 0.0f ? ni : 0u;
            off = e < 0.0f ? ni : 0u;
            st = valid ? next : st;
        }
        tot_on += on;
        tot_off += off;
        const size_t m = row0 + t;
        if constexpr (PLANE) {
            a.plane[m * a.ldp + k] = enc_bf16(on);
            if constexpr (CODE == SPARCH_ENCODE_DELTA) a.plane[m * a.ldp + K + k] = enc_bf16(off);
        }
        if constexpr (COUNTS) {
            a.counts[m * KW + k] = (uint8_t)on;
            if constexpr (CODE == SPARCH_ENCODE_DELTA) a.counts[m * KW + K + k] = (uint8_t)off;
        }
        if constexpr (DENSE) {
            a.dense[m * KW + k] = (float)on;
            if constexpr (CODE == SPARCH_ENCODE_DELTA) a.dense[m * KW + K + k] = (float)off;
        }
    };

    float ring[D];
#pragma unroll
    for (int q = 0; q < D; ++q) fetch(ring[q], q);
    int t0 = 0;
    for (; t0 + D <= T; t0 += D) {
#pragma unroll
        for (int q = 0; q < D; ++q) {
            step(t0 + q, ring[q]);          // consume, then refill the slot (cell.hip: the ring keeps its registers)
            fetch(ring[q], t0 + q + D);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int q = 0; q < D; ++q) {
        if (t0 + q >= T) break;
        step(t0 + q, ring[q]);
    }
    a.state[(size_t)b * K + k] = st;
    if (a.totals) {
        if (tot_on) atomicAdd(a.totals + k, tot_on);
        if (CODE == SPARCH_ENCODE_DELTA && tot_off) atomicAdd(a.totals + K + k, tot_off);
    }
}

template <int CODE, bool PLANE, bool COUNTS, bool DENSE>
int scan_launch(const EncArgs& a, hipStream_t st) {
    const long long n = (long long)a.B * (a.K + (PLANE ? a.ldp - a.KW : 0));
    hipLaunchKernelGGL((encode_scan_kernel<CODE, PLANE, COUNTS, DENSE>), dim3((unsigned)((n + ENC_NT - 1) / ENC_NT)),
                       dim3(ENC_NT), 0, st, a);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}
template <int CODE>
int scan_dispatch(const EncArgs& a, hipStream_t st) {
    const int which = (a.plane ? 4 : 0) | (a.counts ? 2 : 0) | (a.dense ? 1 : 0);
    switch (which) {
        case 1: return scan_launch<CODE, false, false, true>(a, st);
        case 2: return scan_launch<CODE, false, true, false>(a, st);
        case 3: return scan_launch<CODE, false, true, true>(a, st);
        case 4: return scan_launch<CODE, true, false, false>(a, st);
        case 5: return scan_launch<CODE, true, false, true>(a, st);
        case 6: return scan_launch<CODE, true, true, false>(a, st);
        default: return scan_launch<CODE, true, true, true>(a, st);
    }
}

}  // namespace

extern "C" int sparch_spike_encode_width(int code, int K) {
    if (K < 1) return 0;
    if (code == SPARCH_ENCODE_RATE || code == SPARCH_ENCODE_IF) return K;
    if (code == SPARCH_ENCODE_DELTA) return K <= 0x3fffffff ? 2 * K : 0;
    return 0;
}

extern "C" int sparch_spike_encode(int code, int B, int T, int K, const float* x, const float* lo, const float* scale,
                                   float* state, int fresh, long long t0, uint64_t seed, const int* lengths,
                                   uint16_t* plane, int ldp, uint8_t* counts, float* dense, uint32_t* totals,
                                   void* stream) {
    SPARCH_ENTER();
    if (code != SPARCH_ENCODE_RATE && code != SPARCH_ENCODE_IF && code != SPARCH_ENCODE_DELTA) return SPARCH_EINVAL;
    if (B < 1 || T < 1 || K < 1 || !x || !lo || !scale || (!plane && !counts && !dense) || t0 < 0) return SPARCH_EINVAL;
    if (code != SPARCH_ENCODE_RATE && !state) return SPARCH_EINVAL;
    const long long kw = code == SPARCH_ENCODE_DELTA ? 2LL * K : (long long)K;
    if (kw > 65535 || ldp < kw || (ldp % 8) != 0) return SPARCH_EINVAL;
    if (plane && !aligned16(plane)) return SPARCH_EALIGN;
    const EncArgs a{B, T, K, (int)kw, ldp, x, lo, scale, state, fresh, t0, seed, lengths, plane, counts, dense, totals};
    hipStream_t st = (hipStream_t)stream;
    if (code == SPARCH_ENCODE_IF) return scan_dispatch<SPARCH_ENCODE_IF>(a, st);
    if (code == SPARCH_ENCODE_DELTA) return scan_dispatch<SPARCH_ENCODE_DELTA>(a, st);
    // RATE: G column groups per row (the plane's, or the data's without a plane), R row lanes — about 2^18 threads
    // (measured at (256, 250, 700): 2^16 134 us, 2^17 84 us, 2^18 65 us, 2^19 73 us)
    const int G = plane ? ldp / 8 : (K + 7) / 8;
    const long long M = (long long)B * T;
    long long R = (1 << 18) / G;
    R = R < 1 ? 1 : (R > M ? M : R);
    const long long n = R * G;
    hipLaunchKernelGGL(encode_rate_kernel, dim3((unsigned)((n + ENC_NT - 1) / ENC_NT)), dim3(ENC_NT), 0, st, a, G, R);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

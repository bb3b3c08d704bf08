// Synaptic currents: a learnable exponential synapse in front of a spiking cell ("Synaptic
// currents").
//
// gamma (H,) fp32 is the parameter; every kernel clamps it itself, g_h = clamp(gamma_h, lo, hi) with 0 <= lo <= hi < 1,
// and takes oma_h = 1.0f - g_h once per column.  z is the cell's input as the cell forms it (neuron_input of neuron.h on
// Wx, bias, scale, shift), len_b the row's own length (T without lengths), i[b,-1,h] = i0[b,h] (0 without i0):
//     i[b,t,h]   = g_h * i[b,t-1,h] + oma_h * z[b,t,h]            0 <= t < len_b          (sparch_synapse_fwd)
//     a[b,t,h]   = g_i[b,t,h] + g_h * a[b,t+1,h],  a[b,len_b,h] = 0                       (sparch_synapse_bwd)
//     g_z[b,t,h] = oma_h * a[b,t,h]
//     g_gamma[h] = gate_h * ( sum_b sum_{t < len_b} a[b,t,h] * (i[b,t-1,h] - i[b,t,h]) ) / oma_h
//     gate_h     = 1 if lo <= gamma_h <= hi else 0  (torch.clamp's backward)
// Two products and one add per step, never fused (-ffp-contract=off): one expression tree, one set of bits
// (tests/synapse_numpy.py restates it in fp32).  i[t-1] - z[t] = (i[t-1] - i[t]) / oma, so backward reads the saved i
// only.
// Both directions are a scan over time that is linear in the state: a lane owns SYN_VEC consecutive columns of one
// sequence (single columns where H, a row stride or a base address does not allow 16-byte pieces) and walks its steps
// with the loads of the next SYN_D steps in flight — they do not depend on the state (the register ring of the LIF scan
// in cell.hip and of encode.hip).
// g_gamma: every lane writes the sum over its sequence's steps to a workspace slab (B, H); a second launch adds the B
// slabs in a fixed order — no atomics, the same bits on every run.
// Under BatchNorm the backward scan also adds the normalisation's column sums of g_z (SynBwdArgs::bn_x), which the cell's
// backward kernel adds for a layer without a synapse.
// Layouts as in delay.hip: dense (B,T,H) with a row stride; lengths (B,): steps t >= len_b are written as zeros and do
// not advance the state; offsets non-NULL: the packed layout of a PackPlan — sequence j owns rows [offsets[j],
// offsets[j] + lengths[j]), rows t >= lengths[j] do not exist and are not written.
#include <type_traits>

#include "neuron.h"

namespace {

constexpr int SYN_NT = 64;  // lanes per workgroup: B H / 4 lanes are few (one wave per SIMD at 256 x 1024), so they spread
constexpr int SYN_D = 8;    // steps in flight

template <int N> struct SyVec { float v[N]; };
template <> struct alignas(16) SyVec<4> { float v[4]; };

struct SynFwdArgs {
    int B, T, H;
    const float* Wx; long long ldwx;
    const float* bias; const float* scale; const float* shift;
    const float* gamma; float lo, hi;
    const float* i0; float* i_out; long long ldi; float* i_T;
    const int* lengths; const int* offsets;
};

template <int N>
__global__ __launch_bounds__(SYN_NT) void synapse_fwd_kernel(SynFwdArgs a) {
    constexpr int D = SYN_D;
    const int groups = a.H / N;
    const long long idx = (long long)blockIdx.x * SYN_NT + threadIdx.x;
    if (idx >= (long long)a.B * groups) return;
    const int j = (int)(idx / groups), col = (int)(idx - (long long)j * groups) * N;
    const int len = a.lengths ? min(max(a.lengths[j], 0), a.T) : a.T;
    const long long base = a.offsets ? (long long)a.offsets[j] : (long long)j * a.T;
    const int tend = a.offsets ? len : a.T;  // rows of this sequence that exist
    const bool has_bias = a.bias != nullptr, has_scale = a.scale != nullptr;
    float g[N], oma[N], bi[N], sc[N], sh[N], st[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        g[e] = clampf(a.gamma[col + e], a.lo, a.hi);
        oma[e] = 1.0f - g[e];
        bi[e] = has_bias ? a.bias[col + e] : 0.0f;
        sc[e] = has_scale ? a.scale[col + e] : 1.0f;
        sh[e] = (has_scale && a.shift) ? a.shift[col + e] : 0.0f;
        st[e] = a.i0 ? a.i0[(size_t)j * a.H + col + e] : 0.0f;
    }
    if (tend > 0) {
        const float* src = a.Wx + base * a.ldwx + col;
        float* dst = a.i_out + base * a.ldi + col;
        auto fetch = [&](SyVec<N>& x, int t) __attribute__((always_inline)) {
            const int tc = min(t, tend - 1);  // past the end: a row that exists and is never used
            x = *reinterpret_cast<const SyVec<N>*>(src + (long long)tc * a.ldwx);
        };
        auto step = [&](int t, const SyVec<N>& x) __attribute__((always_inline)) {
            const bool valid = t < len;
            SyVec<N> out;
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const float z = neuron_input(x.v[e], has_bias, bi[e], has_scale, sc[e], sh[e]);
                const float n = g[e] * st[e] + oma[e] * z;
                st[e] = valid ? n : st[e];
                out.v[e] = valid ? n : 0.0f;
            }
            *reinterpret_cast<SyVec<N>*>(dst + (long long)t * a.ldi) = out;
        };
        SyVec<N> ring[D];
#pragma unroll
        for (int q = 0; q < D; ++q) fetch(ring[q], q);
        int t0 = 0;
        for (; t0 + D <= tend; t0 += D) {
#pragma unroll
            for (int q = 0; q < D; ++q) {
                step(t0 + q, ring[q]);  // consume, then refill the slot: the ring keeps its registers
                fetch(ring[q], t0 + q + D);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int q = 0; q < D; ++q) {
            if (t0 + q >= tend) break;
            step(t0 + q, ring[q]);
        }
    }
    if (a.i_T) {
#pragma unroll
        for (int e = 0; e < N; ++e) a.i_T[(size_t)j * a.H + col + e] = st[e];
    }
}

struct SynBwdArgs {
    int B, T, H;
    const float* g_i; long long ldg;
    const float* i; long long ldi;
    const float* i0;
    const float* gamma; float lo, hi;
    float* g_z; long long ldgz;
    float* ws;  // (B, H): every sequence's sum for g_gamma, or NULL
    const int* lengths; const int* offsets;
    // BatchNorm backward's column sums of the layer's projection x (bn_x, rows ldbn apart), folded in as the cell's
    // backward kernel folds them in where there is no synapse: per sequence sum_t g_z and sum_t g_z * xhat with
    // xhat = (x - mean) * invstd, into bn_ws (2, B, H); or NULL
    const float* bn_x; long long ldbn; const float* bn_mean; const float* bn_invstd; float* bn_ws;
};

// GG: the sum for g_gamma is wanted (the saved i is read only then).  BNS: BatchNorm's sums are wanted (bn_x is read
// only then); they are added in the cell backward kernel's order — per sequence, from the last step to the first,
// acc_dy += g_z; acc_dyx += g_z * ((x - mean) * invstd) — so that at gamma = 0, where g_z is the cell's dWx, they are the
// sums that kernel makes.  Time runs backwards from the row's last valid step; the term of step t + 1,
// a[t+1] (i[t] - i[t+1]), is added at step t, where i[t] arrives, and the term of step 0 after the loop, with i0.
template <int N, bool GG, bool BNS>
__global__ __launch_bounds__(SYN_NT) void synapse_bwd_kernel(SynBwdArgs a) {
    constexpr int D = (N == 4 && GG && BNS) ? 6 : SYN_D;  // three rings of four columns: 8 steps would not fit the registers
    const int groups = a.H / N;
    const long long idx = (long long)blockIdx.x * SYN_NT + threadIdx.x;
    if (idx >= (long long)a.B * groups) return;
    const int j = (int)(idx / groups), col = (int)(idx - (long long)j * groups) * N;
    const int len = a.lengths ? min(max(a.lengths[j], 0), a.T) : a.T;
    const long long base = a.offsets ? (long long)a.offsets[j] : (long long)j * a.T;
    float g[N], oma[N], adj[N], a_up[N], i_up[N], acc[N], mu[N], is[N], acc_dy[N], acc_dyx[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        g[e] = clampf(a.gamma[col + e], a.lo, a.hi);
        oma[e] = 1.0f - g[e];
        adj[e] = a_up[e] = i_up[e] = acc[e] = acc_dy[e] = acc_dyx[e] = 0.0f;
        mu[e] = BNS ? a.bn_mean[col + e] : 0.0f;
        is[e] = BNS ? a.bn_invstd[col + e] : 0.0f;
    }
    if (a.g_z && !a.offsets) {  // the padded steps of the masked layout: exact zeros
        SyVec<N> zero;
#pragma unroll
        for (int e = 0; e < N; ++e) zero.v[e] = 0.0f;
        for (int t = len; t < a.T; ++t) *reinterpret_cast<SyVec<N>*>(a.g_z + (base + t) * a.ldgz + col) = zero;
    }
    if (len > 0) {
        const float* gsrc = a.g_i + base * a.ldg + col;
        const float* isrc = GG ? a.i + base * a.ldi + col : nullptr;
        const float* xsrc = BNS ? a.bn_x + base * a.ldbn + col : nullptr;
        auto fetch = [&](SyVec<N>& gv, SyVec<N>& iv, SyVec<N>& xv, int k) __attribute__((always_inline)) {
            const int t = max(len - 1 - k, 0);  // before the start: a row that exists and is never used
            gv = *reinterpret_cast<const SyVec<N>*>(gsrc + (long long)t * a.ldg);
            if (GG) iv = *reinterpret_cast<const SyVec<N>*>(isrc + (long long)t * a.ldi);
            if (BNS) xv = *reinterpret_cast<const SyVec<N>*>(xsrc + (long long)t * a.ldbn);
        };
        auto step = [&](int k, const SyVec<N>& gv, const SyVec<N>& iv, const SyVec<N>& xv) __attribute__((always_inline)) {
            const int t = len - 1 - k;
            SyVec<N> out;
#pragma unroll
            for (int e = 0; e < N; ++e) {
                adj[e] = gv.v[e] + g[e] * adj[e];
                out.v[e] = oma[e] * adj[e];
                if (BNS) {
                    acc_dy[e] += out.v[e];
                    acc_dyx[e] += out.v[e] * ((xv.v[e] - mu[e]) * is[e]);
                }
                if (GG) {
                    acc[e] += a_up[e] * (iv.v[e] - i_up[e]);  // (0 at k = 0: a_up is 0)
                    a_up[e] = adj[e];
                    i_up[e] = iv.v[e];
                }
            }
            if (a.g_z) *reinterpret_cast<SyVec<N>*>(a.g_z + (base + t) * a.ldgz + col) = out;
        };
        SyVec<N> rg[D], ri[GG ? D : 1], rx[BNS ? D : 1];
#pragma unroll
        for (int q = 0; q < D; ++q) fetch(rg[q], ri[GG ? q : 0], rx[BNS ? q : 0], q);
        int k0 = 0;
        for (; k0 + D <= len; k0 += D) {
#pragma unroll
            for (int q = 0; q < D; ++q) {
                step(k0 + q, rg[q], ri[GG ? q : 0], rx[BNS ? q : 0]);
                fetch(rg[q], ri[GG ? q : 0], rx[BNS ? q : 0], k0 + q + D);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int q = 0; q < D; ++q) {
            if (k0 + q >= len) break;
            step(k0 + q, rg[q], ri[GG ? q : 0], rx[BNS ? q : 0]);
        }
    }
    if (GG) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float first = a.i0 ? a.i0[(size_t)j * a.H + col + e] : 0.0f;
            a.ws[(size_t)j * a.H + col + e] = acc[e] + a_up[e] * (first - i_up[e]);
        }
    }
    if (BNS) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            a.bn_ws[(size_t)j * a.H + col + e] = acc_dy[e];
            a.bn_ws[((size_t)a.B + j) * a.H + col + e] = acc_dyx[e];
        }
    }
}

// g_gamma[h] = gate_h * (slab 0 + slab 1 + ...) / oma_h: thread (c, r) of SYN_FC x SYN_FR adds slabs r, r + SYN_FR, ...
// for column c, the SYN_FR sums are added in the order r = 0, 1, ....  16 columns per workgroup: H / 16 workgroups (64 at
// the headline width), each thread B / 64 loads in turn — with 64 columns and 4 row groups the launch was 16 workgroups
// of 64 dependent loads per thread, a latency-bound tail.
constexpr int SYN_FC = 16, SYN_FR = 64;
__global__ __launch_bounds__(SYN_FC * SYN_FR) void synapse_grad_finish_kernel(int B, int H, const float* gamma, float lo,
                                                                              float hi, const float* ws, float* g_gamma) {
    __shared__ float part[SYN_FR][SYN_FC];
    const int c = threadIdx.x % SYN_FC, r = threadIdx.x / SYN_FC;
    const int h = blockIdx.x * SYN_FC + c;
    float s = 0.0f;
    if (h < H)
        for (int j = r; j < B; j += SYN_FR) s += ws[(size_t)j * H + h];
    part[r][c] = s;
    __syncthreads();
    if (r == 0 && h < H) {
        const float raw = gamma[h];
        const float oma = 1.0f - clampf(raw, lo, hi);
        float sum = part[0][c];
        for (int q = 1; q < SYN_FR; ++q) sum += part[q][c];
        g_gamma[h] = (raw >= lo && raw <= hi) ? sum / oma : 0.0f;
    }
}

static bool limits_ok(float lo, float hi) { return lo >= 0.0f && lo <= hi && hi < 1.0f; }  // (a NaN fails)

// columns per lane: 4 where H, every row stride and every base address allow 16-byte pieces, else 1
static int lane_cols(int H, long long ld0, long long ld1, long long ld2, const void* p0, const void* p1, const void* p2) {
    const bool ok = H % 4 == 0 && ld0 % 4 == 0 && ld1 % 4 == 0 && ld2 % 4 == 0;
    return (ok && aligned16(p0) && aligned16(p1) && aligned16(p2)) ? 4 : 1;
}

}  // namespace

extern "C" int sparch_synapse_fwd(int B, int T, int H, const float* Wx, long long ldwx, const float* bias,
                                  const float* scale, const float* shift, const float* gamma, float lo, float hi,
                                  const float* i0, float* i_out, long long ldi, float* i_T, const int* lengths,
                                  const int* offsets, void* stream) {
    SPARCH_ENTER();
    if (B < 1 || T < 1 || H < 1 || !Wx || !gamma || !i_out || ldwx < H || ldi < H) return SPARCH_EINVAL;
    if ((offsets && !lengths) || !limits_ok(lo, hi)) return SPARCH_EINVAL;
    const int n = lane_cols(H, ldwx, ldi, 4, Wx, i_out, nullptr);
    const unsigned long long blocks = ((unsigned long long)B * (H / n) + SYN_NT - 1) / SYN_NT;
    if (blocks > 0x7FFFFFFFull) return SPARCH_EINVAL;
    SynFwdArgs a{B, T, H, Wx, ldwx, bias, scale, shift, gamma, lo, hi, i0, i_out, ldi, i_T, lengths, offsets};
    const dim3 grid((unsigned)blocks), block(SYN_NT);
    hipStream_t st = (hipStream_t)stream;
    if (n == 4) hipLaunchKernelGGL(synapse_fwd_kernel<4>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(synapse_fwd_kernel<1>, grid, block, 0, st, a);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" size_t sparch_synapse_bwd_workspace_bytes(int B, int T, int H) {
    if (B < 1 || T < 1 || H < 1) return 0;
    return (size_t)B * (size_t)H * sizeof(float);
}

extern "C" int sparch_synapse_bwd(int B, int T, int H, const float* g_i, long long ldg, const float* i, long long ldi,
                                  const float* i0, const float* gamma, float lo, float hi, float* g_z, long long ldgz,
                                  float* g_gamma, void* ws, size_t ws_bytes, const float* bn_x, long long ldbn,
                                  const float* bn_mean, const float* bn_invstd, float* bn_ws, const int* lengths,
                                  const int* offsets, void* stream) {
    SPARCH_ENTER();
    if (B < 1 || T < 1 || H < 1 || !g_i || !gamma || ldg < H || (!g_z && !g_gamma)) return SPARCH_EINVAL;
    if ((offsets && !lengths) || !limits_ok(lo, hi)) return SPARCH_EINVAL;
    if (g_z && ldgz < H) return SPARCH_EINVAL;
    if (g_gamma && (!i || ldi < H || !ws)) return SPARCH_EINVAL;
    if (bn_x && (!bn_mean || !bn_invstd || !bn_ws || !g_z || ldbn < H)) return SPARCH_EINVAL;
    if (g_gamma && ws_bytes < sparch_synapse_bwd_workspace_bytes(B, T, H)) return SPARCH_EWORKSPACE;
    int n = lane_cols(H, ldg, g_gamma ? ldi : 4, g_z ? ldgz : 4, g_i, g_gamma ? i : nullptr, g_z);
    if (bn_x && (ldbn % 4 != 0 || !aligned16(bn_x))) n = 1;
    const unsigned long long blocks = ((unsigned long long)B * (H / n) + SYN_NT - 1) / SYN_NT;
    if (blocks > 0x7FFFFFFFull) return SPARCH_EINVAL;
    SynBwdArgs a{B, T, H, g_i, ldg, i, ldi, i0, gamma, lo, hi, g_z, ldgz, g_gamma ? (float*)ws : nullptr, lengths, offsets,
                 bn_x, ldbn, bn_mean, bn_invstd, bn_ws};
    const dim3 grid((unsigned)blocks), block(SYN_NT);
    hipStream_t st = (hipStream_t)stream;
    auto go = [&](auto gg, auto bns) {
        if (n == 4)
            hipLaunchKernelGGL((synapse_bwd_kernel<4, decltype(gg)::value, decltype(bns)::value>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((synapse_bwd_kernel<1, decltype(gg)::value, decltype(bns)::value>), grid, block, 0, st, a);
    };
    if (g_gamma) { if (bn_x) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{}); }
    else         { if (bn_x) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{}); }
    SPARCH_CHECK_LAUNCH();
    if (g_gamma) {
        hipLaunchKernelGGL(synapse_grad_finish_kernel, dim3((unsigned)cdiv(H, SYN_FC)), dim3(SYN_FC * SYN_FR), 0, st, B,
                           H, gamma, lo, hi, (const float*)ws, g_gamma);
        SPARCH_CHECK_LAUNCH();
    }
    return SPARCH_OK;
}

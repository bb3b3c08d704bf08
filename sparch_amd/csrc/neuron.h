// The spiking neuron's FORWARD arithmetic, once.  A stream may take a step through the chunk kernels
// (cell_fwd_pipe_kernel, rec_fwd_kernel, readout_fwd_kernel), the dense fused step (streamstep.hip) or the event-driven
// one (streamsparse.hip) and switches between them mid-stream, so all of them must round alike: they call the helpers
// below, and their files are built with -ffp-contract=off, so one expression tree gives one set of bits
// (tests/test_spiking_bits_gpu.py).
//
//     x_t = Wx_t (+ bias), then * scale + shift where a scale is given             neuron_input
//     w_t = (beta w + a u) + b s                          adaptive kinds           neuron_step
//     u_t = alpha (u - s) + (1 - alpha) (x_t [+ s V] [- w_t])
//     s_t = [u_t - theta > 0]                                                      spike_of
//     u_t = alpha u + (1 - alpha) x_t                     readout                  readout_step
//
// The backward kernels' device code must not move, so they call these helpers only where every
// instantiation compiles to the same bytes as before: cell_bwd_pipe_kernel uses neuron_load and spike_of,
// rec_bwd_kernel spike_of.  Remaining copies: the reverse-step arithmetic of the three backward kernels (rec_bwd_kernel
// splits it around its poll in a measured instruction order); the alpha clamp of readout_bwd_kernel (cell.hip), the
// four clamps of rec_bwd_kernel (reccell.hip: parked in LDS as four-column vectors) and its pack of s_{t-1} for the dV
// product — with the helper in their place hipcc emits other code for them; the pack of gemm_spike.hip (a keep mask).
#pragma once
#include "common.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
// ---- the clamped parameters of one neuron (snns.py:229, 356-359, 631-634; the SP_* bounds: common.h)
template <bool ADAPT>
struct Neuron {
    float al, oma, be, pa, pb;  // alpha, 1 - alpha, beta, a, b (the last three 0 for the non-adaptive kinds)
};
// the raw values of neuron i: for a kernel that issues the loads early and clamps behind other work (the fused steps)
template <bool ADAPT>
__device__ __forceinline__ Neuron<ADAPT> neuron_load_raw(const float* alpha, const float* beta, const float* a,
                                                         const float* b, int i) {
    return {alpha[i], 0.f, ADAPT ? beta[i] : 0.f, ADAPT ? a[i] : 0.f, ADAPT ? b[i] : 0.f};
}
template <bool ADAPT>
__device__ __forceinline__ Neuron<ADAPT> neuron_clamp(const Neuron<ADAPT>& raw) {
    const float al = clampf(raw.al, SP_ALPHA_LO, SP_ALPHA_HI);
    return {al, 1.0f - al, ADAPT ? clampf(raw.be, SP_BETA_LO, SP_BETA_HI) : 0.f,
            ADAPT ? clampf(raw.pa, SP_A_LO, SP_A_HI) : 0.f, ADAPT ? clampf(raw.pb, SP_B_LO, SP_B_HI) : 0.f};
}
template <bool ADAPT>
__device__ __forceinline__ Neuron<ADAPT> neuron_load(const float* alpha, const float* beta, const float* a,
                                                     const float* b, int i) {
    return neuron_clamp(neuron_load_raw<ADAPT>(alpha, beta, a, b, i));
}

// ---- the cell's input: the projection (+ bias; the chunk kernels' projection has it already), then the folded
//      BatchNorm affine where a scale is given
__device__ __forceinline__ float neuron_input(float wx, bool has_bias, float bias, bool has_scale, float sc, float sh) {
    if (has_bias) wx = wx + bias;
    return has_scale ? bn_affine(wx, sc, sh) : wx;
}
__device__ __forceinline__ bool spike_of(float u, float theta) { return (u - theta) > 0.0f; }  // snns.py:29

// ---- one membrane step in place: u, w (adaptive kinds), s from the input xn and, for the recurrent kinds, rec = s V.
//      (A non-recurrent cell adds no `+ 0`: that would turn a drive of -0 into +0.)
template <bool ADAPT, bool REC>
__device__ __forceinline__ void neuron_step(float& u, float& w, float& s, float xn, float rec, const Neuron<ADAPT>& p,
                                            float theta) {
    float drive = REC ? xn + rec : xn;                       // snns.py:572 / 720
    if (ADAPT) {
        w = (p.be * w + p.pa * u) + p.pb * s;                // snns.py:438 / 718
        drive = drive - w;
    }
    u = p.al * (u - s) + p.oma * drive;                      // snns.py:297 / 439 / 572 / 719
    s = spike_of(u, theta) ? 1.0f : 0.0f;
}
__device__ __forceinline__ float readout_step(float u, float xn, float al, float oma) {
    return al * u + oma * xn;                                // snns.py:822
}

// ---- spikes as bf16 0 / 1.0: one, two in a 32-bit word (lo in the low half), four in two words (v[e] != 0 spikes)
__device__ __forceinline__ unsigned spike_pair16(bool lo, bool hi) {
    return (lo ? 0x3F80u : 0u) | (hi ? 0x3F800000u : 0u);
}
__device__ __forceinline__ uint16_t spike_bf16(bool on) { return on ? (uint16_t)0x3F80u : (uint16_t)0u; }
template <class V>
__device__ __forceinline__ u32x2 spike_quad16(const V& v) {
    u32x2 h;
    h.x = spike_pair16(v[0] != 0.f, v[1] != 0.f);
    h.y = spike_pair16(v[2] != 0.f, v[3] != 0.f);
    return h;
}

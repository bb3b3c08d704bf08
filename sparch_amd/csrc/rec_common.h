// Shared device helpers of the persistent recurrent kernels (reccell.hip, gatedcell.hip): types, the hand-off
// ring constants, bare LDS barriers, exact-split MFMA wrappers, and the sentinel ring's machinery — tile issue /
// settle, the truncation split, the six-term ring product, the cross-wave sum, the publish, the abort epilogue.
// At the end, the host side the two files share: kernel-table rows, launch and clear helpers, the entry points'
// argument checks.  The launch policy is rec_plan.h.  See the header comment of reccell.hip for the design.
#pragma once
#include "common.h"
#include "rec_plan.h"

#include <initializer_list>

namespace {

typedef unsigned long long u64;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) unsigned gu32;

constexpr int RT = 32;       // rows per batch tile
constexpr int CT = 32;       // columns per workgroup (= one k-group of its consumers)
constexpr int RED_LD = 33;   // padded row of the cross-wave reduction tiles (read with 4-byte accesses)
constexpr int RED16 = 17;    // ... of the 16-column products' tiles
constexpr int RED_LD4 = 32;  // ... of the spiking cells' tiles, read with one 16-byte access per partial tile
constexpr int RING = 4;      // depth of the backward hand-off ring (2 suffices, see header)
constexpr int TILE_BYTES = RT * CT * 4;  // one fp32 hand-off tile (= ptile_bytes<2>(), see issue_ptile)
// Cache-policy operand of the hand-off buffer accesses: sc1.  Every hand-off load and store is agent scope / sc1,
// the only combination that is correct for any placement of the workgroups (a narrower scope stays in an XCD's L2,
// invisible to the other XCDs; plain stores are used only where xcd_agree has VERIFIED a shared XCD, see below).
constexpr int AUX_SC1 = 16;
constexpr int TILES_AHEAD = 1;  // k-groups whose tile loads are issued ahead of the one being multiplied
constexpr u64 TIMEOUT_TICKS = 200000000ull;  // 2 s of s_memrealtime (100 MHz)
// "not written yet" pattern of the backward / dense hand-off ring: a SIGNALLING NaN.  Arithmetic results are
// never signalling (the hardware quiets every NaN it produces or propagates, IEEE mode), so no tile value
// can equal it.
constexpr unsigned SENTINEL = 0x7FA5A5A5u;


__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// Non-temporal hints for what a time loop touches ONCE (round 3).  The loops stream their inputs (projection rows,
// incoming gradient, saved states) and outputs (saved states, spike planes, dWx) through the same L2 that holds what
// they re-read every step — the hand-off granules / ring tiles, the V pack — and at 2-4 MB per step per XCD the
// streams push those lines out: the backward ring (6 MB, rewritten every 4 steps) was written back to HBM on every
// pass (WRITE_SIZE 734 -> 490 MiB per launch with the hints: the ring now stays in L2), and the forward's polls and
// LUT / V reads missed.  Measured in one call, per launch in isolation: forward 0.636 -> 0.615 (loads) -> 0.597 ms
// (loads + stores), backward 1.024 -> 1.004 -> 1.003; in the cfg3 step (two layers): forward 1.195 -> 1.15 (loads),
// 1.09 (stores), 1.04 ms (both), step 6.58 -> 6.38 ms.  (The same hints on the split GEMMs' activation operands and
// C tiles LOSE: 6.49 -> 6.55-6.77 ms — a GEMM's output is the next kernel's input and should stay in the 256 MB
// infinity cache; `rec_bwd` right behind the dX product slowed down by 3-7 %.)
__device__ __forceinline__ f32x4 ld4s(const float* p) {  // a streaming input: read once
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
}
__device__ __forceinline__ void st4(float* p, f32x4 v) {  // a bulk output of the recurrent kernels
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
}
__device__ __forceinline__ void st2(void* p, u32x2 v) {  // an 8-byte bulk output (bf16 plane quads, bf16 saves)
    __builtin_nontemporal_store(v, reinterpret_cast<u32x2*>(p));
}
// saved states (u, w) as fp32 or bf16 (element index i)
__device__ __forceinline__ f32x4 ld4_saved(const float* base, size_t i, bool s16) {
    if (!s16) return ld4(base + i);
    const unsigned long long raw = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned short*>(base) + i);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = bf16_to_f32((unsigned short)(raw >> (16 * e)));
    return v;
}
// ... the same load with the storage type fixed at compile time, the packed form kept as it comes off the wire
// (expanded at the use, so that nothing waits for the load where it is issued)
template <bool S16> struct SavedRaw { typedef f32x4 type; };
template <> struct SavedRaw<true> { typedef u32x2 type; };
template <bool S16>
__device__ __forceinline__ typename SavedRaw<S16>::type ld_saved_raw(const float* base, size_t i) {
    if constexpr (S16) return *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(base) + i);
    else return ld4s(base + i);
}
__device__ __forceinline__ f32x4 expand_saved(const f32x4& r) { return r; }
__device__ __forceinline__ f32x4 expand_saved(const u32x2& r) {
    f32x4 v;
    v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xFFFF0000u);
    v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xFFFF0000u);
    return v;
}
template <bool IS_U>
__device__ __forceinline__ void st4_saved(float* base, size_t i, f32x4 v, bool s16, float theta) {
    if (!s16) { st4(base + i, v); return; }
    unsigned long long raw = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        raw |= (unsigned long long)(IS_U ? save_u16(v[e], theta) : f32_to_bf16_rne(v[e])) << (16 * e);
    st2(reinterpret_cast<unsigned short*>(base) + i, u32x2{(unsigned)raw, (unsigned)(raw >> 32)});
}

// Workgroup barrier for LDS hand-offs inside the time loops.  __syncthreads() also carries workgroup-scope
// release / acquire fences on GLOBAL memory, i.e. an `s_waitcnt vmcnt(0)`: every wave would wait for the
// acknowledgement of its write-through hand-off stores (~2 k cycles) and of its bulk output stores at every
// barrier.  The loops only exchange LDS data across these barriers (cross-workgroup data goes through sc1
// accesses that need no fence), so: LDS operations retired, then the bare barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// `s_waitcnt vmcnt(0)` as the builtin (the compiler's wait-count pass sees it and clears its scoreboard, unlike
// an asm statement).  Placed where every outstanding vector-memory operation is long complete anyway, it keeps
// hipcc from inserting its own conservative vmcnt(0) at a later join — e.g. behind the hand-off stores, where
// it would wait ~2 k cycles for their write-through acknowledgements.
__device__ __forceinline__ void vm_settled() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// The workgroup's abort flags live in LDS and are read once per step behind a barrier.  Spelled as `volatile`
// accesses through a generic pointer they compile to FLAT loads / stores, which count on vmcnt AND lgkmcnt and
// complete out of order — hipcc then waits `vmcnt(0) lgkmcnt(0)` behind every flag read, i.e. behind every
// barrier of the time loops each wave sat out the acknowledgements of the previous step's bulk HBM stores and
// of its HBM prefetch (round 3, found in the ISA).  Through an LDS-address-space pointer they are ds_read /
// ds_write and touch lgkmcnt only.
typedef __attribute__((address_space(3))) int lds_i32;
typedef __attribute__((address_space(3))) void lds_void;        // LDS destination of an LDS-DMA load
typedef __attribute__((address_space(1))) const void g_void;    // ... and its global source
// LDS-DMA: 16 bytes per lane from the lane's own global address to lds_wave_base + 16 * lane (wave-uniform base).
// Inline asm: the load is then absent from hipcc's wait-count bookkeeping (its own counted waits only get
// stricter by that), and the caller guarantees a covering `s_waitcnt vmcnt` of the ISSUING wave before the data
// is read.  M0 (the destination base) is compiler-reserved: saved and restored inside the statement
// (cdna_hip_programming.md, inline-asm rules).
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(lds_void*)lds_wave_base);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}
__device__ __forceinline__ int lds_flag_read(const int* p) { return *(const volatile lds_i32*)p; }
__device__ __forceinline__ void lds_flag_set(int* p) { *(volatile lds_i32*)p = 1; }
__device__ __forceinline__ void lds_flag_store(int* p, int v) { *(volatile lds_i32*)p = v; }

// The status word of a device is FOUR uint32 (include/sparch_hip.h): [0] raised, [1] optimizer steps skipped while it
// was raised (sparch_adam_step counts them), [2] id of the kernel that raised it (SPARCH_STATUS_*), [3] the time step
// (processing order) it gave up at.  Diagnostics first, the flag last.
__device__ __forceinline__ void status_raise(unsigned* status, unsigned kernel_id, int step) {
    __hip_atomic_store((gu32*)status + 2, kernel_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu32*)status + 3, (unsigned)step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu32*)status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void raise_timeout(unsigned* status, int* abort_slot, unsigned kernel_id, int step) {
    status_raise(status, kernel_id, step);
    lds_flag_set(abort_slot);
}

__device__ __forceinline__ f32x16 mfma_bf16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                   c, 0, 0, 0);
}
// v_mfma_f32_16x16x32_bf16: A fragment = lane (row lane & 15, k-quarter lane >> 4) holds k = 8*(lane>>4) .. +7;
// B fragment = lane (column lane & 15, same k-quarter); C = 4 rows (4*(lane>>4) .. +3) of column lane & 15.
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// exact 3-way bf16 split of an fp32 value: x == hi + mid + lo (round-to-nearest-even at each step)
__device__ __forceinline__ void split3(float x, unsigned short& hi, unsigned short& mid, unsigned short& lo) {
    const __bf16 h = (__bf16)x;
    const float r1 = x - (float)h;
    const __bf16 m = (__bf16)r1;
    const float r2 = r1 - (float)m;
    const __bf16 l = (__bf16)r2;
    hi = __builtin_bit_cast(unsigned short, h);
    mid = __builtin_bit_cast(unsigned short, m);
    lo = __builtin_bit_cast(unsigned short, l);
}

// Packing a recurrent matrix.  rne (the bf16 operand mode, sparch_set_operand_precision): plane 0 = the value
// rounded once to bf16, planes 1 and 2 = 0 — the kernels of that mode read plane 0 only, and any three-plane
// kernel given such a pack computes products with the same rounded weights.
__device__ __forceinline__ void vsplit(float v, int rne, unsigned short& hi, unsigned short& mid, unsigned short& lo) {
    split3(v, hi, mid, lo);
    if (rne) { mid = 0; lo = 0; }
}

// V (or V^T) slice -> registers: per k-group, 2 k16-steps x NP planes of 8 bf16 (4 VGPRs) each (the packed
// layout always has room for three planes; the bf16 operand mode keeps its one rounded plane in plane 0)
template <int KGW, int NW, int NP = 3>
__device__ __forceinline__ void load_vslice(u32x4 (&vb)[KGW][2][NP], const u32x4* __restrict__ vpack, int ct,
                                            int nkg, int wave, int lane) {
#pragma unroll
    for (int kk = 0; kk < KGW; ++kk) {
        const int kg = wave + NW * kk;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int p = 0; p < NP; ++p)
                vb[kk][ks][p] = vpack[((((size_t)ct * nkg + kg) * 2 + ks) * 3 + p) * 64 + lane];
    }
}


// A 16-byte piece of a hand-off tile that still holds the sentinel has not been written yet.
__device__ __forceinline__ bool piece_missing(const u32x4& v) { return v[0] == SENTINEL || v[3] == SENTINEL; }

// ---- hand-off tiles as PRE-SPLIT bf16 planes (round 2, with the XCD-local stores).  The producer
// splits its dWx values once (x = t1 + t2 + t3, truncation split) and publishes the three planes; a consumer
// loads MFMA fragments and nothing else: 6 KB per tile instead of 4, no split VALU in the 32 consumers (each of
// which used to split the same 32 x 1024 values: 2.8 k VALU cycles per SIMD and step).  Tile layout: 16-byte
// piece ((ks*3 + p)*64 + h*32 + row) = plane p, k = 16 ks + 8 h + 0..7 of that row — the wave-load of one
// (k16-step, plane) is one contiguous 1 KiB.  A producer thread owns 4 consecutive k: half a piece, written
// with 8-byte stores (first / last word of a piece sit in different halves: the sentinel check covers both).
// No plane word can equal the sentinel: its upper half would be a signalling-NaN bf16, and every plane value
// is the upper half of an arithmetic fp32 result.
// NP planes per tile: 3 = the exact split, 1 = the bf16 operand mode (one nearest-even rounding by the producer,
// 2 KB per tile; the same layout with NP in place of 3).  A rounded plane word cannot equal the sentinel either:
// v_cvt_pk_bf16_f32 quiets every NaN it converts.
// A dense fp32 tile (the gated kernels' rings, 4 KB) is, as far as LOADING goes, a tile of NP = 2 "planes": lane
// (row li, k-half hh) of k16-step ks needs k = 16*ks + 8*hh + 4q + 0..3, which its producers store as piece
// (ks*2 + q)*64 + lane — the same four contiguous 1 KiB wave-loads, the same sentinel check per piece; the consumer
// splits the two pieces of a k16-step into the three fragments (split_pieces).
// issue_ptile: the 2 NP wave-loads of ONE k-group.  Padding k-groups (beyond n_ct) read past the end of the buffer
// resource: the hardware returns zeros for out-of-range buffer loads — no branch, and zeros are never "missing".
// settle_ptile: wait for the pieces of ONE k-group (the others stay in flight) and re-load what still reads as the
// sentinel until it has landed (bounded spin; on a timeout the abort flag is set and the status word is raised at the
// kernel's exit).  Fast path: 2 NP compares and one wave-uniform branch.  Slow path: re-loads go to temporaries and
// are waited for right there (builtin wait: the compiler's scoreboard stays exact), then merged by select — the
// pending loads of the later k-groups are not touched, so the fast path keeps its precise vmcnt(N) waits after the
// join.
constexpr int PTILE_BYTES = RT * CT * 6;  // what the host sizes the ring for (three planes)
template <int NP> constexpr int ptile_bytes() { return RT * CT * 2 * NP; }
template <int NW, int NP = 3>
__device__ __forceinline__ void issue_ptile(u32x4 (&g)[2][NP], __amdgpu_buffer_rsrc_t rsrc, unsigned base, int kg, int n_ct) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const unsigned off = kg < n_ct ? base + (unsigned)kg * ptile_bytes<NP>() + (unsigned)((ks * NP + p) * 1024) : 0xFFFFFF00u;
            g[ks][p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, AUX_SC1);
        }
}
template <int NP = 3>
__device__ __forceinline__ void settle_ptile(u32x4 (&g)[2][NP], __amdgpu_buffer_rsrc_t rsrc, unsigned tile_base, int* abort_slot) {
    unsigned miss = 0;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int p = 0; p < NP; ++p) miss |= piece_missing(g[ks][p]) ? (1u << (ks * NP + p)) : 0u;
    if (__any(miss != 0)) {  // slow path: temporaries, builtin wait, merge by select
        const u64 t_start = __builtin_amdgcn_s_memrealtime();
        for (unsigned spins = 0;; ++spins) {
            __builtin_amdgcn_s_sleep(1);
            u32x4 tmp[2][NP];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    tmp[ks][p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, tile_base + (unsigned)((ks * NP + p) * 1024), 0, AUX_SC1);
            vm_settled();
            unsigned still = 0;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const unsigned bit = 1u << (ks * NP + p);
                    const bool m = (miss & bit) != 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) g[ks][p][e] = m ? tmp[ks][p][e] : g[ks][p][e];
                    if (m && piece_missing(tmp[ks][p])) still |= bit;
                }
            miss = still;
            if (!__any(miss != 0)) break;
            if ((spins & 63u) == 63u && __builtin_amdgcn_s_memrealtime() - t_start > TIMEOUT_TICKS) {
                lds_flag_set(abort_slot);
                break;
            }
        }
    }
}

// THE exact truncation split, two values at a time: x = t1 + t2 + t3 with t1 the upper half of x, t2 the upper half of
// the residual, t3 of what remains; w[0..2] = the bf16 pairs t1, t2, t3 (x1's in the upper half).  v_perm for the
// packing, AND + SUB for the residuals: ~5.5 VALU instructions per value.
struct SplitPair { unsigned w[3]; };
__device__ __forceinline__ SplitPair split_pair(unsigned x0, unsigned x1) {
    const float r0 = __uint_as_float(x0) - __uint_as_float(x0 & 0xFFFF0000u);
    const float r1 = __uint_as_float(x1) - __uint_as_float(x1 & 0xFFFF0000u);
    const unsigned y0 = __float_as_uint(r0), y1 = __float_as_uint(r1);
    const float q0 = r0 - __uint_as_float(y0 & 0xFFFF0000u);
    const float q1 = r1 - __uint_as_float(y1 & 0xFFFF0000u);
    return {{__builtin_amdgcn_perm(x1, x0, 0x07060302u), __builtin_amdgcn_perm(y1, y0, 0x07060302u),
             __builtin_amdgcn_perm(__float_as_uint(q1), __float_as_uint(q0), 0x07060302u)}};
}
// consumer side: 8 fp32 values (the two 16-byte pieces of a fragment's k range) -> the three bf16 fragments
__device__ __forceinline__ void split_pieces(const u32x4& lo4, const u32x4& hi4, u32x4& p1, u32x4& p2, u32x4& p3) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const SplitPair t = split_pair((q ? hi4 : lo4)[2 * pr], (q ? hi4 : lo4)[2 * pr + 1]);
            p1[2 * q + pr] = t.w[0]; p2[2 * q + pr] = t.w[1]; p3[2 * q + pr] = t.w[2];
        }
}
// producer side: a thread's 4 fp32 values -> one word pair (4 bf16) per plane
__device__ __forceinline__ void split4_planes(const f32x4& v, u32x2 (&w)[3]) {
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const SplitPair t = split_pair(__float_as_uint(v[2 * pr]), __float_as_uint(v[2 * pr + 1]));
#pragma unroll
        for (int p = 0; p < 3; ++p) w[p][pr] = t.w[p];
    }
}
// one plane-tile half piece per plane (8 bytes each, 1 KiB apart) at byte offset `off`; `plain`: XCD-local stores
__device__ __forceinline__ void store_planes(const u32x2 (&w)[3], __amdgpu_buffer_rsrc_t rsrc, unsigned off, bool plain) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        if (plain) __builtin_amdgcn_raw_buffer_store_b64(w[p], rsrc, off + (unsigned)(p * 1024), 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b64(w[p], rsrc, off + (unsigned)(p * 1024), 0, AUX_SC1);
    }
}

// ---- the ring product: one step's recurrent product of a workgroup, written once.
// The six cross terms of (t1 + t2 + t3) x (hi + mid + lo) that matter, smallest first.  THIS ORDER IS PART OF THE
// RESULT'S BITS (tests/golden/baseline_rec_bits.json).  MFMA: mfma_bf16 (32x32x16, f32x16) or mfma16 (16x16x32, f32x4).
template <auto MFMA, class Acc>
__device__ __forceinline__ Acc six_terms(const u32x4& p1, const u32x4& p2, const u32x4& p3, const u32x4& hi,
                                         const u32x4& mid, const u32x4& lo, Acc acc) {
    acc = MFMA(p2, mid, acc);  // t2*mid
    acc = MFMA(p3, hi, acc);   // t3*hi
    acc = MFMA(p1, lo, acc);   // t1*lo
    acc = MFMA(p2, hi, acc);   // t2*hi
    acc = MFMA(p1, mid, acc);  // t1*mid
    acc = MFMA(p1, hi, acc);   // t1*hi
    return acc;
}

// This wave's KGW tiles (k-groups wave, wave + NW, ...) of a row tile, from the ring slot at `base` (slot + row tile +
// lane * 16), handed to body(kk, tile) one after the other with the next tile's loads in flight (TILES_AHEAD; more
// loses, see rec_bwd_kernel).  The sched_barrier pair keeps hipcc from moving the issue above the settle's wait or the
// MFMAs into the pair.  Everything is unrolled: kk is a constant where body indexes registers with it.
template <int KGW, int NW, int NP, class Body>
__device__ __forceinline__ void ring_tiles(__amdgpu_buffer_rsrc_t rsrc, unsigned base, int ntiles, int wave,
                                           int* abort_slot, Body&& body) {
    constexpr int AHEAD = KGW < TILES_AHEAD ? KGW : TILES_AHEAD;
    u32x4 raw[KGW][2][NP];
#pragma unroll
    for (int kk = 0; kk < AHEAD; ++kk) issue_ptile<NW, NP>(raw[kk], rsrc, base, wave + NW * kk, ntiles);
#pragma unroll
    for (int kk = 0; kk < KGW; ++kk) {
        __builtin_amdgcn_sched_barrier(0);
        if (wave + NW * kk < ntiles)
            settle_ptile<NP>(raw[kk], rsrc, base + (unsigned)(wave + NW * kk) * ptile_bytes<NP>(), abort_slot);
        if (kk + AHEAD < KGW) issue_ptile<NW, NP>(raw[kk + AHEAD], rsrc, base, wave + NW * (kk + AHEAD), ntiles);
        __builtin_amdgcn_sched_barrier(0);
        body(kk, raw[kk]);
    }
}

// 32 columns (32x32x16 MFMA): a tile is two k16-steps of one 32 x 32 product.  vb[kk][ks] = hi, mid fragments of the
// slice, vlo_w[kk][ks][lane] = its lo fragment (LDS); NP = 3: the tile arrives as planes, NP = 2: as fp32 to split.
// The wave's partial tile goes to red_w (RT x RED_LD).
template <int KGW, int NW, int NP>
__device__ __forceinline__ void ring_product32(const u32x4 (&vb)[KGW][2][2], const u32x4 (&vlo_w)[KGW][2][64],
                                               __amdgpu_buffer_rsrc_t rsrc, unsigned base, int ntiles, int wave, int lane,
                                               int* abort_slot, float* red_w) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    ring_tiles<KGW, NW, NP>(rsrc, base, ntiles, wave, abort_slot, [&](int kk, const u32x4 (&g)[2][NP]) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 p1, p2, p3;
            if constexpr (NP == 3) { p1 = g[ks][0]; p2 = g[ks][1]; p3 = g[ks][2]; }
            else split_pieces(g[ks][0], g[ks][1], p1, p2, p3);
            acc = six_terms<mfma_bf16>(p1, p2, p3, vb[kk][ks][0], vb[kk][ks][1], vlo_w[kk][ks][lane], acc);
        }
    });
    const int li = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
        red_w[row * RED_LD + li] = acc[i];
    }
}

// 16 columns (16x16x32 MFMA, nothing of the matrix pipe spent on padding columns): a tile is one 32-deep k step of
// two 16-row blocks, fp32, pieces ((mb*2 + half)*64 + lane) — the ptile offsets with (mb, half) for (ks, q).
// vb[kk] = hi, mid, vlo_w[kk][lane] = lo.  The wave's two partial 16 x 16 tiles go to red_w (RT x RED16).
template <int KGW, int NW>
__device__ __forceinline__ void ring_product16(const u32x4 (&vb)[KGW][2], const u32x4 (&vlo_w)[KGW][64],
                                               __amdgpu_buffer_rsrc_t rsrc, unsigned base, int ntiles, int wave, int lane,
                                               int* abort_slot, float* red_w) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2] = {zero4, zero4};
    ring_tiles<KGW, NW, 2>(rsrc, base, ntiles, wave, abort_slot, [&](int kk, const u32x4 (&g)[2][2]) {
        const u32x4 vl = vlo_w[kk][lane];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            u32x4 p1, p2, p3;
            split_pieces(g[mb][0], g[mb][1], p1, p2, p3);
            acc[mb] = six_terms<mfma16>(p1, p2, p3, vb[kk][0], vb[kk][1], vl, acc[mb]);
        }
    });
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int i = 0; i < 4; ++i) red_w[(16 * mb + 4 * (lane >> 4) + i) * RED16 + (lane & 15)] = acc[mb][i];
}

// the resident slice of a ring product: hi and mid fragments in registers, lo in LDS (vlo_w = this wave's part)
template <int KGW, int NW>
__device__ __forceinline__ void load_slice32(u32x4 (&vb)[KGW][2][2], u32x4 (&vlo_w)[KGW][2][64], const u32x4* vpack,
                                             int ct, int nkg, int wave, int lane) {
#pragma unroll
    for (int kk = 0; kk < KGW; ++kk)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const u32x4* src = vpack + ((((size_t)ct * nkg + wave + NW * kk) * 2 + ks) * 3) * 64 + lane;
            vb[kk][ks][0] = src[0];
            vb[kk][ks][1] = src[64];
            vlo_w[kk][ks][lane] = src[128];
        }
}
template <int KGW, int NW>
__device__ __forceinline__ void load_slice16(u32x4 (&vb)[KGW][2], u32x4 (&vlo_w)[KGW][64], const u32x4* vpack, int ct,
                                             int wave, int lane) {
#pragma unroll
    for (int kk = 0; kk < KGW; ++kk) {
        const u32x4* src = vpack + (((size_t)ct * (NW * KGW) + wave + NW * kk) * 3) * 64 + lane;
        vb[kk][0] = src[0];
        vb[kk][1] = src[64];
        vlo_w[kk][lane] = src[128];
    }
}

// element o of the product: the waves' partial tiles summed in wave order 0 .. NW-1 (part of the result's bits)
template <int NW, int N>
__device__ __forceinline__ float wave_sum(const float (&red)[NW][N], int o) {
    float sum = red[0][o];
#pragma unroll
    for (int w = 1; w < NW; ++w) sum = sum + red[w][o];
    return sum;
}

// Publish a thread's part of step s at byte offset `off` of a ring slot (row tile + tile + piece): the data into slot
// s % RING where someone will read it (`live`), and the sentinel back into the slot of step s-2 — every peer has
// consumed that one: they have all published step s-1 since.  Write-through (sc1) stores.
__device__ __forceinline__ void publish_piece(__amdgpu_buffer_rsrc_t rsrc, unsigned slot_bytes, unsigned off, int s,
                                              bool live, const f32x4& v) {
    if (live)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc, (unsigned)(s % RING) * slot_bytes + off, 0, AUX_SC1);
    if (s >= 2) {
        const u32x4 sent = {SENTINEL, SENTINEL, SENTINEL, SENTINEL};
        __builtin_amdgcn_raw_buffer_store_b128(sent, rsrc, (unsigned)((s - 2) % RING) * slot_bytes + off, 0, AUX_SC1);
    }
}
// ... of a plane tile: the 4 values split here, once, for all consumers; `plain`: XCD-local stores
__device__ __forceinline__ void publish_planes(__amdgpu_buffer_rsrc_t rsrc, unsigned slot_bytes, unsigned off, int s,
                                               bool live, const f32x4& v, bool plain) {
    if (live) {
        u32x2 w[3];
        split4_planes(v, w);
        store_planes(w, rsrc, (unsigned)(s % RING) * slot_bytes + off, plain);
    }
    if (s >= 2) {
        const u32x2 sent[3] = {{SENTINEL, SENTINEL}, {SENTINEL, SENTINEL}, {SENTINEL, SENTINEL}};
        store_planes(sent, rsrc, (unsigned)((s - 2) % RING) * slot_bytes + off, plain);
    }
}

// the end of a ring kernel: a settle that timed out (either parity) raises the device's status word
__device__ __forceinline__ void raise_if_aborted(const int (&abort_flag)[2], unsigned* status, unsigned kernel_id, int tid) {
    if (tid == 0 && (lds_flag_read(&abort_flag[0]) | lds_flag_read(&abort_flag[1]))) status_raise(status, kernel_id, -1);
}

// ---- XCD-local hand-off stores (speed option, VERIFIED at run time).
// Agent-scope (sc1) stores are write-through and drop the line from the XCD's L2: a consumer on the same XCD
// then fetches it at the cross-XCD rate and latency.  A plain store keeps the line in that L2, where an sc1
// load of any CU of the XCD finds it (sc1 loads bypass L1 only) — but it is invisible to the other XCDs.
// Placement is not part of HIP's contract, so nothing may ASSUME that a row tile's workgroups share an XCD:
// they establish it.  Every workgroup publishes the XCC id of the XCD it runs on (HW_REG_XCC_ID) with an
// agent-scope store into a table the host cleared, reads the entries of all workgroups of its row tile with
// agent-scope loads (bounded spin), and only if all are there and equal do these workgroups — all of which
// see the same entries — use plain stores among themselves.  Anything else (different XCDs, a workgroup
// that never arrives, chunked launches, an absent table) keeps the sc1 stores.  A wave that finds itself
// on another XCD later (queue preemption with save / restore) raises the launch's abort flag: the step is
// discarded and the host goes to per-step launches, exactly as after a timeout.
constexpr int GETREG_XCC_ID = (3 << 11) | 20;  // hwreg(HW_REG_XCC_ID, 0, 4)
__device__ __forceinline__ unsigned xcc_id() { return (unsigned)__builtin_amdgcn_s_getreg(GETREG_XCC_ID) & 0xFu; }

// tab: this row tile's n_ct (<= 64) words, all `empty` before the launch.  Called by every thread of the
// workgroup BEFORE a __syncthreads() the caller already has; the result is read from *lds_flag after it.
__device__ __forceinline__ void xcd_agree(gu32* tab, unsigned empty, int n_ct, int ct, unsigned my_xcc, int tid,
                                          int* lds_flag) {
    if (tid >= 64) return;
    bool ok = tab != nullptr && n_ct <= 64;
    if (ok) {
        if (tid == 0) __hip_atomic_store(tab + ct, my_xcc + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < n_ct) {
            const u64 t_start = __builtin_amdgcn_s_memrealtime();
            unsigned v = empty;
            for (unsigned spins = 0;; ++spins) {
                v = __hip_atomic_load(tab + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (v != empty) break;
                __builtin_amdgcn_s_sleep(2);
                if ((spins & 63u) == 63u && __builtin_amdgcn_s_memrealtime() - t_start > TIMEOUT_TICKS / 100) break;  // 20 ms
            }
            ok = v == my_xcc + 1u;
        }
    }
    const bool all = __all(ok);
    if (tid == 0) *lds_flag = all ? 1 : 0;
}

// ---- host side: what the entry points and the launch code of reccell.hip and gatedcell.hip share.  The launch
// policy itself (groups of row tiles x chunks of steps, the kgw -> kernel shape rule) is rec_plan.h.

// One row of a kernel family's table: what is launched and with how many threads; per_cu (the kinds that ask the
// occupancy calculator only) answers how many workgroups of THIS kernel the runtime fits on a CU.
template <class Args>
struct KernelRef {
    void (*fn)(Args) = nullptr;
    int threads = 0;
    int (*per_cu)() = nullptr;
};
// Occupancy as the runtime computes it for this kernel's registers / LDS; asked once per kernel and process (host time
// per launch is inside every training step).  A failed query counts as 1.
template <auto Kernel, int THREADS>
int occupancy_per_cu() {
    static const int per_cu = [] {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, Kernel, THREADS, 0) != hipSuccess) n = 1;
        (void)hipGetLastError();
        return n;
    }();
    return per_cu;
}
template <class Args, void (*Kernel)(Args), int THREADS>
constexpr KernelRef<Args> kernel_with_occupancy() { return {Kernel, THREADS, &occupancy_per_cu<Kernel, THREADS>}; }
// Can `grid` workgroups of this kernel be resident at once?  (The persistent launches wait for each other inside the
// kernel.)  The in-kernel spins are bounded anyway — this keeps a foreseeable miss (fewer CUs than assumed, a build
// with more registers) from costing a 2 s timeout before the per-step fallback takes over.
template <class Args>
bool co_resident(const KernelRef<Args>& k, unsigned grid, int cus) {
    return (long long)k.per_cu() * rec_plan::cus_or_default(cus) >= (long long)grid;
}
template <class Args>
int launch_kernel(const KernelRef<Args>& k, unsigned grid, const Args& a, hipStream_t st) {
    if (!k.fn) return SPARCH_EINVAL;
    hipLaunchKernelGGL(k.fn, dim3(grid), dim3((unsigned)k.threads), 0, st, a);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

// Hand-off buffers before a pass: `bytes` of 32-bit `pattern` — 0 for the forward granules ("tag 0"), SENTINEL for the
// rings ("not written yet"); the agreement table behind either is cleared with them, its "empty" being that word.
inline int clear_handoff(void* p, unsigned pattern, size_t bytes, hipStream_t st) {
    const hipError_t e = pattern == 0 ? hipMemsetAsync(p, 0, bytes, st)
                                      : hipMemsetD32Async((hipDeviceptr_t)p, (int)pattern, bytes / 4, st);
    return e == hipSuccess ? SPARCH_OK : SPARCH_ELAUNCH;
}

// argument checks of the entry points
inline bool all_set(std::initializer_list<const void*> ps) {  // mandatory pointers
    for (const void* p : ps)
        if (!p) return false;
    return true;
}
inline bool al16(std::initializer_list<const void*> ps) {  // pointers the kernels access 16 bytes at a time (or NULL)
    for (const void* p : ps)
        if (p && !aligned16(p)) return false;
    return true;
}
inline bool paired(const void* scale, const void* shift) { return (scale == nullptr) == (shift == nullptr); }
inline bool p_drop_ok(float p) { return p >= 0.0f && p < 1.0f; }  // false for a NaN
inline bool shape_ok(int B, int dirs, int T, int H, int h_multiple) {
    return B > 0 && T > 0 && H > 0 && H % h_multiple == 0 && (dirs == 1 || dirs == 2);
}
// the fields every Args struct starts from
template <class Args>
Args base_args(int B, int dirs, int T, int H, float p_drop, uint64_t seed) {
    Args a{};
    a.B = B; a.dirs = dirs; a.T = T; a.H = H; a.Bp = B * dirs;
    a.p_drop = p_drop; a.inv_keep = 1.0f / (1.0f - p_drop); a.seed = seed;
    return a;
}
// geometry of a step entry (RecArgs / AnnArgs): one launch over all row tiles, the recurrent product supplied by the
// caller (one k-group class)
template <class Args>
unsigned step_geometry(Args& a) {
    a.n_ct = cdiv(a.H, CT); a.nkg = 4; a.n_rt_total = cdiv(a.Bp, RT); a.rt_base = 0; a.n_rt_launch = a.n_rt_total;
    return (unsigned)(a.n_ct * a.n_rt_total);
}

}  // namespace

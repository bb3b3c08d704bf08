// f-3: event lists -> dense binned spike counts on the device.
//
// Replaces SpikingDataset.__getitem__ (spiking_datasets.py:66-78): per sample
//     times = np.digitize(firing_times, np.linspace(0, max_time, nb_steps))     # 1-based bin of each event
//     x     = sparse(idx=[times, units], val=1, size=(nb_steps, nb_units)).to_dense()   # duplicates add up
// for a whole batch at once.  np.digitize(t, bins) (right=False) = number of edges <= t, so an event at
// t in [0, bins[1]) lands in row 1 and row 0 stays empty (a quirk of the reference, preserved); an event
// with t >= max_time would index row nb_steps, which the reference's sparse constructor rejects: such
// events (and negative times / out-of-range units) are counted in *n_dropped and skipped.
// Edges are evaluated in fp64 exactly as np.linspace does (start + j*step, last edge = stop).
// sparch_bin_events accumulates with global float atomics of integer values: exact and order-independent.
// sparch_events_gather_bin (below) builds a batch from a device-resident store with counters in LDS instead;
// sparch_events_gather_bin_aug is the same kernel with a per-sample transform of (t, u) in front of the bin.
#include <type_traits>

#include "common.h"

namespace {

// The bin of one event, np.digitize(t, np.linspace(0, max_time, nb_steps)) = the number of edges <= t, and the
// reference's drop rule.  ONE definition for both kernels below (sparch_bin_events and sparch_events_gather_bin
// must place every event alike, bit for bit).  The edges are fp64, as np.linspace evaluates them (j * step, last
// edge = stop), and they ascend, so the answer is the one k with edge(k) <= t < edge(k + 1): the two loops walk to
// it from ANY candidate, so the candidate may be cheap: an fp32 product (it used to be two fp64 divisions per
// event, t / step and max_time / (nb_steps - 1), which cost more than the rest of the event's work).
// Fast path: times are fp16 / fp32 values, x = t * inv_step in fp32 is within x * 2^-23 <= 2^-12 of t / step
// for nb_steps <= 2048 (one rounding of inv_step, one of the product; the fp64 edges are 2^-52 from j * step), so
// when x is at least 2^-10 away from both neighbouring integers and 0 <= floor(x) <= nb_steps - 2, the walk would
// end at floor(x) without moving: no fp64 then (x - floor(x) is exact in fp32).  About one event in 500 walks.
struct BinEdges {
    double step, max_time;
    float inv_step, top;
    int nb_steps;
    __device__ __forceinline__ BinEdges(int nb_steps_, double max_time_)
        : step(max_time_ / (double)(nb_steps_ - 1)), max_time(max_time_),
          inv_step((float)((double)(nb_steps_ - 1) / max_time_)),
          top(nb_steps_ <= 2048 ? (float)(nb_steps_ - 2) : -1.0f), nb_steps(nb_steps_) {}
    __device__ __forceinline__ double edge(int j) const { return j == nb_steps - 1 ? max_time : (double)j * step; }
};
__device__ __forceinline__ int event_bin(float tf, const BinEdges& e) {
    const float x = tf * e.inv_step, fl = floorf(x), frac = x - fl;
    if (fl >= 0.0f && fl <= e.top && frac >= 0x1p-10f && frac <= 1.0f - 0x1p-10f) return (int)fl + 1;
    const double t = (double)tf;
    int k = (int)fl;                          // candidate: edges 0..k are <= t
    k = max(-1, min(k, e.nb_steps - 1));
    while (k + 1 < e.nb_steps && e.edge(k + 1) <= t) ++k;   // walk to the answer, either way
    while (k >= 0 && e.edge(k) > t) --k;
    return k + 1;                             // np.digitize
}
__device__ __forceinline__ bool event_dropped(float t, int bin, int u, int nb_steps, int nb_units) {
    return t < 0.0f || bin >= nb_steps || u < 0 || u >= nb_units;
}

__global__ void bin_events_kernel(long long n_events, const float* __restrict__ times,
                                  const int* __restrict__ units, const long long* __restrict__ offsets,
                                  int n_samples, int nb_steps, int nb_units, double max_time,
                                  float* __restrict__ out, unsigned* __restrict__ n_dropped) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_events) return;
    // sample of event i: largest b with offsets[b] <= i (binary search over the batch)
    int lo = 0, hi = n_samples;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const float t = times[i];
    const int u = units[i];
    const int bin = event_bin(t, BinEdges(nb_steps, max_time));
    if (event_dropped(t, bin, u, nb_steps, nb_units)) {
        atomicAdd(n_dropped, 1u);
        return;
    }
    atomicAdd(out + ((size_t)lo * nb_steps + bin) * nb_units + u, 1.0f);
}

// ---- a11 (exp.py:355-356): a batch of binned spike counts uploaded as ONE BYTE per element and expanded on the
// device.  The reference copies the dense float batch over PCIe every step ((256, 250, 700) fp32 = 179 MB against
// 45 MB as uint8); counts are small non-negative integers (spiking_datasets.py:71-78), exact in uint8 up to 255
// and in bf16 up to 256.  One pass writes the bf16 plane the first layer's GEMMs read (rows padded to ldp
// elements, zeros behind column K — the layout of sparch_plane_bf16_exact) and, on request, the fp32 tensor.
__global__ __launch_bounds__(256) void expand_counts_kernel(long long M, int K, const uint8_t* __restrict__ c,
                                                            uint16_t* __restrict__ plane, int ldp,
                                                            float* __restrict__ x, int ldx) {
    const long long n = M * (long long)ldp;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i / ldp;
        const int k = (int)(i - m * ldp);
        const unsigned v = k < K ? (unsigned)c[m * K + k] : 0u;
        const float f = (float)v;                       // <= 255: exact in bf16 (8 significant bits)
        plane[i] = (uint16_t)(__float_as_uint(f) >> 16);
        if (x && k < K) x[m * ldx + k] = f;
    }
}


// ---- resident event store: a batch from a device-resident store and a device list of sample indices.
//
// A workgroup owns a TILE: one sample of the batch, a slab of `rows` time rows, `cw` columns (all ldp columns
// whenever a row of uint32 counters fits the budget; wider rows are cut into column slabs of GB_MAX_COLS, one row
// high).  It zeroes the tile in LDS, adds its events with LDS atomics (integer adds: exact, order-independent),
// and then writes every output element of the tile exactly once, 16 bytes per store: no memset of the outputs,
// no global atomic.  The tile is sized so that TWO workgroups fit a CU's 160 KiB of LDS (one fills while the
// other writes); the slab height follows from nb_steps (gb_tile), nothing is assumed about it.
//
// Which events a workgroup reads: the bin is a non-decreasing function of t, so in a sample whose times are
// non-decreasing (sorted != 0, established once for the whole store by its owner) the events of rows [r0, r1) are
// one contiguous range, found by a cooperative search (every thread probes one position per round: GB_NT-ary, two
// rounds for a few thousand events, both ends searched in the same rounds).  Otherwise the workgroup scans the
// whole sample.  Either way every event read is filtered by its bin again, so both give the same tile.
// Ownership of an event that is dropped: the row slab that holds min(bin, nb_steps - 1) (t < 0 has bin 0), column
// slab 0 — counted once.  Per-workgroup drop counts go to the workspace and a one-workgroup kernel adds them up.
constexpr int GB_NT = 512;                // measured against 256 and 1024: both slower
constexpr int GB_UNROLL = 8;              // events per thread and trip of the event loop
constexpr int GB_LDS_BUDGET = 80 * 1024 - 512;  // dynamic LDS per workgroup: two of them, with the 256 static bytes
                                                // the block-wide count takes, fit the CU's 160 KiB
constexpr int GB_HDR = 16;                // bytes in front of the tile: word 0 = events dropped by this workgroup
constexpr int GB_MAX_COLS = 16384;        // columns of a tile when a whole row does not fit

struct GbTile {
    int cw, rows, n_rslabs, n_cslabs;
};
inline GbTile gb_tile(int nb_steps, int ldp) {
    GbTile g;
    g.cw = ldp < GB_MAX_COLS ? ldp : GB_MAX_COLS;
    const int max_rows = (GB_LDS_BUDGET - GB_HDR) / (g.cw * 4);  // >= 1: GB_MAX_COLS * 4 = 64 KiB
    g.n_rslabs = cdiv(nb_steps, max_rows);
    g.rows = cdiv(nb_steps, g.n_rslabs);  // equal slabs: 100 rows of 704 columns -> 4 x 25, 250 -> 9 x 28
    g.n_rslabs = cdiv(nb_steps, g.rows);
    g.n_cslabs = cdiv(ldp, g.cw);
    return g;
}

__device__ __forceinline__ float gb_time(const float* t, long long i) { return t[i]; }
__device__ __forceinline__ float gb_time(const _Float16* t, long long i) { return (float)t[i]; }   // exact

__device__ __forceinline__ unsigned gb_bf16(unsigned count) { return __float_as_uint((float)count) >> 16; }

// n elements of the tile -> n contiguous output elements at dst (aligned to sizeof(T) only): scalar stores up to
// the first 16-byte boundary, 16-byte stores, scalar stores behind the last one.  Element e of the segment is
// tile[(e / width) * cw + e % width].
template <typename T>
__device__ __forceinline__ void gb_store_segment(const unsigned* tile, int cw, int width, int n, T* dst) {
    constexpr int V = 16 / (int)sizeof(T);
    auto value = [](unsigned c) -> T {
        if constexpr (sizeof(T) == 1) return (T)(c < 255u ? c : 255u); else return (T)c;
    };
    const int mis = (int)((reinterpret_cast<uintptr_t>(dst) & 15u) / sizeof(T));
    const int head = min((V - mis) % V, n);
    const int nv = (n - head) / V;
    const int tail0 = head + nv * V;
    const int tid = threadIdx.x;
    if (tid < head) dst[tid] = value(tile[(tid / width) * cw + tid % width]);
    if (tid < n - tail0) {
        const int e = tail0 + tid;
        dst[e] = value(tile[(e / width) * cw + e % width]);
    }
    for (int v = tid; v < nv; v += GB_NT) {
        const int e = head + v * V;
        int row = e / width, col = e - row * width;
        T vals[V] __attribute__((aligned(16)));
#pragma unroll
        for (int j = 0; j < V; ++j) {
            vals[j] = value(tile[row * cw + col]);
            if (++col == width) { col = 0; ++row; }
        }
        *reinterpret_cast<uint4*>(dst + e) = *reinterpret_cast<const uint4*>(vals);
    }
}

// ---- per-sample augmentation of the events in front of event_bin (sparch_events_gather_bin_aug).  GbPlain is the
// unaugmented kernel: every `if constexpr (kAug)` below falls away and its code is what it was.  GbAugment carries
// the table; a workgroup reads the row of its batch row once.  With a > 0 the transformed time is a non-decreasing
// function of t (one fp32 product, one fp32 sum: both monotone), so a sorted sample stays sorted and the search
// keeps working on the transformed times.
struct GbPlain {};
struct GbAugment {
    const float* table;   // (batch, SPARCH_EVAUG_FIELDS) fp32
    uint64_t seed;
};
struct GbAugRow {
    int d;
    float a, c, p, m0, m1, k0, k1;
    uint64_t seed, row;
    __device__ __forceinline__ GbAugRow(const GbAugment& g, int b) : seed(g.seed), row((uint64_t)(uint32_t)b << 32) {
        const float* r = g.table + (size_t)b * SPARCH_EVAUG_FIELDS;
        d = (int)fminf(fmaxf(r[0], -65536.0f), 65536.0f);   // the host checks |d| <= 65535; a bad row stays harmless
        a = r[1]; c = r[2]; p = r[3]; m0 = r[4]; m1 = r[5]; k0 = r[6]; k1 = r[7];
    }
    // two roundings, never an FMA: restatable with any fp32 arithmetic
    __device__ __forceinline__ float time(float t) const { return __fadd_rn(__fmul_rn(a, t), c); }
    // event j of the sample, stored unit u, transformed time tp: is it removed before binning?  The stored marker
    // 0xFFFF, the drop draw (the dropout hash of common.h on (seed, row b : position j), removed iff uniform < p),
    // the time mask on tp and the unit band on u + d (|u + d| < 2^18: exact as a float).
    __device__ __forceinline__ bool removed(int u, uint32_t j, float tp) const {
        const float up = (float)(u + d);
        // (p is the same for the whole workgroup: no draw is computed for a row that drops nothing)
        return u == 0xFFFF || (p > 0.0f && keep_scale(seed, row | j, p, 1.0f) == 0.0f) || (tp >= m0 && tp < m1) ||
               (up >= k0 && up < k1);
    }
};

template <typename TT, typename AUG>
__global__ __launch_bounds__(GB_NT) void gather_bin_kernel(
    const TT* __restrict__ times, const uint16_t* __restrict__ units, const long long* __restrict__ offsets,
    const long long* __restrict__ labels, long long n_store, const long long* __restrict__ idx, int nb_steps,
    int nb_units, int ldp, double max_time, int sorted, GbTile g, uint16_t* __restrict__ plane,
    float* __restrict__ dense, uint8_t* __restrict__ counts, long long* __restrict__ y,
    unsigned* __restrict__ partial, AUG aug) {
    constexpr bool kAug = !std::is_same<AUG, GbPlain>::value;
    extern __shared__ __attribute__((aligned(16))) unsigned gb_lds[];
    unsigned* const tile = gb_lds + GB_HDR / 4;
    const int tid = threadIdx.x;
    const int per_sample = g.n_rslabs * g.n_cslabs;
    const int b = (int)(blockIdx.x / (unsigned)per_sample);
    const int rem = (int)(blockIdx.x - (unsigned)b * (unsigned)per_sample);
    const int rs = rem / g.n_cslabs, cs = rem - rs * g.n_cslabs;
    const int r0 = rs * g.rows, r1 = min(r0 + g.rows, nb_steps);
    const int c0 = cs * g.cw, c1 = min(c0 + g.cw, ldp);
    const int cw = c1 - c0;                      // pitch of the tile in LDS
    const bool last = rs == g.n_rslabs - 1;

    const BinEdges edges(nb_steps, max_time);
    const long long s = idx[b];
    const bool valid = s >= 0 && s < n_store;    // an index outside the store: an empty sample, label -1
    const long long e0 = valid ? offsets[s] : 0, e1 = valid ? offsets[s + 1] : 0;
    if (y && rem == 0 && tid == 0) y[b] = valid ? labels[s] : -1;
    const auto xf = [&] { if constexpr (kAug) return GbAugRow(aug, b); else return GbPlain(); }();
    auto time_at = [&](long long i) {
        if constexpr (kAug) return xf.time(gb_time(times, i)); else return gb_time(times, i);
    };

    {   // zero the header and the tile
        const int n4 = (GB_HDR + (r1 - r0) * cw * 4) / 16;   // cw % 8 == 0
        uint4* z = reinterpret_cast<uint4*>(gb_lds);
        for (int i = tid; i < n4; i += GB_NT) z[i] = make_uint4(0u, 0u, 0u, 0u);
    }

    long long ea = e0, eb = e1;
    if (sorted) {
        // first event with bin >= r0 (q = 0) and first with bin >= r1 (q = 1); the first slab starts at e0 (t < 0
        // has bin 0) and the last one ends at e1 (bin == nb_steps: dropped there)
        long long lo[2] = {e0, last ? e1 : e0}, hi[2] = {rs > 0 ? e1 : e0, e1};
        const int target[2] = {r0, r1};
        while (lo[0] < hi[0] || lo[1] < hi[1]) {
            long long stride[2];
            bool below[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const long long n = hi[q] - lo[q];
                stride[q] = (n + GB_NT - 1) / GB_NT;
                const long long p = lo[q] + (long long)(tid + 1) * stride[q] - 1;
                below[q] = n > 0 && p < hi[q] && event_bin(time_at(p), edges) < target[q];
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const long long c = __syncthreads_count(below[q]);   // the predicate is monotone: c = first "not below"
                if (hi[q] > lo[q]) {
                    const long long nlo = lo[q] + c * stride[q], nhi = lo[q] + (c + 1) * stride[q] - 1;
                    hi[q] = nhi < hi[q] ? nhi : hi[q];
                    lo[q] = nlo < hi[q] ? nlo : hi[q];
                }
            }
        }
        ea = lo[0];
        eb = lo[1];
    }
    __syncthreads();

    unsigned dropped = 0;
    // GB_UNROLL events per thread and trip, every load issued before the first use: one memory latency per trip
    // (the slab of a short utterance's first rows holds most of its sample, so this loop is the long pole)
    for (long long base = ea; base < eb; base += (long long)GB_NT * GB_UNROLL) {
        float t[GB_UNROLL];
        int u[GB_UNROLL];
#pragma unroll
        for (int j = 0; j < GB_UNROLL; ++j) {
            const long long i = base + j * GB_NT + tid;
            t[j] = i < eb ? time_at(i) : -1.0f;
            u[j] = i < eb ? (int)units[i] : -1;
        }
#pragma unroll
        for (int j = 0; j < GB_UNROLL; ++j) {
            if (base + j * GB_NT + tid >= eb) continue;
            const int bin = event_bin(t[j], edges);
            if (bin < r0 || (bin >= r1 && !last)) continue;   // another row slab's event
            bool gone = false;
            if constexpr (kAug) {
                gone = xf.removed(u[j], (uint32_t)(base + j * GB_NT + tid - e0), t[j]);
                u[j] += xf.d;
            }
            if (gone || event_dropped(t[j], bin, u[j], nb_steps, nb_units)) {
                dropped += cs == 0 ? 1u : 0u;
                continue;
            }
            if (u[j] >= c0 && u[j] < c1) atomicAdd(&tile[(bin - r0) * cw + (u[j] - c0)], 1u);
        }
    }
    if (partial && dropped) atomicAdd(&gb_lds[0], dropped);
    __syncthreads();
    if (partial && tid == 0) partial[blockIdx.x] = gb_lds[0];

    const int rows = r1 - r0;
    const long long row_base = (long long)b * nb_steps + r0;
    if (plane) {
        // the tile IS the plane's image (pitch cw = the plane's pitch, or one row of a column slab; the columns
        // behind nb_units were zeroed and never added to): 8 counters -> 8 bf16 -> one 16-byte store
        uint4* dst = reinterpret_cast<uint4*>(plane + row_base * ldp + c0);
        const uint4* src = reinterpret_cast<const uint4*>(tile);
        const int nv = rows * cw / 8;
        for (int v = tid; v < nv; v += GB_NT) {
            const uint4 a = src[2 * v], c = src[2 * v + 1];
            dst[v] = make_uint4(gb_bf16(a.x) | gb_bf16(a.y) << 16, gb_bf16(a.z) | gb_bf16(a.w) << 16,
                                gb_bf16(c.x) | gb_bf16(c.y) << 16, gb_bf16(c.z) | gb_bf16(c.w) << 16);
        }
    }
    if (c0 < nb_units) {
        // dense / byte outputs have rows of nb_units elements: all rows of a full-width tile are one contiguous
        // run; a column slab (one row high) is a piece of one row
        const bool full = g.n_cslabs == 1;
        const int width = full ? nb_units : min(c1, nb_units) - c0;
        const int n = (full ? rows : 1) * width;   // at most the tile: < 2^15
        const long long at = row_base * nb_units + c0;
        if (dense) gb_store_segment<float>(tile, cw, width, n, dense + at);
        if (counts) gb_store_segment<uint8_t>(tile, cw, width, n, counts + at);
    }
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const unsigned* __restrict__ partial, int n,
                                                           unsigned* __restrict__ total) {
    __shared__ unsigned acc;
    if (threadIdx.x == 0) acc = 0;
    __syncthreads();
    unsigned v = 0;
    for (int i = threadIdx.x; i < n; i += 256) v += partial[i];
    if (v) atomicAdd(&acc, v);   // LDS
    __syncthreads();
    if (threadIdx.x == 0) *total = acc;
}

template <typename TT, typename AUG>
int gb_launch(const void* times, const uint16_t* units, const long long* offsets, const long long* labels,
              long long n_store, const long long* idx, int batch, int nb_steps, int nb_units, int ldp, double max_time,
              int sorted, const GbTile& g, uint16_t* plane, float* dense, uint8_t* counts, long long* y,
              unsigned* partial, AUG aug, hipStream_t st) {
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(gather_bin_kernel<TT, AUG>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, GB_LDS_BUDGET);
    if (attr != hipSuccess) { sparch_note_hip_error((int)attr); return SPARCH_ELAUNCH; }
    const size_t lds = (size_t)GB_HDR + (size_t)g.rows * g.cw * 4;
    const unsigned grid = (unsigned)batch * (unsigned)(g.n_rslabs * g.n_cslabs);
    hipLaunchKernelGGL((gather_bin_kernel<TT, AUG>), dim3(grid), dim3(GB_NT), lds, st, static_cast<const TT*>(times), units,
                       offsets, labels, n_store, idx, nb_steps, nb_units, ldp, max_time, sorted, g, plane, dense,
                       counts, y, partial, aug);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

}  // namespace

extern "C" int sparch_expand_counts_u8(long long M, int K, const uint8_t* counts, uint16_t* plane, int ldp,
                                       float* x, int ldx, void* stream) {
    SPARCH_ENTER();
    if (M <= 0 || K <= 0 || !counts || !plane || ldp < K || (ldp % 8) != 0 || (x && ldx < K)) return SPARCH_EINVAL;
    if (!aligned16(plane)) return SPARCH_EALIGN;
    const long long n = M * (long long)ldp;
    const unsigned grid = (unsigned)((n + 256 * 8 - 1) / (256 * 8) < 65535 * 16 ? (n + 256 * 8 - 1) / (256 * 8) : 65535 * 16);
    hipLaunchKernelGGL(expand_counts_kernel, dim3(grid ? grid : 1), dim3(256), 0, (hipStream_t)stream, M, K, counts,
                       plane, ldp, x, ldx);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

extern "C" int sparch_bin_events(long long n_events, const float* times, const int* units,
                                 const long long* sample_offsets, int n_samples, int nb_steps, int nb_units,
                                 double max_time, float* out, uint32_t* n_dropped, void* stream) {
    SPARCH_ENTER();
    if (n_events < 0 || n_samples <= 0 || nb_steps < 2 || nb_units <= 0 || !(max_time > 0.0) || !sample_offsets ||
        !out || !n_dropped || (n_events > 0 && (!times || !units)))
        return SPARCH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, (size_t)n_samples * nb_steps * nb_units * sizeof(float), st) != hipSuccess)
        return SPARCH_ELAUNCH;
    if (hipMemsetAsync(n_dropped, 0, sizeof(uint32_t), st) != hipSuccess) return SPARCH_ELAUNCH;
    if (n_events == 0) return SPARCH_OK;
    hipLaunchKernelGGL(bin_events_kernel, dim3((unsigned)((n_events + 255) / 256)), dim3(256), 0, st, n_events,
                       times, units, sample_offsets, n_samples, nb_steps, nb_units, max_time, out, n_dropped);
    SPARCH_CHECK_LAUNCH();
    return SPARCH_OK;
}

static bool gb_shape_ok(int batch, int nb_steps, int nb_units) {
    return batch > 0 && nb_steps >= 2 && nb_units > 0 && nb_units <= 65535;
}

extern "C" size_t sparch_events_gather_bin_workspace_bytes(int batch, int nb_steps, int nb_units) {
    if (!gb_shape_ok(batch, nb_steps, nb_units)) return 0;
    const GbTile g = gb_tile(nb_steps, (nb_units + 7) / 8 * 8);
    return (size_t)batch * g.n_rslabs * g.n_cslabs * sizeof(uint32_t);
}

template <typename AUG>
static int gb_entry(const void* times, int times_dtype, const uint16_t* units, const long long* offsets,
                    const long long* labels, long long n_store, const long long* idx, int batch, int nb_steps,
                    int nb_units, double max_time, int sorted, uint16_t* plane, float* dense, uint8_t* counts,
                    long long* y, uint32_t* n_dropped, void* workspace, size_t workspace_bytes, AUG aug,
                    void* stream) {
    if (!gb_shape_ok(batch, nb_steps, nb_units) || !(max_time > 0.0) || (times_dtype != 0 && times_dtype != 1) ||
        n_store <= 0 || !times || !units || !offsets || !idx || (y && !labels) || (!plane && !dense && !counts))
        return SPARCH_EINVAL;
    const int ldp = (nb_units + 7) / 8 * 8;
    const GbTile g = gb_tile(nb_steps, ldp);
    const long long n_wg = (long long)batch * g.n_rslabs * g.n_cslabs;
    if (n_wg > 0x7fffffffLL) return SPARCH_EINVAL;
    if (plane && !aligned16(plane)) return SPARCH_EALIGN;
    if (n_dropped && (!workspace || workspace_bytes < (size_t)n_wg * sizeof(uint32_t))) return SPARCH_EWORKSPACE;
    if (n_dropped && (reinterpret_cast<uintptr_t>(workspace) & 3u)) return SPARCH_EALIGN;
    unsigned* partial = n_dropped ? static_cast<unsigned*>(workspace) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const int rc = times_dtype == 0
        ? gb_launch<float>(times, units, offsets, labels, n_store, idx, batch, nb_steps, nb_units, ldp, max_time,
                           sorted, g, plane, dense, counts, y, partial, aug, st)
        : gb_launch<_Float16>(times, units, offsets, labels, n_store, idx, batch, nb_steps, nb_units, ldp, max_time,
                              sorted, g, plane, dense, counts, y, partial, aug, st);
    if (rc != SPARCH_OK) return rc;
    if (n_dropped) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, st, partial, (int)n_wg, n_dropped);
        SPARCH_CHECK_LAUNCH();
    }
    return SPARCH_OK;
}

extern "C" int sparch_events_gather_bin(const void* times, int times_dtype, const uint16_t* units,
                                        const long long* offsets, const long long* labels, long long n_store,
                                        const long long* idx, int batch, int nb_steps, int nb_units, double max_time,
                                        int sorted, uint16_t* plane, float* dense, uint8_t* counts, long long* y,
                                        uint32_t* n_dropped, void* workspace, size_t workspace_bytes, void* stream) {
    SPARCH_ENTER();
    return gb_entry(times, times_dtype, units, offsets, labels, n_store, idx, batch, nb_steps, nb_units, max_time,
                    sorted, plane, dense, counts, y, n_dropped, workspace, workspace_bytes, GbPlain(), stream);
}

extern "C" int sparch_events_gather_bin_aug(const void* times, int times_dtype, const uint16_t* units,
                                            const long long* offsets, const long long* labels, long long n_store,
                                            const long long* idx, int batch, int nb_steps, int nb_units,
                                            double max_time, int sorted, uint16_t* plane, float* dense,
                                            uint8_t* counts, long long* y, uint32_t* n_dropped, void* workspace,
                                            size_t workspace_bytes, const float* aug, uint64_t seed, void* stream) {
    SPARCH_ENTER();
    if (!aug) return SPARCH_EINVAL;
    return gb_entry(times, times_dtype, units, offsets, labels, n_store, idx, batch, nb_steps, nb_units, max_time,
                    sorted, plane, dense, counts, y, n_dropped, workspace, workspace_bytes, GbAugment{aug, seed},
                    stream);
}

/*
 * sparch_hip.h — C ABI of libsparch_hip.so, the MI355X (gfx950) implementation of
 * sparch's recurrent spiking-layer training path.
 *
 * The reference (thebarnable/sparch) has NO native/FFI interface: its hot path is
 * eager PyTorch inside Python `for t in range(T)` loops.  Each entry point below
 * therefore replaces a *group of eager ops* of the reference, cited as
 * snns.py:LINE (= /root/reference/sparch/models/snns.py) or exp.py:LINE.  The
 * Python binding a maintainer adds is a ctypes stub; ours lives in
 * sparch_amd/_capi.py.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocator);
 *     the library never allocates, frees, copies to host or synchronises;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*);
 *   - tensors are fp32, dense, row-major; (B,T,H) means b-major, h contiguous;
 *   - return value: 0 = SPARCH_OK, negative = error (nothing was launched);
 *     sparch_strerror() maps codes to text.  Python maps them to ValueError /
 *     RuntimeError, the reference's error convention;
 *   - re-entrant per stream; no global mutable state.
 *
 * "kind" of a spiking cell: 0 LIF, 1 adLIF, 2 RLIF, 3 RadLIF
 *   bit0 = adaptive (w state, beta/a/b), bit1 = recurrent (V).
 */
#ifndef SPARCH_HIP_H
#define SPARCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#define SPARCH_SEED_IN_MEMORY (1ull << 63)

#ifdef __cplusplus
extern "C" {
#endif

#define SPARCH_OK 0
#define SPARCH_EINVAL (-1)      /* bad shape / null pointer / unsupported size        */
#define SPARCH_EALIGN (-2)      /* a pointer that MUST be 16-byte aligned is not (see below) */
#define SPARCH_EWORKSPACE (-3)  /* workspace too small (see *_workspace_bytes)        */
#define SPARCH_ELAUNCH (-4)     /* HIP reported a launch error                        */
#define SPARCH_ETIMEOUT (-5)    /* reported through a status word: in-kernel wait gave up */

/* Alignment and leading dimensions (pinned by tests/test_gemm_layouts_gpu.py).
 *   - The matrix products of G1 (every sparch_gemm*) take ANY pointer alignment and any leading dimension >= the row
 *     width (smaller: SPARCH_EINVAL), independently per operand; none of them returns SPARCH_EALIGN.  An operand
 *     whose base is 16-byte aligned and whose ld is a multiple of 16 bytes (ld % 4 == 0 for fp32, ld % 8 == 0 for a
 *     uint16 plane) is staged with 16-byte loads — also when its row width is not (the tail of a row is then read
 *     element by element; nothing behind the row's last element is read) — any other operand with scalar loads: same
 *     results, slower.  The pipelined kernels additionally need whole tiles and K % 32 == 0; pre-split planes
 *     (_wp / _pp / _ap) are read only where those kernels apply and share the fp32 operand's ld, plane p of an R-row
 *     operand starting p * R * ld elements behind the first.  C is written in columns 0..N-1 of each row only.
 *   - SPARCH_EALIGN is returned (and nothing launched) by sparch_split3 (x, planes), sparch_plane_bf16_exact and
 *     sparch_expand_counts_u8 (plane; an ldp that is not a multiple of 8 is SPARCH_EINVAL), and by the element-wise /
 *     scan kernels of G2-G7 and f-4 for their tensor arguments (cell, norm, act, softmax_sum entry points).
 *   - A workspace smaller than its query: SPARCH_EWORKSPACE, nothing launched. */

/* The status word of a device: FOUR uint32 the caller keeps zeroed.  [0] != 0: an in-kernel wait of a persistent
 * recurrent launch gave up (SPARCH_ETIMEOUT) and the results of that training step are invalid;
 * [1] the number of optimizer steps sparch_adam_step skipped while [0] was raised; [2] which kernel raised it
 * (SPARCH_STATUS_*); [3] the time step, in processing order, it gave up at (0xFFFFFFFF: not recorded). */
#define SPARCH_STATUS_WORDS 4
#define SPARCH_STATUS_REC_FWD 1
#define SPARCH_STATUS_REC_BWD 2
#define SPARCH_STATUS_ANN_REC_FWD 3
#define SPARCH_STATUS_ANN_REC_BWD 4
#define SPARCH_STATUS_LIGRU_FWD 5
#define SPARCH_STATUS_LIGRU_BWD 6
#define SPARCH_STATUS_GRU_FWD 7
#define SPARCH_STATUS_GRU_BWD 8

#define SPARCH_KIND_LIF 0
#define SPARCH_KIND_ADLIF 1
#define SPARCH_KIND_RLIF 2
#define SPARCH_KIND_RADLIF 3

/* The surrogate gradient of the spike function, gate(ds, x) with x = u_t - theta in fp32 (the difference the spike
 * decision uses) and a scale k > 0.  The forward pass does not depend on it.
 *   BOXCAR        the reference's (snns.py:31-36): ds where -0.5 < x <= 0.5, else 0 (assignment); takes no scale
 *   TRIANGLE      ds * max(0, 1 - k*|x|)              area 1/k
 *   FAST_SIGMOID  ds / ((1 + k*|x|) * (1 + k*|x|))    area 2/k
 *   ATAN          ds / (1 + (k*x)*(k*x))              area pi/k
 * The smooth forms are plain fp32 products and correctly rounded quotients in this operation order; a NaN in ds or x
 * propagates.  They read u continuously and therefore need fp32 saves (save_bf16 = 0).                            */
#define SPARCH_SURROGATE_BOXCAR 0
#define SPARCH_SURROGATE_TRIANGLE 1
#define SPARCH_SURROGATE_FAST_SIGMOID 2
#define SPARCH_SURROGATE_ATAN 3

int sparch_abi_version(void);
const char* sparch_strerror(int code);
/* Text of the HIP error behind the calling thread's most recent SPARCH_ELAUNCH. */
const char* sparch_last_hip_error(void);
/* Number of compute units / XCDs the library sizes its persistent grids for. */
int sparch_device_cus(void);

/* Operand precision of a matrix product: the `precision` argument — the last one — of every entry point that
 * multiplies (the split GEMMs below, the V packs, the recurrent cells' s_{t-1} @ V / dWx_{t+1} @ V^T, G3/G4).  The
 * reference has no such choice (it is fp32-only: snns.py:29 casts the spikes to float and snns.py:572 then requires
 * a float V); BASELINE.json configs[4] names a bf16 run.
 *   SPARCH_PRECISION_FP32_EXACT: fp32 operands split exactly into bf16 planes, exact products, fp32 accumulation —
 *       fp32 results.
 *   SPARCH_PRECISION_BF16: every fp32 operand is rounded ONCE to bf16 (nearest-even) as it is staged, one bf16
 *       MFMA per product, fp32 accumulation; states, statistics, outputs and parameter updates stay fp32.
 *       Spike operands (0 / 1) and bf16-representable weights lose nothing: a network whose weights are
 *       bf16-exact has a bit-identical forward pass in both modes.
 * Per call (ABI v5): the library keeps no precision state — rounds 1-2 had a process-wide
 * sparch_set_operand_precision().  A V pack must be consumed by cell calls of the precision it was made with; a
 * *_workspace_bytes query takes the precision of the call it sizes.  Unknown value: SPARCH_EINVAL (0 bytes). */
#define SPARCH_PRECISION_FP32_EXACT 0
#define SPARCH_PRECISION_BF16 1

/* ------------------------------------------------------------------------------------
 * G1  feed-forward projection  (replaces `self.W(x)` = nn.Linear, snns.py:261/398/533/675/796,
 *     and its autograd backward).  Hand-written fp32 MFMA (v_mfma_f32_32x32x2_f32) GEMMs.
 * ---------------------------------------------------------------------------------- */

/* C[M,N] = A[M,K] * B[N,K]^T (+ bias[N]).  Optional fused column statistics for
 * BatchNorm: if colstat_ws != NULL it receives per-row-tile partial sums
 * (2 * ceil(M/128) * N floats: [tile][N] sums then [tile][N] sums of squares) of the
 * values written to C, to be finished by sparch_bn_finalize().                       */
int sparch_gemm_nt(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                   float* C, int ldc, const float* bias, float* colstat_ws, void* stream);

/* C[M,N] = A[M,K] * B[K,N]          (dX = dWx * W; rec0 = s0 * Vmasked)            */
int sparch_gemm_nn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                   float* C, int ldc, void* stream);

/* C[M,N] = A[K,M]^T * B[K,N], contraction over the long K axis (dW = dWx^T * x,
 * dV = s_prev^T * dWx).  Split-K over `splits` slabs held in `ws`
 * (sparch_gemm_tn_workspace_bytes), reduced in fixed order => bitwise reproducible.  */
size_t sparch_gemm_tn_workspace_bytes(int M, int N, int K);
int sparch_gemm_tn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                   float* C, int ldc, int zero_diag, int accumulate /* C += */, void* ws,
                   size_t ws_bytes, void* stream);

/* The same products when one operand is a spike tensor (entries 0 or one constant c, as produced
 * by the cell kernels: c = 1/(1-p_drop)): the spike operand is used as (x != 0) in bf16, the fp32
 * operand is split exactly into three bf16 planes, products are exact on the bf16 MFMA with fp32
 * accumulation, and `scale` (= c) is applied once in the epilogue.
 *   spike_nt: C[M,N] = scale * spike(A)[M,K] * B[N,K]^T (+bias) (+BatchNorm column statistics)
 *   spike_tn: C[M,N] (+)= scale * A[K,M]^T * B[K,N], spike_side 0: A is the spike operand, 1: B. */
int sparch_gemm_spike_nt(int M, int N, int K, const float* A_spk, int lda, float scale,
                         const float* B, int ldb, float* C, int ldc, const float* bias,
                         float* colstat_ws, void* stream, int precision);
size_t sparch_gemm_spike_tn_workspace_bytes(int M, int N, int K, int precision);

/* The same products with the spike operand given as a bf16 PLANE (uint16 bit patterns, entries 0 or
 * 0x3F80 = 1.0; any bf16 value is taken as is): the cell kernels write this plane next to their fp32
 * output (s16 below), and the GEMMs then pull half the operand bytes.  lda / ldb of the plane are in
 * elements.  spike16_tn: the operand named by spike_side is the uint16 plane, the other one fp32;
 * workspace as sparch_gemm_spike_tn_workspace_bytes.                                               */
int sparch_gemm_spike16_nt(int M, int N, int K, const uint16_t* A_spk16, int lda, float scale,
                           const float* B, int ldb, float* C, int ldc, const float* bias,
                           float* colstat_ws, void* stream, int precision);
int sparch_gemm_spike16_tn(int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                           int spike_side, float scale, float* C, int ldc, int zero_diag,
                           int accumulate, void* ws, size_t ws_bytes, void* stream, int precision);

/* Dense x dense products on the same exact-split machinery: BOTH fp32 operands are split into three
 * bf16 planes and the six largest cross terms are accumulated in fp32 (the rest measures ~1e-8 of
 * sum|a||b|, below an fp32 sgemm's own rounding): fp32-faithful results at 6/16 of the fp32-MFMA cost.  Same argument meaning as
 * sparch_gemm_nt / _nn / _tn (the tn workspace is sparch_gemm_spike_tn_workspace_bytes).          */
/* Split-K forms for small M*N with a long K (per-step recurrent products of the gated baselines): the
 * contraction is cut into slabs in `ws` (sparch_gemm6_splitk_workspace_bytes; 0 = not needed) and reduced in
 * fixed order.  No bias / statistics epilogue.                                                         */
size_t sparch_gemm6_splitk_workspace_bytes(int M, int N, int K, int precision);
int sparch_gemm6_nt_splitk(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                           float* C, int ldc, void* ws, size_t ws_bytes, void* stream, int precision);
int sparch_gemm6_nn_splitk(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                           float* C, int ldc, void* ws, size_t ws_bytes, void* stream, int precision);
int sparch_gemm6_nt(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, const float* bias, float* colstat_ws, void* stream, int precision);
int sparch_gemm6_nn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, void* stream, int precision);
int sparch_gemm6_tn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                    float* C, int ldc, int zero_diag, int accumulate, void* ws, size_t ws_bytes,
                    void* stream, int precision);

/* Weight operands pre-split into their bf16 planes.  A spiking layer's W (H x K) is the B operand of its
 * projection (snns.py:261, x W^T) and of backward's dx = dWx W; both kernels would re-convert the same
 * tile of W in every workgroup that stages it (250 row tiles at B*T = 32000).  sparch_split3 writes the
 * exact truncation split x = p0 + p1 + p2 once: planes[p*n + i], bf16 bit patterns, n % 8 == 0 (else SPARCH_EINVAL),
 * x and planes 16-byte aligned (else SPARCH_EALIGN).  The _wp
 * entries take B together with those planes (same layout and ldb; B_planes may be NULL) and return the
 * same bits as sparch_gemm_spike16_nt / sparch_gemm6_nn: where the pipelined kernel applies (K % 32 == 0,
 * ldb % 8 == 0, full tiles) it copies the planes into LDS, elsewhere it converts B as before.        */
int sparch_split3(size_t n, const float* x, uint16_t* planes, void* stream);
int sparch_gemm_spike16_nt_wp(int M, int N, int K, const uint16_t* A_spk16, int lda, float scale,
                              const float* B, const uint16_t* B_planes, int ldb, float* C, int ldc,
                              const float* bias, float* colstat_ws, void* stream, int precision);
int sparch_gemm6_nn_wp(int M, int N, int K, const float* A, int lda, const float* B,
                       const uint16_t* B_planes, int ldb, float* C, int ldc, void* stream, int precision);

/* First-layer input (snns.py:261 on the network input): SHD/SSC-style binned spike counts are small
 * integers, exactly representable in bf16, but the library cannot know that on the host.
 * sparch_flag_bf16_exact sets *flag (device uint32) to 1 iff every element of x is bf16-exact — and x is 16-byte
 * aligned with n % 4 == 0: otherwise the flag is 0 without looking at x (the safe answer: the six-term kernel) —; the
 * _auto_ GEMMs then enqueue BOTH the single-plane exact kernel and the 6-term kernel, each gated on
 * the device by *flag, so exactly one runs — no host round trip.  nt: A is the flagged operand;
 * tn: B is (dW = dWx^T x).                                                                       */
int sparch_flag_bf16_exact(size_t n, const float* x, uint32_t* flag, void* stream);
int sparch_gemm_auto_nt(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, const float* bias, float* colstat_ws,
                        const uint32_t* a_exact_flag, void* stream, int precision);
int sparch_gemm_auto_tn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                        float* C, int ldc, int zero_diag, int accumulate,
                        const uint32_t* b_exact_flag, void* ws, size_t ws_bytes, void* stream, int precision);
/* The same with the flagged operand's bf16 plane made by the check itself: sparch_plane_bf16_exact writes
 * plane[m][k] = upper 16 bits of x[m][k] (the exact value whenever the flag stays 1; rows of ldp >= K elements,
 * ldp % 8 == 0, ALL ldp columns of a row are written, K.. with zeros; plane 16-byte aligned, x and ldx >= K free) in the pass that computes the flag, and the _auto16_ GEMMs read that plane
 * (2 bytes per element through the spike-plane kernels) when *flag == 1, the fp32 operand through the six-term
 * kernels otherwise.  One pass over the network input per step instead of three. */
int sparch_plane_bf16_exact(int M, int K, const float* x, int ldx, uint16_t* plane, int ldp, uint32_t* flag,
                            void* stream);
int sparch_gemm_auto16_nt(int M, int N, int K, const float* A, int lda, const uint16_t* A16, int lda16,
                          const float* B, int ldb, float* C, int ldc, const float* bias, float* colstat_ws,
                          const uint32_t* a_exact_flag, void* stream, int precision);
int sparch_gemm_auto16_tn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                          const uint16_t* B16, int ldb16, float* C, int ldc, int zero_diag, int accumulate,
                          const uint32_t* b_exact_flag, void* ws, size_t ws_bytes, void* stream, int precision);
int sparch_gemm_spike_tn(int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                         int spike_side, float scale, float* C, int ldc, int zero_diag,
                         int accumulate, void* ws, size_t ws_bytes, void* stream, int precision);

/* ------------------------------------------------------------------------------------
 * G2  normalisation on the (M = B*T, H) view  (replaces nn.BatchNorm1d(momentum=0.05) /
 *     nn.LayerNorm, snns.py:240-243, 264-266).  BatchNorm is folded into a per-column
 *     (scale, shift) that the cell kernels apply on load.
 * ---------------------------------------------------------------------------------- */

/* Train: finish the statistics from colstat_ws (n_tiles partial rows, count = M rows,
 * `dup` = 2 when a bidirectional layer sees every row twice: running_var uses
 * n = dup*M), write scale = gamma*invstd, shift = beta - mean*scale, save mean/invstd,
 * update running stats in place (momentum m, unbiased variance) — unless the device word
 * skip_if_nonzero (nullable; the recurrent kernels' status word) is non-zero.
 * num_batches_tracked (nullable, ABI v5): BatchNorm1d's int64 counter, incremented by the same launch under the
 * same guard (the reference's `norm(...)` call does it, snns.py:264; a separate host-side `+= 1` was one more
 * kernel per layer and advanced on skipped steps too).
 * Training needs dup*M >= 2 values per column (the unbiased variance divides by n - 1; nn.BatchNorm1d raises for a
 * single value per channel): dup*M < 2 is SPARCH_EINVAL, nothing launched.
 * Eval (training = 0): scale/shift from running stats; colstat_ws ignored.           */
int sparch_bn_finalize(int H, int M, int n_tiles, int dup, const float* colstat_ws,
                       const float* gamma, const float* beta, float* running_mean,
                       float* running_var, float momentum, float eps, int training,
                       float* scale, float* shift, float* save_mean, float* save_invstd,
                       const uint32_t* skip_if_nonzero, int64_t* num_batches_tracked, void* stream);

/* Statistics partials of a projection with few rows, for sparch_bn_finalize with n_tiles = 3: the fp64 column sums
 * of x and of x*x over the M rows of the contiguous (M,H) x, each as three fp32 terms (hi, mid, lo), written as
 * colstat_ws[2][3][H].  The GEMM epilogue's fp32 partials lose log2((mean^2 + var) / var) bits of the variance; these
 * lose none.  Rows that are exactly zero (the padding of a ragged batch) add nothing, as in the epilogue's.          */
int sparch_bn_colstat_exact(int M, int H, const float* x, float* colstat_ws, void* stream);

/* Column sums of dy and dy*xhat over M rows (xhat = (x-mean)*invstd), partials in ws
 * (2 * ceil(M/256) * H floats), finished into dgamma[H], dbeta[H].                   */
size_t sparch_bn_bwd_workspace_bytes(int M, int H);
int sparch_bn_bwd_reduce(int M, int H, const float* dy, const float* x, const float* mean,
                         const float* invstd, float* dgamma, float* dbeta, void* ws,
                         size_t ws_bytes, void* stream);
/* dx = scale * (dy - dbeta/M - xhat * dgamma/M), in place allowed (dx == dy).        */
int sparch_bn_bwd_apply(int M, int H, const float* dy, const float* x, const float* mean,
                        const float* invstd, const float* gamma, const float* dgamma,
                        const float* dbeta, float* dx, void* stream);

/* LayerNorm per row over the leading Hn of H columns (Hn == H normally; Hn < H: columns
 * Hn..H-1 are zero padding of a layer run at a padded width — y and dx are written 0 there
 * and they take no part in the statistics): y = (x-mu)*rstd*gamma + beta; saves mu, rstd
 * (M each).                                                                            */
int sparch_layernorm_fwd(int M, int H, int Hn, const float* x, const float* gamma, const float* beta,
                         float eps, float* y, float* mu, float* rstd, void* stream);
/* dx per row; dgamma/dbeta column sums via ws (2*ceil(M/256)*H floats).               */
int sparch_layernorm_bwd(int M, int H, int Hn, const float* dy, const float* x, const float* mu,
                         const float* rstd, const float* gamma, float* dx, float* dgamma,
                         float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * G3/G4/G6/G7  spiking cells, time loop inside the kernel  (replaces _lif_cell
 *     snns.py:282-303, _adlif_cell 419-445, _rlif_cell 554-578, _radlif_cell 696-727,
 *     SpikeFunctionBoxcar 20-36, the bidirectional flip/cat glue 252-254 / 272-275 and
 *     nn.Dropout 278, plus their autograd replay).
 *
 * Geometry: B = batch, dirs = 1 | 2 (bidirectional), Bp = B*dirs virtual rows.
 *   Wx      (B,T,H)  raw projection; the cell applies x*scale[h]+shift[h] when scale != NULL.
 *           Virtual row b' >= B reads Wx[b'-B, T-1-t] (time-flipped copy, never materialised).
 *   u0,w0,s0 (Bp,H)  random initial states drawn by the host in the reference's order.
 *   s_out   (B,T,H*dirs)  post-dropout output; direction d lands in features [d*H,(d+1)*H)
 *           at its ORIGINAL time index (un-flipped), as snns.py:272-275.  NULL => not written (ABI v5): a
 *           caller that feeds the next layer from s16_out alone saves the 4 bytes per element; at least
 *           one of s_out / s16_out must be given.
 *   s16_out (B,T,H*dirs)  the same spikes as a bf16 plane (uint16 bit patterns: 0x3F80 where
 *           s_out != 0, else 0) for sparch_gemm_spike16_*; NULL => not written.
 *   u_save, w_save (Bp,T,H) in cell time order; needed by the backward (NULL => not saved).
 *   spike_count (H*dirs) uint32: number of spikes surviving dropout per output feature;
 *           firing rate = count * keep_scale / (B*T)  (snns.py:174 after 278).
 *   Dropout: keep iff hash(seed, output element index) >= p; kept values scale by 1/(1-p).  The index is the
 *   element's position in the (B,T,H*dirs) tensor THIS launch writes: a caller that runs a layer zero-padded to a
 *   wider H gets the padded tensor's mask (restated in numpy, padding included: tests/dropout_numpy.py).
 *   `seed` (every entry point that takes one): the 63-bit seed itself, or SPARCH_SEED_IN_MEMORY | the device
 *   address of a uint64 holding it — for a step captured in a HIP graph, whose arguments are frozen.
 * ---------------------------------------------------------------------------------- */

/* Non-recurrent kinds (LIF, adLIF): one thread per (row, 4 columns), T-loop in registers. */
int sparch_cell_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                    const float* scale, const float* shift, const float* alpha,
                    const float* beta, const float* a, const float* b, const float* u0,
                    const float* w0, const float* s0, float theta, float p_drop,
                    uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                    int save_bf16, uint32_t* spike_count, void* stream);

/* Streaming inference: the same cells over one CHUNK (B,T,H) of a longer sequence, state in, state out, nothing
 * saved.  u / w / s (B,H) hold the state the previous chunk ended in (for the first chunk: the initial states) and
 * are updated in place; s is the last step's raw spikes.  Chunks of any length >= 1, fed in order, give bit for bit
 * the spikes of one call over the whole sequence: the arithmetic of a step does not know where a chunk ends.
 * One direction and no dropout (a stream is causal and runs in eval): dirs != 1, p_drop != 0, a NULL state
 * pointer or a recurrent kind are SPARCH_EINVAL.  spike_count is ADDED to (the caller owns and clears it).     */
int sparch_cell_stream_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                           const float* scale, const float* shift, const float* alpha,
                           const float* beta, const float* a, const float* b, float* u, float* w,
                           float* s, float theta, float p_drop, float* s_out, uint16_t* s16_out,
                           uint32_t* spike_count, void* stream);

/* save_bf16 (forward and backward alike): u_save / w_save are (Bp,T,H) bf16 instead of fp32 — half the bytes
 * of the two largest tensors a layer keeps for its backward pass.  The stored membrane potential is rounded
 * so that the backward's three discrete decisions (spike u-theta > 0, box-car edges) are EXACTLY the fp32
 * ones (csrc/common.h save_u16): recomputed spikes never flip, dWx / dW / dV are unchanged, only the
 * continuous uses of u and w (dalpha, dbeta, da) carry the 2^-9 relative rounding.  The recurrent kernels
 * accept it for whole-sequence launches only (steps_per_launch >= T).
 * g_out (B,T,H*dirs) upstream gradient of s_out; g_rate (H*dirs) upstream gradient of the
 * firing rates (NULL = none).  dWx (Bp,T,H): gradient w.r.t. the normalised projection,
 * virtual-row order but ORIGINAL time index (so rows b and b+B add elementwise).
 * dparam_ws: (4,Bp,H) per-row partials of (dalpha,dbeta,da,db); finish with
 * sparch_colsum_clamped().
 * BatchNorm backward folded in (SURVEY §8 b2 `bn_dsum` / `bn_dxhat`): with bn_x = the raw projection
 * (B,T,H), bn_mean / bn_invstd (H) non-NULL the kernel also leaves sum_t dWx and sum_t dWx*xhat,
 * xhat = (x - mean)*invstd, per (row, column) in planes 4 and 5 of dparam_ws ((6,Bp,H) then): their
 * column sums are BatchNorm's dbeta / dgamma — no separate pass over dy and x.            */
int sparch_cell_bwd(int kind, int B, int dirs, int T, int H, const float* g_out,
                    const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                    const float* alpha, const float* beta, const float* a, const float* b,
                    const float* u0, const float* w0, const float* s0, float theta,
                    float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                    const float* bn_mean, const float* bn_invstd, void* stream);
/* The same with a selectable surrogate (SPARCH_SURROGATE_*); sparch_cell_bwd is surrogate = BOXCAR.  SPARCH_EINVAL,
 * before any device work, for an unknown id, for a smooth form with a scale that is not finite and > 0, and for a
 * smooth form with save_bf16 != 0.  The scale is ignored for BOXCAR.                                           */
int sparch_cell_bwd_sg(int kind, int B, int dirs, int T, int H, const float* g_out,
                       const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                       const float* alpha, const float* beta, const float* a, const float* b,
                       const float* u0, const float* w0, const float* s0, float theta,
                       float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                       const float* bn_mean, const float* bn_invstd, int surrogate, float surrogate_scale,
                       void* stream);
/* Ragged batches ("Ragged batches"): the `_len` forms of the cell and readout entry points take
 * lengths (B,) int32 on the device, 1 <= lengths[b] <= T, and n_valid = sum(lengths).  Row b then comes out as the
 * row run alone over its first lengths[b] steps would:
 *   forward : s_out / s16_out are exactly 0 for t >= lengths[b], and those steps are not counted in spike_count
 *             (the state runs on over the padding: u_save / w_save hold values there that nothing valid depends on);
 *   backward: the incoming gradient (g_out plus the rate term) counts as 0 for t >= lengths[b] — whatever g_out
 *             holds there, a NaN included — so dWx is exactly 0 there and the partial sums see valid steps only;
 *             the rate gradient is scaled by 1 / n_valid instead of 1 / (B T); `surrogate` as in the _sg forms.
 * SPARCH_EINVAL, before any device work, for dirs != 1, lengths == NULL and n_valid < 1; everything else as the
 * entry point without lengths.                                                                                  */
int sparch_cell_fwd_len(int kind, int B, int dirs, int T, int H, const float* Wx,
                        const float* scale, const float* shift, const float* alpha,
                        const float* beta, const float* a, const float* b, const float* u0,
                        const float* w0, const float* s0, float theta, float p_drop,
                        uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                        int save_bf16, uint32_t* spike_count, const int* lengths, long long n_valid,
                        void* stream);
int sparch_cell_bwd_len(int kind, int B, int dirs, int T, int H, const float* g_out,
                        const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                        const float* alpha, const float* beta, const float* a, const float* b,
                        const float* u0, const float* w0, const float* s0, float theta,
                        float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                        const float* bn_mean, const float* bn_invstd, const int* lengths, long long n_valid,
                        int surrogate, float surrogate_scale, void* stream);
/* Packed ragged batches ("Packed ragged batches"): the `_pk` forms skip the padded steps instead
 * of masking them.  The batch's B sequences are sorted by length, descending; sequence j has lengths[j] steps and owns
 * rows [offsets[j], offsets[j] + lengths[j]) of every per-step tensor, which is (N, .) with N = n_valid = offsets[B]
 * instead of (B, T, .): Wx, s_out, s16_out, u_save, w_save, g_out, dWx, bn_x.  lengths (B,) and offsets (B + 1,) are
 * int32 on the device; T is the longest length; the per-sequence tensors (u0, w0, s0, dparam_ws, out) keep B rows, in
 * the sorted order.  A sequence runs exactly its own steps: there is no padded step, no saved state behind a
 * sequence's end, and the dropout mask's element index is the position in the packed tensor.  The rate gradient is
 * scaled by 1 / n_valid.  SPARCH_EINVAL, before any device work, for dirs != 1, lengths == NULL, offsets == NULL and
 * n_valid < 1; everything else as the entry point without lengths.                                              */
int sparch_cell_fwd_pk(int kind, int B, int dirs, int T, int H, const float* Wx,
                       const float* scale, const float* shift, const float* alpha,
                       const float* beta, const float* a, const float* b, const float* u0,
                       const float* w0, const float* s0, float theta, float p_drop,
                       uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                       int save_bf16, uint32_t* spike_count, const int* lengths, const int* offsets,
                       long long n_valid, void* stream);
int sparch_cell_bwd_pk(int kind, int B, int dirs, int T, int H, const float* g_out,
                       const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                       const float* alpha, const float* beta, const float* a, const float* b,
                       const float* u0, const float* w0, const float* s0, float theta,
                       float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                       const float* bn_mean, const float* bn_invstd, const int* lengths, const int* offsets,
                       long long n_valid, int surrogate, float surrogate_scale, void* stream);
/* The row gather / scatter between a padded (B,T,C) tensor and the packed (N,C) one, for elements of elem_size = 1, 2
 * or 4 bytes (moved as raw bytes).  order (B,) int32: sequence j is batch row order[j].  sparch_pack_rows copies step
 * t < lengths[j] of batch row order[j] to packed row offsets[j] + t; sparch_unpack_rows copies it back and writes
 * zeros to every step t >= lengths[j], so every element of dst (B,T,C) is written.  SPARCH_EINVAL for a NULL pointer,
 * another element size, n_valid < 1 or n_valid > B T.                                                            */
int sparch_pack_rows(int B, int T, int C, int elem_size, const void* src, void* dst, const int* order,
                     const int* lengths, const int* offsets, long long n_valid, void* stream);
int sparch_unpack_rows(int B, int T, int C, int elem_size, const void* src, void* dst, const int* order,
                       const int* lengths, const int* offsets, long long n_valid, void* stream);
/* Bidirectional layers on ragged batches ("Bidirectional ragged batches"): the movements in front
 * of and behind the one-direction `_len` / `_pk` cell entry points, which then run on 2B sequences — sequence b is clip
 * b, sequence B + b is clip b read backwards inside its own length.  lengths (B,) int32 on the device, n_valid their sum.
 *   split     : src (B,T,C), elements of elem_size = 1, 2 or 4 bytes moved as raw bytes -> dst (2B,T,C):
 *               dst[b,t] = src[b,t], dst[B+b,t] = src[b, lengths[b]-1-t] for t < lengths[b], zeros behind: every element
 *               of dst is written.
 *   split_bwd : its adjoint, fp32: g_src[b,t] = g[b,t] + g[B+b, lengths[b]-1-t] (one fp32 sum), 0 for t >= lengths[b].
 *   join      : s16 (2B,T,H) bf16 0/1 plane -> y16 (B,T,2H): y16[b,t,:H] = s16[b,t], y16[b,t,H:] = s16[B+b,
 *               lengths[b]-1-t], zeros behind; y32 (B,T,2H) fp32 or NULL: the same values times `scale`; the non-zero
 *               values of every output column are ADDED to spike_count (2H,) (the caller owns and clears it; integer
 *               atomics: the result does not depend on the order).
 *   join_bwd  : its adjoint: g2[b,t] = g[b,t,:H] + r, g2[B+b, lengths[b]-1-t] = g[b,t,H:] + r with r =
 *               g_rate[column] * rate_scale (g_rate (2H,) or NULL: r = 0; one fp32 product and one fp32 sum), 0 on the
 *               tails of g2 (2B,T,H): every element is written.
 * The `_pk` forms: the single tensors are packed (n_valid, .) by lengths (sorted descending) and offsets (B + 1,), as
 * sparch_pack_rows makes them, T is the longest length; the doubled tensors have 2 n_valid rows, and fwd / rev (B,) int32
 * hold, per sequence, the first row of its forward and of its reversed copy there.  There are no tails.
 * SPARCH_EINVAL, before any device work: B, T, C / H < 1, a NULL pointer (y32 and g_rate may be NULL), n_valid < 1 or
 * > B T, an element size other than 1, 2, 4.  Then SPARCH_EALIGN: a pointer that is not aligned to its element.  Rows
 * move in the widest pieces (16, 4, 2, 1 bytes) that the row size and the addresses allow.                        */
int sparch_bidir_split_len(int B, int T, int C, int elem_size, const void* src, void* dst, const int* lengths,
                           long long n_valid, void* stream);
int sparch_bidir_split_pk(int B, int T, int C, int elem_size, const void* src, void* dst, const int* lengths,
                          const int* offsets, const int* fwd, const int* rev, long long n_valid, void* stream);
int sparch_bidir_split_bwd_len(int B, int T, int C, const float* g, float* g_src, const int* lengths,
                               long long n_valid, void* stream);
int sparch_bidir_split_bwd_pk(int B, int T, int C, const float* g, float* g_src, const int* lengths,
                              const int* offsets, const int* fwd, const int* rev, long long n_valid, void* stream);
int sparch_bidir_join_len(int B, int T, int H, const uint16_t* s16, uint16_t* y16, float* y32, float scale,
                          uint32_t* spike_count, const int* lengths, long long n_valid, void* stream);
int sparch_bidir_join_pk(int B, int T, int H, const uint16_t* s16, uint16_t* y16, float* y32, float scale,
                         uint32_t* spike_count, const int* lengths, const int* offsets, const int* fwd,
                         const int* rev, long long n_valid, void* stream);
int sparch_bidir_join_bwd_len(int B, int T, int H, const float* g, const float* g_rate, float rate_scale,
                              float* g2, const int* lengths, long long n_valid, void* stream);
int sparch_bidir_join_bwd_pk(int B, int T, int H, const float* g, const float* g_rate, float rate_scale,
                             float* g2, const int* lengths, const int* offsets, const int* fwd, const int* rev,
                             long long n_valid, void* stream);

/* Recurrent kinds (RLIF, RadLIF).  V (H,H) = V.weight; the diagonal is masked inside
 * (snns.py:566/712).  The recurrent product s_{t-1}*V runs on MFMA with the V slice of
 * each workgroup resident in registers; workgroups of one 32-row batch tile exchange
 * spikes through `chan` (tagged 8-byte granules, agent-scope write-through).
 *   vpack   prepacked V from sparch_vpack (forward: transpose=0, backward: transpose=1)
 *   rec0    (Bp,H) = s0 * Vmasked, the t=0 recurrent drive (s0 is not binary)
 *   chan    sparch_rec_chan_bytes(Bp,T,H) bytes, zeroed by the call itself
 *   status  the device's status word (SPARCH_STATUS_WORDS uint32, see above): [0] set non-zero if an in-kernel
 *           wait gave up (SPARCH_ETIMEOUT), [2] / [3] which kernel and at which step
 *   steps_per_launch: T => one persistent launch per batch-tile group; 1 => one launch
 *           per time step (no inter-workgroup waiting at all; the safe fallback).     */
size_t sparch_vpack_bytes(int H);
/* transpose: bit 0 = pack V^T, bit 1 = keep the diagonal (dense cells of the ANN baselines) */
int sparch_vpack(int H, const float* V, int transpose, float* vpack, float* vmasked,
                 void* stream, int precision);
/* The forward fragments, the backward (transposed) fragments and the masked copy in one launch (a training step
 * needs all three; vmasked may be NULL).                                                                    */
int sparch_vpack_both(int H, const float* V, float* vpack_fwd, float* vpack_bwd, float* vmasked, void* stream, int precision);
/* vmasked (H,H) = V with its diagonal zeroed (snns.py:566/712), any H */
int sparch_vmask(int H, const float* V, float* vmasked, void* stream);
/* XCD-local hand-off stores of the spiking recurrent kernels (whole-sequence launches): the workgroups of a row
 * tile establish at run time (HW_REG_XCC_ID exchanged through agent-scope accesses) that they share an XCD and
 * then hand their tiles over with plain stores, which stay in that XCD's L2; anything else keeps the
 * write-through agent-scope stores.  Same results bit for bit; on by default (SPARCH_XCD_LOCAL=0 turns it off).
 * sparch_set_xcd_local(0 / 1) overrides, -1 returns to the environment's setting; returns the previous state.  */
int sparch_set_xcd_local(int on);
size_t sparch_rec_chan_bytes(int Bp, int T, int H);
int sparch_rec_cell_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                        const float* scale, const float* shift, const float* alpha,
                        const float* beta, const float* a, const float* b,
                        const float* vpack, const float* rec0, const float* u0,
                        const float* w0, const float* s0, float theta, float p_drop,
                        uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save,
                        void* w_save, int save_bf16, uint32_t* spike_count, void* chan,
                        size_t chan_bytes, uint32_t* status, int steps_per_launch, void* stream, int precision);
/* Streaming form of sparch_rec_cell_fwd (see sparch_cell_stream_fwd): one chunk (B,T,H), no save tensors.
 *   u, w, s (B,H)     state, in place; s = the last step's raw spikes (fp32)
 *   s16_state (B,H)   the same spikes as a bf16 0/1 plane, written behind the chunk's last step
 *   rec0 (B,H)        s * Vmasked for the state the chunk starts from, by the caller: a dense product for drawn
 *                     initial states, the exact spike product on s16_state from the second chunk on
 *   chan              sparch_rec_chan_bytes(B,T,H) bytes for THIS chunk's T; steps_per_launch as above.          */
int sparch_rec_cell_stream_fwd(int kind, int B, int dirs, int T, int H, const float* Wx,
                               const float* scale, const float* shift, const float* alpha,
                               const float* beta, const float* a, const float* b,
                               const float* vpack, const float* rec0, float* u, float* w, float* s,
                               uint16_t* s16_state, float theta, float p_drop, float* s_out,
                               uint16_t* s16_out, uint32_t* spike_count, void* chan, size_t chan_bytes,
                               uint32_t* status, int steps_per_launch, void* stream, int precision);
/* Backward: each step's 32x32 dWx tile is handed to the other workgroups through `chan`.
 * s_prev16 (Bp,T,H) receives s_{t-1} as a bf16 plane (binary for t >= 1, a zero row at
 * t = 0: the non-binary s0 term is added by the caller) for dV = s_prev^T * dWx
 * (sparch_gemm_spike16_tn, spike_side 0).  dparam_ws: (6,Bp,H) = per-row partials of
 * (dalpha,dbeta,da,db) + the du / dw carries of chunked launches; with bn_x / bn_mean / bn_invstd
 * non-NULL (see sparch_cell_bwd) planes 6 and 7 receive BatchNorm's sums ((8,Bp,H) then).   */
int sparch_rec_cell_bwd(int kind, int B, int dirs, int T, int H, const float* g_out,
                        const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                        const float* alpha, const float* beta, const float* a,
                        const float* b, const float* vpack_t, const float* u0,
                        const float* w0, const float* s0, float theta, float p_drop,
                        uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                        const float* bn_x, const float* bn_mean, const float* bn_invstd,
                        void* chan, size_t chan_bytes, uint32_t* status,
                        int steps_per_launch, void* stream, int precision);
/* The same with a selectable surrogate (see sparch_cell_bwd_sg for the refusals); chunked launches carry du / dw
 * through dparam_ws exactly as the box-car's do.                                                              */
int sparch_rec_cell_bwd_sg(int kind, int B, int dirs, int T, int H, const float* g_out,
                           const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                           const float* alpha, const float* beta, const float* a,
                           const float* b, const float* vpack_t, const float* u0,
                           const float* w0, const float* s0, float theta, float p_drop,
                           uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                           const float* bn_x, const float* bn_mean, const float* bn_invstd,
                           void* chan, size_t chan_bytes, uint32_t* status,
                           int steps_per_launch, int surrogate, float surrogate_scale, void* stream, int precision);
/* The ragged forms (see sparch_cell_fwd_len): persistent and chunked steps_per_launch, both operand precisions, fp32
 * and bf16 saves (bf16 with the box-car only, as above).  The spikes the workgroups hand each other stay unmasked —
 * a row's padded steps never reach one of its valid steps.  H <= 1024 (there is no ragged per-step form).      */
int sparch_rec_cell_fwd_len(int kind, int B, int dirs, int T, int H, const float* Wx,
                            const float* scale, const float* shift, const float* alpha,
                            const float* beta, const float* a, const float* b,
                            const float* vpack, const float* rec0, const float* u0,
                            const float* w0, const float* s0, float theta, float p_drop,
                            uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save,
                            void* w_save, int save_bf16, uint32_t* spike_count, const int* lengths,
                            long long n_valid, void* chan, size_t chan_bytes, uint32_t* status,
                            int steps_per_launch, void* stream, int precision);
/* The packed forms (see sparch_cell_fwd_pk): tensors per step are (N, .), sequence j at rows offsets[j] ...; T is the
 * longest length and sizes chan (sparch_rec_chan_bytes(B, T, H)).  A 32-row tile runs to the length of its first row, its
 * longest; a shorter row's loads are clamped into its own rows and its stores end at its own length.  Whole-sequence
 * launches only: SPARCH_EINVAL for steps_per_launch < T (and where the grid cannot be co-resident), besides what the
 * `_len` forms refuse.  s_prev16 (backward) is (N, H) like dWx.                                                  */
int sparch_rec_cell_fwd_pk(int kind, int B, int dirs, int T, int H, const float* Wx,
                           const float* scale, const float* shift, const float* alpha,
                           const float* beta, const float* a, const float* b,
                           const float* vpack, const float* rec0, const float* u0,
                           const float* w0, const float* s0, float theta, float p_drop,
                           uint64_t seed, float* s_out, uint16_t* s16_out, void* u_save, void* w_save,
                           int save_bf16, uint32_t* spike_count, const int* lengths, const int* offsets,
                           long long n_valid, void* chan, size_t chan_bytes, uint32_t* status,
                           int steps_per_launch, void* stream, int precision);
int sparch_rec_cell_bwd_pk(int kind, int B, int dirs, int T, int H, const float* g_out,
                           const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                           const float* alpha, const float* beta, const float* a,
                           const float* b, const float* vpack_t, const float* u0,
                           const float* w0, const float* s0, float theta, float p_drop,
                           uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                           const float* bn_x, const float* bn_mean, const float* bn_invstd,
                           const int* lengths, const int* offsets, long long n_valid, void* chan,
                           size_t chan_bytes, uint32_t* status, int steps_per_launch, int surrogate,
                           float surrogate_scale, void* stream, int precision);
int sparch_rec_cell_bwd_len(int kind, int B, int dirs, int T, int H, const float* g_out,
                            const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                            const float* alpha, const float* beta, const float* a,
                            const float* b, const float* vpack_t, const float* u0,
                            const float* w0, const float* s0, float theta, float p_drop,
                            uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                            const float* bn_x, const float* bn_mean, const float* bn_invstd,
                            const int* lengths, long long n_valid, void* chan, size_t chan_bytes,
                            uint32_t* status, int steps_per_launch, int surrogate, float surrogate_scale,
                            void* stream, int precision);
/* ONE time step t of the same cells with the recurrent product supplied by the caller — the path for hidden
 * sizes whose V slice does not fit the persistent kernels' register-resident layout (H > 1024; the reference
 * accepts any nb_hiddens, snns.py:608-661): any grid size, nothing waits inside a launch.
 *   forward : rec (Bp,H) = s_{t-1} @ V  (t = 0: s0 @ V, V with its diagonal zeroed); the step's raw
 *             (pre-dropout) spikes also go to s_step16 (Bp,H) bf16 0/1, the operand of the next product;
 *             membrane / adaptation state is carried through u_save / w_save (row t-1 is read)
 *   backward: steps run t = T-1 ... 0; rec (Bp,H) = dWx_{t+1} @ V^T (ignored at t = T-1); the step's dWx
 *             also goes to dwx_step (Bp,H); du / dw carries and the parameter partial sums live in
 *             dparam_ws (6 planes of Bp*H) between calls.                                          */
int sparch_rec_cell_step_fwd(int kind, int B, int dirs, int T, int H, int t, const float* Wx,
                             const float* scale, const float* shift, const float* alpha,
                             const float* beta, const float* a, const float* b, const float* rec,
                             const float* u0, const float* w0, const float* s0, float theta,
                             float p_drop, uint64_t seed, float* s_out, uint16_t* s16_out,
                             float* u_save, float* w_save, uint32_t* spike_count,
                             uint16_t* s_step16, void* stream);
/* Streaming form of the forward step (H > 1024): step t of a chunk (B,T,H); u / w / s (B,H) are read and written
 * in place by every step, s16_state (B,H) receives the step's spikes (the operand of the next product, which for
 * t = 0 is the caller's product on the state the chunk starts from).  Nothing the size of the stream is kept. */
int sparch_rec_cell_step_stream_fwd(int kind, int B, int dirs, int T, int H, int t, const float* Wx,
                                    const float* scale, const float* shift, const float* alpha,
                                    const float* beta, const float* a, const float* b, const float* rec,
                                    float* u, float* w, float* s, uint16_t* s16_state, float theta,
                                    float p_drop, float* s_out, uint16_t* s16_out, uint32_t* spike_count,
                                    void* stream);
int sparch_rec_cell_step_bwd(int kind, int B, int dirs, int T, int H, int t, const float* g_out,
                             const float* g_rate, const float* u_save, const float* w_save,
                             const float* alpha, const float* beta, const float* a, const float* b,
                             const float* rec, const float* u0, const float* w0, const float* s0,
                             float theta, float p_drop, uint64_t seed, float* dWx,
                             uint16_t* s_prev16, float* dparam_ws, const float* bn_x,
                             const float* bn_mean, const float* bn_invstd, float* dwx_step, void* stream);
/* The backward step with a selectable surrogate (fp32 saves, as the step path always has). */
int sparch_rec_cell_step_bwd_sg(int kind, int B, int dirs, int T, int H, int t, const float* g_out,
                                const float* g_rate, const float* u_save, const float* w_save,
                                const float* alpha, const float* beta, const float* a, const float* b,
                                const float* rec, const float* u0, const float* w0, const float* s0,
                                float theta, float p_drop, uint64_t seed, float* dWx,
                                uint16_t* s_prev16, float* dparam_ws, const float* bn_x,
                                const float* bn_mean, const float* bn_invstd, float* dwx_step,
                                int surrogate, float surrogate_scale, void* stream);

/* Finish per-row partials: out[j][h] = sum_r ws[j][r][h], zeroed where the raw parameter
 * lies outside [lo_j, hi_j] (torch.clamp's gradient gate).  n_params <= 8; raw[j]/lim may
 * be NULL for "no clamp".                                                             */
int sparch_colsum_clamped(int n_params, int rows, int H, const float* ws,
                          const float* const* raw, const float* lim_lo_hi, float* const* out,
                          void* stream);

/* Elementwise helpers of the layer backward: out = x[0:B] + x[B:2B] (bidirectional
 * halves of dWx share their projection rows), M*H elements.                           */
int sparch_add_halves(size_t n, const float* x, float* out, void* stream);
/* Column sums out[h] = sum_m x[m][h] (bias gradient), fixed order.                    */
int sparch_colsum(int M, int H, const float* x, float* out, void* ws, size_t ws_bytes,
                  void* stream);

/* ------------------------------------------------------------------------------------
 * G5  readout cell  (replaces _readout_cell, snns.py:808-825, and its autograd replay):
 *     u_t = alpha*u + (1-alpha)*(Wx_t*scale+shift);  out += softmax(u_t).
 *     One workgroup per batch row, classes on threads (C <= 256).
 *     Backward: dalpha_ws (1,B,C) per-row partials of dalpha; with bn_x (B,T,C) / bn_mean / bn_invstd
 *     non-NULL also sum_t dWx and sum_t dWx*xhat in planes 1 and 2 ((3,B,C) then), see sparch_cell_bwd.
 * ---------------------------------------------------------------------------------- */
int sparch_readout_fwd(int B, int T, int C, const float* Wx, const float* scale,
                       const float* shift, const float* alpha, const float* u0, float* out,
                       float* u_save, void* stream);
/* Streaming form: u (B,C) is the membrane state and out (B,C) the running sum, both in place.  The accumulator is
 * carried IN, so the one sequential sum over t continues across chunks (adding per-chunk sums rounds differently):
 * out after the last chunk equals sparch_readout_fwd's over the whole sequence bit for bit.                    */
int sparch_readout_stream_fwd(int B, int T, int C, const float* Wx, const float* scale,
                              const float* shift, const float* alpha, float* u, float* out, void* stream);
/* Streaming, chunks of ONE time step: the projection and the cell of a layer in one launch (csrc/streamstep.hip),
 * one launch per layer and step instead of the chain of projection, boundary product and cell launches.
 * sparch_stream_step_fwd — one hidden layer, all B rows, any K, H, B >= 1 (rows in tiles over grid.y):
 *   x (B,K), row stride ldx   the step's input: in_dtype 0 fp32 — the network input, or the previous layer's fresh
 *                             spike state — or 1 uint8 spike counts, read as they are
 *   W (H,K), bias (H) or NULL the projection as stored; scale / shift (H) the folded eval BatchNorm, both or neither
 *   vmask_t (H,H), row stride ld   row h = column h of V with its diagonal zeroed (RLIF / RadLIF; else NULL)
 *   u, w (B,H), row stride ld      membrane / adaptation state, in place
 *   s_in (B,H)  the previous step's spikes (or a drawn real-valued s0: one code path), s_out (B,H) the new ones,
 *               both fp32 with row stride ld; s16_out (B,H) the new spikes as a bf16 0/1 plane (NULL: not wanted),
 *               so the chunk entry points above can continue from the same state.  Every workgroup of a recurrent
 *               layer reads ALL of s_in: s_out must be another buffer there (equal pointers: SPARCH_EINVAL); for
 *               LIF / adLIF they may be one.  Columns >= H of a row are never written.
 *   spike_count (H) is ADDED to (integer atomics; NULL: not counted).
 * The membrane update is the expression tree of the chunk kernels: a stream stepped here equals the chunked stream bit
 * for bit wherever the projection sums are exact (fp32 FMA chains here, in another order than the MFMA products).
 * Nothing waits inside a launch.  W, vmask_t, u, w, s_in, s_out, s16_out 16-byte aligned (else SPARCH_EALIGN).
 * sparch_stream_step_readout — Wx = x W^T (+ bias), affine, u = alpha u + (1 - alpha) Wx, out += softmax(u); u and
 * out (B,C) in place as in sparch_readout_stream_fwd, and out equal to its bit for bit on the same Wx; C <= 256.  */
int sparch_stream_step_fwd(int kind, int B, int K, int H, int ld, int in_dtype, const void* x, int ldx,
                           const float* W, const float* bias, const float* scale, const float* shift,
                           const float* alpha, const float* beta, const float* a, const float* b,
                           const float* vmask_t, float* u, float* w, const float* s_in, float* s_out,
                           uint16_t* s16_out, float theta, uint32_t* spike_count, void* stream);
int sparch_stream_step_readout(int B, int K, int C, const float* x, int ldx, const float* W, const float* bias,
                               const float* scale, const float* shift, const float* alpha, float* u, float* out,
                               void* stream);
/* The same step, EVENT-DRIVEN (csrc/streamsparse.hip): only the weights of the ACTIVE inputs (value != 0) are read,
 * about nnz * H * 4 bytes per operand and row tile instead of all of W and V.  The contracts, state buffers, strides,
 * in_dtype, error codes and alignment refusals are those of the two entry points above; the weight operands differ, so
 * that everything one input position contributes is one contiguous row:
 *   Wt (K, ldw)       W TRANSPOSED, fp32; ldw >= H (readout: ldc >= C) a multiple of 4 (else SPARCH_EINVAL), the base
 *                     16-byte aligned (else SPARCH_EALIGN)
 *   vmask (H, ld)     the masked V as sparch_vmask writes it, NOT transposed: row k = what spike k of s_in feeds
 * Per row the (k, value) pairs with value != 0 are listed in ascending k (values are kept: counts above 1, real-valued
 * features and a drawn s0 take the same path; any density up to 100 % is correct).  Hidden layer: entry p of a row's
 * list goes to partial sum p mod 4, each an fp32 FMA chain acc = fma(value, wt, acc) in ascending p, combined as
 * (p0 + p1) + (p2 + p3); readout: one chain per class over the whole list.  Leaving out a zero input removes an exact
 * +-0 from a sum that starts at +0, so only the ORDER of the non-zero terms differs from the dense step: results are
 * bit-equal to it wherever the sums are exact in any order (dyadic weights on 0/1 spikes, counts, dyadic states), and
 * within the last bits of any other fp32 order otherwise.  No float atomics: a pure function of the inputs.       */
int sparch_stream_step_sparse_fwd(int kind, int B, int K, int H, int ld, int in_dtype, const void* x, int ldx,
                                  const float* Wt, int ldw, const float* bias, const float* scale, const float* shift,
                                  const float* alpha, const float* beta, const float* a, const float* b,
                                  const float* vmask, float* u, float* w, const float* s_in, float* s_out,
                                  uint16_t* s16_out, float theta, uint32_t* spike_count, void* stream);
int sparch_stream_step_sparse_readout(int B, int K, int C, const float* x, int ldx, const float* Wt, int ldc,
                                      const float* bias, const float* scale, const float* shift, const float* alpha,
                                      float* u, float* out, void* stream);
int sparch_readout_bwd(int B, int T, int C, const float* g_out, const float* bn_x,
                       const float* bn_mean, const float* bn_invstd, const float* u_save,
                       const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                       void* stream);
/* The ragged forms (see sparch_cell_fwd_len): out[b] = sum_{t < lengths[b]} softmax(u_t) — a truncated sum, not a
 * mean — with the recurrence, the softmax and the sum bounded by the row's length (u_save is not written past it);
 * the backward starts its reverse recurrence at the row's last step and writes dWx = 0 behind it.              */
int sparch_readout_fwd_len(int B, int T, int C, const float* Wx, const float* scale,
                           const float* shift, const float* alpha, const float* u0, float* out,
                           float* u_save, const int* lengths, long long n_valid, void* stream);
int sparch_readout_bwd_len(int B, int T, int C, const float* g_out, const float* bn_x,
                           const float* bn_mean, const float* bn_invstd, const float* u_save,
                           const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                           const int* lengths, long long n_valid, void* stream);
/* The packed forms (see sparch_cell_fwd_pk): Wx, u_save, dWx and bn_x are (N,C), row b's steps at rows offsets[b] ...;
 * out, u0 and dalpha_ws keep B rows.  Nothing is written outside a row's own packed range.                       */
int sparch_readout_fwd_pk(int B, int T, int C, const float* Wx, const float* scale,
                          const float* shift, const float* alpha, const float* u0, float* out,
                          float* u_save, const int* lengths, const int* offsets, long long n_valid, void* stream);
int sparch_readout_bwd_pk(int B, int T, int C, const float* g_out, const float* bn_x,
                          const float* bn_mean, const float* bn_invstd, const float* u_save,
                          const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                          const int* lengths, const int* offsets, long long n_valid, void* stream);
/* Per-step readout ("Per-step readout"): the `_seq` forms also give the readout's value after
 * every step, seq (B,T,C), and take a gradient per step, g_seq (B,T,C).  seq_mode selects what a step's row is:
 *   SPARCH_SEQ_PROB  seq[b,t,:] = softmax(u_t);                       the gradient of p_t is G_t = fp32(g_out + g_seq[t])
 *   SPARCH_SEQ_SUM   seq[b,t,:] = sum_{t' <= t} softmax(u_t'), the accumulator of `out` after adding step t (the same
 *                    sequential fp32 sum in time order: seq[:, T-1] == out, and row t is what
 *                    sparch_readout_stream_fwd holds after t + 1 steps, bit for bit);  G_t = fp32(g_out + S_t) with the
 *                    reverse running sum S_t = fp32(S_{t+1} + g_seq[t]), S_T = 0, taken sequentially in fp32 per class
 * out, u_save, dWx and dalpha_ws are those of the plain forms (e_t = p_t (G_t - <p_t, G_t>), then the same reverse
 * recurrence).  g_out may be NULL (counts as 0).  The `_len` forms: seq[b,t,:] is written as 0 for t >= lengths[b] (in
 * both modes; the caller need not clear it), g_seq is not read there — whatever it holds, a NaN included — and S starts
 * from 0 at the row's own last step.  There is no packed form.  SPARCH_EINVAL, before any device work, for seq == NULL,
 * g_seq == NULL, seq_mode outside {0, 1}, C > 256 and whatever the plain forms refuse.                           */
#define SPARCH_SEQ_PROB 0
#define SPARCH_SEQ_SUM 1
int sparch_readout_fwd_seq(int B, int T, int C, const float* Wx, const float* scale,
                           const float* shift, const float* alpha, const float* u0, float* out,
                           float* u_save, float* seq, int seq_mode, void* stream);
int sparch_readout_bwd_seq(int B, int T, int C, const float* g_out, const float* g_seq, int seq_mode,
                           const float* bn_x, const float* bn_mean, const float* bn_invstd,
                           const float* u_save, const float* alpha, const float* u0, float* dWx,
                           float* dalpha_ws, void* stream);
int sparch_readout_fwd_seq_len(int B, int T, int C, const float* Wx, const float* scale,
                               const float* shift, const float* alpha, const float* u0, float* out,
                               float* u_save, float* seq, int seq_mode, const int* lengths,
                               long long n_valid, void* stream);
int sparch_readout_bwd_seq_len(int B, int T, int C, const float* g_out, const float* g_seq, int seq_mode,
                               const float* bn_x, const float* bn_mean, const float* bn_invstd,
                               const float* u_save, const float* alpha, const float* u0, float* dWx,
                               float* dalpha_ws, const int* lengths, long long n_valid, void* stream);
/* Time steps per LDS chunk of the readout kernels for a (T, C) problem — what the launchers above pass as `rows`:
 * bwd 0 the forward kernels, 1 the backward; seq 0 the plain / ragged / packed forms, 1 the `_seq` forms (whose backward
 * holds one more chunk image).  Host only, no device work; 0 for T <= 0, C <= 0 or C > 256.                     */
int sparch_readout_chunk_steps(int T, int C, int bwd, int seq);
/* Selectable readout ("Selectable readout"): the `_red` forms take the reduction over time.  With
 * T_b = lengths[b] (T without lengths) and the recurrence, u_save and the layouts of the forms above:
 *   SPARCH_RED_SOFTMAX_SUM   out = sum_{t < T_b} softmax(u_t): the entry points above, called as they are (same bits)
 *   SPARCH_RED_SOFTMAX_MEAN  that fp32 accumulator divided once by (float)T_b;           backward: g / (float)T_b for g
 *   SPARCH_RED_U_MAX         out[b,c] = max_{t < T_b} u_t[c], the earliest t on a tie, u0 no candidate; arg (B,C) int32 is
 *                            that t — the step inside the row's own sequence, also in the packed layout — written by the
 *                            forward and read by the backward, which puts g[c] into du at t = arg[b,c] and nothing else
 *   SPARCH_RED_U_MEAN        (...((u_0 + u_1) + u_2)...) / (float)T_b, one fp32 chain;   backward: g / (float)T_b at every t
 *   SPARCH_RED_U_LAST        u_{T_b - 1};                                                backward: g at t = T_b - 1
 * lengths NULL: every row has T steps (offsets and n_valid are then not looked at beyond the refusals below); lengths
 * alone: the `_len` layout; lengths and offsets: the `_pk` layout.  arg may be NULL unless red is U_MAX.  dWx behind a
 * row's end is written as 0 (padded layout).  SPARCH_EINVAL, before any device work: red outside 0..4, arg NULL with
 * U_MAX, offsets without lengths, n_valid < 1 with lengths, C > 256, and whatever the forms above refuse.
 * sparch_readout_stream_fwd_red: the streaming form.  `out` carries the accumulator in and out: the un-normalised
 * softmax sum (SOFTMAX_SUM and SOFTMAX_MEAN: the kernel of sparch_readout_stream_fwd), the running maximum (U_MAX: the
 * caller starts it at -inf), the un-normalised sum of u_t (U_MEAN) or u itself (U_LAST).  The caller keeps the step
 * count and divides; after the last chunk that equals sparch_readout_fwd_red over the whole sequence bit for bit.   */
#define SPARCH_RED_SOFTMAX_SUM 0
#define SPARCH_RED_SOFTMAX_MEAN 1
#define SPARCH_RED_U_MAX 2
#define SPARCH_RED_U_MEAN 3
#define SPARCH_RED_U_LAST 4
int sparch_readout_fwd_red(int B, int T, int C, const float* Wx, const float* scale,
                           const float* shift, const float* alpha, const float* u0, float* out,
                           float* u_save, int red, int* arg, const int* lengths, const int* offsets,
                           long long n_valid, void* stream);
int sparch_readout_bwd_red(int B, int T, int C, const float* g_out, const float* bn_x,
                           const float* bn_mean, const float* bn_invstd, const float* u_save,
                           const float* alpha, const float* u0, float* dWx, float* dalpha_ws, int red,
                           const int* arg, const int* lengths, const int* offsets, long long n_valid,
                           void* stream);
int sparch_readout_stream_fwd_red(int B, int T, int C, const float* Wx, const float* scale,
                                  const float* shift, const float* alpha, float* u, float* out, int red,
                                  void* stream);

/* Stateful training ("Stateful training"): the reverse pass of a chunk whose final state
 * (u_T, w_T, s_T = 1[u_T > theta]) was handed on to the next chunk and whose initial state came from the one before.
 * The forward is the plain one (sparch_cell_fwd / sparch_readout_fwd with fp32 saves: u_save[:, T-1], w_save[:, T-1]
 * ARE the final membranes).  With du_t, dw_t the total gradients of u_t, w_t, k the dropout scale:
 *   into the chunk, at the reverse pass's first step only (du_{T+1} = dw_{T+1} = 0 there), from g_uT / g_wT / g_sT,
 *   the gradient arriving on the final state ((B,H) each, NULL = 0):
 *     ds_T = (g_T + g_rate) k + g_sT        du_T = gate(ds_T) + g_uT        dw_T = g_wT - (1 - alpha) du_T
 *     (g_sT is the RAW spike's: it enters behind the dropout scale, which scales the layer's output, not its state)
 *   out of the chunk, from the carries the pass ends with, into g_u0 / g_w0 / g_s0 ((B,H) each, NULL = not wanted):
 *     g_u0 = alpha du_1 + a dw_1            g_w0 = beta dw_1                g_s0 = -alpha du_1 + b dw_1
 *     (LIF: the terms in dw are absent; g_wT / g_w0 are ignored)
 * sparch_cell_bwd_st: the arguments of sparch_cell_bwd_sg, then the six above.  dirs == 1 and save_bf16 == 0 only:
 * anything else is SPARCH_EINVAL before any device work, as are sparch_cell_bwd_sg's own refusals.
 * sparch_readout_bwd_st: the arguments of sparch_readout_bwd, then g_uT and g_u0 ((B,C), nullable):
 *     du_T = softmax'(u_T)^T g_out + g_uT                                   g_u0 = alpha du_1                     */
int sparch_cell_bwd_st(int kind, int B, int dirs, int T, int H, const float* g_out,
                       const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                       const float* alpha, const float* beta, const float* a, const float* b,
                       const float* u0, const float* w0, const float* s0, float theta,
                       float p_drop, uint64_t seed, float* dWx, float* dparam_ws, const float* bn_x,
                       const float* bn_mean, const float* bn_invstd, int surrogate, float surrogate_scale,
                       const float* g_uT, const float* g_wT, const float* g_sT, float* g_u0, float* g_w0,
                       float* g_s0, void* stream);
/* sparch_rec_cell_bwd_st (RLIF / RadLIF): the arguments of sparch_rec_cell_bwd_sg up to surrogate_scale, then the six
 * above ((Bp,H) each, nullable), then stream and precision.  With Vm = V with a zero diagonal and dWx_1 = (1 - alpha) du_1,
 *     g_s0 = -alpha du_1 + b dw_1 + dWx_1 Vm^T:
 * the kernel writes g_u0, g_w0 and the two pointwise terms of g_s0; the product is the caller's, one (Bp x H)(H x H)
 * GEMM on dWx[:, 0, :] through the existing entry points.  dV's s_0 term is what it always was.  Whole-sequence launches
 * only: steps_per_launch < T is SPARCH_EINVAL, as are dirs != 1, save_bf16 != 0, precision != 0 (the bf16 operand mode),
 * H > 1024 and a grid that cannot be co-resident (no degraded mode) — each before any device work.                  */
int sparch_rec_cell_bwd_st(int kind, int B, int dirs, int T, int H, const float* g_out,
                           const float* g_rate, const void* u_save, const void* w_save, int save_bf16,
                           const float* alpha, const float* beta, const float* a,
                           const float* b, const float* vpack_t, const float* u0,
                           const float* w0, const float* s0, float theta, float p_drop,
                           uint64_t seed, float* dWx, uint16_t* s_prev16, float* dparam_ws,
                           const float* bn_x, const float* bn_mean, const float* bn_invstd,
                           void* chan, size_t chan_bytes, uint32_t* status,
                           int steps_per_launch, int surrogate, float surrogate_scale,
                           const float* g_uT, const float* g_wT, const float* g_sT, float* g_u0,
                           float* g_w0, float* g_s0, void* stream, int precision);
int sparch_readout_bwd_st(int B, int T, int C, const float* g_out, const float* bn_x,
                          const float* bn_mean, const float* bn_invstd, const float* u_save,
                          const float* alpha, const float* u0, float* dWx, float* dalpha_ws,
                          const float* g_uT, float* g_u0, void* stream);

/* ------------------------------------------------------------------------------------
 * G9  mel filterbank front-end  (replaces torchaudio.compliance.kaldi.fbank(x,
 *     num_mel_bins=40) at nonspiking_datasets.py:96,194; third-party, parity unpinned).
 *     wave (n_clips, n_samples) fp32 in [-1,1], 16 kHz -> out (n_clips, frames, n_mels),
 *     frames = 1 + (n_samples-400)/160.                                              */
int sparch_fbank_frames(int n_samples);
int sparch_fbank_fwd(int n_clips, int n_samples, int n_mels, const float* wave, float* out,
                     void* stream);

/* G9  variable-length clips, padded (the reference's HD / SC collate: kaldi.fbank per clip, then
 *     pad_sequence(batch_first=True), nonspiking_datasets.py:96,104-111,194,202-209).  Clip i is
 *     row i of wave (n_clips, ld), in_dtype 0 = fp32 in [-1,1], 1 = int16 PCM (scaled by 2^-15 on
 *     load: bit-identical to the fp32 path on pcm/32768).  lengths (n_clips) device int32 samples;
 *     clip i has f_i = sparch_fbank_frames(min(max(lengths[i], 0), ld)) frames.  out (n_clips,
 *     n_frames_out, n_mels): frames t < f_i as sparch_fbank_fwd gives them for the clip alone (same
 *     bits), frames f_i <= t < n_frames_out exactly 0.  Nothing past ld or a clip's own end is read.   */
int sparch_fbank_padded_fwd(int n_clips, int ld, const int* lengths, int n_frames_out, int n_mels,
                            int in_dtype, const void* wave, float* out, void* stream);

/* f-3  Waveform augmentation of HD / SC training clips (replaces torchaudio_augmentations 0.2.4's
 *     ComposeMany of RandomApply(PolarityInversion, .8), (Noise(min_snr, max_snr), p_noise),
 *     (Gain, .3), (Reverb(16000), .6) at nonspiking_datasets.py:71-78,93,170-177,191; restated,
 *     parity unpinned).  Clip i is wave[i, :len_i], len_i = min(max(lengths[i], 0), ld), in_dtype 0 =
 *     fp32, 1 = int16 scaled by 2^-15; lengths (n_clips) device int32.  params (n_clips,
 *     SPARCH_AUGM_FIELDS) device fp32, per clip: polarity, noise, gain, reverb flags (0 / 1), the noise
 *     uniform u, the gain ratio, reverberance, HF damping and room scale in percent (clamped to
 *     [0, 100]).  Noise: std = unbiased std of the clip (len_i >= 2, else no noise), noise_std =
 *     a + (b - a) u with a = min_snr std, b = max_snr std (fp32), normal values from a Philox4x32-10
 *     stream keyed by (noise_seed, i, sample).  Reverb: sox 14.4 `reverb R D S` at sample_rate
 *     (8000-48000), stereo depth 100 %, then `channels 1`; same length out, no tail.  Writes exactly
 *     out[i, :len_i] (out (n_clips, ld) fp32, not overlapping wave) and reads nothing past len_i.
 *     Launch only: no allocation, no synchronisation.  sparch_augment_lds_bytes(sample_rate): the
 *     dynamic LDS of one workgroup (0 outside 8000-48000).                                          */
#define SPARCH_AUGM_FIELDS 9
int sparch_augment_lds_bytes(int sample_rate);
int sparch_augment_padded(int n_clips, int ld, const int* lengths, int in_dtype, const void* wave,
                          const float* params, float min_snr, float max_snr, unsigned long long noise_seed,
                          int sample_rate, float* out, void* stream);

/* f-3  FLAC (RFC 9639) decoding into the padded waveform buffer of the HD collate (replaces
 *     torchaudio.load at nonspiking_datasets.py:90).  bytes (n_bytes, device, n_bytes % 4 == 0) holds
 *     the files of n_clips clips, each starting at a 4-aligned offset; clips (n_clips,
 *     SPARCH_FLAC_CLIP_FIELDS) device int64 describes clip i: byte range [begin, end), absolute offset
 *     of its first frame, STREAMINFO total samples, output row, sample rate, channels (1-8), bits per
 *     sample (4-24), min / max block size, then its workspace share: slot base and slot count (at least
 *     ceil(total / min block): one slot per frame) and, for 2 channels, scratch base (int32 elements,
 *     slots x max block of them).  Slot bases ascend with i.  out (n_rows, ld): out_dtype 0 = fp32
 *     x * 2^-(bps-1), 1 = int16 (16-bit clips only); channel 0 of clip i goes to samples
 *     [0, total) of its row, nothing else is written.  err (2, device int64, 8-aligned), written by the
 *     call: [0] clips in error, [1] (clip << 32) | (frame << 8) | SPARCH_FLAC_E* reason of the lowest
 *     failing clip (all ones when none).  A clip fails when its table row is inconsistent, a frame
 *     header or subframe is invalid, a frame runs past the clip's bytes, a CRC-16 differs, or the frames
 *     do not add up to `total`; no read leaves the clip's bytes, whatever they hold.  Workspace: from
 *     sparch_flac_workspace_bytes(sum of slot counts, sum of scratch sizes), 16-aligned.  Launches
 *     only (stream-ordered memsets included): no allocation, no synchronisation.               */
#define SPARCH_FLAC_CLIP_FIELDS 13
#define SPARCH_FLAC_ETABLE 1     /* table row inconsistent with the buffers, the workspace or out_dtype */
#define SPARCH_FLAC_EHEADER 2    /* no valid frame header (with the expected number) where one must be */
#define SPARCH_FLAC_ESUBFRAME 3  /* reserved or invalid subframe / residual coding                     */
#define SPARCH_FLAC_ETRUNC 4     /* a frame runs past the clip's last byte                             */
#define SPARCH_FLAC_ECRC 5       /* frame CRC-16 mismatch                                              */
#define SPARCH_FLAC_ELENGTH 6    /* the frames do not add up to the STREAMINFO sample count            */
size_t sparch_flac_workspace_bytes(long long n_slots, long long n_scratch);
int sparch_flac_decode_padded(int n_clips, const long long* clips, const unsigned char* bytes, long long n_bytes,
                              long long n_slots, long long n_scratch, int n_rows, int ld, int out_dtype,
                              void* out, long long* err, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------------------------
 * f-3  SHD/SSC event lists -> dense binned spike counts (replaces SpikingDataset.__getitem__,
 *      spiking_datasets.py:66-78: np.digitize into np.linspace(0, max_time, nb_steps) edges, then a
 *      sparse->dense scatter in which duplicates add up).  Events of all samples are concatenated;
 *      sample_offsets (n_samples+1, device int64) delimits them.  out (n_samples, nb_steps, nb_units) is
 *      zeroed by the call.  Events the reference's sparse constructor would reject (t < 0, t >= max_time,
 *      unit out of range) are skipped and counted in *n_dropped (device uint32).                    */
int sparch_bin_events(long long n_events, const float* times, const int* units,
                      const long long* sample_offsets, int n_samples, int nb_steps, int nb_units,
                      double max_time, float* out, uint32_t* n_dropped, void* stream);

/* f-3  A batch from a device-resident event store (the whole of SHD / SSC uploaded once) and a device
 *      list of sample indices: gather and bin in one launch, no memset, no global atomic.
 *      Store: times (n_events; times_dtype 0 = fp32, 1 = fp16), units (n_events, uint16; 0xFFFF marks a
 *      unit that was negative or did not fit and is dropped like any unit >= nb_units), offsets
 *      (n_store + 1, int64, non-decreasing from 0 to n_events: checked by the owner, not here), labels
 *      (n_store, int64; may be NULL when y is).  idx (batch, device int64): sample of each batch row; an
 *      index outside [0, n_store) gives an empty sample and label -1.  nb_units <= 65535.
 *      Outputs, each may be NULL, at least one is not:
 *        plane  (batch * nb_steps, ldp) bf16 bit patterns, ldp = nb_units rounded up to 8, exact zeros
 *               behind column nb_units: the layout and values of sparch_expand_counts_u8 (16-byte
 *               aligned; exact while every count is <= 256, the owner of the store sees to that);
 *        dense  (batch, nb_steps, nb_units) fp32, the tensor sparch_bin_events writes;
 *        counts (batch, nb_steps, nb_units) uint8, saturating at 255.
 *      y (batch, int64) = labels[idx], *n_dropped (device uint32) as sparch_bin_events counts it;
 *      either may be NULL.  n_dropped needs a workspace of sparch_events_gather_bin_workspace_bytes
 *      (one word per workgroup, summed by a second small launch; no workspace without it).
 *      Every event gets the bin sparch_bin_events gives it (one shared device function).  sorted != 0
 *      promises that the times of every sample are non-decreasing (a workgroup then finds the events
 *      of its time slab by search instead of scanning the sample); a wrong promise loses events but
 *      reads nothing out of bounds.  Launch only: no allocation, no synchronisation.              */
size_t sparch_events_gather_bin_workspace_bytes(int batch, int nb_steps, int nb_units);
int sparch_events_gather_bin(const void* times, int times_dtype, const uint16_t* units,
                             const long long* offsets, const long long* labels, long long n_store,
                             const long long* idx, int batch, int nb_steps, int nb_units, double max_time,
                             int sorted, uint16_t* plane, float* dense, uint8_t* counts, long long* y,
                             uint32_t* n_dropped, void* workspace, size_t workspace_bytes, void* stream);

/* f-3  sparch_events_gather_bin with a per-sample augmentation of the events in front of the bin: same
 *      store, outputs, workspace (sparch_events_gather_bin_workspace_bytes) and return codes.  aug is a
 *      device table (batch, SPARCH_EVAUG_FIELDS) fp32, row b for batch row b:
 *        0     unit shift d (integer-valued, |d| <= 65535)
 *        1, 2  time scale a (finite, > 0) and offset c (seconds, finite)
 *        3     drop probability p in [0, 1)
 *        4, 5  time mask [m0, m1) in transformed seconds, empty when m1 <= m0
 *        6, 7  unit band [k0, k1) in shifted units (integer-valued), empty when k1 <= k0
 *      Event i of sample s = idx[b] sits at position j = i - offsets[s] of its sample.  In this order:
 *        1. u = units[i]; the stored marker 0xFFFF is never placed, whatever the shift;
 *        2. r = the 24-bit uniform of the dropout hash (see "Dropout") of (seed, ((uint64)b << 32) | (uint32)j);
 *           the event is removed when r < p, compared in fp32 (b enters, so a sample drawn twice into a
 *           batch gets two masks);
 *        3. t' = fp32(fp32(a * t) + c), two roundings and no FMA, t widened exactly; u' = u + d;
 *        4. the event is removed when m0 <= t' < m1 or k0 <= u' < k1;
 *        5. bin and drop rule of sparch_events_gather_bin (the one shared device function) on (t', u');
 *        6. otherwise 1 is added at (bin, u').
 *      *n_dropped counts every event of the batch that was read and not placed (steps 1, 2, 4 and 5), once.
 *      With a > 0, t' is non-decreasing in t, so `sorted` keeps its meaning.  The table is device data: the
 *      caller validates it.  A row with a <= 0 is a wrong `sorted` promise (events may be lost); no row, however
 *      wrong, makes the kernel read or write out of bounds.  seed is used as given (no SPARCH_SEED_IN_MEMORY). */
#define SPARCH_EVAUG_FIELDS 8
int sparch_events_gather_bin_aug(const void* times, int times_dtype, const uint16_t* units,
                                 const long long* offsets, const long long* labels, long long n_store,
                                 const long long* idx, int batch, int nb_steps, int nb_units, double max_time,
                                 int sorted, uint16_t* plane, float* dense, uint8_t* counts, long long* y,
                                 uint32_t* n_dropped, void* workspace, size_t workspace_bytes,
                                 const float* aug, uint64_t seed, void* stream);

/* f-3  A batch of HD / SC features from a device-resident audio store (every clip of a split in one flat
 *      sample array, uploaded once) and a device list of clip indices.
 *      Store: samples (dtype 0 = fp32 in [-1,1], 1 = int16 PCM scaled by 2^-15 on load), starts (n_store,
 *      int64: first sample of each clip), lengths (n_store, int32 samples; negative counts as 0), labels
 *      (n_store, int64; may be NULL when y is).  The owner has checked that every clip lies inside samples
 *      and that clips do not overlap; the kernels trust it.  idx (batch, device int64): clip of each batch
 *      row; an index outside [0, n_store) gives an empty clip and label -1.  y (batch, int64) = labels[idx],
 *      may be NULL.  Nothing outside a clip's own samples is read.  Launch only: no allocation, no
 *      synchronisation.
 *      sparch_audio_gather_fbank: out (batch, n_frames_out, n_mels); row b holds the frames
 *      t < sparch_fbank_frames(length) of clip idx[b] exactly as sparch_fbank_padded_fwd gives them (one shared
 *      device function), the frames behind them exact zeros (a clip with more than n_frames_out frames is cut).
 *      sparch_audio_gather_augment: out (batch, ld) fp32; row b holds the first min(length, ld) samples of clip
 *      idx[b] augmented exactly as sparch_augment_padded augments row b of a batch buffer holding those clips
 *      (one shared device function; params, the noise stream keyed by (noise_seed, b, sample), min_snr,
 *      max_snr and sample_rate as there) and is not written behind them; out_lengths (batch, device int32)
 *      receives min(length, ld): the `lengths` of the sparch_fbank_padded_fwd launch that follows.          */
int sparch_audio_gather_fbank(const void* samples, int dtype, const long long* starts, const int* lengths,
                              const long long* labels, long long n_store, const long long* idx, int batch,
                              int n_frames_out, int n_mels, float* out, long long* y, void* stream);
int sparch_audio_gather_augment(const void* samples, int dtype, const long long* starts, const int* lengths,
                                const long long* labels, long long n_store, const long long* idx, int batch,
                                int ld, const float* params, float min_snr, float max_snr,
                                unsigned long long noise_seed, int sample_rate, float* out, int* out_lengths,
                                long long* y, void* stream);

/* ---- f-4: non-spiking baselines (anns.py) --------------------------------------------------
 * Element-wise tail of MLPLayer.forward (anns.py:218-227): y = dropout(act(z * scale + shift)) over n
 * elements of an (n/H, H) tensor; scale/shift (H) = the folded BatchNorm affine, NULL for none.
 * Backward: dz = dy * keep * act'(z * scale + shift) — the gradient w.r.t. the NORMALISED
 * pre-activation (feed it to the norm's backward).  H % 4 == 0.
 * relu PROPAGATES NaN, as torch.relu / nn.ReLU do (v <= 0 ? +0 : v; -0.0 gives +0.0), here and in every kernel of
 * the baselines that applies it (the RNN cell, LiGRU's candidate on both of its paths): a network whose
 * pre-activations have gone non-finite shows it in its loss.                                      */
#define SPARCH_ACT_SIGMOID 0
#define SPARCH_ACT_RELU 1
#define SPARCH_ACT_TANH 2
int sparch_act_fwd(int kind, size_t n, int H, const float* z, const float* scale, const float* shift,
                   float p_drop, uint64_t seed, float* y, void* stream);
int sparch_act_bwd(int kind, size_t n, int H, const float* z, const float* scale, const float* shift,
                   const float* dy, float p_drop, uint64_t seed, float* dz, void* stream);
/* ReadoutLayerANN._readout_cell (anns.py:658-665): out[b,:] = sum_t softmax(x[b,t,:]) (softmax over the
 * K features, accumulated in time order); backward dx[b,t,:] = p_t * (g[b,:] - <p_t, g[b,:]>).
 * K % 4 == 0, K <= 4096.                                                                          */
int sparch_softmax_sum_fwd(int B, int T, int K, const float* x, float* out, void* stream);
int sparch_softmax_sum_bwd(int B, int T, int K, const float* x, const float* g, float* dx, void* stream);

/* Dense recurrent cell of the RNN baseline (RNNLayer._rnn_cell, anns.py:328-339):
 *     y_t = act(Wx_t * scale + shift + y_{t-1} V^T),  y_{-1} = 0          (forward)
 *     dpre_t = (g_t + dpre_{t+1} V) * act'(y_t)                            (backward)
 * The same persistent machine as sparch_rec_cell_bwd: V slice resident in registers, the previous step's
 * dense fp32 tiles handed over through `chan` (sparch_rec_chan_bytes) and contracted on the bf16 MFMA
 * with the exact six-term split.  vpack = sparch_vpack(H, V, transpose | 2, ...): bit 1 keeps the
 * diagonal; forward uses transpose = 1 (y V^T), backward transpose = 0 (dpre V).
 *   y_out   (B,T,H*dirs) dropout(y) with the directions concatenated on features (anns.py:319-324)
 *   y_state (Bp,T,H)     y in cell time order: the backward's input
 *   dpre    (Bp,T,H)     gradient w.r.t. the normalised projection, virtual rows, ORIGINAL time index
 *   y_prev  (Bp,T,H)     y_{t-1} at the same index (zero row at the first step): dV = dpre^T y_prev      */
int sparch_ann_rec_fwd(int act, int B, int dirs, int T, int H, const float* Wx, const float* scale,
                       const float* shift, const float* vpack, float p_drop, uint64_t seed,
                       float* y_out, float* y_state, void* chan, size_t chan_bytes, uint32_t* status,
                       int steps_per_launch, void* stream);
int sparch_ann_rec_bwd(int act, int B, int dirs, int T, int H, const float* g_out, const float* y_state,
                       const float* vpack, float p_drop, uint64_t seed, float* dpre, float* y_prev,
                       void* chan, size_t chan_bytes, uint32_t* status, int steps_per_launch,
                       void* stream);
/* ONE step of the same cell with the recurrent product supplied by the caller (hidden sizes > 1024, see
 * sparch_rec_cell_step_fwd).  `s` counts steps in processing order (forward t = s, backward t = T-1-s);
 * rec (Bp,H) = y_{t-1} V^T (forward) / dpre_{t+1} V (backward), ignored at s = 0; the step's y / dpre also
 * goes to the contiguous (Bp,H) buffer y_step / dpre_step.                                          */
int sparch_ann_rec_step_fwd(int act, int B, int dirs, int T, int H, int s, const float* Wx,
                            const float* scale, const float* shift, const float* rec, float p_drop,
                            uint64_t seed, float* y_out, float* y_state, float* y_step, void* stream);
int sparch_ann_rec_step_bwd(int act, int B, int dirs, int T, int H, int s, const float* g_out,
                            const float* y_state, const float* rec, float p_drop, uint64_t seed,
                            float* dpre, float* y_prev, float* dpre_step, void* stream);

/* LiGRU cell (LiGRULayer._ligru_cell, anns.py:449-462) as persistent kernels (gatedcell.hip): hidden sizes that are
 * multiples of 32 up to 1024; a workgroup owns 16 hidden units with its slices of BOTH recurrent matrices.
 *   z = sigmoid(Wzx*scz+shz + y_{t-1} Vz^T), c = relu(Wx*sc+sh + y_{t-1} V^T), y = z y_{t-1} + (1-z) c.
 * vpack = sparch_ligru_vpack(H, Vz, V, backward): the exact three-plane bf16 fragments of the slices.
 * forward outputs: y_out (B,T,H*dirs) = dropout(y), y_state / z_save / c_save (Bp,T,H) in cell time order;
 * backward outputs (Bp,T,H at the ORIGINAL time index): dz_all, dc_all = gradients w.r.t. the two normalised
 * projections, yprev_all = y_{t-1} (dVz = dz_all^T yprev_all, dV = dc_all^T yprev_all); carry (Bp,H): scratch
 * carried between chunked launches.  chan: sparch_ligru_chan_bytes(Bp, H) of scratch — one size for both passes;
 * fewer bytes are SPARCH_EWORKSPACE in either (sparch_gru_chan_bytes likewise for the GRU).                    */
size_t sparch_ligru_vpack_bytes(int H, int backward);
int sparch_ligru_vpack(int H, const float* Vz, const float* V, int backward, float* vpack, void* stream, int precision);
size_t sparch_ligru_chan_bytes(int Bp, int H);
int sparch_ligru_fwd(int B, int dirs, int T, int H, const float* Wx, const float* sc, const float* sh,
                     const float* Wzx, const float* scz, const float* shz, const float* vpack,
                     float p_drop, uint64_t seed, float* y_out, float* y_state, float* z_save,
                     float* c_save, void* chan, size_t chan_bytes, uint32_t* status,
                     int steps_per_launch, void* stream);
int sparch_ligru_bwd(int B, int dirs, int T, int H, const float* g_out, const float* y_state,
                     const float* z_save, const float* c_save, const float* vpack_b, float p_drop,
                     uint64_t seed, float* dz_all, float* dc_all, float* yprev_all, float* carry,
                     void* chan, size_t chan_bytes, uint32_t* status, int steps_per_launch,
                     void* stream);

/* Host routine (no device work): n uniform fp32 numbers in [0, 1) from an MT19937 state, exactly as torch.rand draws
 * them from its CPU generator — one 32-bit output y per element, x = (y & 0xFFFFFF) * 2^-24 — i.e. the reference's
 * initial-state draws (snns.py:286-287, 423-425, 558-559, 700-702, 812) at ~1 ns instead of ~5 ns per number.
 * key: the 624 state words, *pos: index of the next word (624 = regenerate first); both are advanced in place.  The
 * caller moves them out of / back into the generator's serialized state (sparch_amd/snns.py, which also verifies the
 * layout once against torch.rand and otherwise keeps drawing with torch.rand).                              */
int sparch_mt19937_uniform_f32(uint32_t* key, int* pos, size_t n, float* out);

/* GRU cell (GRULayer._gru_cell, anns.py:581-595) as persistent kernels: the same machine with a second hand-off
 * per step (the reset gate sits inside the candidate's recurrent term):
 *   z = sigmoid(xz + y Vz^T), r = sigmoid(xr + y Vr^T), c = tanh(xc + (r y) V^T), y' = z y + (1 - z) c.
 * Two fragment buffers per direction of time (sparch_gru_vpack_bytes(H, backward, which): which 0 = the gates'
 * [Vz | Vr], 1 = the candidate's V), filled by one sparch_gru_vpack call.  forward outputs as the LiGRU plus
 * r_save; backward outputs (Bp,T,H, original time index): dz_all, dr_all, dc_all, yprev_all = y_{t-1},
 * ry_all = r y_{t-1} (dVz = dz_all^T yprev_all, dVr = dr_all^T yprev_all, dV = dc_all^T ry_all).  Every workgroup of
 * a row tile must be resident at once (two hand-offs inside a step): SPARCH_EINVAL when H / 16 exceeds the CU
 * count — callers then use the launch-per-step path (sparch_gate_step).  chan: sparch_gru_chan_bytes(Bp, H).  */
size_t sparch_gru_vpack_bytes(int H, int backward, int which);
int sparch_gru_vpack(int H, const float* Vz, const float* Vr, const float* V, int backward, float* vpack_gate,
                     float* vpack_cand, void* stream, int precision);
size_t sparch_gru_chan_bytes(int Bp, int H);
int sparch_gru_fwd(int B, int dirs, int T, int H, const float* Wx, const float* sc, const float* sh,
                   const float* Wzx, const float* scz, const float* shz, const float* Wrx, const float* scr,
                   const float* shr, const float* vpack_gate, const float* vpack_cand, float p_drop,
                   uint64_t seed, float* y_out, float* y_state, float* z_save, float* r_save, float* c_save,
                   void* chan, size_t chan_bytes, uint32_t* status, int steps_per_launch, void* stream);
int sparch_gru_bwd(int B, int dirs, int T, int H, const float* g_out, const float* y_state, const float* z_save,
                   const float* r_save, const float* c_save, const float* vpack_gate_b,
                   const float* vpack_cand_b, float p_drop, uint64_t seed, float* dz_all, float* dr_all,
                   float* dc_all, float* yprev_all, float* ry_all, float* carry, void* chan, size_t chan_bytes,
                   uint32_t* status, int steps_per_launch, void* stream);

/* Gate arithmetic of ONE time step of the gated baselines (LiGRULayer._ligru_cell anns.py:449-462,
 * GRULayer._gru_cell anns.py:581-595); the recurrent products between the phases are GEMM calls: the
 * launch-per-step path (annstep.hip) for hidden sizes the persistent kernels above do not take.  mode: 0 LiGRU forward, 1 GRU forward gates
 * (z, r, r*y), 2 GRU forward candidate + state, 3 LiGRU backward, 4 GRU backward (dy, dz_pre, dc_pre),
 * 5 GRU backward (dr_pre).  `in` / `out` are HOST arrays of 14 device pointers each (unused slots NULL):
 *   in : Wx sc sh Wzx scz shz Wrx scr shr rec g_out carry_mv carry_dir dry
 *   out: y_state z_save r_save c_save ry y_out carry_dir_out dgate dcp dz_all dr_all dc_all yprev_all ry_all
 * Shapes: projections (B,T,H) with folded BatchNorm (H) each; rec (Bp,2H) or (Bp,H); saves (Bp,T,H) in cell
 * time order; *_all (Bp,T,H) at the original time index; y_out / g_out (B,T,H*dirs).  H % 4 == 0.      */
int sparch_gate_step(int mode, int B, int dirs, int T, int H, int t, const float* const* in,
                     float* const* out, float p_drop, uint64_t seed, void* stream);

/* Streaming, ONE time step of a baseline layer with the state carried by the caller (csrc/streamann.hip): the
 * projection(s), the recurrent product(s) and the cell in one launch, two for a GRU layer.  The whole-sequence entry
 * points above start from y = 0 and return no state; a stream stepped here from a zero state computes what they do.
 * sparch_ann_stream_step — one hidden layer, all B rows, any B, K, H >= 1 (rows in tiles over grid.y):
 *   cell, phase   SPARCH_CELL_MLP / _RNN / _LIGRU with phase 0; SPARCH_CELL_GRU with phase 1 (z, r, r * y) then 2
 *   act           SPARCH_ACT_* of the MLP and RNN cells (the gated cells have their own; ignored there)
 *   x (B,K), row stride ldx >= K   the step's input, fp32, read where it lies; or NULL: the projections are `pre`
 *   W, bias, scale, shift, pre, V   HOST arrays of 3 device pointers each, one slot per gate: 0 the candidate (W, V;
 *               the only one of MLP and RNN), 1 the update gate (Wz, Vz), 2 the reset gate (Wr, Vr).  A NULL array
 *               means three NULL slots.  W? (H,K) and V? (H,H) contiguous AS STORED by the modules (row h of V? is
 *               what y V?^T needs: no transpose, no mask); bias (H) or NULL; scale / shift (H) the folded eval
 *               BatchNorm, both or neither; pre? (B,H) contiguous, the already normalised projection (LayerNorm
 *               layers: GEMM, sparch_layernorm_fwd, then this call with x == NULL).  A launch reads the slots of its
 *               gates only: MLP, RNN, GRU phase 2 slot 0; LiGRU slots 0, 1; GRU phase 1 slots 1, 2.
 *   y_in (B,H)  the previous state, y_out (B,H) the new one, z and ry (B,H) the GRU's update gate and r * y between
 *               its phases (phase 1 writes, phase 2 reads them); all fp32 with row stride ld >= H.  Columns >= H of a
 *               row are never written.  MLP: y_in is not read.
 *   MLP y = act(p)   RNN y' = act(p + y V^T)   LiGRU z = sigm(pz + y Vz^T), c = relu(p + y V^T), y' = z y + (1 - z) c
 *   GRU 1: z = sigm(pz + y Vz^T), r = sigm(pr + y Vr^T), ry = r y      2: c = tanh(p + ry V^T), y' = z y + (1 - z) c
 *   with p? = (x W?^T + bias) * scale + shift, or pre?.  Dot products are fp32 FMA chains (64 lane partials, butterfly).
 * Every workgroup of a recurrent launch reads ALL of y_in (GRU phase 2: all of ry), so what the launch writes must be
 * another buffer: y_out == y_in (RNN, LiGRU), z or ry == y_in or each other (GRU 1), y_out == ry or z (GRU 2) are
 * SPARCH_EINVAL, as are an unknown cell / phase / act, a non-positive size, ld < H, ldx < K, a missing operand of the
 * launch's gates, scale without shift, more than 65535 row tiles.  After those: W?, V?, y_in, y_out, z, ry 16-byte
 * aligned (else SPARCH_EALIGN).  Nothing waits inside a launch; nothing is launched by a refused call.
 * sparch_ann_stream_readout — the readout's step (ReadoutLayerANN, anns.py:644-665), one workgroup per batch row:
 *   acc[b,:] += softmax(y[b,:]) over the K <= 4096 features (y (B,K) row stride ldy; acc (B,K) contiguous, in place:
 *   ONE sequential sum over the steps, in time order), then out[b,:] = norm(acc[b,:] W^T + bias) for C <= 256 classes:
 *   the network's answer as if the sequence ended here.  W (C,K); norm SPARCH_RO_NORM_NONE, _AFFINE (p0 = scale, p1 =
 *   shift: the folded eval BatchNorm) or _LAYERNORM over the C outputs (p0 = gamma, p1 = beta, eps).  SPARCH_EINVAL: a
 *   non-positive size, K > 4096, C > 256, ldy < K, a NULL y / acc / W / out, an unknown norm, a norm without both of
 *   p0 and p1; then W, acc 16-byte aligned (else SPARCH_EALIGN).                                                  */
#define SPARCH_CELL_MLP 0
#define SPARCH_CELL_RNN 1
#define SPARCH_CELL_LIGRU 2
#define SPARCH_CELL_GRU 3
#define SPARCH_RO_NORM_NONE 0
#define SPARCH_RO_NORM_AFFINE 1
#define SPARCH_RO_NORM_LAYERNORM 2
int sparch_ann_stream_step(int cell, int phase, int act, int B, int K, int H, int ld, const float* x, int ldx,
                           const float* const* W, const float* const* bias, const float* const* scale,
                           const float* const* shift, const float* const* pre, const float* const* V,
                           const float* y_in, float* y_out, float* z, float* ry, void* stream);
int sparch_ann_stream_readout(int B, int K, int C, const float* y, int ldy, float* acc, const float* W,
                              const float* bias, int norm, const float* p0, const float* p1, float eps, float* out,
                              void* stream);

/* ---- f-2: optimizer step on the device (replaces torch.optim.Adam.step, exp.py:89, 377) ----------
 * One launch for the whole parameter list; arithmetic identical, operation by operation, to
 * torch.optim.Adam's default path (see optim.hip).  `params`, `grads`, `exp_avg`, `exp_avg_sq` are HOST
 * arrays of n_tensors DEVICE pointers, `numel` a host array of element counts.
 * step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t): formed by the caller in double precision.
 * scalars_dev (nullable): device float[2] = {step_size, bc2_sqrt} read instead of the two arguments — for a
 * step captured in a HIP graph, whose kernel arguments are frozen at capture time.
 * skip_if_nonzero (nullable): a device word, e.g. the recurrent kernels' status word — when it is non-zero
 * the step leaves parameters and moments untouched (a timed-out step must not be applied; no host sync) and
 * adds 1 to skip_if_nonzero[1] — ONCE PER CALL, however many launches the tensor table needs (24 tensors each), and
 * not at all when no tensor is non-empty — hence not const: the caller learns how many steps to take back from its
 * bias-correction counter when it reads the word.  Empty tensors (numel 0) are passed over and may be NULL. */
int sparch_adam_step(int n_tensors, float* const* params, const float* const* grads,
                     float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                     float step_size, float beta1, float beta2, float bc2_sqrt, float eps,
                     float weight_decay, const float* scalars_dev, uint32_t* skip_if_nonzero,
                     void* stream);

/* The per-step factors of a captured step, made on the device by ONE launch: t_dev (double, the step count) += 1;
 * scalars_dev[0] = lr_dev[0] / (1 - beta1^t), scalars_dev[1] = sqrt(1 - beta2^t), evaluated in double precision as the
 * host path does (replaces a dozen captured scalar torch ops per step, ~55 us of a 1 ms BASELINE configs[1] step). */
int sparch_adam_scalars(double* t_dev, const double* lr_dev, double beta1, double beta2, float* scalars_dev,
                        void* stream);

/* ---- gradient clipping by global norm, on the device (gradclip.hip; DESIGN.md section 6, "Gradient clipping") ----
 * sparch_grad_norm: the 2-norm over a whole gradient list (`grads`: a HOST array of n_tensors DEVICE pointers, `numel`
 * a host array, as sparch_adam_step; empty tensors are passed over and may be NULL), accumulated in double in a FIXED
 * order — no atomics: the same table gives the same bits on every call and on every replica, whatever the alignment of
 * the tensors (4-byte aligned views are fine) — and the clip state made from it, 8 words of 32 bits the caller owns and
 * has zeroed once:
 *   clip[0] float  this step's global norm, (float)sqrt(sum of squares in double)
 *   clip[1] float  this step's coefficient fminf(max_norm / (norm + 1e-6f), 1.0f): torch.nn.utils.clip_grad_norm_'s
 *                  formula and epsilon in fp32; max_norm = +inf gives 1 (measure and guard only)
 *   clip[2] u32    1 if this step's norm is not finite (a NaN or inf gradient, or a norm above fp32's range), else 0
 *   clip[3] u32    steps skipped for a non-finite norm since the state was zeroed (+1 per call, not per launch)
 *   clip[4] u32    finite steps counted          clip[5] u32  of those, steps with coefficient < 1
 *   clip[6] float  largest finite norm seen      clip[7] u32  0, reserved
 * tensor_norms (nullable): n_tensors floats, each tensor's own norm (0 for an empty one) — which matrix blew up.
 * skip_if_nonzero (nullable): the recurrent kernels' status word; while it is raised (the step's gradients are garbage)
 * words 3-6 stay as they are and the call writes coefficient 1, flag 0: the optimizer skips on the word itself.
 * ws: sparch_grad_norm_ws_bytes(n_tensors, numel) bytes, 8-byte aligned (one double per 4096 elements of every tensor,
 * plus 24 bytes per tensor); fewer: SPARCH_EWORKSPACE.  SPARCH_EINVAL, before any device work and in front of the
 * workspace check: n_tensors < 0, a NULL table with n_tensors > 0, a negative numel, a NULL pointer behind a non-empty
 * tensor, max_norm NaN or <= 0, clip NULL.  n_tensors == 0 is a valid call: norm 0, coefficient 1. */
size_t sparch_grad_norm_ws_bytes(int n_tensors, const int64_t* numel);
int sparch_grad_norm(int n_tensors, const float* const* grads, const int64_t* numel, float max_norm, void* ws,
                     size_t ws_bytes, uint32_t* clip, float* tensor_norms, const uint32_t* skip_if_nonzero,
                     void* stream);

/* sparch_adam_step on gradients scaled by clip[1] — g * coefficient, one fp32 multiply, then sparch_adam_step's
 * arithmetic bit for bit; the gradients are read, never rewritten.  Checked in this order: skip_if_nonzero (the no-op
 * and the once-per-call count of sparch_adam_step), then clip[2]: when set, parameters and moments stay untouched (the
 * skipped step was counted in clip[3] by sparch_grad_norm).  clip NULL, or any fault of the table: SPARCH_EINVAL before
 * the first launch. */
int sparch_adam_step_clip(int n_tensors, float* const* params, const float* const* grads,
                          float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                          float step_size, float beta1, float beta2, float bc2_sqrt, float eps,
                          float weight_decay, const float* scalars_dev, uint32_t* skip_if_nonzero,
                          const uint32_t* clip, void* stream);

/* g *= clip[1] in place, for callers that keep another optimizer.  When clip[2] is set the gradients are left as they
 * are (torch.nn.utils.clip_grad_norm_ would write NaNs into all of them): check clip[2], or use the fused step. */
int sparch_scale_grads(int n_tensors, float* const* grads, const int64_t* numel, const uint32_t* clip, void* stream);

/* ---- G1/G2, round 3: the gradient of a BatchNorm'd projection as bf16 planes, made ONCE.
 * sparch_bn_bwd_apply_planes = sparch_bn_bwd_apply (dx = gamma*invstd*(dy - dbeta/M - xhat*dgamma/M)) writing dx as
 * its three exact bf16 planes (3 x M x H uint16, truncation split: dx = t1 + t2 + t3 — the split the dense GEMMs
 * otherwise redo in every workgroup that stages a tile of dx); H % 8 == 0.  dy2 (nullable): the second direction's
 * gradient of a bidirectional layer, added in the same pass (dy + dy2; replaces sparch_add_halves); dx (nullable):
 * the fp32 tensor as well.  Consumers: sparch_gemm6_nn_pp (dX = dx * W: both operands as planes) and
 * sparch_gemm_spike16_tn_ap (dW = dx^T * spikes: dense side as planes) — bit-identical to the fp32-operand entry
 * points; where the pipelined plane kernels do not apply (small or ragged shapes) they read the fp32 operand, which
 * may be NULL only if the caller has checked the shape (M, N >= one tile, K % 32 == 0, 16-byte rows). */
int sparch_bn_bwd_apply_planes(int M, int H, const float* dy, const float* dy2, const float* x, const float* mean,
                               const float* invstd, const float* gamma, const float* dgamma, const float* dbeta,
                               uint16_t* planes, float* dx, void* stream);
int sparch_gemm6_nn_pp(int M, int N, int K, const float* A, const uint16_t* A_planes, int lda, const float* B,
                       const uint16_t* B_planes, int ldb, float* C, int ldc, void* stream, int precision);
int sparch_gemm_spike16_tn_ap(int M, int N, int K, const float* A, const uint16_t* A_planes, int lda,
                              const uint16_t* B16, int ldb, float scale, float* C, int ldc, int zero_diag,
                              int accumulate, void* ws, size_t ws_bytes, void* stream, int precision);

/* ---- a11: the batch upload of the train step (exp.py:355-356 copies a dense fp32 batch to the device every step:
 * 179 MB at the headline shape).  counts (M,K) uint8 = the same binned spike counts (spiking_datasets.py:71-78) at
 * one byte per element; the call expands them into the bf16 plane the first layer's GEMMs read — (M, ldp) uint16
 * bit patterns, ldp >= K a multiple of 8, zeros behind column K: the layout and the values of
 * sparch_plane_bf16_exact on the float batch, whose flag would read 1 — and, if x != NULL, into the fp32 tensor
 * (M rows of ldx floats). */
int sparch_expand_counts_u8(long long M, int K, const uint8_t* counts, uint16_t* plane, int ldp, float* x, int ldx,
                            void* stream);

/* ---- a11: the train step's loss (exp.py:100, 362: nn.CrossEntropyLoss()(output, y), mean over the batch) and its
 * gradient with respect to the logits, one launch: loss[0] = mean_b(logsumexp(x_b) - x_b[y_b]),
 * dlogits = (softmax(x) - onehot(y)) / B.  logits (B,C) fp32, labels (B) int64, loss (1) fp32, dlogits (B,C) fp32.
 * A row whose label lies outside [0,C) (compared as 64 bits) is IGNORED: it adds nothing to the loss and its row of
 * dlogits is zero, so loss and gradient agree; the divisor stays B.  This is not torch's ignore_index, which divides
 * by the number of rows it counted; the reference never passes such a label (its datasets number their classes
 * 0..C-1), so the two cannot be told apart there. */
int sparch_ce_loss(int B, int C, const float* logits, const int64_t* labels, float* loss, float* dlogits,
                   void* stream);

/* ---- Axonal delays (csrc/delay.hip): one learnable time shift per input feature of a layer.
 * delay (K) fp32 is the parameter theta; the kernels take d_i = (int)rintf(min(max(theta_i, 0), max_delay)) themselves
 * (ties to even, a NaN gives 0), 1 <= max_delay <= 255: the host never reads theta.  With len_b the row's own length
 * (T without lengths) and x[b,-1,i] = 0:
 *   y[b,t,i]   = x[b,t-d_i,i]   if d_i <= t < len_b,  else 0
 *   g_x[b,t,i] = g_y[b,t+d_i,i] if t + d_i < len_b,   else 0        (what g_y holds at t >= len_b is never read)
 *   g_delay[i] = gate_i * sum_b sum_{t=d_i}^{len_b-1} g_y[b,t,i] * x_scale * (x[b,t-d_i-1,i] - x[b,t-d_i,i]),
 *   gate_i     = 1 if 0 <= theta_i <= max_delay else 0
 * x, y: (B,T,K) elements of elem_size 2 or 4 bytes moved as raw bytes (the bf16 spike plane, fp32 tensors), unit stride
 * along K, rows ldx / ldy ELEMENTS apart (>= K; batch row b starts at row b T); g_y, g_x fp32 likewise (ldg, ldgx).
 * lengths (B) int32 or NULL (dense); offsets (B+1) int32 non-NULL: the packed layout of sparch_pack_rows — sequence j
 * owns rows [offsets[j], offsets[j] + lengths[j]), T is the longest length, lengths are the sorted ones, and rows that
 * do not exist are not written.  16-byte stores where K, the row strides and the base addresses are multiples of 16
 * bytes, single elements otherwise.
 * sparch_delay_bwd: g_x and g_delay are each optional (not both NULL).  g_delay reads x (x_elem_size 2: bf16 bit
 * patterns; 4: fp32) and sums per-workgroup partial sums from ws (sparch_delay_bwd_workspace_bytes(B,T,K) bytes, 0 for
 * a bad shape) in a fixed order: no atomics, the same bits on every run.
 * sparch_delay_stream: the shift on a chunk x (B,Tc,K) of a stream; hist (B,max_delay,K) contiguous, same element
 * type, holds the last max_delay input steps (row max_delay - 1 the newest; zeros at the start of a stream) and is
 * advanced in place by the Tc steps of the chunk.  x, y and hist must not overlap.
 * SPARCH_EINVAL before any device work: B, T, K < 1, max_delay outside [1, 255], a NULL pointer, a row stride < K,
 * another element size, offsets without lengths; SPARCH_EWORKSPACE: ws too small. */
int sparch_delay_fwd(int B, int T, int K, int elem_size, int max_delay, const float* delay, const void* x,
                     long long ldx, void* y, long long ldy, const int* lengths, const int* offsets, void* stream);
size_t sparch_delay_bwd_workspace_bytes(int B, int T, int K);
int sparch_delay_bwd(int B, int T, int K, int x_elem_size, int max_delay, const float* delay, const float* g_y,
                     long long ldg, const void* x, long long ldx, float x_scale, float* g_x, long long ldgx,
                     float* g_delay, void* ws, size_t ws_bytes, const int* lengths, const int* offsets, void* stream);
int sparch_delay_stream(int B, int Tc, int K, int elem_size, int max_delay, const float* delay, const void* x,
                        long long ldx, void* y, long long ldy, void* hist, void* stream);

/* ---- Spike encoders (csrc/encode.hip): real-valued features -> spike counts, on the device.
 * x (B,T,K) fp32 contiguous; lo, scale (K) fp32; z = (x - lo[k]) * scale[k] — two fp32 roundings, never a fused
 * multiply-add.  The outputs are those of sparch_events_gather_bin / sparch_expand_counts_u8, K' =
 * sparch_spike_encode_width(code, K) columns wide: plane (B*T, ldp) bf16 bit patterns, 16-byte aligned, ldp % 8 == 0,
 * ldp >= K', exact zeros behind column K'; counts uint8 and dense fp32, (B,T,K') contiguous; each may be NULL, not all
 * three.  lengths (B) int32 or NULL: a step t >= lengths[b] emits 0 and does not advance the state.  totals (K') uint32
 * or NULL: the spikes emitted per output column are ADDED to it.  t0 >= 0: the steps this stream has emitted before.
 *   SPARCH_ENCODE_RATE (stochastic, no state; state may be NULL): p = z > 0 ? min(z, 1) : 0 (a NaN gives 0); one spike
 *     iff u < p, u the 24-bit uniform of the dropout hash above on (seed, ((t0 + t) * B + b) * K + k) — a 64-bit,
 *     time-major index: a stream cut into chunks draws the numbers the whole sequence draws.
 *   SPARCH_ENCODE_IF (integrate and fire; state v (B,K) in [0, 1), in / out): drive = z > 0 ? min(z, 255) : 0;
 *     v += drive; n = floor(v); v -= n; n (<= 255) is emitted.  fresh != 0: v starts at 0 and state is only written.
 *   SPARCH_ENCODE_DELTA (send-on-delta; state ref (B,K), in / out; K' = 2K): with fresh != 0 the state starts at 0 and
 *     local step 0 sets ref = z (0 if z is not finite) and emits nothing.  Otherwise e = z - ref,
 *     n = min(floor(|e|), 255); column k (ON) gets n if e > 0, column K + k (OFF) gets n if e < 0; then
 *     ref += copysign(n, e).  A z that is not finite emits nothing and leaves ref as it is.  The threshold delta
 *     enters through scale = 1 / delta.
 * IF and DELTA run one thread per (b, k) over the T steps with the loads of the next SPARCH_ENCODE_PREFETCH steps in
 * flight (they do not depend on the state); RATE is one flat pass.
 * SPARCH_EINVAL before any device work: an unknown code; B, T, K < 1; NULL x, lo or scale; all outputs NULL; NULL
 * state for IF or DELTA; t0 < 0; ldp < K' or ldp % 8 != 0; K' > 65535.  SPARCH_EALIGN: plane not 16-byte aligned. */
#define SPARCH_ENCODE_RATE 0
#define SPARCH_ENCODE_IF 1
#define SPARCH_ENCODE_DELTA 2
#define SPARCH_ENCODE_PREFETCH 8
int sparch_spike_encode(int code, int B, int T, int K, const float* x, const float* lo, const float* scale,
                        float* state, int fresh, long long t0, uint64_t seed, const int* lengths, uint16_t* plane,
                        int ldp, uint8_t* counts, float* dense, uint32_t* totals, void* stream);
int sparch_spike_encode_width(int code, int K);  /* K for RATE and IF, 2K for DELTA; 0 for an unknown code or K < 1 */

/* ---- Synaptic currents (csrc/synapse.hip): a learnable exponential synapse per neuron, in front
 * of a spiking cell.  gamma (H) fp32 is the parameter; the kernels take g_h = min(max(gamma_h, lo), hi) and
 * oma_h = 1.0f - g_h themselves, 0 <= lo <= hi < 1.  z[b,t,h] is the cell's input as the cell kernels form it from
 * (Wx, bias, scale, shift): Wx (+ bias), then fma(., scale, shift) where a scale is given (bias, scale, shift (H) or
 * NULL; shift NULL with a scale: 0).  With len_b the row's own length (T without lengths) and i[b,-1,h] = i0[b,h]
 * (i0 (B,H) or NULL: 0):
 *   i[b,t,h]   = g_h * i[b,t-1,h] + oma_h * z[b,t,h]        0 <= t < len_b   (two products, one add, never fused)
 *   a[b,t,h]   = g_i[b,t,h] + g_h * a[b,t+1,h],  a[b,len_b,h] = 0            (what g_i holds at t >= len_b is never read)
 *   g_z[b,t,h] = oma_h * a[b,t,h]
 *   g_gamma[h] = gate_h * (sum_b sum_{t<len_b} a[b,t,h] * (i[b,t-1,h] - i[b,t,h])) / oma_h,
 *   gate_h     = 1 if lo <= gamma_h <= hi else 0
 * All tensors fp32, (B,T,H) with unit stride along H and rows ldwx / ldi / ldg / ldgz ELEMENTS apart (>= H; batch row b
 * starts at row b T).  lengths (B) int32 or NULL (dense): steps t >= len_b of i_out and g_z are written as zeros and
 * do not advance the state.  offsets (B+1) int32 non-NULL: the packed layout of sparch_pack_rows — sequence j owns rows
 * [offsets[j], offsets[j] + lengths[j]), T is the longest length, rows that do not exist are not written; i0, i_T hold
 * the sequences in the plan's order.  16-byte accesses where H, the row strides and the base addresses are multiples of
 * 16 bytes, single elements otherwise.
 * sparch_synapse_fwd: i_T (B,H) or NULL receives each row's state after its last valid step; it may alias i0 (a
 * stream's chunk step: T = the chunk's steps, the carried state advanced in place).
 * sparch_synapse_bwd: i is the forward's i_out, i0 the forward's; g_z and g_gamma are each optional (not both NULL).
 * g_gamma is summed from per-sequence partial sums in ws (sparch_synapse_bwd_workspace_bytes(B,T,H) bytes, 0 for a bad
 * shape) in a fixed order: no atomics, the same bits on every run.
 * bn_x (B,T,H) fp32, rows ldbn apart, or NULL: the layer's raw projection under BatchNorm; with it (and bn_mean,
 * bn_invstd (H), bn_ws (2,B,H), g_z, all required then) the call also writes BatchNorm backward's per-sequence partial
 * sums, bn_ws[0][b][h] = sum_t g_z and bn_ws[1][b][h] = sum_t g_z * ((bn_x - mean) * invstd), added from the row's last
 * step to its first as the cell backward kernels add theirs (sparch_colsum_clamped finishes them).
 * SPARCH_EINVAL before any device work: B, T, H < 1, a NULL required pointer, a row stride < H, offsets without
 * lengths, lo / hi outside 0 <= lo <= hi < 1; SPARCH_EWORKSPACE: ws too small. */
int sparch_synapse_fwd(int B, int T, int H, const float* Wx, long long ldwx, const float* bias, const float* scale,
                       const float* shift, const float* gamma, float lo, float hi, const float* i0, float* i_out,
                       long long ldi, float* i_T, const int* lengths, const int* offsets, void* stream);
size_t sparch_synapse_bwd_workspace_bytes(int B, int T, int H);
int sparch_synapse_bwd(int B, int T, int H, const float* g_i, long long ldg, const float* i, long long ldi,
                       const float* i0, const float* gamma, float lo, float hi, float* g_z, long long ldgz,
                       float* g_gamma, void* ws, size_t ws_bytes, const float* bn_x, long long ldbn, const float* bn_mean,
                       const float* bn_invstd, float* bn_ws, const int* lengths, const int* offsets, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARCH_HIP_H */

// The body of the LIF / adLIF reverse pass (cell.hip includes it once per kernel family, behind the kernel's
// signature): template parameters ADAPT, VEC, S16, BN, DROP, the argument `c` (CellArgs, CellLenArgs or CellPkArgs) and
// the macros below.  The families: cell_bwd_pipe_kernel / cell_bwd_pipe_sg_kernel (no lengths),
// cell_bwd_pipe_len_kernel / cell_bwd_pipe_len_sg_kernel (ragged, masked), cell_bwd_pipe_pk_kernel /
// cell_bwd_pipe_pk_sg_kernel (ragged, packed), cell_bwd_pipe_st_kernel / cell_bwd_pipe_st_sg_kernel (stateful:
// CellStArgs, no lengths, one direction).
//   SURROGATE_GATE(ds, x)  the surrogate gradient's gate: boxcar_gate, or smooth_gate on the `_sg` kernels' second argument
//   ROW_LEN(b)             the row's length; TAIL_ZERO(t, v): the incoming gradient v of step t, 0 at or past that length.
//                          T and v itself except in the `_len` family.  (From a zero gradient the carries du, dw stay zero
//                          over the tail, and with them dWx and every partial sum.)
//   ROW_T(b)               the steps row b runs: c.T; packed: the sequence's own length
//   ROW0(r)                the first row of row r's (rows, H) tensors: r * T; packed: the sequence's offset (row0_pk,
//                          which ROW0_INIT(b) loads once; 0 elsewhere)
//   ROW_THREADS(HQ)        threads per row: HQ; packed: HQ padded to whole waves, so that ROW_T and ROW0 are wave-uniform
//                          (scalars, like c.T), and ROW_GUARD(h) retires the lanes behind the row (empty elsewhere)
//   ST_LOAD               stateful: declares st_gu / st_gw / st_gs, the gradient arriving on the returned final state
//                          (u_T, w_T, s_T), 0 where the pointer is null; empty elsewhere
//   ST_DS(t, gs)           declares ds, the spike's gradient of step t: gs - alpha du_{t+1} [+ b dw_{t+1}], added in this order.
//                          Stateful: gs + S_t with S_t = -alpha du_{t+1} [+ b dw_{t+1}] formed FIRST, and S_T = g_sT at the
//                          reverse pass's first step (t = T - 1, where du_{T+1} = dw_{T+1} = 0) — S_t is what ST_TAIL hands
//                          the chunk before as its g_sT, so a chunk boundary rounds exactly as an inner step does.  g_sT
//                          enters BEHIND the dropout scale: dropout scales the output, not the state
//   ST_DU(t, gate)         declares du: gate + alpha du_{t+1} [+ a dw_{t+1}], in this order.  Stateful: gate + U_t with
//                          U_t = alpha du_{t+1} [+ a dw_{t+1}] formed first, U_T = g_uT
//   ST_ADD(t, v, g)        v + g at the reverse pass's first step, else v; (v) elsewhere (dw_T: g_wT = beta dw_{T+1})
//   ST_TAIL                stateful: stores the initial state's gradient from the last carries du_1, dw_1 —
//                          g_u0 = alpha du_1 + a dw_1, g_w0 = beta dw_1, g_s0 = -alpha du_1 + b dw_1; empty elsewhere
// Text, not a function: inlined from a shared __device__ function the box-car kernels came
// out of the compiler with another schedule, and they are held to the instructions they had (DESIGN.md section 6).
{
    constexpr int D = pipe_depth(VEC, 3 + (ADAPT ? 1 : 0) + (BN ? 1 : 0));
    const int HQ = ROW_THREADS(c.H / VEC);
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Bp = c.B * c.dirs;
    if (idx >= (long long)Bp * HQ) return;
    const int bp = (int)(idx / HQ), h = (int)(idx % HQ) * VEC;
    ROW_GUARD(h)
    const int d = bp / c.B, b = bp - d * c.B;
    [[maybe_unused]] const int row0_pk = ROW0_INIT(b);
    const int T = ROW_T(b), H = c.H, HO = c.H * c.dirs;
    [[maybe_unused]] const int row_len = ROW_LEN(b);

    float al[VEC], oma[VEC], be[VEC], pa[VEC], pb[VEC], gr[VEC];
    float du_n[VEC], dw_n[VEC], u_t[VEC];
    float acc_al[VEC], acc_be[VEC], acc_a[VEC], acc_b[VEC];
    float bn_mu[VEC], bn_is[VEC], acc_dy[VEC], acc_dyx[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        bn_mu[e] = BN ? c.bn_mean[h + e] : 0.f;
        bn_is[e] = BN ? c.bn_invstd[h + e] : 0.f;
        acc_dy[e] = acc_dyx[e] = 0.f;
        const Neuron<ADAPT> p = neuron_load<ADAPT>(c.alpha, c.beta, c.a, c.b, h + e);
        al[e] = p.al; oma[e] = p.oma; be[e] = p.be; pa[e] = p.pa; pb[e] = p.pb;
        gr[e] = c.g_rate ? c.g_rate[(size_t)d * H + h + e] * c.g_rate_scale : 0.0f;
        du_n[e] = dw_n[e] = 0.f;
        acc_al[e] = acc_be[e] = acc_a[e] = acc_b[e] = 0.f;
    }
    ld_saved<VEC>(u_t, c.u_save, (ROW0(bp) + (T - 1)) * H + h, S16);
    // the initial states: read by cell step 0 (the last of the reverse pass) only; fetched here, off the loop
    float u0v[VEC], w0v[VEC], s0v[VEC];
    ldv<VEC>(u0v, c.u0 + (size_t)bp * H + h);
    ldv<VEC>(s0v, c.s0 + (size_t)bp * H + h);
    if (ADAPT) ldv<VEC>(w0v, c.w0 + (size_t)bp * H + h);
    constexpr bool drop = DROP;
    const uint64_t seed = drop ? resolve_seed(c.seed) : 0;
    ST_LOAD

    struct Slot { float g[VEC]; float xr[BN ? VEC : 1]; SavedVec<VEC, S16> up; SavedVec<VEC, S16> wp; };
    const float* grow = c.g_out + ROW0(b) * HO + (size_t)d * H + h;
    const float* xrow = BN ? c.bn_x + ROW0(b) * H + h : nullptr;
    const size_t srow = ROW0(bp) * H + h;
    auto fetch = [&](Slot& q, int t) __attribute__((always_inline)) {
        const int tc = max(t, 0);  // before the start: a step that is in range and never used
        const int tt = d ? (T - 1 - tc) : tc;
        ldv<VEC>(q.g, grow + (size_t)tt * HO);
        if constexpr (BN) ldv<VEC>(q.xr, xrow + (size_t)tt * H);
        const size_t i = srow + (size_t)max(tc - 1, 0) * H;  // cell step 0 reads row 0 (unused: u0 / w0 below)
        q.up.load(c.u_save, i);
        if (ADAPT) q.wp.load(c.w_save, i);
    };
    // FIRST: the step may be cell step 0 (tail of the reverse pass only — the main loop stops before it)
    auto step = [&](int t, const Slot& q, auto first_tag) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const int tt = d ? (T - 1 - t) : t;
        const size_t o = (ROW0(b) + tt) * HO + (size_t)d * H + h;
        float up[VEC], wp[VEC], sp[VEC], dwx[VEC];
        q.up.expand(up);
        if (ADAPT) q.wp.expand(wp);
        const bool t0 = FIRST && t == 0;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (t0) { up[e] = u0v[e]; if (ADAPT) wp[e] = w0v[e]; }
            sp[e] = t0 ? s0v[e] : (spike_of(up[e], c.theta) ? 1.0f : 0.0f);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float k = drop ? keep_scale(seed, o + e, c.p_drop, c.inv_keep) : 1.0f;
            const float gs = TAIL_ZERO(t, (q.g[e] + gr[e]) * k);
            ST_DS(t, gs)
            const float xs = u_t[e] - c.theta;
            ST_DU(t, SURROGATE_GATE(ds, xs))                              // snns.py:33-35
            dwx[e] = oma[e] * du;
            if (BN) {  // BatchNorm backward's column sums (dy = dWx, xhat = (x - mean) * invstd)
                acc_dy[e] += dwx[e];
                acc_dyx[e] += dwx[e] * ((q.xr[BN ? e : 0] - bn_mu[e]) * bn_is[e]);
            }
            const float qq = up[e] - sp[e];
            acc_al[e] += du * (qq - u_t[e]);  // d u_t / d alpha = (q - u_t)/(1-alpha); scaled at the end
            if (ADAPT) {
                const float dw = ST_ADD(t, be[e] * dw_n[e] - dwx[e], st_gw[e]);
                acc_be[e] += dw * wp[e];
                acc_a[e] += dw * up[e];
                acc_b[e] += dw * sp[e];
                dw_n[e] = dw;
            }
            du_n[e] = du;
            // carried into the next step as a COPY made here: kept in the slot's own register the value outlives the
            // slot's refill, the refill needs another register, and hipcc shuffles the whole ring through `v_mov`s in
            // mid-loop — each of which waits for a load issued a few operations earlier
            asm volatile("v_mov_b32 %0, %1" : "=&v"(u_t[e]) : "v"(up[e]));
        }
        stv<VEC>(c.dWx + (ROW0(bp) + tt) * H + h, dwx);
    };

    Slot ring[D];
#pragma unroll
    for (int j = 0; j < D; ++j) fetch(ring[j], T - 1 - j);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // see the forward kernel
    int i0 = 0;  // reverse index: step t = T - 1 - i
    for (; i0 + D <= T - 1; i0 += D) {  // steps t >= 1 only
#pragma unroll
        for (int j = 0; j < D; ++j) {  // consume, then refill (see the forward kernel)
            step(T - 1 - (i0 + j), ring[j], std::false_type{});
            fetch(ring[j], T - 1 - (i0 + j + D));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (i0 + j >= T) break;
        step(T - 1 - (i0 + j), ring[j], std::true_type{});
    }
    const size_t plane = (size_t)Bp * H;
    float* ws = c.dparam_ws + (size_t)bp * H + h;
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc_al[e] = acc_al[e] / oma[e];
    stv<VEC>(ws, acc_al);
    if (ADAPT) {
        stv<VEC>(ws + plane, acc_be);
        stv<VEC>(ws + 2 * plane, acc_a);
        stv<VEC>(ws + 3 * plane, acc_b);
    }
    if (BN) {
        stv<VEC>(ws + 4 * plane, acc_dy);
        stv<VEC>(ws + 5 * plane, acc_dyx);
    }
    ST_TAIL
}

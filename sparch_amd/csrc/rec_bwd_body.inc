// The body of the RLIF / RadLIF reverse pass (reccell.hip includes it once per kernel family, behind the kernel's
// signature): template parameters ADAPT, KGW, NW, EXT, NP, S16, CW, the argument `a` (RecArgs, or RecSgArgs), and
// SURROGATE_GATE(ds, x), the surrogate gradient's gate — boxcar_gate for rec_bwd_kernel, smooth_gate on `a.sg`
// for rec_bwd_sg_kernel, any_gate for the ragged rec_bwd_len_kernel (RecLenArgs) — and ROW_LEN(b) / TAIL_ZERO(t, v), the
// row's length and the select on the incoming gradient of padded steps.  Text, not a function: see cell_bwd_body.inc.
// The packed rec_bwd_pk_kernel (RecPkArgs, whole-sequence launches) differs in five more macros; elsewhere they are the
// expressions this body always had:
//   ROW_PK_INIT         declares row0 (the row's first packed row) and t_tile (the length of the tile's first, longest
//                       row: the same in all of the tile's workgroups, so the hand-off protocol is untouched); else empty
//   T_HI                the step count the launch walks down from: a.t_end; packed: min(a.t_end, t_tile)
//   T_RING              the bound of the ring's conditions (is there a step t + 1 / t + 2): T; packed: t_tile
//   RROW(r, t)          row of step t of row r in the (rows, .) tensors: r * T + t; packed: row0 + min(t, row_len - 1) —
//                       a shorter row's loads stay inside its own packed rows
//   ROW_STORE(t)        whether step t's dWx / s_prev16 are stored: true; packed: t < row_len (a store behind a row's
//                       end would land in the next sequence).  Such a step's incoming gradient is zero (TAIL_ZERO), its
//                       recurrent term is its own zero dWx row times V^T: it computes and publishes zeros.
// The stateful rec_bwd_st_kernel (RecStArgs, whole-sequence launches, fp32 operands and saves) differs in four more, empty
// (ST_PLUS(v, g): v) elsewhere:
//   ST_PRE_LOAD         declares st_s / st_u: at the reverse pass's first step (t = T - 1) g_sT / g_uT of the thread's four
//                       columns, else 0.  g_sT joins the incoming gradient BEHIND the dropout scale; g_uT stands in the
//                       place of alpha du_{T+1} (which is 0 there)
//   ST_POST_LOAD        declares st_w: g_wT at that step, else 0 (dw_T = g_wT - (1 - alpha) du_T)
//   ST_PLUS(v, g)       v + g
//   ST_TAIL             stores g_u0 = alpha du_1 + a dw_1, g_w0 = beta dw_1 and the pointwise part of g_s0,
//                       -alpha du_1 + b dw_1 (the host adds dWx_1 Vm^T)
{
    static_assert(CW == 1 || (CW == 2 && NW == 8 && !EXT && NP == 1), "64-column workgroups: bf16 operand mode, 8 waves");
    // cross-wave reduction tiles: written before the step's first barrier, read after it by the pointwise
    // waves, which reach the second (publish) barrier only when done with them -> one buffer
    __shared__ __attribute__((aligned(16))) float red[NW][CW][RT * RED_LD4];
    // lo plane of the V^T slice lives in LDS (64 KiB at H=1024) so the register file holds the
    // hi/mid planes (128 VGPRs) plus all 32 in-flight fp32 dWx tile loads (128 VGPRs) without spilling
    __shared__ __attribute__((aligned(16))) u32x4 vlo[NP == 3 ? NW : 1][NP == 3 ? KGW : 1][2][64];
    // neuron constants (alpha, beta, a, b, rate gradient, BatchNorm mean / invstd) of the tile's 8 column quads,
    // per direction (the rate gradient depends on it): kept in LDS and re-read each step — the 8-wave kernel's
    // 256-register budget has no room to hold them.  (Rounds 1-2 kept a copy per THREAD: 28 KB for 1.8 KB of data.)
    __shared__ __attribute__((aligned(16))) f32x4 pcol[7][2][8 * CW];
    // initial states of the tile (u0, w0, s0): read by cell step 0 only — from LDS, so that the loop body holds no
    // global load on one path only (hipcc's wait-count pass merges such paths with an `s_waitcnt vmcnt(0)`)
    __shared__ __attribute__((aligned(16))) f32x4 first_tile[3][256 * CW];
    // running parameter-gradient partial sums (alpha, beta, a, b) of the thread's 4 columns: touched once per
    // step, off the critical path -> LDS, so that the hot loop's registers do not spill
    // (in registers they were measured no faster: 1.37 vs 1.36 ms per launch)
    __shared__ __attribute__((aligned(16))) f32x4 pacc[6][256 * CW];  // + BatchNorm's sum dWx, sum dWx*xhat
    __shared__ int abort_flag[2];
    __shared__ int xcd_local_flag;
    // BXS (8-wave kernels): the step's bulk HBM stores (dWx for the GEMMs, the bf16 plane of s_{t-1}) are issued
    // by the four waves that hold NO pointwise state, one step later: the pointwise waves stage the 24 bytes per
    // thread in LDS after the publish barrier, the upper waves pick them up behind the NEXT step's reduction
    // barrier — where they would otherwise idle through the pointwise phase — and issue the stores there, ~2.4 k
    // cycles ahead of their own next tile loads.  On the pointwise waves the stores sat ~0.8 k cycles in front of
    // the next step's tile loads, and `vmcnt` (in order, counts stores) made the first k-group wait for their
    // acknowledgement: timing ablation without the stores 1.29 -> 1.16 ms per launch.
    constexpr bool BXS = NW == 8 && !EXT && CW == 1;
    __shared__ __attribute__((aligned(16))) f32x4 stage_dwx[BXS ? 256 : 1];
    __shared__ __attribute__((aligned(8))) u32x2 stage_sp[BXS ? 256 : 1];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, hh = lane >> 5;
    const int rt = a.rt_base + (int)(blockIdx.x % a.n_rt_launch);
    const int ctw = (int)(blockIdx.x / a.n_rt_launch);  // the workgroup's index among its row tile's workgroups
    const int T = a.T, H = a.H, HO = a.H * a.dirs;

    const bool pw = tid < 256 * CW;  // threads that own a (row, 4 columns) piece of the tile's pointwise state
    const bool pw_wave = NW == 4 || CW == 2 || wave < 4;  // the same, as a scalar
    const int cj = CW == 2 ? tid >> 8 : 0;                // this thread's column group within the workgroup
    const int ct = ctw * CW + cj;                         // ... as a 32-column group of the layer
    const int cqx = cj * 8 + (tid & 7);                   // index of its column quad in the workgroup's tables
    const int r = (tid & 255) >> 3, cq = tid & 7;
    const int bp = rt * RT + r, col = ct * CT + cq * 4;
    const bool valid = pw && bp < a.Bp && col < H;
    const bool valid_hi = !pw && bp < a.Bp && col < H;  // upper-wave thread: same (row, columns) as tid - 256
    const int bpc = min(bp, a.Bp - 1), colc = min(col, H - 4);
    const int d = bpc / a.B, b = bpc - d * a.B;
    [[maybe_unused]] const int row_len = ROW_LEN(b);
    ROW_PK_INIT

    u32x4 vb[CW][KGW][2][NP == 3 ? 2 : 1];
#pragma unroll
    for (int c = 0; c < CW; ++c)
#pragma unroll
    for (int kk = 0; kk < (EXT ? 0 : KGW); ++kk) {
        const int kg = wave + NW * kk;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const u32x4* src = a.vpack + ((((size_t)(ctw * CW + c) * a.nkg + kg) * 2 + ks) * 3) * 64 + lane;
            vb[c][kk][ks][0] = src[0];
            if constexpr (NP == 3) {
                vb[c][kk][ks][1] = src[64];
                vlo[wave][kk][ks][lane] = src[128];
            }
        }
    }

    float du_n[4], dw_n[4], u_t[4];
    if (tid < 16 * CW) {  // thread = (direction, column quad of the workgroup)
        const int dq = tid / (8 * CW), qx = tid % (8 * CW);
        const int cc = min(ctw * CW * CT + qx * 4, H - 4), dd = min(dq, a.dirs - 1);
        f32x4 c_al, c_be, c_a, c_b, c_gr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            c_al[e] = clampf(a.alpha[cc + e], SP_ALPHA_LO, SP_ALPHA_HI);  // (neuron.h: these four copies stay)
            c_be[e] = ADAPT ? clampf(a.beta[cc + e], SP_BETA_LO, SP_BETA_HI) : 0.f;
            c_a[e] = ADAPT ? clampf(a.a[cc + e], SP_A_LO, SP_A_HI) : 0.f;
            c_b[e] = ADAPT ? clampf(a.b[cc + e], SP_B_LO, SP_B_HI) : 0.f;
            c_gr[e] = a.g_rate ? a.g_rate[(size_t)dd * H + cc + e] * a.g_rate_scale : 0.0f;
        }
        pcol[0][dq][qx] = c_al; pcol[1][dq][qx] = c_be; pcol[2][dq][qx] = c_a;
        pcol[3][dq][qx] = c_b; pcol[4][dq][qx] = c_gr;
        if (a.bn_x) { pcol[5][dq][qx] = ld4(a.bn_mean + cc); pcol[6][dq][qx] = ld4(a.bn_invstd + cc); }
    }
    if (pw && a.t_begin == 0) {
        first_tile[0][tid] = ld4(a.u0 + (size_t)bpc * H + colc);
        if (ADAPT) first_tile[1][tid] = ld4(a.w0 + (size_t)bpc * H + colc);
        first_tile[2][tid] = ld4(a.s0 + (size_t)bpc * H + colc);
    }
    const bool bn = a.bn_x != nullptr;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        du_n[e] = dw_n[e] = 0.f;
    }
    const size_t plane = (size_t)a.Bp * H;
    float* ws = a.dparam_ws + (size_t)bpc * H + colc;
    if (pw) {
        const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
        f32x4 v_al = z4, v_be = z4, v_a = z4, v_b = z4;
        if (a.t_end < T) {  // resume a chunked pass: carried state + partial sums
            f32x4 v;
            v_al = ld4(ws);
            v = ld4(ws + 4 * plane); du_n[0] = v.x; du_n[1] = v.y; du_n[2] = v.z; du_n[3] = v.w;
            if (ADAPT) {
                v_be = ld4(ws + plane); v_a = ld4(ws + 2 * plane); v_b = ld4(ws + 3 * plane);
                v = ld4(ws + 5 * plane); dw_n[0] = v.x; dw_n[1] = v.y; dw_n[2] = v.z; dw_n[3] = v.w;
            }
        }
        pacc[0][tid] = v_al; pacc[1][tid] = v_be; pacc[2][tid] = v_a; pacc[3][tid] = v_b;
        if (bn) {
            pacc[4][tid] = a.t_end < T ? ld4(ws + 6 * plane) : z4;
            pacc[5][tid] = a.t_end < T ? ld4(ws + 7 * plane) : z4;
        }
    }
    {
        const f32x4 v = expand_saved(ld_saved_raw<S16>(a.u_save, RROW(bpc, T_HI - 1) * H + colc));
        u_t[0] = v.x; u_t[1] = v.y; u_t[2] = v.z; u_t[3] = v.w;
    }
    if (tid < 2) abort_flag[tid] = 0;
    const unsigned my_xcc = xcc_id();
    xcd_agree((EXT || !a.xcd_tab) ? nullptr : (gu32*)a.xcd_tab + (size_t)rt * a.n_ct, SENTINEL, a.n_ct / CW, ctw, my_xcc, tid, &xcd_local_flag);
    __syncthreads();
    const bool xcd_local = xcd_local_flag != 0;  // this row tile's workgroups share an XCD: plain hand-off stores

    // hand-off ring: ring[slot][rt][ct] = one 4 KiB fp32 tile in fragment order; one buffer resource
    constexpr unsigned PT = (unsigned)ptile_bytes<NP>();  // bytes of one hand-off tile
    const unsigned slot_bytes = (unsigned)((size_t)a.n_rt_total * a.n_ct * PT);
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(a.ring, 0, (int)(RING * slot_bytes), 0x00020000);
    const unsigned rt_off = (unsigned)((size_t)rt * a.n_ct * PT);

    const bool drop = a.p_drop > 0.0f;
    const uint64_t seed = drop ? resolve_seed(a.seed) : 0;
    // The inputs of a reverse step (incoming gradient, raw projection for BatchNorm's sums, the saved u / w of the
    // step before) as FOUR UNCONDITIONAL loads (three without adaptation): every path through the time loop then
    // issues the same vector-memory instructions and hipcc's counted waits are exact.  (Rounds 1-2: `if (bn)`,
    // `if (t > 0) .. else u0`, and a width switch for bf16 saves around them — on the merged paths the wait-count
    // pass fell back to `vmcnt(0)`, and register reuse between the arms serialized the loads.)  Without BatchNorm
    // the host points `bn_src` at the incoming gradient (a readable range of the same extent); cell step 0 reads row 0
    // of the saves and is given u0 / w0 from LDS at its use; bf16 saves stay packed until then (`expand_saved`).
    typedef typename SavedRaw<S16>::type saved_raw;
    auto load_step = [&](int t, f32x4& g, saved_raw& up, saved_raw& wp, f32x4& xr) {
        const int tt = d ? (T - 1 - t) : t;
        const float* gp = a.g_out + RROW(b, tt) * HO + (size_t)d * H + colc;
        g = ld4s(gp);
        xr = ld4s(a.bn_src + RROW(b, tt) * H + colc);
        const size_t o = RROW(bpc, (size_t)max(t - 1, 0)) * H + colc;
        up = ld_saved_raw<S16>(a.u_save, o);
        if (ADAPT) wp = ld_saved_raw<S16>(a.w_save, o);
    };
    f32x4 g_nx = {0.f, 0.f, 0.f, 0.f}, xr_nx = g_nx;
    saved_raw up_nx = {}, wp_nx = {};
    if (pw) load_step(T_HI - 1, g_nx, up_nx, wp_nx, xr_nx);
    vm_settled();  // every prologue load is in: the loop is entered with nothing outstanding
    // (Unlike the forward, holding this kernel's fp32 stores / prefetch back until after the tag poll does
    // not pay: measured 16.8k -> 18.2k cycles per step, the deferred traffic then competes with the tile loads.)
    PROF_DECL

    int t_stop = -1;  // the step an abort was seen at (diagnostics of the status word)
    for (int t = T_HI - 1; t >= a.t_begin; --t) {
        PROF_STAMP(-1);
        const int pt = CW == 2 ? tid : (tid & 255);
        const f32x4 gv = g_nx, xrv = xr_nx;
        f32x4 upv = expand_saved(up_nx), wpv = expand_saved(wp_nx);
        if (t == 0) {  // cell step 0: the initial states (LDS; filled in the prologue when the launch ends at t = 0)
            upv = first_tile[0][pt];
            if (ADAPT) wpv = first_tile[1][pt];
        }
        float rec[4] = {0.f, 0.f, 0.f, 0.f};
        const int par = t & 1;
        // Everything of the reverse step that does not depend on the recurrent product — the dropout factor's
        // hash, the incoming gradient, alpha * du_{t+1}, the adaptation terms — is computed BEFORE the reduction
        // barrier, behind the first tile loads' issue (the pointwise waves would only wait there): the chain
        // behind the barrier is then `+ rec`, the box-car gate, two adds and a multiply.  Same operations in the
        // same order as the reference's autograd replay: bit-identical results.
        const int tt = d ? (T - 1 - t) : t;
        const size_t o_out = RROW(b, tt) * HO + (size_t)d * H + colc;
        float pre_ds[4], pre_aldu[4], pre_padw[4];
        auto pre_pointwise = [&]() __attribute__((always_inline)) {
            const f32x4 al = pcol[0][d][cqx], pa = pcol[2][d][cqx], pb = pcol[3][d][cqx], gr = pcol[4][d][cqx];
            ST_PRE_LOAD
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float k = drop ? keep_scale(seed, o_out + e, a.p_drop, a.inv_keep) : 1.0f;
                const float gs = ST_PLUS(TAIL_ZERO(t, (gv[e] + gr[e]) * k), st_s[e]);
                pre_aldu[e] = al[e] * du_n[e];
                float ds = gs - pre_aldu[e];
                pre_padw[e] = ADAPT ? pa[e] * dw_n[e] : 0.f;
                if (ADAPT) ds = ds + pb[e] * dw_n[e];
                pre_aldu[e] = ST_PLUS(pre_aldu[e], st_u[e]);
                pre_ds[e] = ds;
                asm volatile("" : "+v"(pre_ds[e]), "+v"(pre_aldu[e]), "+v"(pre_padw[e]));  // not sunk behind the barrier
            }
        };
        if (!(t + 1 < T_RING && !EXT) && pw) pre_pointwise();

        if (t + 1 < T_RING && !EXT) {
            // ---- the dWx_{t+1} tiles of this wave's producers: load, re-load what has not landed yet
            const unsigned slot = (unsigned)((t + 1) % RING);
            const unsigned base = slot * slot_bytes + rt_off + (unsigned)lane * 16u;
            // The CU's fill rate from L2 (~70 GB/s: 128 KiB of tiles per step take ~3.7 k cycles) holds a wave
            // in the ISSUE of its loads once the memory pipeline is full, so the issue is spread out: two
            // k-groups ahead of the one being multiplied, the rest of the loads interleaved with the MFMAs
            // (the partner wave on the SIMD computes while this one is stuck issuing).
            // Tried on top (round 2, not kept): splitting group kk+1 INSIDE the MFMAs of group kk (software
            // pipeline with sched_group_barrier 1 MFMA : 8 VALU, and hand-placed half-pairs between the MFMAs
            // with scheduling barriers) — hipcc hoists the ~90 split instructions above the MFMAs in every block
            // that ends in the next group's branch, and the launch time did not move (1.37 vs 1.34-1.39 ms); pinned
            // with one asm statement per MFMA + 5-6 split instructions (bit-exact, 255 VGPRs) it was 1.39-1.43 ms:
            // the SIMD's issue port is NOT what bounds the phase.
            // With the producers' data always ready (consuming step t+2's tiles, a timing experiment) the step is
            // 9.7 k cycles against 10.2 k: the phase is throughput-, not hand-off-latency-bound — L2 port
            // 3.7 k, and MFMA (3.1 k) + split VALU (2.8 k) add up on the SIMD instead of overlapping.
            // (bf16 operand mode, NP = 1: a third of the bytes — all k-groups are issued at once; one group ahead
            // made that mode's tile phase four sequential L2 round trips, 3.2 k cycles with 16 MFMAs per SIMD)
            constexpr int AHEAD = NP == 1 ? KGW : (KGW < TILES_AHEAD ? KGW : TILES_AHEAD);
            u32x4 raw[KGW][2][NP];  // [k-group][k16-step][plane]: MFMA A fragments as they come off the wire
            // (More than one k-group in flight at the step's start only loses time — a tile load issued before its
            // producer's stores have landed returns sentinels and costs a second, serialized round trip in
            // `settle_ptile`: 10.3 k -> 11.4 k cycles per step with all loads up front, 1.04 -> 1.34 ms per launch with
            // two groups ahead.  Probing one dword per producer sample before the burst is one more round trip: 1.117
            // vs 1.040 ms.  Delaying the upper waves' first loads loses too — they are the LATE ones at the reduction
            // barrier.  DESIGN.md, "Retired experiment switches".)
#pragma unroll
            for (int kk = 0; kk < AHEAD; ++kk) issue_ptile<NW, NP>(raw[kk], rsrc, base, wave + NW * kk, a.n_ct);
            PROF_STAMP(0);  // first tile load issue
            if (pw) pre_pointwise();
            f32x16 acc[CW];
#pragma unroll
            for (int c = 0; c < CW; ++c)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[c][i] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KGW; ++kk) {
                // k-group by k-group: the MFMAs of one run while the loads of the next are still in flight
                // (scheduling barriers: hipcc otherwise hoists the next group's check, and its wait, into this
                // group's MFMAs)
                __builtin_amdgcn_sched_barrier(0);
                settle_ptile<NP>(raw[kk], rsrc, base + (unsigned)(wave + NW * kk) * PT, &abort_flag[par]);
                if (kk + AHEAD < KGW) issue_ptile<NW, NP>(raw[kk + AHEAD], rsrc, base, wave + NW * (kk + AHEAD), a.n_ct);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if constexpr (NP == 1) {  // bf16 operand mode: bf16(dWx) x bf16(V^T), one product
#pragma unroll
                        for (int c = 0; c < CW; ++c) acc[c] = mfma_bf16(raw[kk][ks][0], vb[c][kk][ks][0], acc[c]);
                    } else {
                    const u32x4 p1 = raw[kk][ks][0], p2 = raw[kk][ks][NP - 2], p3 = raw[kk][ks][NP - 1];
                    const u32x4 vl = vlo[wave][kk][ks][lane];
                    // six largest cross terms of (t1+t2+t3)(V_hi+V_mid+V_lo), small first.  Dropped:
                    // t3*mid (|t3| < 2^-14 |x| after two 8-bit truncations, |V_mid| <= 2^-8 |V|: <= 2^-22 of
                    // |x||V|), t2*lo (<= 2^-23) and t3*lo.  Worst-case per product; summed over a row the
                    // dropped part measures 3e-9 of sum|x||V| (7 terms: 1.4e-9; an fp32 sgemm's own
                    // rounding: 1e-7) — the same kind of cut as the dense 6-term GEMM.
                    acc[0] = mfma_bf16(p2, vb[0][kk][ks][NP == 3], acc[0]);  // t2*mid
                    acc[0] = mfma_bf16(p3, vb[0][kk][ks][0], acc[0]);  // t3*hi
                    acc[0] = mfma_bf16(p1, vl, acc[0]);       // t1*lo
                    acc[0] = mfma_bf16(p2, vb[0][kk][ks][0], acc[0]);  // t2*hi
                    acc[0] = mfma_bf16(p1, vb[0][kk][ks][NP == 3], acc[0]);  // t1*mid
                    acc[0] = mfma_bf16(p1, vb[0][kk][ks][0], acc[0]);  // t1*hi
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                float* rd = red[wave][c];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
                    rd[row * RED_LD4 + li] = acc[c][i];
                }
            }
            PROF_STAMP(1);  // per k-group: wait, split, MFMA; LDS write
        }
        if (xcd_local && xcc_id() != my_xcc) lds_flag_set(&abort_flag[par]);  // moved to another XCD
        lds_barrier();
        vm_settled();  // tile loads are in, last step's stores and this step's prefetch long complete
        PROF_STAMP(2);  // barrier
        if (lds_flag_read(&abort_flag[par])) { t_stop = t; break; }
        // The next step's inputs (g, u, w, raw projection: HBM loads) are requested HERE, behind the reduction barrier:
        // a pointwise phase and a publish ahead of the next tile loads, so that no HBM round trip sits between the
        // pointwise waves and their first k-group (`vmcnt` is in order).  Measured per launch, A/B in one call: at the
        // loop top 1.083 ms, behind the last tile load 1.057, here 1.036, behind the publish stores 1.049, behind the
        // publish barrier 1.097 (DESIGN.md, "Retired experiment switches").
        if (pw && t - 1 >= a.t_begin) load_step(t - 1, g_nx, up_nx, wp_nx, xr_nx);
        if (BXS && !pw) {
            // The sentinels go back into this workgroup's tile of step t+2 (every peer has consumed it: see the
            // header) from the waves WITHOUT pointwise state, which idle from here to the publish barrier — as
            // 16-byte stores, one or two per thread, instead of three 8-byte stores per pointwise thread between
            // the publish stores and the publish barrier, i.e. on the step's critical chain (round 3).  These
            // waves' `vm_settled()` behind the next reduction barrier retires them two barriers before the slot
            // is written again (the publish of step t-2).
            const u32x4 sent4 = {SENTINEL, SENTINEL, SENTINEL, SENTINEL};
            const unsigned so = (unsigned)((t + 2) % RING) * slot_bytes + rt_off + (unsigned)ct * PT;
            constexpr int PIECES = NP * 128;  // 16-byte pieces of one tile
#pragma unroll
            for (int q = 0; q < (PIECES + 255) / 256; ++q) {
                const int piece = (tid - 256) + 256 * q;
                // (nothing to reset: an offset beyond the buffer resource — chosen per piece, a base of 0xFFFFF000
                // plus 16 * piece would wrap around into the ring's first tile)
                const unsigned o = (t + 2 < T_RING && piece < PIECES) ? so + (unsigned)piece * 16u : 0xFFFFF000u;
                if (xcd_local) __builtin_amdgcn_raw_buffer_store_b128(sent4, rsrc, o, 0, 0);
                else __builtin_amdgcn_raw_buffer_store_b128(sent4, rsrc, o, 0, AUX_SC1);
            }
        }
        if (BXS && valid_hi && t + 1 < T_HI) {  // the previous step's staged outputs -> HBM (upper waves)
            const int t1 = t + 1, tt1 = d ? (T - 1 - t1) : t1;
            if (ROW_STORE(t1)) {
                st4(a.dWx + RROW(bp, tt1) * H + col, stage_dwx[tid & 255]);
                st2(a.s_prev16 + RROW(bp, tt1) * H + col, stage_sp[tid & 255]);
            }
        }
        // From here to the publish barrier: the waves that own pointwise state only (a WAVE-UNIFORM branch, round 3
        // — until then the upper four waves ran the reduction reads and the whole reverse step on dead values and
        // took vector issue slots and LDS cycles from the pointwise waves they share a SIMD with).
        float sp[4] = {0.f, 0.f, 0.f, 0.f}, du_new[4] = {0.f, 0.f, 0.f, 0.f}, dw_new[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4 dwx = {0.f, 0.f, 0.f, 0.f}, spv = dwx;
        PROF_STAMP(6);  // behind the barrier: settle, flag read, prefetch issue, staged stores
        // (u_{t-1}, u_t — and w_{t-1}, the raw projection below — as separate locals: hipcc's register assignment in the
        // NP = 1 kernels follows these declarations, and the shipped instruction order is the measured one)
        f32x4 up_use = upv, ut_use = {u_t[0], u_t[1], u_t[2], u_t[3]};
        if (pw_wave) {
        if (t + 1 < T_RING && EXT) {
            const f32x4 v = ld4(a.rec0 + (size_t)bpc * H + colc);
            rec[0] = v.x; rec[1] = v.y; rec[2] = v.z; rec[3] = v.w;
        } else if (t + 1 < T_RING) {
            f32x4 sum = *reinterpret_cast<const f32x4*>(&red[0][cj][r * RED_LD4 + cq * 4]);  // (see the forward)
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(&red[w][cj][r * RED_LD4 + cq * 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[e] = sum[e] + v[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) rec[e] = sum[e];
        }

        PROF_STAMP(7);  // partial-tile reduction
        // ---- pointwise reverse step (its rec-independent part: pre_pointwise above)
        if (t > 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sp[e] = spike_of(up_use[e], a.theta) ? 1.0f : 0.0f;
        } else {
            const f32x4 v = first_tile[2][pt];
            sp[0] = v.x; sp[1] = v.y; sp[2] = v.z; sp[3] = v.w;
        }
        const f32x4 al = pcol[0][d][cqx], be = pcol[1][d][cqx];
        ST_POST_LOAD
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ds = pre_ds[e] + rec[e];
            const float xs = ut_use[e] - a.theta;
            float du = SURROGATE_GATE(ds, xs) + pre_aldu[e];                  // snns.py:33-35
            if (ADAPT) du = du + pre_padw[e];
            dwx[e] = valid ? (1.0f - al[e]) * du : 0.0f;
            du_new[e] = du;
            dw_new[e] = ADAPT ? ST_PLUS(be[e] * dw_n[e] - dwx[e], st_w[e]) : 0.f;
            spv[e] = (t > 0) ? sp[e] : 0.0f;  // binary rows only: the s0 term of dV is added by the host
        }
        PROF_STAMP(8);  // reverse-step arithmetic
        // ---- publish dWx_t first: this thread's 4 values are one 16-byte piece of the tile in fragment
        //      order (columns cq*4.. -> k16-step ks = cq>>2, k-half h = (cq>>1)&1, quad q = cq&1), one
        //      write-through store; then the sentinel goes back into the slot of step t+2 (see header)
        if (EXT) {
            if (valid) st4(a.dwx_step + (size_t)bp * H + col, dwx);  // operand of the caller's dWx_t @ V^T product
        } else if (pw) {
            // this thread's 4 values = k 4 cq .. +3 of its row: k16-step cq >> 2, k-half (cq >> 1) & 1, first or
            // second 8 bytes of that piece; the three planes of a piece are 1 KiB apart
            const unsigned piece = (unsigned)(((cq >> 2) * NP * 64 + ((cq >> 1) & 1) * 32 + r) * 16 + (cq & 1) * 8);
            const unsigned tile_off = rt_off + (unsigned)ct * PT + piece;
            {
                u32x2 w[3];
                if constexpr (NP == 1) {  // one nearest-even rounding (v_cvt_pk_bf16_f32)
                    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
                    w[0].x = __builtin_bit_cast(unsigned, bf16x2{(__bf16)dwx[0], (__bf16)dwx[1]});
                    w[0].y = __builtin_bit_cast(unsigned, bf16x2{(__bf16)dwx[2], (__bf16)dwx[3]});
                } else {
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const unsigned x0 = __float_as_uint(dwx[2 * pr]), x1 = __float_as_uint(dwx[2 * pr + 1]);
                    const float r0 = dwx[2 * pr] - __uint_as_float(x0 & 0xFFFF0000u);
                    const float r1 = dwx[2 * pr + 1] - __uint_as_float(x1 & 0xFFFF0000u);
                    const unsigned y0 = __float_as_uint(r0), y1 = __float_as_uint(r1);
                    const float q0 = r0 - __uint_as_float(y0 & 0xFFFF0000u);
                    const float q1 = r1 - __uint_as_float(y1 & 0xFFFF0000u);
                    w[0][pr] = __builtin_amdgcn_perm(x1, x0, 0x07060302u);
                    w[1][pr] = __builtin_amdgcn_perm(y1, y0, 0x07060302u);
                    w[2][pr] = __builtin_amdgcn_perm(__float_as_uint(q1), __float_as_uint(q0), 0x07060302u);
                }
                }
                // (no branch around the stores: where there is nothing to publish — cell step 0 — or to reset, the
                // offset lies beyond the buffer resource and the hardware drops the store; the instruction count
                // of a step is then the same on every path)
                const unsigned so = t > 0 ? (unsigned)(t % RING) * slot_bytes + tile_off : 0xFFFFF000u;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    if (xcd_local) __builtin_amdgcn_raw_buffer_store_b64(w[p], rsrc, so + (unsigned)(p * 1024), 0, 0);
                    else __builtin_amdgcn_raw_buffer_store_b64(w[p], rsrc, so + (unsigned)(p * 1024), 0, AUX_SC1);
                }
            }
            if (!BXS) {  // (8-wave kernels: the upper waves put the sentinels back, see above)
                const u32x2 sent = {SENTINEL, SENTINEL};
                const unsigned so = t + 2 < T_RING ? (unsigned)((t + 2) % RING) * slot_bytes + tile_off : 0xFFFFF000u;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    if (xcd_local) __builtin_amdgcn_raw_buffer_store_b64(sent, rsrc, so + (unsigned)(p * 1024), 0, 0);
                    else __builtin_amdgcn_raw_buffer_store_b64(sent, rsrc, so + (unsigned)(p * 1024), 0, AUX_SC1);
                }
            }
        }
        }
        PROF_STAMP(3);  // pointwise + tile store issue
        lds_barrier();  // the non-pointwise waves start polling only once this workgroup's own tile is on its way
        PROF_STAMP(4);  // publish barrier
        // ---- off the critical path: fp32 outputs for the following GEMMs, parameter partial sums
        if (valid) {
            u32x2 h;  // s_{t-1} (binary; a zero row at t = 0) as a bf16 plane for dV (this copy stays: neuron.h)
            h.x = (spv[0] != 0.f ? 0x3F80u : 0u) | (spv[1] != 0.f ? 0x3F800000u : 0u);
            h.y = (spv[2] != 0.f ? 0x3F80u : 0u) | (spv[3] != 0.f ? 0x3F800000u : 0u);
            if (BXS) {
                stage_dwx[tid] = dwx; stage_sp[tid] = h;
            } else if (ROW_STORE(t)) {
                st4(a.dWx + RROW(bp, tt) * H + col, dwx);
                st2(a.s_prev16 + RROW(bp, tt) * H + col, h);
            }
        }
        if (pw) {
            f32x4 wp_use = wpv, xr_use = xrv;
            f32x4 v_al = pacc[0][pt], v_be, v_a, v_b;
            if (ADAPT) { v_be = pacc[1][pt]; v_a = pacc[2][pt]; v_b = pacc[3][pt]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float q = up_use[e] - sp[e];
                v_al[e] += du_new[e] * (q - ut_use[e]);  // x 1/(1-alpha) once, at the end
                if (ADAPT) {
                    v_be[e] += dw_new[e] * wp_use[e];
                    v_a[e] += dw_new[e] * up_use[e];
                    v_b[e] += dw_new[e] * sp[e];
                }
            }
            pacc[0][pt] = v_al;
            if (ADAPT) { pacc[1][pt] = v_be; pacc[2][pt] = v_a; pacc[3][pt] = v_b; }
            if (bn) {  // BatchNorm backward's column sums (dy = dWx, xhat = (x - mean) * invstd)
                f32x4 v_dy = pacc[4][pt], v_dyx = pacc[5][pt];
                const f32x4 mu = pcol[5][d][cqx], is = pcol[6][d][cqx];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v_dy[e] += dwx[e];
                    v_dyx[e] += dwx[e] * ((xr_use[e] - mu[e]) * is[e]);
                }
                pacc[4][pt] = v_dy; pacc[5][pt] = v_dyx;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (ADAPT) dw_n[e] = dw_new[e];
            du_n[e] = du_new[e];
            u_t[e] = upv[e];
        }
        PROF_STAMP(5);  // fp32 stores + partial sums
    }
    PROF_FLUSH(1)
    if (BXS) {  // the launch's last step is still staged (after an abort the step is discarded anyway)
        const bool aborted = (lds_flag_read(&abort_flag[0]) | lds_flag_read(&abort_flag[1])) != 0;
        __syncthreads();
        if (!aborted && valid_hi && a.t_end > a.t_begin) {
            const int t1 = a.t_begin, tt1 = d ? (T - 1 - t1) : t1;
            st4(a.dWx + RROW(bp, tt1) * H + col, stage_dwx[tid & 255]);      // (step 0: every row has it)
            st2(a.s_prev16 + RROW(bp, tt1) * H + col, stage_sp[tid & 255]);
        }
    }
    if (tid == 0 && (lds_flag_read(&abort_flag[0]) | lds_flag_read(&abort_flag[1])))
        status_raise(a.status, SPARCH_STATUS_REC_BWD, t_stop);

    if (valid) {
        f32x4 v = pacc[0][tid];
        if (a.t_begin == 0) {  // last chunk of the pass: d u_t / d alpha = (q - u_t) / (1 - alpha)
            const f32x4 al = pcol[0][d][cqx];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f - al[e]);
        }
        st4(ws, v);
        v.x = du_n[0]; v.y = du_n[1]; v.z = du_n[2]; v.w = du_n[3]; st4(ws + 4 * plane, v);
        if (ADAPT) {
            st4(ws + plane, pacc[1][tid]);
            st4(ws + 2 * plane, pacc[2][tid]);
            st4(ws + 3 * plane, pacc[3][tid]);
            v.x = dw_n[0]; v.y = dw_n[1]; v.z = dw_n[2]; v.w = dw_n[3]; st4(ws + 5 * plane, v);
        }
        if (bn) {
            st4(ws + 6 * plane, pacc[4][tid]);
            st4(ws + 7 * plane, pacc[5][tid]);
        }
        ST_TAIL
    }
}

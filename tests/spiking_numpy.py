"""
TEST INFRASTRUCTURE ONLY: the four spiking cells (LIF, adLIF, RLIF, RadLIF) restated in plain numpy at the level of
sparch_amd.functional.cell_forward / cell_backward.  It shares no code with the product and is generic in dtype:
float64 is the reference of tests/test_rec_cell_real_V_gpu.py, float32 (the recurrent products accumulated over 32-wide
k blocks, ascending and descending) is the yardstick its bounds are made from.  tests/test_spiking_numpy_host.py pins it
to oracle.bptt_numpy (bit for bit, fp32) and to torch autograd of oracle.snn_oracle.spiking_cell (float64).

Geometry (the header's): B batch rows, dirs = 1 | 2, Bp = B * dirs virtual rows.  Virtual row b + B * d reads the
projection of batch row b, for d = 1 at time T - 1 - t.  "Cell time order" indexes a (Bp,T,H) tensor by the step t the
cell processed (u_save, w_save); "original time index" by tt = t (d = 0) or T - 1 - t (d = 1) (dWx); the output layout
is (B,T,H*dirs), directions side by side on features at the original time index (s_out, g_out).

    x_t = Wx_t * scale + shift                                   (both optional)
    w_t = (beta w + a u) + b s                                   (adaptive kinds; previous u, s)
    u_t = alpha (u - s) + (1 - alpha) (x_t [+ s Vm] [- w_t])     Vm = V with its diagonal zeroed
    s_t = [u_t - theta > 0]

alpha, beta, a, b are the raw parameters clamped to the float32 limits the kernels clamp them to; s before the first
step is s0, real-valued.  In reverse, on SAVED u / w only (the backward kernels never see the projection), with
du_{T} = dw_{T} = 0 and s_{t-1} = [u_{t-1} - theta > 0] (s0 at t = 0):

    g_t   = g_out_t + g_rate / (B T)
    ds_t  = g_t - alpha du_{t+1} [+ b dw_{t+1}] [+ dWx_{t+1} Vm^T]
    du_t  = box(ds_t, u_t - theta) + alpha du_{t+1} [+ a dw_{t+1}]        box: ds where -0.5 < x <= 0.5, else 0
    dWx_t = (1 - alpha) du_t              dw_t = beta dw_{t+1} - dWx_t
    per virtual row:  ws_alpha = (sum_t du_t ((u_{t-1} - s_{t-1}) - u_t)) / (1 - alpha)
                      ws_beta = sum_t dw_t w_{t-1}    ws_a = sum_t dw_t u_{t-1}    ws_b = sum_t dw_t s_{t-1}
    dV = sum_t s_{t-1}^T dWx_t over the virtual rows, diagonal zeroed (the t = 0 term has the non-binary s0)

((q - u_t) / (1 - alpha) = q - drive_t by the forward relation: the kernels' form, needing no projection.)  The
parameter gradients are the column sums of the per-row partials, gated by the clamp range of the raw parameter
(sparch_colsum_clamped).  With bn = (Wx_raw, mean, invstd) the two BatchNorm column sums sum dWx and
sum dWx * (Wx_raw - mean) * invstd come out as "bn_sums" (both directions of a batch row read the same Wx_raw row).

The given states of a step are exact inputs, so a teacher-forced forward and a backward on supplied saves are
continuous in everything else: no spike decision is taken from a value the function itself computed, except the saved
one's own sign.

bf16 operand mode (sparch_set_operand_precision): pass operand=bf16_round — every dense product then multiplies its
operands rounded once to bf16 (V everywhere; s0 in the t = 0 products; dWx in dWx Vm^T and in dV).  `rec_operand`
(backward) supplies the dWx values those two products read in place of the function's own: with the rounded dWx of
the run under test there, a rounding that falls on the other side of a bf16 tie in the reference is not an error.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
KINDS = ("LIF", "adLIF", "RLIF", "RadLIF")
ADAPTIVE = {"LIF": False, "adLIF": True, "RLIF": False, "RadLIF": True}
RECURRENT = {"LIF": False, "adLIF": False, "RLIF": True, "RadLIF": True}
# the float32 clamp limits of sparch_amd/csrc/common.h (SP_*_LO / _HI)
LIMS = {"alpha": (F32(math.exp(-1 / 5)), F32(math.exp(-1 / 25))), "beta": (F32(math.exp(-1 / 30)), F32(math.exp(-1 / 120))),
        "a": (F32(-1.0), F32(1.0)), "b": (F32(0.0), F32(2.0))}
KB = 32     # one k-group of the recurrent kernels


# ------------------------------------------------------------------------------------------------ layouts
def virtual_rows(x, dirs):
    """(B,T,H) at the original time index -> (Bp,T,H) in cell time order."""
    return x if dirs == 1 else np.concatenate([x, x[:, ::-1]], axis=0)


def to_original(a, B, dirs):
    """(Bp,T,H): cell time order <-> original time index (the map is its own inverse)."""
    return a if dirs == 1 else np.concatenate([a[:B], a[B:, ::-1]], axis=0)


def out_layout(a, B, dirs):
    """(Bp,T,H) in cell time order -> (B,T,H*dirs)."""
    o = to_original(a, B, dirs)
    return o if dirs == 1 else np.concatenate([o[:B], o[B:]], axis=2)


def from_out_layout(g, dirs):
    """(B,T,H*dirs) -> (Bp,T,H) in cell time order (the inverse of out_layout)."""
    if dirs == 1:
        return g
    H = g.shape[2] // 2
    return np.concatenate([g[:, :, :H], g[:, ::-1, H:]], axis=0)


# ------------------------------------------------------------------------------------------------ bf16 planes
def bf16_round(x):
    """x rounded once to bf16 (nearest-even), in x's dtype (through float32, as the kernels round fp32 values)."""
    import torch

    x = np.asarray(x)
    r = torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16).to(torch.float32).numpy()
    return r.astype(x.dtype if x.dtype in (F32, F64) else F32)


def split3(x):
    """The exact TRUNCATION split x = t1 + t2 + t3 of an fp32 array as three fp32 arrays (what the backward kernels do
    to dWx; tests/test_gemm_layouts_gpu.split3_host, not a second restatement)."""
    import torch

    from tests.test_gemm_layouts_gpu import split3_host
    x = np.ascontiguousarray(x, dtype=F32)
    p = split3_host(torch.from_numpy(x.reshape(-1, x.shape[-1]))).to(torch.float32).numpy()
    return tuple(p.reshape((3,) + x.shape))


def split3_rne(x):
    """The exact NEAREST-EVEN split x = hi + mid + lo of an fp32 array (rec_common.h split3: what the V pack kernels do;
    |lo| <= 2^-17 |x|, half of what the truncation split leaves in its third plane)."""
    x = np.ascontiguousarray(x, dtype=F32)
    hi = bf16_round(x)
    r1 = x - hi
    mid = bf16_round(r1)
    lo = bf16_round(r1 - mid)
    return hi, mid, lo


def V_without_plane2(V, k_fraction=1.0, split="trunc"):
    """MUTANT (tests/test_spiking_numpy_host.py only): V as a pack reads that lost plane 2 of its first k_fraction of
    k — the rows of V, the index s @ V contracts.  split "trunc": the planes of split3 (non-negative third planes of
    up to 2^-16 |x|: they add up coherently); "rne": those of split3_rne, what the pack kernels of reccell.hip would
    lose (signed, at most 2^-17 |x|: a quarter of the root mean square, and no common sign)."""
    p0, p1, p2 = (split3 if split == "trunc" else split3_rne)(V)
    p2 = p2.copy()
    p2[:int(round(V.shape[0] * k_fraction))] = 0
    return ((p0.astype(F64) + p1) + p2).astype(F32)      # two or three bf16 values: exact in fp32


def rec_bwd_without_t3_hi(dwx, VmT, k_order=None):
    """MUTANT (host test only): dWx @ Vm^T with the cross term t3 * hi left out."""
    t3 = split3(np.asarray(dwx, dtype=F32))[2]
    hi = split3_rne(np.asarray(VmT, dtype=F32))[0]
    return matmul_blocks(dwx, VmT, k_order) - t3.astype(dwx.dtype) @ hi.astype(dwx.dtype)


# ------------------------------------------------------------------------------------------------ pieces
def matmul_blocks(a, b, k_order=None):
    """a (M,K) @ b (K,N).  k_order None: numpy's matmul.  "asc" / "desc" / a sequence of block indices: the contraction
    cut into 32-wide k blocks whose partial products are added up in that order, in the operands' dtype."""
    if k_order is None:
        return a @ b
    nb = -(-a.shape[1] // KB)
    order = {"asc": range(nb), "desc": range(nb - 1, -1, -1)}[k_order] if isinstance(k_order, str) else k_order
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.result_type(a, b))
    for kb in order:
        acc = acc + a[:, kb * KB:(kb + 1) * KB] @ b[kb * KB:(kb + 1) * KB]
    return acc


class Params:
    """The clamped parameters of one cell in `dtype` (raw fp32 values, widened before anything is computed)."""

    def __init__(self, kind, dtype, p, theta=1.0, operand=None):
        self.kind, self.dtype = kind, dtype
        self.adaptive, self.recurrent = ADAPTIVE[kind], RECURRENT[kind]
        self.theta = dtype(theta)
        self.raw = {k: np.asarray(v, dtype=F32) for k, v in p.items()}
        for k in ("alpha",) + (("beta", "a", "b") if self.adaptive else ()):
            lo, hi = LIMS[k]
            setattr(self, k, np.minimum(np.maximum(self.raw[k].astype(dtype), dtype(lo)), dtype(hi)))
        self.oma = dtype(1) - self.alpha
        self.operand = operand
        if self.recurrent:
            Vm = self.raw["V"].copy()
            np.fill_diagonal(Vm, 0)
            self.Vm = self.op(Vm.astype(dtype))          # (k, n): s @ Vm
            self.VmT = np.ascontiguousarray(self.Vm.T)   # (k, n): dWx @ Vm^T

    def op(self, x):
        return x if self.operand is None else self.operand(x)


def inside(raw, lim):
    """torch.clamp passes the gradient where lo <= raw <= hi (inclusive)."""
    return (raw >= lim[0]) & (raw <= lim[1])


def affine(Wx, scale, shift, dirs, dtype):
    """The cell's input (Bp,T,H) in cell time order."""
    x = np.asarray(Wx, dtype=dtype)
    if scale is not None:
        x = x * np.asarray(scale, dtype=dtype) + np.asarray(shift, dtype=dtype)
    return virtual_rows(x, dirs)


# ------------------------------------------------------------------------------------------------ forward
def step_forward(kind, dtype, state, Wx_t, P, k_order=None, first=False):
    """One step from state = (u, w, s) of the step before (w None for the non-adaptive kinds), all (Bp,H); Wx_t the
    cell's input of this step (after scale / shift); P a Params.  first: s is the real-valued s0 (a dense operand in the
    bf16 operand mode).  Returns the new (u, w, s)."""
    assert P.kind == kind and P.dtype == dtype
    u, w, s = state
    drive = np.asarray(Wx_t, dtype=dtype)
    if P.adaptive:
        w = (P.beta * w + P.a * u) + P.b * s
    if P.recurrent:
        drive = drive + matmul_blocks(P.op(s) if first else s, P.Vm, k_order)
    if P.adaptive:
        drive = drive - w
    u = P.alpha * (u - s) + P.oma * drive
    return u, w, ((u - P.theta) > 0).astype(dtype)


def _pack_forward(P, B, dirs, U, W, S):
    out = {"u_save": U, "w_save": W, "s": S, "s_out": out_layout(S, B, dirs)}
    out["count"] = out["s_out"].sum((0, 1)).astype(np.int64)
    return out


def forward(kind, dtype, Wx, scale, shift, p, u0, w0, s0, *, B, dirs, theta=1.0, k_order=None, operand=None):
    """Free-running forward.  Wx (B,T,H); u0 / w0 / s0 (Bp,H).  Returns a dict: u_save, w_save, s (Bp,T,H) in cell time
    order, s_out (B,T,H*dirs), count (H*dirs)."""
    P = Params(kind, dtype, p, theta, operand)
    x = affine(Wx, scale, shift, dirs, dtype)
    Bp, T, H = x.shape
    U, S = np.empty((Bp, T, H), dtype), np.empty((Bp, T, H), dtype)
    W = np.empty((Bp, T, H), dtype) if P.adaptive else None
    st = (np.asarray(u0, dtype=dtype), np.asarray(w0, dtype=dtype) if P.adaptive else None, np.asarray(s0, dtype=dtype))
    for t in range(T):
        st = step_forward(kind, dtype, st, x[:, t], P, k_order, first=(t == 0))
        U[:, t], S[:, t] = st[0], st[2]
        if P.adaptive:
            W[:, t] = st[1]
    return _pack_forward(P, B, dirs, U, W, S)


def teacher_forced_forward(kind, dtype, Wx, scale, shift, p, u0, w0, s0, u_save, w_save, *, B, dirs, theta=1.0,
                           k_order=None, operand=None):
    """step_forward applied to every t from the SUPPLIED state of the step before: u_save[t-1], w_save[t-1] and
    s_{t-1} = (u_save[t-1] - theta > 0) decided in the save's own type (u0 / w0 / s0 at t = 0).  Same returns as forward()."""
    P = Params(kind, dtype, p, theta, operand)
    x = affine(Wx, scale, shift, dirs, dtype)
    Bp, T, H = x.shape
    us = np.asarray(u_save)                               # float32 from a kernel (float64 from forward(F64, ...))
    U, S = np.empty((Bp, T, H), dtype), np.empty((Bp, T, H), dtype)
    W = np.empty((Bp, T, H), dtype) if P.adaptive else None
    for t in range(T):
        if t == 0:
            st = (np.asarray(u0, dtype=dtype), np.asarray(w0, dtype=dtype) if P.adaptive else None, np.asarray(s0, dtype=dtype))
        else:
            st = (us[:, t - 1].astype(dtype), np.asarray(w_save[:, t - 1], dtype=dtype) if P.adaptive else None,
                  ((us[:, t - 1] - us.dtype.type(theta)) > 0).astype(dtype))
        u, w, s = step_forward(kind, dtype, st, x[:, t], P, k_order, first=(t == 0))
        U[:, t], S[:, t] = u, s
        if P.adaptive:
            W[:, t] = w
    return _pack_forward(P, B, dirs, U, W, S)


# ------------------------------------------------------------------------------------------------ backward
def backward(kind, dtype, g_out, g_rate, u_save, w_save, p, u0, w0, s0, *, B, dirs, theta=1.0, k_order=None,
             operand=None, rec_operand=None, rec_product=None, bn=None):
    """The reverse recurrences on supplied saves (module docstring).  g_out (B,T,H*dirs); g_rate (H*dirs) or None;
    u_save / w_save (Bp,T,H) in cell time order.  rec_operand: (Bp,T,H) at the original time index, the dWx values
    the dense products read; rec_product(dwx, VmT, k_order) replaces dWx @ Vm^T (the host test's mutant).
    Returns dWx (Bp,T,H) at the original time index, the per-row partials ws_alpha [ws_beta, ws_a, ws_b] (Bp,H), the
    gradients alpha [beta, a, b] [V] and, with bn, bn_sums = (sum dWx, sum dWx xhat)."""
    P = Params(kind, dtype, p, theta, operand)
    Bp, T, H = u_save.shape
    g = from_out_layout(np.asarray(g_out, dtype=dtype), dirs)
    if g_rate is not None:
        gr = np.asarray(g_rate, dtype=dtype).reshape(dirs, H) * (dtype(1) / (dtype(B) * dtype(T)))
        g = g + np.repeat(gr, B, axis=0)[:, None, :]
    us = np.asarray(u_save)
    U = us.astype(dtype)
    S = ((us - us.dtype.type(theta)) > 0).astype(dtype)  # the decision as the kernels take it: in the save's own type
    W = np.asarray(w_save, dtype=dtype) if P.adaptive else None
    u0, s0 = np.asarray(u0, dtype=dtype), np.asarray(s0, dtype=dtype)
    w0 = np.asarray(w0, dtype=dtype) if P.adaptive else None
    rec_op = None if rec_operand is None else to_original(np.asarray(rec_operand, dtype=dtype), B, dirs)  # cell order
    du_n, dw_n = np.zeros((Bp, H), dtype), np.zeros((Bp, H), dtype)
    dWx = np.empty((Bp, T, H), dtype)
    acc = {k: np.zeros((Bp, H), dtype) for k in ("alpha", "beta", "a", "b")}
    dV = np.zeros((H, H), dtype) if P.recurrent else None
    dwx_next = None
    for t in range(T - 1, -1, -1):
        u_prev, s_prev = (U[:, t - 1], S[:, t - 1]) if t > 0 else (u0, s0)
        aldu = P.alpha * du_n
        ds = g[:, t] - aldu
        if P.adaptive:
            ds = ds + P.b * dw_n
        if P.recurrent and t + 1 < T:
            x_op = P.op(dwx_next if rec_op is None else rec_op[:, t + 1])
            ds = ds + (rec_product or matmul_blocks)(x_op, P.VmT, k_order)
        xs = U[:, t] - P.theta
        du = np.where((xs <= -0.5) | (xs > 0.5), dtype(0), ds) + aldu
        if P.adaptive:
            du = du + P.a * dw_n
        dwx = P.oma * du
        dWx[:, t] = dwx
        acc["alpha"] = acc["alpha"] + du * ((u_prev - s_prev) - U[:, t])
        if P.adaptive:
            dw = P.beta * dw_n - dwx
            acc["beta"] = acc["beta"] + dw * (W[:, t - 1] if t > 0 else w0)
            acc["a"] = acc["a"] + dw * u_prev
            acc["b"] = acc["b"] + dw * s_prev
            dw_n = dw
        if P.recurrent:
            x_op = P.op(dwx if rec_op is None else rec_op[:, t])
            dV = dV + (P.op(s_prev) if t == 0 else s_prev).T @ x_op
        du_n, dwx_next = du, dwx
    acc["alpha"] = acc["alpha"] / P.oma
    out = {"dWx": to_original(dWx, B, dirs)}
    for k in ("alpha",) + (("beta", "a", "b") if P.adaptive else ()):
        out["ws_" + k] = acc[k]
        out[k] = np.where(inside(P.raw[k], LIMS[k]), acc[k].sum(0), dtype(0))
    if P.recurrent:
        np.fill_diagonal(dV, 0)
        out["V"] = dV
    if bn is not None:
        x_raw, mean, invstd = (np.asarray(v, dtype=dtype) for v in bn)
        xhat = (x_raw - mean) * invstd                                  # (B,T,H) at the original time index
        dy = out["dWx"].reshape(dirs, B, T, H)
        out["bn_sums"] = (dy.sum((0, 1, 2)), (dy * xhat[None]).sum((0, 1, 2)))
    return out


# ------------------------------------------------------------------------------------------------ shared cases
def make_inputs(kind, B, dirs, T, H, seed, regime="drive", affine_in=False):
    """Inputs of one case, float32.  Wx ~ 1.5 N(0,1) + 0.4; the raw parameters inside their clamp ranges; w0 uniform in
    [0, 1), s0 REAL-valued uniform in [0, 1), as the reference draws them.
    regime "drive": V ~ N(0, 0.5^2) with every significand bit live — the recurrent term dominates u; theta = 0.25 and
                    alpha in [0.90, 0.96], u0 in [0, 1): 5 .. 35 % spikes at every H, and |u| stays within a few
                    units over the T steps (the rounding of u itself, half an ulp of the LARGEST |u| of the tensor,
                    is what the bound is made of: a membrane that runs off to |u| ~ 20 hides plane 2 behind it);
           "init":  V orthogonal, as the reference initialises it; theta = 1, alpha in [0.82, 0.96], u0 in [0, 3).
    The rows of a partial last row tile (Bp % 32 of them) get u0 + 2: few rows, and every 32-wide k-group of them is
    still to carry a spike."""
    rng = np.random.default_rng(seed)
    Bp = B * dirs
    drive = regime == "drive"
    c = {"kind": kind, "B": B, "dirs": dirs, "T": T, "H": H, "Bp": Bp, "regime": regime, "theta": 0.25 if drive else 1.0}
    p = {"alpha": rng.uniform(0.90 if drive else 0.82, 0.96, H).astype(F32)}
    if ADAPTIVE[kind]:
        p.update(beta=rng.uniform(0.968, 0.991, H).astype(F32), a=rng.uniform(-0.9, 0.9, H).astype(F32),
                 b=rng.uniform(0.1, 1.9, H).astype(F32))
    if RECURRENT[kind]:
        if drive:
            p["V"] = (0.5 * rng.standard_normal((H, H))).astype(F32)
        else:
            import torch

            V = torch.empty(H, H)
            torch.nn.init.orthogonal_(V, generator=torch.Generator().manual_seed(seed))
            p["V"] = V.numpy().copy()
    c["p"] = p
    c["Wx"] = (1.5 * rng.standard_normal((B, T, H)) + 0.4).astype(F32)
    c["scale"] = rng.uniform(0.7, 1.3, H).astype(F32) if affine_in else None
    c["shift"] = rng.uniform(-0.2, 0.2, H).astype(F32) if affine_in else None
    c["u0"] = rng.uniform(0, 1 if drive else 3, (Bp, H)).astype(F32)
    c["u0"][Bp - Bp % 32:] += F32(2)      # the rows of a partial last row tile start high: each of its k-groups spikes
    c["w0"] = rng.uniform(0, 1, (Bp, H)).astype(F32) if ADAPTIVE[kind] else None
    c["s0"] = rng.uniform(0, 1, (Bp, H)).astype(F32)
    c["g_out"] = rng.standard_normal((B, T, H * dirs)).astype(F32)
    c["g_rate"] = rng.standard_normal(H * dirs).astype(F32)
    return c


# (kind, B, dirs, T, H): the shapes of tests/test_rec_cell_real_V_gpu.py — the smallest that reach each kernel shape of
# the launch planner (kgw 1 / 2 / 4 / 8), Bp = 33: two row tiles, the second with one row; T = 6: the backward's
# depth-4 ring wraps.
REC_SHAPES = [(k, 33, 1, 6, H) for H in (96, 132, 384, 1024) for k in ("RLIF", "RadLIF")]
BIDIR_SHAPES = [(k, 17, 2, 6, 132) for k in ("RLIF", "RadLIF")]


def case_seed(kind, B, dirs, T, H):
    return 1000003 * B + 1009 * T + 31 * H + 7 * dirs + len(kind)


FWD_TENSORS = {False: ("u_save",), True: ("u_save", "w_save")}


def bwd_tensors(kind, bn=False):
    return (("dWx", "alpha") + (("beta", "a", "b") if ADAPTIVE[kind] else ()) + (("V",) if RECURRENT[kind] else ())
            + (("bn_dy", "bn_dyx") if bn else ()))


def flat(res):
    """A result dict with bn_sums spread into bn_dy / bn_dyx."""
    if "bn_sums" in res:
        res = dict(res, bn_dy=res["bn_sums"][0], bn_dyx=res["bn_sums"][1])
    return res


def bound_of(runs32, run64, names):
    """The rule of tests/test_gated_kernels_gpu.py: per tensor, FOUR times the worst max-abs error of the fp32 runs of
    the restatement against its fp64 run on the same inputs."""
    return {k: 4.0 * max(float(np.abs(r[k].astype(F64) - run64[k]).max()) for r in runs32) for k in names}

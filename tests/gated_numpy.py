"""
TEST INFRASTRUCTURE ONLY: the recurrent cells of the non-spiking baselines restated in plain numpy, at the level of
the C ABI (include/sparch_hip.h: sparch_ann_rec_fwd/_bwd, sparch_ligru_fwd/_bwd, sparch_gru_fwd/_bwd and their
launch-per-step forms sparch_ann_rec_step_fwd/_bwd, sparch_gate_step).  It shares no code with the product and is
generic in dtype: float64 is the reference of tests/test_gated_kernels_gpu.py, float32 (with numpy's matmul, and with
the recurrent product accumulated over K in chunks of 32) is the yardstick its bounds are made from.
tests/test_gated_numpy_host.py pins it to oracle.ann_oracle.hidden_layer and torch autograd in float64.

Geometry (the header's): B batch rows, dirs = 1 | 2, Bp = B * dirs virtual rows.  Virtual row b + B * d reads the
projections of batch row b, for d = 1 at time T - 1 - t.  "Cell time order" indexes a (Bp,T,H) tensor by the step t
the cell processed; "original time index" by tt = t (d = 0) or T - 1 - t (d = 1).

    RNN    y = act(Wx * scale + shift + y V^T)
    LiGRU  z = sigmoid(xz + y Vz^T)   c = relu(xc + y V^T)                              y' = z y + (1 - z) c
    GRU    z = sigmoid(xz + y Vz^T)   r = sigmoid(xr + y Vr^T)   c = tanh(xc + (r y) V^T)   y' = z y + (1 - z) c

with y = 0 before the first step, and in reverse

    RNN    dpre = (g k + dpre_{t+1} V) act'(y)
    LiGRU  dy = g k + [dz | dc]_{t+1} [Vz ; V] + (dy z)_{t+1}
           dz = (dy (y_{t-1} - c)) (z (1 - z))      dc = dy (1 - z) where the SAVED c > 0, else 0
    GRU    dy = g k + [dz | dr]_{t+1} [Vz ; Vr] + (dy z + dq r)_{t+1}
           dz as above      dc = (dy (1 - z)) (1 - c^2)      dq = dc V      dr = (dq y_{t-1}) (r (1 - r))

k = the dropout factor of tests/dropout_numpy.keep_mask(seed, (B,T,H*dirs), p) at the output element.

Forward functions return a dict: y_state, z_save, r_save, c_save (Bp,T,H) in cell time order, y_out (B,T,H*dirs), and
the recurrent products each step consumed (rec*, cell time order; zero at the first step) — what a caller of the
launch-per-step kernels supplies.  Backward functions return their outputs (Bp,T,H) at the original time index and,
in cell time order, the products each step consumed (carry_mv, dry).
"""
import numpy as np

from tests.dropout_numpy import keep_mask

ACT_KIND = {"sigmoid": 0, "relu": 1, "tanh": 2}         # SPARCH_ACT_*
GATED_MATS = {"LiGRU": ("c", "z"), "GRU": ("c", "z", "r")}


# ------------------------------------------------------------------------------------------------ pointwise pieces
def sigmoid(v):
    one = v.dtype.type(1)
    return one / (one + np.exp(-v))


def relu(v):
    """v <= 0 ? +0 : v — a NaN stays a NaN."""
    return np.where(v <= 0, v.dtype.type(0), v)


def act(kind, v):
    return {"sigmoid": sigmoid, "relu": relu, "tanh": np.tanh}[kind](v)


def dact(kind, a):
    """The derivative through the activation's OUTPUT a."""
    one = a.dtype.type(1)
    if kind == "sigmoid":
        return a * (one - a)
    if kind == "relu":
        return np.where(a > 0, one, a.dtype.type(0))
    return one - a * a


def matmul_chunked(a, b, chunk=32):
    """a (M,K) @ b (K,N), the contraction cut into chunks of `chunk` whose partial products are added up one after
    the other in the operands' dtype (the blocked accumulation of a tiled kernel)."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.result_type(a, b))
    for k0 in range(0, a.shape[1], chunk):
        acc = acc + np.matmul(a[:, k0:k0 + chunk], b[k0:k0 + chunk])
    return acc


# ------------------------------------------------------------------------------------------------ layouts
def virtual_rows(x, dirs):
    """(B,T,H) at the original time index -> (Bp,T,H) in cell time order."""
    return x if dirs == 1 else np.concatenate([x, x[:, ::-1]], axis=0)


def to_original(a, B, dirs):
    """(Bp,T,H): cell time order <-> original time index (the map is its own inverse)."""
    if dirs == 1:
        return a
    return np.concatenate([a[:B], a[B:, ::-1]], axis=0)


def out_layout(a, B, dirs):
    """(Bp,T,H) in cell time order -> (B,T,H*dirs): directions side by side on features, original time index."""
    o = to_original(a, B, dirs)
    return o if dirs == 1 else np.concatenate([o[:B], o[B:]], axis=2)


def from_out_layout(g, dirs):
    """(B,T,H*dirs) -> (Bp,T,H) in cell time order (the inverse of out_layout)."""
    if dirs == 1:
        return g
    H = g.shape[2] // 2
    return np.concatenate([g[:, :, :H], g[:, ::-1, H:]], axis=0)


_mask_cache = {}


def mask_of(seed, shape, p_drop, dtype):
    """keep_mask as `dtype` (all ones for p_drop = 0); the last few are kept (the per-step forms ask once a step)."""
    if not p_drop > 0:
        return np.ones(shape, dtype=dtype)
    key = (int(seed), tuple(shape), float(p_drop))
    if key not in _mask_cache:
        if len(_mask_cache) > 8:
            _mask_cache.clear()
        _mask_cache[key] = keep_mask(seed, shape, p_drop)
    return _mask_cache[key].astype(dtype)


def _affine(x, dirs, dtype):
    """x = (W, scale, shift) with scale / shift (H) or None -> the cell's input (Bp,T,H) in cell time order."""
    W, sc, sh = x
    v = np.asarray(W, dtype=dtype)
    if sc is not None:
        v = v * np.asarray(sc, dtype=dtype) + np.asarray(sh, dtype=dtype)
    return virtual_rows(v, dirs)


def shift_one_step(y_state):
    """y_{t-1} in cell time order: y_state moved one step, a zero row at the first step."""
    yp = np.zeros_like(y_state)
    yp[:, 1:] = y_state[:, :-1]
    return yp


# ------------------------------------------------------------------------------------------------ RNN
def rnn_forward(kind, Wx, scale, shift, V, dirs, p_drop, seed, dtype=np.float64, matmul=np.matmul):
    B, T, H = Wx.shape
    x = _affine((Wx, scale, shift), dirs, dtype)
    Vt = np.asarray(V, dtype=dtype).T
    Bp = B * dirs
    y_state, rec = np.zeros((Bp, T, H), dtype), np.zeros((Bp, T, H), dtype)
    y = np.zeros((Bp, H), dtype)
    for t in range(T):
        if t > 0:
            rec[:, t] = matmul(y, Vt)
        y = act(kind, x[:, t] + rec[:, t])
        y_state[:, t] = y
    y_out = out_layout(y_state, B, dirs) * mask_of(seed, (B, T, H * dirs), p_drop, dtype)
    return {"y_state": y_state, "y_out": y_out, "rec": rec}


def rnn_backward(kind, g_out, y_state, V, dirs, p_drop, seed, dtype=np.float64, matmul=np.matmul):
    Bp, T, H = y_state.shape
    B = Bp // dirs
    y = np.asarray(y_state, dtype=dtype)
    Vm = np.asarray(V, dtype=dtype)
    g = from_out_layout(np.asarray(g_out, dtype=dtype) * mask_of(seed, g_out.shape, p_drop, dtype), dirs)
    dpre, rec = np.zeros((Bp, T, H), dtype), np.zeros((Bp, T, H), dtype)
    dp = None
    for t in range(T - 1, -1, -1):
        if t + 1 < T:
            rec[:, t] = matmul(dp, Vm)
        dp = (g[:, t] + rec[:, t]) * dact(kind, y[:, t])
        dpre[:, t] = dp
    return {"dpre": to_original(dpre, B, dirs), "y_prev": to_original(shift_one_step(y), B, dirs), "rec": rec}


def rnn_step_fwd(kind, B, dirs, T, H, s, Wx, scale, shift, rec, p_drop, seed, y_out, y_state):
    """sparch_ann_rec_step_fwd on numpy arrays, in place; returns y_step (Bp,H).  rec is ignored at s = 0."""
    dtype = y_state.dtype
    y_step = np.zeros((B * dirs, H), dtype)
    mask = mask_of(seed, (B, T, H * dirs), p_drop, dtype)
    for d in range(dirs):
        tt = T - 1 - s if d else s
        rows = slice(d * B, (d + 1) * B)
        xn = np.asarray(Wx[:, tt], dtype=dtype)
        if scale is not None:
            xn = xn * np.asarray(scale, dtype=dtype) + np.asarray(shift, dtype=dtype)
        y = act(kind, xn + (rec[rows] if s > 0 else np.zeros((B, H), dtype)))
        y_state[rows, s] = y
        y_out[:, tt, d * H:(d + 1) * H] = y * mask[:, tt, d * H:(d + 1) * H]
        y_step[rows] = y
    return y_step


def rnn_step_bwd(kind, B, dirs, T, H, s, g_out, y_state, rec, p_drop, seed, dpre, y_prev):
    """sparch_ann_rec_step_bwd (processing step s is cell step t = T - 1 - s), in place; returns dpre_step (Bp,H)."""
    dtype = dpre.dtype
    t = T - 1 - s
    dpre_step = np.zeros((B * dirs, H), dtype)
    mask = mask_of(seed, (B, T, H * dirs), p_drop, dtype)
    for d in range(dirs):
        tt = T - 1 - t if d else t
        rows = slice(d * B, (d + 1) * B)
        g = np.asarray(g_out[:, tt, d * H:(d + 1) * H], dtype=dtype) * mask[:, tt, d * H:(d + 1) * H]
        dp = (g + (rec[rows] if s > 0 else np.zeros((B, H), dtype))) * dact(kind, np.asarray(y_state[rows, t], dtype))
        dpre[rows, tt] = dp
        y_prev[rows, tt] = y_state[rows, t - 1] if t > 0 else 0
        dpre_step[rows] = dp
    return dpre_step


# ------------------------------------------------------------------------------------------------ LiGRU / GRU
def gated_forward(cell, X, V, dirs, p_drop, seed, dtype=np.float64, matmul=np.matmul):
    """X: {"c": (Wx, scale, shift), "z": (Wzx, scz, shz), "r": (Wrx, scr, shr)} (r: GRU), projections (B,T,H);
    V: {"c": V, "z": Vz, "r": Vr}, each (H,H)."""
    gru, dtype = cell == "GRU", np.dtype(dtype).type
    B, T, H = X["c"][0].shape
    Bp = B * dirs
    x = {m: _affine(X[m], dirs, dtype) for m in GATED_MATS[cell]}
    Vt = {m: np.asarray(V[m], dtype=dtype).T for m in GATED_MATS[cell]}
    new = lambda: np.zeros((Bp, T, H), dtype)  # noqa: E731
    out = {"y_state": new(), "z_save": new(), "c_save": new(), "rec_z": new(), "rec_c": new()}
    if gru:
        out.update(r_save=new(), rec_r=new())
    y = np.zeros((Bp, H), dtype)
    one = dtype(1)
    for t in range(T):
        if t > 0:
            out["rec_z"][:, t] = matmul(y, Vt["z"])
        z = sigmoid(x["z"][:, t] + out["rec_z"][:, t])
        if gru:
            if t > 0:
                out["rec_r"][:, t] = matmul(y, Vt["r"])
            r = sigmoid(x["r"][:, t] + out["rec_r"][:, t])
            if t > 0:
                out["rec_c"][:, t] = matmul(r * y, Vt["c"])
            c = np.tanh(x["c"][:, t] + out["rec_c"][:, t])
            out["r_save"][:, t] = r
        else:
            if t > 0:
                out["rec_c"][:, t] = matmul(y, Vt["c"])
            c = relu(x["c"][:, t] + out["rec_c"][:, t])
        y = z * y + (one - z) * c
        out["y_state"][:, t], out["z_save"][:, t], out["c_save"][:, t] = y, z, c
    out["y_out"] = out_layout(out["y_state"], B, dirs) * mask_of(seed, (B, T, H * dirs), p_drop, dtype)
    return out


def gated_backward(cell, g_out, saves, V, dirs, p_drop, seed, dtype=np.float64, matmul=np.matmul):
    """saves: {"y_state", "z_save", "c_save", "r_save" (GRU)} (Bp,T,H) in cell time order."""
    gru, dtype = cell == "GRU", np.dtype(dtype).type
    y, z, c = (np.asarray(saves[k], dtype=dtype) for k in ("y_state", "z_save", "c_save"))
    r = np.asarray(saves["r_save"], dtype=dtype) if gru else None
    Bp, T, H = y.shape
    B = Bp // dirs
    Vc = np.asarray(V["c"], dtype=dtype)
    Vgate = np.concatenate([np.asarray(V["z"], dtype=dtype), np.asarray(V["r"], dtype=dtype) if gru else Vc], axis=0)
    g = from_out_layout(np.asarray(g_out, dtype=dtype) * mask_of(seed, g_out.shape, p_drop, dtype), dirs)
    yp = shift_one_step(y)
    new = lambda: np.zeros((Bp, T, H), dtype)  # noqa: E731
    dz, dc, dr, carry_mv, dry = new(), new(), new(), new(), new()
    cdir = np.zeros((Bp, H), dtype)
    one, zero = dtype(1), dtype(0)
    dgate = None                                       # [dz | dr] (GRU) or [dz | dc] (LiGRU) of step t + 1
    for t in range(T - 1, -1, -1):
        if t + 1 < T:
            carry_mv[:, t] = matmul(dgate, Vgate)
        dy = g[:, t] + carry_mv[:, t] + cdir
        dzp = (dy * (yp[:, t] - c[:, t])) * (z[:, t] * (one - z[:, t]))
        if gru:
            dcp = (dy * (one - z[:, t])) * (one - c[:, t] * c[:, t])
            dry[:, t] = matmul(dcp, Vc)
            drp = (dry[:, t] * yp[:, t]) * (r[:, t] * (one - r[:, t]))
            cdir = dy * z[:, t] + dry[:, t] * r[:, t]
            dr[:, t] = drp
            dgate = np.concatenate([dzp, drp], axis=1)
        else:
            dcp = np.where(c[:, t] > 0, dy * (one - z[:, t]), zero)
            cdir = dy * z[:, t]
            dgate = np.concatenate([dzp, dcp], axis=1)
        dz[:, t], dc[:, t] = dzp, dcp
    out = {"dz_all": to_original(dz, B, dirs), "dc_all": to_original(dc, B, dirs),
           "yprev_all": to_original(yp, B, dirs), "carry_mv": carry_mv}
    if gru:
        out.update(dr_all=to_original(dr, B, dirs), ry_all=to_original(r * yp, B, dirs), dry=dry)
    return out


IN_SLOTS = ("Wx", "sc", "sh", "Wzx", "scz", "shz", "Wrx", "scr", "shr", "rec", "g_out", "carry_mv", "carry_dir", "dry")
OUT_SLOTS = ("y_state", "z_save", "r_save", "c_save", "ry", "y_out", "carry_dir_out", "dgate", "dcp", "dz_all",
             "dr_all", "dc_all", "yprev_all", "ry_all")


def gate_step(mode, B, dirs, T, H, t, ins, outs, p_drop, seed):
    """sparch_gate_step on numpy arrays, in place.  ins / outs: dicts slot name -> array (IN_SLOTS / OUT_SLOTS; the
    saves are read through `outs` by the backward modes, as the C entry point does).  mode 0 LiGRU forward, 1 GRU
    gates, 2 GRU candidate and state, 3 LiGRU backward, 4 GRU backward first half, 5 GRU backward second half."""
    dtype = outs["y_state"].dtype.type
    one, zero = dtype(1), dtype(0)
    mask = mask_of(seed, (B, T, H * dirs), p_drop, dtype)

    def xin(d, tt, W, sc, sh):
        v = np.asarray(ins[W][:, tt], dtype=dtype)
        if ins.get(sc) is not None:
            v = v * np.asarray(ins[sc], dtype=dtype) + np.asarray(ins[sh], dtype=dtype)
        return v

    for d in range(dirs):
        tt = T - 1 - t if d else t
        rows = slice(d * B, (d + 1) * B)
        cols = slice(d * H, (d + 1) * H)
        yp = outs["y_state"][rows, t - 1] if t > 0 else np.zeros((B, H), dtype)
        rec = ins.get("rec")
        rec = np.zeros((B, 2 * H), dtype) if rec is None else rec[rows]
        if mode == 0:
            z = sigmoid(xin(d, tt, "Wzx", "scz", "shz") + rec[:, :H])
            c = relu(xin(d, tt, "Wx", "sc", "sh") + rec[:, H:2 * H])
            y = z * yp + (one - z) * c
            outs["y_state"][rows, t], outs["z_save"][rows, t], outs["c_save"][rows, t] = y, z, c
            outs["y_out"][:, tt, cols] = y * mask[:, tt, cols]
        elif mode == 1:
            z = sigmoid(xin(d, tt, "Wzx", "scz", "shz") + rec[:, :H])
            r = sigmoid(xin(d, tt, "Wrx", "scr", "shr") + rec[:, H:2 * H])
            outs["z_save"][rows, t], outs["r_save"][rows, t], outs["ry"][rows] = z, r, r * yp
        elif mode == 2:
            z = outs["z_save"][rows, t]
            c = np.tanh(xin(d, tt, "Wx", "sc", "sh") + rec[:, :H])
            y = z * yp + (one - z) * c
            outs["y_state"][rows, t], outs["c_save"][rows, t] = y, c
            outs["y_out"][:, tt, cols] = y * mask[:, tt, cols]
        elif mode in (3, 4):
            cm = ins["carry_mv"][rows] if ins.get("carry_mv") is not None else zero
            cd = ins["carry_dir"][rows] if ins.get("carry_dir") is not None else zero
            dy = np.asarray(ins["g_out"][:, tt, cols], dtype=dtype) * mask[:, tt, cols] + cm + cd
            z, c = outs["z_save"][rows, t], outs["c_save"][rows, t]
            dzp = (dy * (yp - c)) * (z * (one - z))
            if mode == 3:
                dcp = np.where(c > 0, dy * (one - z), zero)
                outs["dgate"][rows, H:] = dcp
            else:
                dcp = (dy * (one - z)) * (one - c * c)
                outs["dcp"][rows] = dcp
                outs["ry_all"][rows, tt] = outs["r_save"][rows, t] * yp
            outs["dgate"][rows, :H] = dzp
            outs["carry_dir_out"][rows] = dy * z
            outs["dz_all"][rows, tt], outs["dc_all"][rows, tt], outs["yprev_all"][rows, tt] = dzp, dcp, yp
        else:
            r, dry = outs["r_save"][rows, t], ins["dry"][rows]
            drp = (dry * yp) * (r * (one - r))
            outs["dgate"][rows, H:] = drp
            outs["carry_dir_out"][rows] = outs["carry_dir_out"][rows] + dry * r
            outs["dr_all"][rows, tt] = drp


# ------------------------------------------------------------------------------------------------ inputs of the tests
def inputs(cell, B, T, H, dirs, seed):
    """fp32 inputs of one case: X = {m: (projection (B,T,H) standard normal, scale (H) in [0.7, 1.3], shift (H) in
    [-0.2, 0.2])}, V = {m: (H,H) with entries of standard deviation 0.5 / sqrt(H)} — the LiGRU's unbounded candidate
    then does not grow over T —, g_out (B,T,H*dirs) standard normal.  cell: "RNN" (m = "c" only), "LiGRU", "GRU"."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    X, V = {}, {}
    for m in GATED_MATS.get(cell, ("c",)):
        X[m] = (f(rng.standard_normal((B, T, H))), f(rng.uniform(0.7, 1.3, H)), f(rng.uniform(-0.2, 0.2, H)))
        V[m] = f(rng.standard_normal((H, H)) * (0.5 / np.sqrt(H)))
    return X, V, f(rng.standard_normal((B, T, H * dirs)))

"""
tests/gated_numpy.py — the numpy restatement of the RNN, LiGRU and GRU cells that tests/test_gated_kernels_gpu.py
holds the HIP kernels to — pinned without a GPU:

  * to oracle.ann_oracle.hidden_layer run in float64 (normalization "none"; the projection matrices select and scale
    the columns of the input, so the oracle's projections ARE the cell's inputs x * scale + shift) and to torch
    autograd's gradients, 1e-12 relative to each tensor's largest entry (fp64 round-off with a wide margin), with and
    without dropout (the oracle's output times the restated mask);
  * structurally, bit for bit: yprev_all is y_state moved one cell step and re-indexed to the original time, its first
    cell step is zero, ry_all = r_save * yprev;
  * the per-step forms (rnn_step_fwd / _bwd, gate_step modes 0-5) chained over t with numpy matmuls in between give
    the whole-sequence functions bit for bit, in float64 and in float32.
"""
import numpy as np
import pytest
import torch

from oracle import ann_oracle as ao
from tests import gated_numpy as gn
from tests.kit import same_bits

B, T, H = 5, 7, 8
CELLS = [("RNN", "sigmoid"), ("RNN", "relu"), ("RNN", "tanh"), ("LiGRU", None), ("GRU", None)]
IDS = ["rnn_sigmoid", "rnn_relu", "rnn_tanh", "ligru", "gru"]
KEYS = {"c": ("W", "V"), "z": ("Wz", "Vz"), "r": ("Wr", "Vr")}
SEED = 0x5EED1234ABCD


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    scale = np.abs(want).max()
    assert scale > 0, f"{what}: the reference is all zero"
    assert np.abs(got - want).max() <= 1e-12 * scale, f"{what}: {np.abs(got - want).max() / scale:.3e} relative"


def forward(cell, kind, X, V, dirs, p, dtype=np.float64, matmul=np.matmul):
    if cell == "RNN":
        return gn.rnn_forward(kind, *X["c"], V["c"], dirs, p, SEED, dtype, matmul)
    return gn.gated_forward(cell, X, V, dirs, p, SEED, dtype, matmul)


def backward(cell, kind, g_out, fwd, V, dirs, p, dtype=np.float64, matmul=np.matmul):
    if cell == "RNN":
        return gn.rnn_backward(kind, g_out, fwd["y_state"], V["c"], dirs, p, SEED, dtype, matmul)
    return gn.gated_backward(cell, g_out, fwd, V, dirs, p, SEED, dtype, matmul)


def oracle_run(cell, kind, X, V, dirs, g_out, mask, monkeypatch):
    """hidden_layer in float64 and autograd: output, d loss / d (normalised projection) per matrix (the two directions
    already added, as they share their projection rows) and d loss / d V per matrix; loss = sum(out * mask * g_out)."""
    mats = list(X)
    if cell == "RNN":
        monkeypatch.setitem(ao.ACT, "RNN", {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh}[kind])
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        x = torch.from_numpy(np.concatenate([X[m][0] for m in mats], axis=2).astype(np.float64)).requires_grad_(True)
        p = {}
        for i, m in enumerate(mats):
            sel = np.zeros((H, H * len(mats)))
            sel[np.arange(H), i * H + np.arange(H)] = X[m][1].astype(np.float64)
            p[f"ann.0.{KEYS[m][0]}.weight"] = torch.from_numpy(sel)
            p[f"ann.0.{KEYS[m][0]}.bias"] = torch.from_numpy(X[m][2].astype(np.float64))
            p[f"ann.0.{KEYS[m][1]}.weight"] = torch.from_numpy(V[m].astype(np.float64)).requires_grad_(True)
        out = ao.hidden_layer(cell, x, p, "ann.0", "none", dirs == 2)
        assert out.dtype == torch.float64
        (out * torch.from_numpy(mask.astype(np.float64) * g_out.astype(np.float64))).sum().backward()
    finally:
        torch.set_default_dtype(old)
    dx = x.grad.numpy()
    dproj = {m: dx[:, :, i * H:(i + 1) * H] / X[m][1].astype(np.float64) for i, m in enumerate(mats)}
    dV = {m: p[f"ann.0.{KEYS[m][1]}.weight"].grad.numpy() for m in mats}
    return out.detach().numpy(), dproj, dV


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("cell,kind", CELLS, ids=IDS)
def test_restatement_equals_the_oracle_and_autograd_in_fp64(cell, kind, dirs, p_drop, monkeypatch):
    X, V, g_out = gn.inputs(cell, B, T, H, dirs, 11)
    mask = gn.mask_of(SEED, (B, T, H * dirs), p_drop, np.float64)
    if p_drop:
        assert 0 < (mask == 0).sum() < mask.size
    want_y, want_dproj, want_dV = oracle_run(cell, kind, X, V, dirs, g_out, mask, monkeypatch)
    fwd = forward(cell, kind, X, V, dirs, p_drop)
    close(fwd["y_out"], want_y * mask, "y_out")
    bwd = backward(cell, kind, g_out, fwd, V, dirs, p_drop)
    both = lambda a: a[:B] + a[B:] if dirs == 2 else a            # noqa: E731  (second direction already un-flipped)
    dVof = lambda d, yp: np.einsum("bti,btj->ij", d, yp)          # noqa: E731
    if cell == "RNN":
        close(both(bwd["dpre"]), want_dproj["c"], "dWx")
        close(dVof(bwd["dpre"], bwd["y_prev"]), want_dV["c"], "dV")
        return
    close(both(bwd["dz_all"]), want_dproj["z"], "dWzx")
    close(both(bwd["dc_all"]), want_dproj["c"], "dWx")
    close(dVof(bwd["dz_all"], bwd["yprev_all"]), want_dV["z"], "dVz")
    if cell == "GRU":
        close(both(bwd["dr_all"]), want_dproj["r"], "dWrx")
        close(dVof(bwd["dr_all"], bwd["yprev_all"]), want_dV["r"], "dVr")
        close(dVof(bwd["dc_all"], bwd["ry_all"]), want_dV["c"], "dV")
    else:
        close(dVof(bwd["dc_all"], bwd["yprev_all"]), want_dV["c"], "dV")


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("cell,kind", CELLS, ids=IDS)
def test_structural_identities_bit_for_bit(cell, kind, dirs):
    X, V, g_out = gn.inputs(cell, B, T, H, dirs, 12)
    fwd = forward(cell, kind, X, V, dirs, 0.25)
    bwd = backward(cell, kind, g_out, fwd, V, dirs, 0.25)
    yprev = bwd["y_prev" if cell == "RNN" else "yprev_all"]
    y = fwd["y_state"]
    for b in range(B * dirs):
        for t in range(T):
            tt = T - 1 - t if b >= B else t
            want = y[b, t - 1] if t > 0 else np.zeros(H)
            assert same_bits(yprev[b, tt], want), (b, t)
    first = yprev[:B, 0] if dirs == 1 else np.concatenate([yprev[:B, 0], yprev[B:, T - 1]])
    assert same_bits(first, np.zeros_like(first))                       # +0.0, not -0.0
    if cell == "GRU":
        r_orig = gn.to_original(fwd["r_save"], B, dirs)
        assert same_bits(bwd["ry_all"], r_orig * yprev)
        assert np.abs(bwd["ry_all"]).max() > 0
    # y_out: directions side by side at the original time index, times the mask
    mask = gn.mask_of(SEED, (B, T, H * dirs), 0.25, np.float64)
    for d in range(dirs):
        for t in range(T):
            tt = T - 1 - t if d else t
            assert same_bits(fwd["y_out"][:, tt, d * H:(d + 1) * H],
                             y[d * B:(d + 1) * B, t] * mask[:, tt, d * H:(d + 1) * H])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("cell,kind", CELLS, ids=IDS)
def test_per_step_forms_chain_to_the_whole_sequence(cell, kind, dirs, dtype):
    p = 0.25
    X, V, g_out = gn.inputs(cell, B, T, H, dirs, 13)
    fwd = forward(cell, kind, X, V, dirs, p, dtype)
    bwd = backward(cell, kind, g_out, fwd, V, dirs, p, dtype)
    Bp = B * dirs
    Vd = {m: V[m].astype(dtype) for m in V}
    new = lambda *s: np.full(s, np.nan, dtype)                    # noqa: E731
    c_ = np.ascontiguousarray
    if cell == "RNN":
        y_out, y_state, y_step = new(B, T, H * dirs), new(Bp, T, H), None
        for s in range(T):
            rec = np.matmul(y_step, Vd["c"].T) if s else None
            y_step = gn.rnn_step_fwd(kind, B, dirs, T, H, s, *X["c"], rec, p, SEED, y_out, y_state)
        assert same_bits(y_out, fwd["y_out"]) and same_bits(y_state, fwd["y_state"])
        dpre, y_prev, step = new(Bp, T, H), new(Bp, T, H), None
        for s in range(T):
            rec = np.matmul(step, Vd["c"]) if s else None
            step = gn.rnn_step_bwd(kind, B, dirs, T, H, s, g_out, y_state, rec, p, SEED, dpre, y_prev)
        assert same_bits(dpre, bwd["dpre"]) and same_bits(y_prev, bwd["y_prev"])
        return
    gru = cell == "GRU"
    ins = {"Wx": X["c"][0], "sc": X["c"][1], "sh": X["c"][2], "Wzx": X["z"][0], "scz": X["z"][1], "shz": X["z"][2]}
    if gru:
        ins.update(Wrx=X["r"][0], scr=X["r"][1], shr=X["r"][2])
    outs = {k: new(Bp, T, H) for k in ("y_state", "z_save", "c_save", "r_save", "dz_all", "dr_all", "dc_all",
                                       "yprev_all", "ry_all")}
    outs.update(ry=new(Bp, H), y_out=new(B, T, H * dirs), dgate=new(Bp, 2 * H), dcp=new(Bp, H))
    for t in range(T):
        yp = c_(outs["y_state"][:, t - 1])
        second = "r" if gru else "c"
        rec = np.concatenate([np.matmul(yp, Vd["z"].T), np.matmul(yp, Vd[second].T)], axis=1) if t else None
        if gru:
            gn.gate_step(1, B, dirs, T, H, t, dict(ins, rec=rec), outs, p, SEED)
            gn.gate_step(2, B, dirs, T, H, t, dict(ins, rec=np.matmul(outs["ry"], Vd["c"].T) if t else None), outs, p, SEED)
        else:
            gn.gate_step(0, B, dirs, T, H, t, dict(ins, rec=rec), outs, p, SEED)
    for k in ("y_state", "z_save", "c_save", "y_out") + (("r_save",) if gru else ()):
        assert same_bits(outs[k], fwd[k]), k
    Vgate = np.concatenate([Vd["z"], Vd["r"] if gru else Vd["c"]], axis=0)
    cdir = [new(Bp, H), new(Bp, H)]
    carry_mv = carry_dir = None
    for t in range(T - 1, -1, -1):
        o = dict(outs, carry_dir_out=cdir[t & 1])
        i = {"g_out": g_out, "carry_mv": carry_mv, "carry_dir": carry_dir}
        if gru:
            gn.gate_step(4, B, dirs, T, H, t, i, o, p, SEED)
            gn.gate_step(5, B, dirs, T, H, t, {"dry": np.matmul(outs["dcp"], Vd["c"])}, o, p, SEED)
        else:
            gn.gate_step(3, B, dirs, T, H, t, i, o, p, SEED)
        carry_mv, carry_dir = np.matmul(outs["dgate"], Vgate), cdir[t & 1]
    for k in ("dz_all", "dc_all", "yprev_all") + (("dr_all", "ry_all") if gru else ()):
        assert same_bits(outs[k], bwd[k]), k


def test_fp32_restatements_stay_close_to_fp64():
    """The yardstick of the GPU test's bounds is an fp32 run's error: it is fp32 round-off, not a different formula."""
    for cell, kind in CELLS:
        X, V, g_out = gn.inputs(cell, 6, 9, 64, 2, 14)
        ref = forward(cell, kind, X, V, 2, 0.25)
        for mm in (np.matmul, gn.matmul_chunked):
            got = forward(cell, kind, X, V, 2, 0.25, np.float32, mm)
            assert got["y_state"].dtype == np.float32
            err = np.abs(got["y_state"].astype(np.float64) - ref["y_state"]).max()
            assert 0 < err < 2e-5, (cell, kind, err)

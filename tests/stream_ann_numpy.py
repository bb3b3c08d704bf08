"""
TEST INFRASTRUCTURE ONLY: one STREAM STEP of the non-spiking baselines restated in plain numpy, at the level of the C
ABI (include/sparch_hip.h: sparch_ann_stream_step, sparch_ann_stream_readout), and a small stepper over a whole
network built from a tests/golden/ann_*.npz fixture.  It shares no code with the product and is generic in dtype:
float64 is the reference of tests/test_stream_ann_gpu.py, float32 (with numpy's matmul, and with the products
accumulated over K in chunks of 32) is the yardstick its bounds are made from.  tests/test_stream_ann_host.py pins it
to the real reference's eval-mode outputs.

    p?     = (x W?^T + bias?) * scale? + shift?       or  layernorm(x W?^T + bias?) * gamma? + beta?
    MLP    y  = act(p)
    RNN    y' = act(p + y V^T)
    LiGRU  z = sigmoid(pz + y Vz^T)   c = relu(p + y V^T)                               y' = z y + (1 - z) c
    GRU    z = sigmoid(pz + y Vz^T)   r = sigmoid(pr + y Vr^T)   c = tanh(p + (r y) V^T)   y' = z y + (1 - z) c
    readout  acc += softmax(y_t)      out = norm(acc W^T + bias)

A gate is a dict: W (H,K), V (H,H) or None, bias / scale / shift / gamma / beta (H) or None.  Gates are keyed "c" (the
candidate: W, V — the only one of MLP and RNN), "z", "r".
"""
import json

import numpy as np

EPS = 1e-5
GATES = {"MLP": ("c",), "RNN": ("c",), "LiGRU": ("c", "z"), "GRU": ("c", "z", "r")}
SUFFIX = {"c": "", "z": "z", "r": "r"}


def sigmoid(v):
    one = v.dtype.type(1)
    return one / (one + np.exp(-v))


def relu(v):
    return np.where(v <= 0, v.dtype.type(0), v)     # a NaN stays a NaN


ACTS = {"sigmoid": sigmoid, "relu": relu, "tanh": np.tanh}


def matmul_chunked(a, b, chunk=32):
    """a (M,K) @ b (K,N) with the contraction cut into chunks added up one after the other in the operands' dtype."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.result_type(a, b))
    for k0 in range(0, a.shape[1], chunk):
        acc = acc + np.matmul(a[:, k0:k0 + chunk], b[k0:k0 + chunk])
    return acc


def _as(a, dtype):
    return None if a is None else np.asarray(a, dtype=dtype)


def layernorm(v, gamma, beta, eps=EPS):
    mu = v.mean(axis=1, keepdims=True)
    var = ((v - mu) ** 2).mean(axis=1, keepdims=True)
    return (v - mu) / np.sqrt(var + v.dtype.type(eps)) * gamma + beta


def projection(x, gate, dtype, matmul):
    """The projection term of one gate from the step's input x (B,K)."""
    p = matmul(_as(x, dtype), _as(gate["W"], dtype).T)
    if gate.get("bias") is not None:
        p = p + _as(gate["bias"], dtype)
    if gate.get("scale") is not None:
        p = p * _as(gate["scale"], dtype) + _as(gate["shift"], dtype)
    if gate.get("gamma") is not None:
        p = layernorm(p, _as(gate["gamma"], dtype), _as(gate["beta"], dtype))
    return p


def hidden_step(cell, x, y, gates, act="sigmoid", dtype=np.float64, matmul=np.matmul):
    """One step of a hidden layer: x (B,K), y (B,H) the previous state (ignored by the MLP) -> dict with the new state
    "y" and, for the GRU, what its first phase hands to the second ("z", "ry")."""
    dtype = np.dtype(dtype).type
    p = {g: projection(x, gates[g], dtype, matmul) for g in GATES[cell]}
    one = dtype(1)
    if cell == "MLP":
        return {"y": ACTS[act](p["c"])}
    y = _as(y, dtype)
    rec = lambda v, g: matmul(v, _as(gates[g]["V"], dtype).T)  # noqa: E731
    if cell == "RNN":
        return {"y": ACTS[act](p["c"] + rec(y, "c"))}
    z = sigmoid(p["z"] + rec(y, "z"))
    if cell == "LiGRU":
        c = relu(p["c"] + rec(y, "c"))
        return {"y": z * y + (one - z) * c}
    r = sigmoid(p["r"] + rec(y, "r"))
    ry = r * y
    c = np.tanh(p["c"] + rec(ry, "c"))
    return {"y": z * y + (one - z) * c, "z": z, "ry": ry}


def readout_step(y_t, acc, W, bias=None, norm="none", p0=None, p1=None, dtype=np.float64, matmul=np.matmul):
    """acc (B,K) + softmax(y_t (B,K)) -> (new acc, out (B,C)); norm "none" | "affine" (p0 scale, p1 shift) |
    "layernorm" over the C outputs (p0 gamma, p1 beta)."""
    dtype = np.dtype(dtype).type
    v = _as(y_t, dtype)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    acc = _as(acc, dtype) + e / e.sum(axis=1, keepdims=True)
    out = matmul(acc, _as(W, dtype).T)
    if bias is not None:
        out = out + _as(bias, dtype)
    if norm == "affine":
        out = out * _as(p0, dtype) + _as(p1, dtype)
    elif norm == "layernorm":
        out = layernorm(out, _as(p0, dtype), _as(p1, dtype))
    return acc, out


# ------------------------------------------------------------------------------------------------ a fixture's network
def _norm_of(z, prefix, normalization):
    """The eval form of the normalisation stored under `prefix` ("ann.0.normz"): running statistics from after.*."""
    if normalization == "batchnorm":
        g, b = z[f"param.{prefix}.weight"].astype(np.float64), z[f"param.{prefix}.bias"].astype(np.float64)
        rm, rv = (z[f"after.{prefix}.running_{k}"].astype(np.float64) for k in ("mean", "var"))
        scale = g / np.sqrt(rv + EPS)
        return {"scale": scale, "shift": b - rm * scale}
    if normalization == "layernorm":
        return {"gamma": z[f"param.{prefix}.weight"], "beta": z[f"param.{prefix}.bias"]}
    return {}


def network(z):
    """(cfg, layers) of a tests/golden/ann_*.npz fixture: parameters param.*, running statistics after.*."""
    cfg = json.loads(str(z["cfg"]))
    n = len(cfg["layer_sizes"])
    layers = []
    for i in range(n):
        if cfg["use_readout_layer"] and i == n - 1:
            nm = _norm_of(z, f"ann.{i}.norm", cfg["normalization"])
            kind = {"batchnorm": "affine", "layernorm": "layernorm", "none": "none"}[cfg["normalization"]]
            layers.append({"readout": True, "W": z[f"param.ann.{i}.W.weight"], "bias": z.get(f"param.ann.{i}.W.bias"),
                           "norm": kind, "p0": nm.get("scale", nm.get("gamma")), "p1": nm.get("shift", nm.get("beta"))})
            continue
        gates = {}
        for g in GATES[cfg["ann_type"]]:
            s = SUFFIX[g]
            gates[g] = dict(W=z[f"param.ann.{i}.W{s}.weight"], bias=z.get(f"param.ann.{i}.W{s}.bias"),
                            V=z.get(f"param.ann.{i}.V{s}.weight"), **_norm_of(z, f"ann.{i}.norm{s}", cfg["normalization"]))
        layers.append({"readout": False, "cell": cfg["ann_type"], "gates": gates})
    return cfg, layers


def zero_state(layers, B, dtype=np.float64):
    return [np.zeros((B, L["W"].shape[1] if L["readout"] else L["gates"]["c"]["W"].shape[0]), dtype) for L in layers]


def stream(layers, state, x_chunk, dtype=np.float64, matmul=np.matmul):
    """x_chunk (B,Tc,C) through every layer step by step; `state` (zero_state's list: y per hidden layer, acc for the
    readout) is updated in place.  Returns the readout's output after the chunk's last step, or the last layer's
    outputs (B,Tc,H)."""
    outs = []
    for t in range(x_chunk.shape[1]):
        v = x_chunk[:, t]
        for i, L in enumerate(layers):
            if L["readout"]:
                state[i], v = readout_step(v, state[i], L["W"], L["bias"], L["norm"], L["p0"], L["p1"], dtype, matmul)
            else:
                state[i] = v = hidden_step(L["cell"], v, state[i], L["gates"], "sigmoid", dtype, matmul)["y"]
        outs.append(v)
    return outs[-1] if layers[-1]["readout"] else np.stack(outs, axis=1)

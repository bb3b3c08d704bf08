"""
TEST INFRASTRUCTURE ONLY: ANN.forward of the non-spiking baselines restated in plain torch, in the dtype of its inputs
(float32 or float64), for tests/ann_cases.py.

It builds on oracle/ann_oracle.py (pinned to the reference by tests/golden/ann_*.npz): the projections, the
normalisations and the readout are that module's own functions, which keep the dtype they are given; the recurrent
loops are restated here in the same order of operations, because ann_oracle.hidden_layer makes its initial state with
torch.zeros(Bp, H) and so runs in float32 only.  In float32, without masks and with running=None, ann_forward here gives
the bits of ann_oracle.ann_forward (tests/test_ann_fuzz_host.py).

What it adds to ann_oracle.ann_forward:
  masks     per-hidden-layer dropout masks (B, T, dirs * H), multiplied onto the layer's output only: the recurrent
            state a cell carries stays undropped (anns.py:226, 325: self.drop on the layer's result)
  running   BatchNorm running statistics in and out: the dict is updated in place by F.batch_norm (momentum 0.05, the
            unbiased batch variance), and used as they are in eval mode
  4-D input flattened to (B, T, F * channels) (anns.py:137-141)
  record    dict(relu=[...], hidden=[...]): every LiGRU candidate pre-activation (the argument of relu) as
            (rows, T, H) per layer, and every hidden layer's output before dropout

Three functions are looked up in the module at call time, so that tests/test_ann_fuzz_host.py can state a wrong network
by replacing one: `drop` (the mask on a layer's output), `carry` (the state a cell hands to its next step) and, through
ann_oracle.F, the normalisations and the softmax.
"""
import torch
import torch.nn.functional as F

from oracle import ann_oracle as ao

GATES = {"MLP": ("",), "RNN": ("",), "LiGRU": ("", "z"), "GRU": ("", "z", "r")}
RECURRENT = {"MLP": False, "RNN": True, "LiGRU": True, "GRU": True}


def drop(y, mask, layer):
    """Dropout with a given mask (0 or 1 / (1 - p)) on the output of hidden layer `layer`."""
    return y * mask


def carry(yt, t, layer):
    """The state a recurrent cell of hidden layer `layer` carries from step t to step t + 1: the undropped output."""
    return yt


def n_hidden(cfg):
    return len(cfg["layer_sizes"]) - 1 if cfg["use_readout_layer"] else len(cfg["layer_sizes"])


def hidden_layer(kind, x, p, pre, normalization, bidirectional, training=True, running=None, layer=0, relu_args=None):
    """ann_oracle.hidden_layer in x's dtype (same operations in the same order); relu_args: a list that receives the
    LiGRU's candidate pre-activations, (rows, T, H)."""
    act = ao.ACT[kind]
    if kind == "MLP":
        return act(ao._proj(x, p, pre + ".W", pre + ".norm", normalization, training, running))
    if bidirectional:
        x = torch.cat([x, x.flip(1)], dim=0)
    Wx = ao._proj(x, p, pre + ".W", pre + ".norm", normalization, training, running)
    Bp, T, H = Wx.shape
    V = p[pre + ".V.weight"]
    yt = torch.zeros(Bp, H, dtype=Wx.dtype)
    ys, args = [], []
    if kind == "RNN":
        for t in range(T):
            yt = act(Wx[:, t] + F.linear(yt, V))
            ys.append(yt)
            yt = carry(yt, t, layer)
    else:
        Wzx = ao._proj(x, p, pre + ".Wz", pre + ".normz", normalization, training, running)
        Vz = p[pre + ".Vz.weight"]
        if kind == "GRU":
            Wrx = ao._proj(x, p, pre + ".Wr", pre + ".normr", normalization, training, running)
            Vr = p[pre + ".Vr.weight"]
        for t in range(T):
            zt = torch.sigmoid(Wzx[:, t] + F.linear(yt, Vz))
            if kind == "GRU":
                rt = torch.sigmoid(Wrx[:, t] + F.linear(yt, Vr))
                ct = act(Wx[:, t] + F.linear(rt * yt, V))
            else:
                a = Wx[:, t] + F.linear(yt, V)
                args.append(a.detach())
                ct = act(a)
            yt = zt * yt + (1 - zt) * ct
            ys.append(yt)
            yt = carry(yt, t, layer)
    if relu_args is not None and args:
        relu_args.append(torch.stack(args, dim=1))
    y = torch.stack(ys, dim=1)
    if bidirectional:
        y_f, y_b = y.chunk(2, dim=0)
        y = torch.cat([y_f, y_b.flip(1)], dim=2)
    return y


def ann_forward(cfg, p, x, training=True, running=None, masks=None, record=None):
    """ANN.forward (anns.py:133-146).  cfg: ann_type, layer_sizes, use_readout_layer, normalization, bidirectional.
    p: parameters under the reference's state_dict keys, in x's dtype.  running: {key: running_mean / running_var} in
    x's dtype, updated in place by a train-mode pass, or None (batch statistics, nothing kept).  masks: one
    (B, T, dirs * H) mask per hidden layer, or None.  record: a dict that receives `relu` and `hidden`."""
    kind = cfg["ann_type"]
    if x.ndim == 4:
        x = x.flatten(2)
    relu_args, hidden = [], []
    for k in range(n_hidden(cfg)):
        x = hidden_layer(kind, x, p, f"ann.{k}", cfg["normalization"], cfg["bidirectional"], training, running, k,
                         relu_args)
        hidden.append(x.detach())
        if masks is not None:
            x = drop(x, masks[k], k)
    if cfg["use_readout_layer"]:
        x = ao.readout_layer(x, p, f"ann.{n_hidden(cfg)}", cfg["normalization"], training, running)
    if record is not None:
        record.update(relu=relu_args, hidden=hidden)
    return x

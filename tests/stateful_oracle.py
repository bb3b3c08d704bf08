"""
Stateful-training oracle (torch, CPU, autograd): what SNN.forward(x, state=st, return_state=True) must compute.

One invariant defines it: feeding x in chunks, each chunk started from the state the previous one returned, is the
whole-sequence forward started from the first chunk's state.  Built from the reference-faithful oracle's own pieces
(oracle.snn_oracle: spike, the clamp ranges, _normalise, BatchNorm's constants) with one change: the cells take a state
in and hand the state they ended in out —

  * spiking_cell returns (spikes, {"u": u_T, ["w": w_T,] "s": s_T}); s_T is the cell's own last spike, the raw one,
    before dropout (dropout scales the layer's output, not its state);
  * readout_cell returns (out, {"u": u_T}); out is the chunk's own softmax-sum.

The returned tensors are nodes of the graph: kept, autograd carries the gradient across the chunk boundary; detached, it
is classic truncated BPTT.  BatchNorm in train mode takes each chunk as the batch it is.

closed_form_state_grads() restates the three products that turn the reverse pass's last carries into the gradient of the
initial state ("Stateful training").  tests/test_stateful_oracle_host.py pins all of it against
oracle.snn_oracle.snn_forward and against autograd.
"""
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc


def spiking_cell(kind, Wx, p, u0, w0, s0, theta=1.0):
    """oracle.snn_oracle.spiking_cell (same operations in the same order: bit-identical spikes) that also returns the
    state it ended in."""
    adaptive, recurrent = orc.ADAPTIVE[kind], orc.RECURRENT[kind]
    alpha = torch.clamp(p["alpha"], min=orc.ALPHA_LIM[0], max=orc.ALPHA_LIM[1])
    if adaptive:
        beta = torch.clamp(p["beta"], min=orc.BETA_LIM[0], max=orc.BETA_LIM[1])
        a = torch.clamp(p["a"], min=orc.A_LIM[0], max=orc.A_LIM[1])
        b = torch.clamp(p["b"], min=orc.B_LIM[0], max=orc.B_LIM[1])
    if recurrent:
        Vm = p["V"].clone().fill_diagonal_(0)
    u, s, w = u0, s0, w0
    out = []
    for t in range(Wx.shape[1]):
        drive = Wx[:, t, :]
        if adaptive:
            w = beta * w + a * u + b * s
        if recurrent:
            drive = drive + torch.matmul(s, Vm)
        if adaptive:
            drive = drive - w
        u = alpha * (u - s) + (1 - alpha) * drive
        s = orc.spike(u - theta)
        out.append(s)
    state = {"u": u, "w": w, "s": s} if adaptive else {"u": u, "s": s}
    return torch.stack(out, dim=1), state


def readout_cell(Wx, alpha_raw, u0):
    """oracle.snn_oracle.readout_cell that also returns the membrane it ended on."""
    alpha = torch.clamp(alpha_raw, min=orc.ALPHA_LIM[0], max=orc.ALPHA_LIM[1])
    u = u0
    out = torch.zeros(Wx.shape[0], Wx.shape[2], dtype=Wx.dtype)
    for t in range(Wx.shape[1]):
        u = alpha * u + (1 - alpha) * Wx[:, t, :]
        out = out + F.softmax(u, dim=1)
    return out, {"u": u}


def _get(st, key):
    """A state entry under "u" / "w" / "s" or the oracle's "u0" / "w0" / "s0"."""
    return st.get(key, st.get(key + "0"))


def hidden_layer(kind, x, p, prefix, st, *, normalization="batchnorm", training=True, theta=1.0, stats=None,
                 drop_mask=None):
    """oracle.snn_oracle.hidden_layer, one direction, from the state `st`: (output after dropout, final state)."""
    Wx = F.linear(x, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    Wx = orc._normalise(Wx, p, prefix, normalization, training, stats)
    cell_p = {"alpha": p[prefix + "alpha"]}
    if orc.ADAPTIVE[kind]:
        cell_p.update(beta=p[prefix + "beta"], a=p[prefix + "a"], b=p[prefix + "b"])
    if orc.RECURRENT[kind]:
        cell_p["V"] = p[prefix + "V.weight"]
    s, final = spiking_cell(kind, Wx, cell_p, _get(st, "u"), _get(st, "w"), _get(st, "s"), theta)
    if drop_mask is not None:
        s = s * drop_mask
    return s, final


def readout_layer(x, p, prefix, st, *, normalization="batchnorm", training=True, stats=None):
    Wx = F.linear(x, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    Wx = orc._normalise(Wx, p, prefix, normalization, training, stats)
    return readout_cell(Wx, p[prefix + "alpha"], _get(st, "u"))


def snn_forward(x, p, *, neuron_type, num_layers, state, normalization="batchnorm", use_readout_layer=True,
                training=True, theta=1.0, stats=None, drop_masks=None, spikes_out=None):
    """oracle.snn_oracle.snn_forward from `state` (one entry per layer) -> (out, rates, the state it ended in)."""
    n_hidden = num_layers - 1 if use_readout_layer else num_layers
    spikes, final = [], []
    for i in range(n_hidden):
        x, st = hidden_layer(neuron_type, x, p, f"snn.{i}.", state[i], normalization=normalization, training=training,
                             theta=theta, stats=stats, drop_mask=None if drop_masks is None else drop_masks[i])
        spikes.append(x)
        final.append(st)
    if spikes_out is not None:
        spikes_out.extend(spikes)
    rates = torch.cat(spikes, dim=2).mean(dim=(0, 1))
    if use_readout_layer:
        x, st = readout_layer(x, p, f"snn.{n_hidden}.", state[n_hidden], normalization=normalization, training=training,
                              stats=stats)
        final.append(st)
    return x, rates, final


def chained(x, chunks, p, state, **kw):
    """x fed in `chunks` (step counts), each from the state the one before returned: (sum of out, the chunks' rates,
    the last state, every hidden layer's spikes over the whole sequence)."""
    assert sum(chunks) == x.shape[1]
    total, rates, t0, spikes = None, [], 0, None
    masks = kw.pop("drop_masks", None)
    for n in chunks:
        sp_c = []
        dm = None if masks is None else [m[:, t0:t0 + n] for m in masks]
        out, r, state = snn_forward(x[:, t0:t0 + n], p, state=state, drop_masks=dm, spikes_out=sp_c, **kw)
        total = out if total is None else total + out
        rates.append(r)
        spikes = [[s] for s in sp_c] if spikes is None else [a + [s] for a, s in zip(spikes, sp_c)]
        t0 += n
    return total, rates, state, [torch.cat(s, dim=1) for s in spikes]


def closed_form_state_grads(kind, p, du1, dw1):
    """The gradient of the initial state from the reverse pass's last carries du_1, dw_1 (the total gradients of u_1,
    w_1):  g_u0 = alpha du_1 + a dw_1,  g_w0 = beta dw_1,  g_s0 = -alpha du_1 + b dw_1 + ((1 - alpha) du_1) Vm^T."""
    alpha = torch.clamp(p["alpha"], min=orc.ALPHA_LIM[0], max=orc.ALPHA_LIM[1])
    g_u0, g_s0, g_w0 = alpha * du1, -alpha * du1, None
    if orc.ADAPTIVE[kind]:
        beta = torch.clamp(p["beta"], min=orc.BETA_LIM[0], max=orc.BETA_LIM[1])
        a = torch.clamp(p["a"], min=orc.A_LIM[0], max=orc.A_LIM[1])
        b = torch.clamp(p["b"], min=orc.B_LIM[0], max=orc.B_LIM[1])
        g_u0, g_w0, g_s0 = g_u0 + a * dw1, beta * dw1, g_s0 + b * dw1
    if orc.RECURRENT[kind]:
        Vm = p["V"].clone().fill_diagonal_(0)
        g_s0 = g_s0 + torch.matmul((1 - alpha) * du1, Vm.t())
    return g_u0, g_w0, g_s0

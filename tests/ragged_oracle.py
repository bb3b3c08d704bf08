"""
Ragged-batch oracle (torch, CPU, autograd): what SNN.forward(x, lengths) must compute.

One invariant defines it: row b of every output is what the network gives for x[b:b+1, :lengths[b]] run on its own,
with the same initial-state rows and, in train mode, the same normalisation statistics.  Built from the
reference-faithful oracle's own pieces (oracle.snn_oracle: spiking_cell, readout_cell, the clamp ranges and BatchNorm
constants), with three changes:

  * hidden spikes are multiplied by the validity mask (t < lengths[b]); the cells are causal and rows do not mix, so
    the valid steps are the truncated run's, and the product makes the gradient that arrives at padded steps vanish;
  * BatchNorm in train mode takes its statistics over the N = sum(lengths) valid rows, packed, through the same
    F.batch_norm call (running statistics with the unbiased variance over N);
  * the readout runs readout_cell per row on the row's own steps (a truncated sum), and firing rates are
    sum(spikes) / N.

tests/test_ragged_oracle_host.py pins it against oracle.snn_oracle.snn_forward where the two must agree.
"""
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc


def valid_mask(lengths, T):
    """(B, T) bool: t < lengths[b]."""
    return torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]


def _normalise(Wx, mask, p, prefix, normalization, training, stats):
    """oracle._normalise on the valid rows: BatchNorm over the packed (N, H) rows, LayerNorm row by row.  Padded rows
    come out as zeros: nothing valid reads them."""
    if normalization not in ("batchnorm", "layernorm"):
        return Wx
    B, T, H = Wx.shape
    packed = Wx[mask]  # (N, H), row-major over (b, t)
    if normalization == "batchnorm":
        rm = p[prefix + "norm.running_mean"].clone()
        rv = p[prefix + "norm.running_var"].clone()
        packed = F.batch_norm(packed, rm, rv, p[prefix + "norm.weight"], p[prefix + "norm.bias"], training,
                              orc.BN_MOMENTUM, orc.BN_EPS)
        if stats is not None:
            stats[prefix + "norm.running_mean"] = rm
            stats[prefix + "norm.running_var"] = rv
    else:
        packed = F.layer_norm(packed, (H,), p[prefix + "norm.weight"], p[prefix + "norm.bias"], orc.BN_EPS)
    out = torch.zeros(B, T, H, dtype=Wx.dtype)
    out[mask] = packed
    return out


def hidden_layer(kind, x, mask, p, prefix, init, *, normalization, training, theta=1.0, stats=None, drop_mask=None):
    Wx = F.linear(x, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    Wx = _normalise(Wx, mask, p, prefix, normalization, training, stats)
    cell_p = {"alpha": p[prefix + "alpha"]}
    if orc.ADAPTIVE[kind]:
        cell_p.update(beta=p[prefix + "beta"], a=p[prefix + "a"], b=p[prefix + "b"])
    if orc.RECURRENT[kind]:
        cell_p["V"] = p[prefix + "V.weight"]
    s = orc.spiking_cell(kind, Wx, cell_p, init["u0"], init.get("w0"), init["s0"], theta)
    if drop_mask is not None:
        s = s * drop_mask
    return s * mask[:, :, None].to(s.dtype)


def readout_layer(x, lengths, mask, p, prefix, u0, *, normalization, training, stats=None):
    Wx = F.linear(x, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    Wx = _normalise(Wx, mask, p, prefix, normalization, training, stats)
    rows = [orc.readout_cell(Wx[b:b + 1, :int(L)], p[prefix + "alpha"], u0[b:b + 1]) for b, L in enumerate(lengths)]
    return torch.cat(rows, dim=0)


def snn_forward(x, lengths, p, *, neuron_type, num_layers, init_states, normalization="batchnorm", training=True,
                theta=1.0, stats=None, drop_masks=None, spikes_out=None):
    """oracle.snn_forward with lengths (B,) — one direction, a readout layer.  x must be zero at padded steps (the
    caller's contract); the result does not depend on it without a bias, and this oracle does not check it."""
    lengths = [int(v) for v in torch.as_tensor(lengths).tolist()]
    B, T = x.shape[0], x.shape[1]
    assert len(lengths) == B and all(1 <= v <= T for v in lengths)
    mask = valid_mask(lengths, T)
    n_hidden = num_layers - 1
    spikes = []
    for i in range(n_hidden):
        x = hidden_layer(neuron_type, x, mask, p, f"snn.{i}.", init_states[i], normalization=normalization,
                         training=training, theta=theta, stats=stats,
                         drop_mask=None if drop_masks is None else drop_masks[i])
        spikes.append(x)
    if spikes_out is not None:
        spikes_out.extend(spikes)
    rates = torch.cat(spikes, dim=2).sum(dim=(0, 1)) / float(sum(lengths))
    out = readout_layer(x, lengths, mask, p, f"snn.{n_hidden}.", init_states[n_hidden]["u0"],
                        normalization=normalization, training=training, stats=stats)
    return out, rates

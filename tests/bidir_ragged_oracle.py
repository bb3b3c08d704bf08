"""
Bidirectional ragged-batch oracle (torch, CPU, autograd): what SNN(bidirectional=True).forward(x, lengths) must compute.

One invariant defines it: row b of every output is what the bidirectional network gives for x[b:b+1, :lengths[b]] run on
its own (oracle.snn_oracle.snn_forward(bidirectional=True)) with the initial-state rows b and B + b and, in train mode,
the batch's normalisation statistics.  Built from tests/ragged_oracle.py's pieces on the 2B-row batch:

  * the layer's input is stacked with its copy flipped INSIDE each clip's own length (step t of row B + b is step
    lengths[b] - 1 - t of clip b; zeros behind) — the reference's cat([x, x.flip(1)]) when every length is T;
  * the normalisation runs on the 2N valid rows (ragged_oracle._normalise with the mask twice): mean and biased variance
    are one direction's, the running variance's unbiased correction sees 2N samples;
  * the cell runs on the 2B rows, spikes are masked, the reverse half is flipped back inside each length and stacked on
    the features (forward columns first);
  * firing rates are sum(spikes) / N per column: each direction is its own count over N = sum(lengths).

tests/test_bidir_ragged_oracle_host.py pins it against oracle.snn_oracle.snn_forward where the two must agree.
"""
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc
from tests import ragged_oracle as rag


class _Step(torch.autograd.Function):
    """oracle._Boxcar in the input's own dtype (the oracle's returns float32 whatever it is given)."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return (x > 0).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g_x = g.clone()
        g_x[x <= -0.5] = 0
        g_x[x > 0.5] = 0
        return g_x


class own_dtype_spikes:
    """For the `with` block, oracle.snn_oracle.spike keeps its input's dtype (an fp64 run stays fp64) and every
    u - theta it sees is appended to `.seen` (one (rows, H) tensor per layer and step)."""

    def __init__(self):
        self.seen = []

    def __enter__(self):
        def step(d):
            self.seen.append(d.detach())
            return _Step.apply(d)
        self.old, orc.spike = orc.spike, step
        return self

    def __exit__(self, *exc):
        orc.spike = self.old


def flip_in_length(x, lengths):
    """x (B,T,...) -> the same with every row's first lengths[b] steps reversed and zeros behind them."""
    B, T = x.shape[0], x.shape[1]
    L = torch.as_tensor(lengths)[:, None]
    t = torch.arange(T)[None, :]
    src = torch.where(t < L, L - 1 - t, t)                         # (B,T)
    idx = src.reshape(B, T, *([1] * (x.ndim - 2))).expand_as(x)
    keep = (t < L).reshape(B, T, *([1] * (x.ndim - 2))).to(x.dtype)
    return torch.gather(x, 1, idx) * keep


def hidden_layer(kind, x, lengths, mask, p, prefix, init, *, normalization, training, theta=1.0, stats=None,
                 drop_mask=None):
    """init: u0 / [w0] / s0 with 2B rows, row B + b the reverse direction of clip b.  drop_mask (B,T,2H) or None."""
    x2 = torch.cat([x, flip_in_length(x, lengths)], dim=0)
    mask2 = torch.cat([mask, mask], dim=0)
    Wx = F.linear(x2, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    Wx = rag._normalise(Wx, mask2, p, prefix, normalization, training, stats)
    cell_p = {"alpha": p[prefix + "alpha"]}
    if orc.ADAPTIVE[kind]:
        cell_p.update(beta=p[prefix + "beta"], a=p[prefix + "a"], b=p[prefix + "b"])
    if orc.RECURRENT[kind]:
        cell_p["V"] = p[prefix + "V.weight"]
    s = orc.spiking_cell(kind, Wx, cell_p, init["u0"], init.get("w0"), init["s0"], theta)
    s = s * mask2[:, :, None].to(s.dtype)
    s_f, s_b = s.chunk(2, dim=0)
    s = torch.cat([s_f, flip_in_length(s_b, lengths)], dim=2)
    if drop_mask is not None:
        s = s * drop_mask
    return s


def snn_forward(x, lengths, p, *, neuron_type, num_layers, init_states, normalization="batchnorm", training=True,
                theta=1.0, stats=None, drop_masks=None, spikes_out=None):
    """ragged_oracle.snn_forward with bidirectional hidden layers and a readout layer.  x must be zero at padded steps."""
    lengths = [int(v) for v in torch.as_tensor(lengths).tolist()]
    B, T = x.shape[0], x.shape[1]
    assert len(lengths) == B and all(1 <= v <= T for v in lengths)
    mask = rag.valid_mask(lengths, T)
    n_hidden = num_layers - 1
    spikes = []
    for i in range(n_hidden):
        x = hidden_layer(neuron_type, x, lengths, mask, p, f"snn.{i}.", init_states[i], normalization=normalization,
                         training=training, theta=theta, stats=stats,
                         drop_mask=None if drop_masks is None else drop_masks[i])
        spikes.append(x)
    if spikes_out is not None:
        spikes_out.extend(spikes)
    rates = torch.cat(spikes, dim=2).sum(dim=(0, 1)) / float(sum(lengths))
    out = rag.readout_layer(x, lengths, mask, p, f"snn.{n_hidden}.", init_states[n_hidden]["u0"],
                            normalization=normalization, training=training, stats=stats)
    return out, rates


def rows_of(init_states, b, B):
    """The initial states of clip b run alone: rows b and B + b of every hidden layer, row b of the readout."""
    return [{k: (torch.cat([v[b:b + 1], v[B + b:B + b + 1]]) if v.shape[0] == 2 * B else v[b:b + 1]) for k, v in st.items()}
            for st in init_states]

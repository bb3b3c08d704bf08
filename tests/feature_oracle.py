"""
One composed oracle (torch, CPU, autograd, any dtype) of a whole spiking network with every feature the layer host code
joins: layouts (dense, `lengths`; `pack=True` shares the `lengths` contract), two directions, axonal delays, synaptic
currents, dropout, the selectable and the per-step readouts.  For tests/feature_cases.py.

Nothing here comes from the package.  Every piece is one the tests already trust:

  delays       tests/delay_numpy.py forward / backward_x / backward_theta behind a torch.autograd.Function (Delay): the
               shift d = rint(clamp(delay, 0, D)) inside each row's own length, spikes shifted past the end dropped, the
               gated finite difference as delay's gradient.  In fp64 that gradient is delay_numpy.backward_theta itself.
               In any other dtype it is the same sum taken in that dtype — sum g_y * (forward(x, d + 1) - forward(x, d)),
               both shifts by delay_numpy.forward — so that an fp32 run of the oracle is a sample of fp32 arithmetic and
               not an fp64 sum rounded once; tests/test_feature_fuzz_host.py holds the two forms to each other.
  projection   F.linear, then oracle.snn_oracle._normalise (no lengths) or tests/ragged_oracle._normalise (statistics
               over the valid steps; on the doubled batch with the mask twice).
  synapse      tests/synapse_cases.synapse_filter between the normalisation and the cell, on the doubled batch for two
               directions (each direction filtered causally in its own time order).
  cells        oracle.snn_oracle.spiking_cell; two directions stacked as oracle.snn_oracle.hidden_layer stacks them (no
               lengths) or with tests/bidir_ragged_oracle.flip_in_length (lengths).
  dropout      a constant multiplier per hidden layer that the caller makes on the host (feature_cases.case).
  readout      the default softmax-sum through oracle.snn_oracle.readout_cell / tests/ragged_oracle.readout_layer — so
               that with every new feature off this file IS the existing oracles, bit for bit —; the other four modes
               (and the default, in the host test, against the former) through tests/readout_modes_numpy.torch_forward;
               per_step through tests/readout_seq_numpy.torch_forward.  With lengths every reduction runs over the row's
               own steps.

The operation order of each branch is that of the oracle it extends (oracle.snn_oracle.hidden_layer,
ragged_oracle.hidden_layer, bidir_ragged_oracle.hidden_layer), which is what makes the three bit-for-bit checks of
tests/test_feature_fuzz_host.py possible.

Dropout on the doubled ragged batch (two directions with lengths or pack, and two directions with a synapse, which
takes that route without lengths too): tests/ has no host restatement of the mask index there, and none is written
here — feature_cases.draw() gives those cases dropout = 0.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc
from tests import bidir_ragged_oracle as bro
from tests import delay_numpy as dn
from tests import ragged_oracle as rag
from tests import readout_modes_numpy as rmn
from tests import readout_seq_numpy as rsq
from tests.synapse_cases import synapse_filter


class Delay(torch.autograd.Function):
    """y = delay_numpy.forward(x, delay, D, lengths); backward: delay_numpy.backward_x and the gated finite difference
    (module docstring).  delay holds fp32 values in whatever dtype it arrives."""

    @staticmethod
    def forward(ctx, x, delay, D, lengths):
        ctx.save_for_backward(x, delay)
        ctx.D, ctx.lengths = D, lengths
        return torch.from_numpy(dn.forward(x.detach().numpy(), delay.detach().numpy(), D, lengths))

    @staticmethod
    def backward(ctx, g_y):
        x, delay = ctx.saved_tensors
        D, lengths = ctx.D, ctx.lengths
        theta, g = delay.detach().numpy(), g_y.contiguous().numpy()
        g_x = torch.from_numpy(dn.backward_x(g, theta, D, lengths)) if ctx.needs_input_grad[0] else None
        g_theta = None
        if ctx.needs_input_grad[1]:
            if g_y.dtype == torch.float64:
                g_theta = torch.from_numpy(dn.backward_theta(g, x.numpy(), theta, D, lengths)[0])
            else:
                g_theta = finite_difference(g_y, x, theta, D, lengths).to(delay.dtype)
        return g_x, g_theta, None, None


def finite_difference(g_y, x, theta, D, lengths):
    """delay_numpy.backward_theta's sum in g_y's own dtype: forward(x, d) is x[t - d] on d <= t < len and forward(x,
    d + 1) is x[t - d - 1] there (0 at t = d), both 0 elsewhere, so their difference times g_y summed over (b, t) is the
    restatement's sum."""
    d = dn.steps(theta, D)
    xs = x.detach().numpy()
    near = dn.forward(xs, d.astype(np.float32), D, lengths)
    far = dn.forward(xs, (d + 1).astype(np.float32), D + 1, lengths)
    total = (g_y * torch.from_numpy(far - near)).sum(dim=(0, 1))
    return total * torch.from_numpy(dn.gate(theta, D)).to(total.dtype)


def _cell_params(kind, p, prefix):
    cell_p = {"alpha": p[prefix + "alpha"]}
    if orc.ADAPTIVE[kind]:
        cell_p.update(beta=p[prefix + "beta"], a=p[prefix + "a"], b=p[prefix + "b"])
    if orc.RECURRENT[kind]:
        cell_p["V"] = p[prefix + "V.weight"]
    return cell_p


def hidden_layer(kind, x, lengths, p, prefix, init, *, normalization, bidirectional, training, theta=1.0, stats=None,
                 drop_mask=None, max_delay=0, synapse=None, pre_cell=None):
    """One hidden layer.  lengths: None or a list; a `delay` / `gamma` under the prefix switches that feature on.
    pre_cell (a list): receives the cell's input (rows, T, H), for the host tests."""
    T = x.shape[1]
    if prefix + "delay" in p:
        x = Delay.apply(x, p[prefix + "delay"], max_delay, lengths)
    mask = None if lengths is None else rag.valid_mask(lengths, T)
    if bidirectional and lengths is None:
        x = torch.cat([x, x.flip(1)], dim=0)
    elif bidirectional:
        x, mask = torch.cat([x, bro.flip_in_length(x, lengths)], dim=0), torch.cat([mask, mask], dim=0)
    Wx = F.linear(x, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    if lengths is None:
        Wx = orc._normalise(Wx, p, prefix, normalization, training, stats)
    else:
        Wx = rag._normalise(Wx, mask, p, prefix, normalization, training, stats)
    if prefix + "gamma" in p:
        Wx = synapse_filter(Wx, p[prefix + "gamma"], synapse)
    if pre_cell is not None:
        pre_cell.append(Wx.detach())
    s = orc.spiking_cell(kind, Wx, _cell_params(kind, p, prefix), init["u0"], init.get("w0"), init["s0"], theta)
    if lengths is None:                         # oracle.snn_oracle.hidden_layer
        if bidirectional:
            s_f, s_b = s.chunk(2, dim=0)
            s = torch.cat([s_f, s_b.flip(1)], dim=2)
        if drop_mask is not None:
            s = s * drop_mask
    elif not bidirectional:                     # ragged_oracle.hidden_layer
        if drop_mask is not None:
            s = s * drop_mask
        s = s * mask[:, :, None].to(s.dtype)
    else:                                       # bidir_ragged_oracle.hidden_layer
        s = s * mask[:, :, None].to(s.dtype)
        s_f, s_b = s.chunk(2, dim=0)
        s = torch.cat([s_f, bro.flip_in_length(s_b, lengths)], dim=2)
        if drop_mask is not None:
            s = s * drop_mask
    return s


def readout_layer(x, lengths, p, prefix, u0, *, normalization, training, stats=None, max_delay=0,
                  readout="softmax_sum", per_step=None, force_modes=False):
    """out, or (out, seq) with per_step.  force_modes: the default readout through readout_modes_numpy.torch_forward
    too (the host test compares the two forms)."""
    T = x.shape[1]
    if prefix + "delay" in p:
        x = Delay.apply(x, p[prefix + "delay"], max_delay, lengths)
    Wx = F.linear(x, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    if lengths is None:
        Wx = orc._normalise(Wx, p, prefix, normalization, training, stats)
    else:
        Wx = rag._normalise(Wx, rag.valid_mask(lengths, T), p, prefix, normalization, training, stats)
    if per_step is not None:
        assert readout == "softmax_sum"
        return rsq.torch_forward(Wx, p[prefix + "alpha"], u0, per_step, lengths)
    if readout == "softmax_sum" and not force_modes:
        if lengths is None:
            return orc.readout_cell(Wx, p[prefix + "alpha"], u0)
        rows = [orc.readout_cell(Wx[b:b + 1, :int(L)], p[prefix + "alpha"], u0[b:b + 1]) for b, L in enumerate(lengths)]
        return torch.cat(rows, dim=0)           # (ragged_oracle.readout_layer's two lines)
    return rmn.torch_forward(Wx, p[prefix + "alpha"], u0, readout, lengths)


def snn_forward(x, p, *, neuron_type, num_layers, init_states, lengths=None, normalization="batchnorm",
                bidirectional=False, use_readout_layer=True, training=True, theta=1.0, stats=None, drop_masks=None,
                spikes_out=None, max_delay=0, synapse=None, readout="softmax_sum", per_step=None, force_modes=False,
                pre_cell=None):
    """(out, rates), with per_step (out, rates, seq).  p is keyed like the package's state_dict: the reference's keys
    plus `snn.{i}.delay` and `snn.{i}.gamma` for the layers that have the feature.  With lengths x must be zero at
    padded steps; masked and packed calls share this function (the contract is the same; the caller's dropout masks
    carry the one difference in values)."""
    if lengths is not None:
        lengths = [int(v) for v in torch.as_tensor(lengths).tolist()]
        assert len(lengths) == x.shape[0] and all(1 <= v <= x.shape[1] for v in lengths)
    n_hidden = num_layers - 1 if use_readout_layer else num_layers
    spikes = []
    for i in range(n_hidden):
        x = hidden_layer(neuron_type, x, lengths, p, f"snn.{i}.", init_states[i], normalization=normalization,
                         bidirectional=bidirectional, training=training, theta=theta, stats=stats,
                         drop_mask=None if drop_masks is None else drop_masks[i], max_delay=max_delay, synapse=synapse,
                         pre_cell=pre_cell)
        spikes.append(x)
    if spikes_out is not None:
        spikes_out.extend(spikes)
    if lengths is None:
        rates = torch.cat(spikes, dim=2).mean(dim=(0, 1))
    else:
        rates = torch.cat(spikes, dim=2).sum(dim=(0, 1)) / float(sum(lengths))
    if not use_readout_layer:
        assert per_step is None
        return x, rates
    res = readout_layer(x, lengths, p, f"snn.{n_hidden}.", init_states[n_hidden]["u0"], normalization=normalization,
                        training=training, stats=stats, max_delay=max_delay, readout=readout, per_step=per_step,
                        force_modes=force_modes)
    if per_step is not None:
        return res[0], rates, res[1]
    return res, rates

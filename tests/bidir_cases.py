"""
The whole-network cases of the bidirectional ragged tests (tests/test_bidir_ragged_gpu.py on the device,
tests/test_bidir_ragged_oracle_host.py for the data seed's margin): the small recipe of tests/test_ragged_gpu.py — sizes
[64, 64, 20], 6 clips of up to 23 steps and 40 features with the lengths [23, 1, 9, 17, 2, 22], dyadic weights, initial
states on a 2^-4 grid, 12 rows per hidden layer (row 6 + b the reverse direction of clip b) — and one oracle step of it.
"""
import numpy as np
import torch

from oracle import snn_oracle as orc
from tests import bidir_ragged_oracle as bro
from tests import packed_cases as pc
from tests import packed_numpy as pn

NB, NT, NC, SIZES, LENGTHS = pc.NB, pc.NT, pc.NC, pc.SIZES, pc.NET_LENGTHS
KINDS = ["LIF", "adLIF", "RLIF", "RadLIF"]
NORMS = ["batchnorm", "layernorm", "none"]
# The data seed of the oracle comparison (inputs, labels, initial states; the network's own seed is make_net's 3).  Count
# equality is a condition on the data: every u - theta of the oracle must be further from 0 than the arithmetic
# differences between two correct evaluations.  On the CPU, for the seeds 11 .. 30, the oracle was run in fp32 and in fp64
# for all 24 (kind, normalisation, train / eval) cases.  The two runs agree on every spike of every valid step at every one
# of these seeds.  An absolute margin of 1e-3 is out of reach at this shape: a case has 2 x 2 x 74 x 64 = 18944 valid
# values of u - theta spread over a range of a few units, several of them fall within 1e-3 of 0 whatever the seed, and the
# smallest |u - theta| over the 24 cases lies between 1.2e-7 and 1.3e-5 for the twenty seeds.  So the margin is taken
# relative to the rounding that could flip a spike, element by element: MARGIN_RATIO is the smallest |u - theta| (fp64)
# over that element's own fp32-versus-fp64 difference.  DATA_SEED = 13 is the first seed at which it is at least 32 in
# every case (48.0; seeds 11 and 12 give 6.2 and 8.4) — four times the factor 8 that tests/network_cases.py asks of a kept
# case.  tests/test_bidir_ragged_oracle_host.py::test_the_data_seed_keeps_its_margin recomputes it for all 24 cases.
DATA_SEED = 13
MARGIN_RATIO = 32.0


class _TwoDirections:
    """oracle.snn_oracle's draws for a bidirectional network (2 NB rows per hidden layer), as packed_cases.net_inputs
    calls them."""

    @staticmethod
    def draw_init_states(batch, sizes, kind):
        return orc.draw_init_states(batch, sizes, kind, bidirectional=True)


def make_net(sp, kind, normalization, dropout=0.0, seed=3, **kw):
    """packed_cases.make_net's dyadic network with bidirectional hidden layers."""
    torch.manual_seed(seed)
    net = sp.SNN((NB, None, NC), SIZES, neuron_type=kind, dropout=dropout, normalization=normalization, bidirectional=True,
                 **kw)
    with torch.no_grad():
        for lay in net.snn:
            lay.W.weight.copy_(torch.round((lay.W.weight * 4 + 0.25) * 64) / 64)   # (a positive drive: every layer spikes)
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
            if normalization in ("batchnorm", "layernorm"):   # (a live affine: the normalised drive reaches the threshold)
                lay.norm.weight.copy_(torch.round((torch.rand_like(lay.norm.weight) + 1.0) * 16) / 16)
                lay.norm.bias.copy_(torch.round((torch.rand_like(lay.norm.bias) * 0.5 + 0.25) * 16) / 16)
    return net


def net_inputs(kind, seed=DATA_SEED, lengths=LENGTHS):
    return pc.net_inputs(_TwoDirections, kind, seed=seed, lengths=lengths)


def oracle_step(kind, normalization, training, params, x, y, init, dtype=torch.float32):
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t  # noqa: E731
    po = {k: cast(v).clone().requires_grad_(v.dtype == torch.float32 and "running" not in k) for k, v in params.items()
          if "num_batches" not in k}
    stats, spikes = {}, []
    with bro.own_dtype_spikes() as rec:
        out_o, rates_o = bro.snn_forward(cast(x), LENGTHS, po, neuron_type=kind, num_layers=3,
                                         init_states=[{k: cast(v) for k, v in st.items()} for st in init],
                                         normalization=normalization, training=training, stats=stats, spikes_out=spikes)
        loss_o = orc.train_step_loss(out_o, rates_o, y, use_regularizers=True)
        loss_o.backward()
    # u - theta of the valid steps: per hidden layer NT tensors of (2 NB, H), in time order of the doubled batch
    m2 = torch.from_numpy(np.concatenate([pn.valid_mask(LENGTHS, NT)] * 2))
    diffs = torch.cat([torch.stack(rec.seen[i * NT:(i + 1) * NT], dim=1)[m2].reshape(-1) for i in range(2)])
    return po, out_o, rates_o, loss_o, stats, spikes, diffs

"""
Cases and references of tests/test_packed_gpu.py: the ragged scan reference and bounds of tests/test_ragged_gpu.py restated
for the packed kernels (no test module imports another), and the small dyadic networks of the whole-network tests.

The reverse pass's reference is the fp64 restatement tests/spiking_numpy.py / tests/surrogate_numpy.py with the validity
mask as its keep multiplier — g = (g_out + g_rate / N) * keep * [t < L_b] — run on PADDED arrays: the packed kernel's
saves and results are unpacked to (B,T,H) with zero tails first.  From a zero incoming gradient the carries stay zero over
a row's tail, so the padded run is the row run alone on its own steps.
"""
import functools

import numpy as np
import torch

from tests import packed_numpy as pn
from tests import spiking_numpy as sn
from tests import surrogate_numpy as sg
from tests.dropout_numpy import keep_mask
from tests.kit import F32, F64, SEED

POOL_SEEDS = 8


def sorted_lengths(B, T, seed):
    """The descending sort of {T, T - 1, 2, 1} and random ones: B lengths, already in packed order."""
    rng = np.random.default_rng(seed)
    fixed = [v for v in (1, 2, T - 1, T) if 1 <= v <= T]
    lens = (fixed + [int(v) for v in rng.integers(1, T + 1, max(B - len(fixed), 0))])[:B]
    return np.asarray(sorted(lens, reverse=True), np.int64)


def packed_keep(lens, T, H, p_drop, seed=SEED):
    """The packed kernels' dropout multiplier — the mask of tests/dropout_numpy.py on the element index of the packed
    (N,H) tensor — as a padded (B,T,H) array with zero tails; lens in packed order."""
    return pn.unpack_sorted(keep_mask(seed, (int(np.sum(lens)), H), p_drop), lens, T)


def seeded_scan_case(kind, B, T, H, salt):
    """spiking_numpy.scan_case's recipe on another seed."""
    seed = sn.case_seed(kind, B, 1, T, H) + 7919 * salt
    c = sn.make_inputs(kind, B, 1, T, H, seed, "drive", affine_in=True)
    c["g_rate"] = c["g_rate"] * F32(B * T)
    for k in c["p"]:
        c["p"][k][0], c["p"][k][1] = sn.OUTSIDE[k]
    rng = np.random.default_rng(seed + 1)
    c["bn"] = ((c["Wx"] * F32(0.8) + F32(0.3)).astype(F32), rng.uniform(0.2, 0.6, H).astype(F32),
               rng.uniform(0.5, 1.5, H).astype(F32))
    return c


def ragged_backward_runs(c, lens, us, ws, keep, with_bn, surrogate=None):
    """The restatement's reverse pass with the mask as its keep multiplier, on the padded saves us / ws: (fp64 run,
    [fp32 runs])."""
    kind, B, T, H = c["kind"], c["B"], c["T"], c["H"]
    m = pn.valid_mask(lens, T)[:, :, None]
    g_clean = np.where(m, c["g_out"], 0).astype(F32)
    # the restatement applies g = (g_out + g_rate / (B T)) * keep: the mask is the keep multiplier, N the rate's count
    g_rate = (c["g_rate"].astype(F64) * (B * T / int(np.sum(lens)))).astype(F32)
    keep_m = (m * (keep if keep is not None else F32(1))).astype(F32) * np.ones((1, 1, H), F32)

    def bw(dt, ko, ro):
        return sn.flat(sg.backward(kind, dt, g_clean, g_rate, us, ws, c["p"], c["u0"], c["w0"], c["s0"], B=B, dirs=1,
                                   surrogate=surrogate or ("boxcar", None), theta=c["theta"], k_order=ko,
                                   bn=c["bn"] if with_bn else None, keep=keep_m, row_order=ro))
    return bw(F64, None, None), [bw(F32, "asc", "asc"), bw(F32, "desc", "desc")]


@functools.lru_cache(maxsize=None)
def pooled_relative_error(kind, B, T, H, lens, p_drop, with_bn, surrogate=None):
    """tests/test_ragged_gpu.py's pooled sample of the fp32 error: the worst fp32 error RELATIVE to the fp64 tensor's
    max-abs over POOL_SEEDS further cases of the same recipe, shape, lengths and keep mask, each on the restatement's own
    free-running saves — nothing of the kernel enters."""
    lens = np.asarray(lens)
    names = sn.bwd_tensors(kind, with_bn)
    worst = {k: 0.0 for k in names}
    keep = packed_keep(lens, T, H, p_drop) if p_drop else None
    for salt in range(1, POOL_SEEDS + 1):
        c = seeded_scan_case(kind, B, T, H, salt)
        f = sn.forward(kind, F32, c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], B=B, dirs=1,
                       theta=c["theta"])
        ref, runs = ragged_backward_runs(c, lens, f["u_save"], f["w_save"], keep, with_bn, surrogate)
        for k in names:
            top = float(np.abs(ref[k]).max())
            worst[k] = max(worst[k], max(float(np.abs(r[k].astype(F64) - ref[k]).max()) for r in runs) / top)
    return worst


# ------------------------------------------------------------------------------------------------ whole networks
SIZES, NB, NT, NC = [64, 64, 20], 6, 23, 40
NET_LENGTHS = [23, 1, 9, 17, 2, 22]           # unsorted: the sort and the un-sort are on the path


def make_net(sp, kind, normalization, dropout=0.0, seed=3, use_bias=False, use_readout_layer=True):
    """tests/test_ragged_gpu.py's dyadic network (weights on a 2^-6 grid, a live affine on a 2^-4 grid)."""
    torch.manual_seed(seed)
    net = sp.SNN((NB, None, NC), SIZES, neuron_type=kind, dropout=dropout, normalization=normalization, use_bias=use_bias,
                 use_readout_layer=use_readout_layer)
    with torch.no_grad():
        for lay in net.snn:
            lay.W.weight.copy_(torch.round((lay.W.weight * 4 + 0.25) * 64) / 64)   # (a positive drive: every layer spikes)
            if use_bias:
                lay.W.bias.copy_(torch.round(lay.W.bias * 16) / 16)
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
            if normalization in ("batchnorm", "layernorm"):   # (a live affine: the normalised drive reaches the threshold)
                lay.norm.weight.copy_(torch.round((torch.rand_like(lay.norm.weight) + 1.0) * 16) / 16)
                lay.norm.bias.copy_(torch.round((torch.rand_like(lay.norm.bias) * 0.5 + 0.25) * 16) / 16)
    return net


def net_inputs(orc, kind, seed=11, lengths=NET_LENGTHS, zero_padding=True):
    """0/1 inputs (zero on the padding unless zero_padding=False: the packed path never reads it), labels, and initial
    states on a 2^-4 grid."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(NB, NT, NC, generator=g) < 0.3).float()
    if zero_padding:
        x = x * torch.from_numpy(pn.valid_mask(lengths, NT))[:, :, None]
    y = torch.randint(0, SIZES[-1], (NB,), generator=g)
    torch.manual_seed(seed + 1)
    init = orc.draw_init_states(NB, SIZES, kind)
    init = [{k: torch.floor(v * 16) / 16 for k, v in st.items()} for st in init]
    return x, y, init


class injected_states:
    """The initial states of `init` (row range `rows`) handed to the network's draws, in the reference's order."""

    def __init__(self, init, rows=slice(None)):
        self.order = [st[k][rows] for st in init for k in ("u0", "w0", "s0") if k in st]

    def __enter__(self):
        from sparch_amd import snns as snn_mod
        it = iter(self.order)
        self.mod, self.old = snn_mod, snn_mod._rand_to
        snn_mod._rand_to = lambda rows, cols, device: next(it).to(device)

    def __exit__(self, *exc):
        self.mod._rand_to = self.old


def packed_drop_masks(lengths, p_drop, seeds, widths, T=NT, run_widths=None):
    """The hidden layers' dropout multipliers of a packed forward as padded (B,T,H) tensors in the caller's row order:
    the mask of tests/dropout_numpy.py on the packed element index, zero on the padding.  run_widths: the widths the
    layers run at where they differ (a recurrent width that is not a multiple of 4 runs zero-padded to the next one, and
    the mask's index is that tensor's: tests/dropout_numpy.py keep_mask_padded)."""
    masks = []
    for seed, H, Hp in zip(seeds, widths, run_widths or widths):
        flat = keep_mask(seed, (int(np.sum(lengths)), Hp), p_drop)[:, :H]
        masks.append(torch.from_numpy(pn.unpack(np.ascontiguousarray(flat), lengths, T)))
    return masks

"""
Cases of the axonal-delay tests: the kernels' shapes and parameters (tests/test_delay_gpu.py), and the small dyadic
networks of the whole-network checks with their CPU restatement (tests/spiking_numpy.py for the cells,
tests/delay_numpy.py for the shift), which picks the data seed before anything runs on a GPU: every hidden layer's
firing rate has to lie in RATE_WINDOW (tests/test_delay_host.py holds the committed seeds to it).
"""
import numpy as np
import torch

from tests import delay_numpy as dn
from tests import spiking_numpy as sn
from tests.kit import F64

# ------------------------------------------------------------------------------------------------ kernels
B, T = 3, 9
WIDTHS = (5, 8, 36)             # odd; one 16-byte group of bf16 (two of fp32); several groups (scalar in bf16: 72-byte rows)
CAPS = (1, 4, 11)               # 11 > T: whole columns come out zero
LENGTHS = [9, 1, 4]
DENSITY = 0.3
HIDDEN_DENSITY = 0.125          # what the first hidden layer fires at under PLAIN_DRIVE: the next layers' expected input


def thetas(K, D, seed):
    """(K,) fp32 delays: 0, the ties 2.5 -> 2 and 3.5 -> 4, negatives, values above D, a value on D, and random ones —
    every column class in the first five columns, so that K = 5 has them all."""
    rng = np.random.default_rng([seed, K, D])
    fixed = np.array([0.0, 2.5, 3.5, -0.75, D + 0.5, float(D), -3.0, D + 40.0, 0.5, 1.5], np.float32)
    th = rng.uniform(-0.5, D + 0.5, K).astype(np.float32)
    n = min(K, len(fixed))
    th[:n] = fixed[:n]
    return th


def kernel_data(K, D):
    """Bernoulli(DENSITY) 0/1 input, a real-valued cotangent, the delays: the first data seed at which every column
    with d < T - 1 has a spike edge under its window, so that the delay's gradient sums something there (the tests
    assert it)."""
    th = thetas(K, D, 0)
    d = dn.steps(th, D)
    for seed in range(256):
        rng = np.random.default_rng([seed, K, D, 1])
        x = (rng.random((B, T, K)) < DENSITY).astype(np.float32)
        g = rng.standard_normal((B, T, K)).astype(np.float32)
        if (dn.backward_theta(g, x, th, D)[1][d < T - 1] > 0).all():
            return x, g, th
    raise AssertionError((K, D))


# more than one tile of the staged gather (64 steps x 8 pieces of 16 bytes) in both directions, T > 64 + D so that a
# tile reaches back over a whole earlier one; 136 columns: 34 pieces in fp32 (5 column tiles, the last with 2 pieces), 17
# in bf16 (3 tiles, the last with 1); B T = 450 rows: 15 slabs of the delay gradient's partial sums
BIG_T, BIG_K, BIG_D = 150, 136, 25
BIG_LENGTHS = [150, 70, 3]      # a whole row, one that ends inside the second tile, one shorter than most delays


def big_kernel_data():
    """kernel_data's recipe at (B, BIG_T, BIG_K) with delays over the whole range [0, BIG_D] and outside it."""
    rng = np.random.default_rng([7, BIG_K, BIG_D])
    x = (rng.random((B, BIG_T, BIG_K)) < DENSITY).astype(np.float32)
    g = rng.standard_normal((B, BIG_T, BIG_K)).astype(np.float32)
    th = thetas(BIG_K, BIG_D, 7)
    th[10:] = (np.arange(BIG_K - 10) % (BIG_D + 1) + rng.uniform(-0.4, 0.4, BIG_K - 10)).astype(np.float32)  # every d
    return x, g, th


# ------------------------------------------------------------------------------------------------ networks
KINDS = ("LIF", "adLIF", "RLIF", "RadLIF")
NB, NT, NC, ND = 3, 12, 8, 3
SIZES = [12, 12, 5]
ODD_SIZES = [10, 10, 5]         # a recurrent width that is not a multiple of 4
NET_LENGTHS = [12, 1, 5]
RATE_WINDOW = (0.02, 0.6)
PICK_WINDOW = (0.03, 0.5)       # what the seed is picked with: a margin for the spikes an fp32 run decides the other way
PLAIN_DRIVE = 2.5               # the mean drive without a normalisation (tests/network_cases.py: 3.5 at T = 7, 1.5 at T = 19)
# (kind, sizes, bidirectional) -> the data seed, the first of 0, 1, ... whose CPU restatement puts every hidden layer's
# firing rate inside RATE_WINDOW, with and without delays (picked by pick_seed(), re-derived by the host test)
SEEDS = {
    ("LIF", (12, 12, 5), False): 0, ("LIF", (12, 12, 5), True): 0, ("LIF", (10, 10, 5), False): 0,
    ("adLIF", (12, 12, 5), False): 0, ("adLIF", (12, 12, 5), True): 0, ("adLIF", (10, 10, 5), False): 1,
    ("RLIF", (12, 12, 5), False): 0, ("RLIF", (12, 12, 5), True): 0, ("RLIF", (10, 10, 5), False): 0,
    ("RadLIF", (12, 12, 5), False): 1, ("RadLIF", (12, 12, 5), True): 1, ("RadLIF", (10, 10, 5), False): 12,
}


def seed_of(kind, sizes=SIZES, bidirectional=False):
    return SEEDS[(kind, tuple(sizes), bool(bidirectional))]


def make_net(sp, kind, sizes=SIZES, bidirectional=False, seed=3, **kw):
    """The dyadic network of tests/network_cases.py / tests/packed_cases.py at this file's sizes, without a
    normalisation: nn.Linear's initialisation times 4 plus the offset that carries the mean drive, on the 2^-6 grid, V
    on that grid."""
    torch.manual_seed(seed)
    net = sp.SNN((NB, None, NC), list(sizes), neuron_type=kind, normalization="none", bidirectional=bidirectional, **kw)
    density = DENSITY
    with torch.no_grad():
        for lay in net.snn:     # the offset carries the mean drive: PLAIN_DRIVE over the expected number of active inputs
            offset = PLAIN_DRIVE / (density * lay.input_size)
            lay.W.weight.copy_(torch.round((lay.W.weight * 4 + offset) * 64) / 64)
            density = HIDDEN_DENSITY
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
    return net


def net_delays(net, seed=5):
    """Delays for every delayed layer of net: 0, the two ties, a negative, one above the cap, then random ones."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i, lay in enumerate(net.snn):
        if getattr(lay, "max_delay", 0):
            th = torch.rand(lay.input_size, generator=g) * (lay.max_delay + 1.0) - 0.5
            head = torch.tensor([0.0, 2.5, 3.5, -0.75, lay.max_delay + 0.5])[:lay.input_size]
            th[:len(head)] = head
            out[i] = th
    return out


def set_delays(net, delays):
    with torch.no_grad():
        for i, th in delays.items():
            net.snn[i].delay.copy_(th)


def net_inputs(kind, sizes=SIZES, bidirectional=False, seed=0):
    """0/1 input (NB, NT, NC), labels, initial states on a 2^-4 grid (one dict per layer, the readout's last)."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = (torch.rand(NB, NT, NC, generator=g) < DENSITY).float()
    y = torch.randint(0, sizes[-1], (NB,), generator=g)
    rows = NB * (2 if bidirectional else 1)
    init = []
    for k, H in enumerate(sizes):
        hidden = k < len(sizes) - 1
        names = (("u0", "w0", "s0") if sn.ADAPTIVE[kind] else ("u0", "s0")) if hidden else ("u0",)
        init.append({n: torch.floor(torch.rand(rows if hidden else NB, H, generator=g) * 16) / 16 for n in names})
    return x, y, init


def cpu_rates(net, kind, x, init, delays=None, bidirectional=False):
    """Every hidden layer's firing rate (one number per layer) in the fp64 restatement: the layer's input shifted by
    its delays (tests/delay_numpy.py), the projection, the cell (tests/spiking_numpy.py)."""
    a = x.numpy().astype(F64)
    dirs = 2 if bidirectional else 1
    rates = []
    for k, lay in enumerate(list(net.snn)[:-1]):
        if delays is not None and k in delays:
            a = dn.forward(a, delays[k].numpy(), lay.max_delay)
        p = {n: getattr(lay, n).detach().numpy() for n in ("alpha", "beta", "a", "b") if hasattr(lay, n)}
        if hasattr(lay, "V"):
            p["V"] = lay.V.weight.detach().numpy().T.copy()     # (k, n): s @ V^T of nn.Linear
        Wx = a @ lay.W.weight.detach().numpy().astype(F64).T
        st = init[k]
        f = sn.forward(kind, F64, Wx, None, None, p, st["u0"].numpy(), st["w0"].numpy() if "w0" in st else None,
                       st["s0"].numpy(), B=a.shape[0], dirs=dirs)
        a = f["s_out"]
        rates.append(float(a.mean()))
    return rates


def cpu_rates_ragged(net, kind, x, init, delays, lengths):
    """cpu_rates with lengths: every clip run alone on its own steps (what the masked and the packed mode compute),
    the spikes counted over the valid steps."""
    total = np.zeros(len(net.snn) - 1)
    for b, m in enumerate(lengths):
        rows = [{k: v[b:b + 1] for k, v in st.items()} for st in init]
        total += np.asarray(cpu_rates(net, kind, x[b:b + 1, :m], rows, delays)) * m
    return [float(v) for v in total / sum(lengths)]


def in_window(rates, window=RATE_WINDOW):
    return all(window[0] <= r <= window[1] for r in rates)


def pick_seed(sp, kind, sizes=SIZES, bidirectional=False, limit=64):
    """The first data seed whose restated firing rates lie in the window with zero delays and with net_delays()."""
    for seed in range(limit):
        net = make_net(sp, kind, sizes, bidirectional, max_delay=ND)
        x, _, init = net_inputs(kind, sizes, bidirectional, seed)
        if in_window(cpu_rates(net, kind, x, init, None, bidirectional), PICK_WINDOW) and \
                in_window(cpu_rates(net, kind, x, init, net_delays(net), bidirectional), PICK_WINDOW):
            return seed
    raise AssertionError(f"no seed below {limit} puts {kind} {sizes} inside the firing-rate window")


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

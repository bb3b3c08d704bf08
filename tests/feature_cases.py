"""
Whole spiking networks drawn at random over the feature matrix of the layer host code — layout (dense, `lengths`,
`pack=True`), axonal delays, synaptic currents, the readout's mode / the per-step readout — on top of the axes of
tests/network_cases.py, for tests/test_feature_fuzz_host.py and tests/test_feature_fuzz_gpu.py.  The oracle is
tests/feature_oracle.py, run in fp64; nothing of the package enters a reference, the keep rule or a bound.

draw(i)          the configuration of index i, a pure function of i.  0 <= i < FILL_BASE: every axis drawn at random,
                 redrawn (from the same stream) until no entry of REFUSED matches.  i >= FILL_BASE: the fill pass — pair
                 (i - FILL_BASE) // FILL_TRIES of required_pairs() forced, the rest drawn as before; FILL_TRIES data /
                 configuration attempts per pair.  WIDE, DX_PLANES: the two fixed cases.
case(i)          draw(i) plus every tensor of the case, from seeds on the CPU (parameters under the package's state_dict
                 keys, `snn.{k}.delay` and `snn.{k}.gamma` among them; some delays outside [0, D] and some gamma outside
                 [lo, hi], as tests/delay_cases.py thetas and tests/synapse_cases.py gammas draw them).
build, device_run, oracle_run, verdict, bounds, KEPT     as in tests/network_cases.py, whose MARGIN, RATE_WINDOW, relative
                 caps and project bars are imported unchanged.  KEPT is a literal: the kept ones of the random indices
                 0 .. N_RANDOM - 1, then for every required pair those leave uncovered the first kept attempt of the
                 fill pass (derive_kept() recomputes it; the host test re-derives it with the slack band).
REFUSED          the combinations of axis values SNN.forward refuses, with words of the ValueError: collected from
                 snns._check_synapse_call, _check_packed_layer, _check_ragged_layer, SNN.forward's per_step checks and
                 DESIGN.md section 7.  Pairs, and the triples whose every pair is legal.  (per_step with another
                 readout mode and per_step without a readout layer are refused too: the output axis holds one of them
                 at a time, so no case can ask for either; the host test checks both refusals beside the table.)

Coverage: every pair of values of two different new axes (layout, delay, synapse, output) and every pair of a new-axis
value with a value of kind, norm, dirs, dropout, surrogate is in REFUSED or occurs in a kept case
(tests/test_feature_fuzz_host.py asserts it).

Dropout on the doubled ragged batch (two directions with lengths or pack; two directions with a synapse, which takes
that route in the dense layout too) has no host restatement of its mask index in tests/: draw() gives those cases
dropout = 0.  The dense layout and the masked one-direction layout take tests/dropout_numpy.keep_mask_padded, the packed
one-direction layout tests/packed_cases.packed_drop_masks.

The drive is tuned toward the firing-rate window (tests/network_cases.py says why): AFFINE_GAIN and PLAIN_DRIVE per
sequence length, times SYN_BOOST for a layer with a synapse (the filter starts from zero and low-passes the drive) and
DELAY_BOOST for a layer with delays (a delay removes input steps from short clips).

Kept share: 87 of the 96 random indices (0.91), which leave five required pairs uncovered; the first attempt of each
of the five fill pairs is kept: 92 of 101 indices tried (0.91).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc
from tests import dropout_numpy as dn
from tests import feature_oracle as fo
from tests import packed_cases as pc
from tests import packed_numpy as pn
from tests import ragged_oracle as rag
from tests import surrogate_numpy as sg
from tests.kit import DEV, SEED
from tests.network_cases import (GRAD_CAP, GRAD_RTOL, LOSS_CAP, LOSS_RTOL, MARGIN, OUT_CAP, OUT_RTOL,  # noqa: F401
                                 RATE_WINDOW, _grid, _Step, injected_states, maxabs, residue)

KINDS = ("LIF", "adLIF", "RLIF", "RadLIF")
BATCHES, STEPS, CHANNELS = (2, 3, 5), (5, 9, 12), (5, 8, 36)
WIDTHS, CLASSES = (5, 10, 12, 36, 66), (3, 5, 20, 35)
NORMS = ("batchnorm", "layernorm", "none")
INPUTS = ("binary", "counts", "real")
SURROGATES = ("boxcar", "triangle", "fast_sigmoid", "atan")
LAYOUTS = ("dense", "lengths", "pack")
DELAYS = ("off", "fixed", "all", "hidden")          # fixed: learn_delays=False; all / hidden: learnable, delay_layers=
SYNAPSES = ("off", "fixed", "all", "hidden")        # fixed: learn_synapse=False; all / hidden: learnable, synapse_layers=
OUTPUTS = ("none", "softmax_sum", "softmax_mean", "u_max", "u_mean", "u_last", "prob", "sum")
MAX_DELAYS = (1, 3)
SYN_LIMITS = (0.0, 0.9)
SYN_LIMITS_F32 = tuple(float(np.float32(v)) for v in SYN_LIMITS)     # as the kernels take them (tests/synapse_numpy.py clamped)
P_DROP = 0.25
REG_F = 0.21
DRAW_SEED = 5
N_RANDOM = 96
FILL_BASE, FILL_TRIES = 1000, 4
WIDE, DX_PLANES = -1, -2
FIXED_SEEDS = {WIDE: 0, DX_PLANES: 29}    # the first data seed at which the margin is 32 x the fp32 error (4 x the rule's)
ROLES = ("W.weight", "W.bias", "V.weight", "alpha", "beta", "a", "b", "norm.weight", "norm.bias", "delay", "gamma",
         "out", "seq", "loss")

NEW_AXES = {"layout": LAYOUTS, "delay": DELAYS, "synapse": SYNAPSES, "output": OUTPUTS}
OLD_AXES = {"kind": KINDS, "norm": NORMS, "dirs": (1, 2), "dropout": (0.0, P_DROP), "surrogate": SURROGATES}

# What SNN.forward refuses, as combinations of axis values, with words its ValueError contains.
REFUSED = {
    ("layout=pack", "output=prob"): "per_step with pack=True is not supported",
    ("layout=pack", "output=sum"): "per_step with pack=True is not supported",
    ("layout=lengths", "norm=batchnorm", "bias=True"): "lengths with BatchNorm and use_bias=True is not supported",
    ("layout=pack", "dirs=2", "synapse=fixed"): "pack=True with bidirectional=True and a synapse is not supported",
    ("layout=pack", "dirs=2", "synapse=all"): "pack=True with bidirectional=True and a synapse is not supported",
    ("layout=pack", "dirs=2", "synapse=hidden"): "pack=True with bidirectional=True and a synapse is not supported",
}

# the affine gain of the normalised drive and the mean drive without a normalisation, per sequence length
AFFINE_GAIN = {5: 4.0, 8: 2.0, 9: 2.0, 12: 1.75}
PLAIN_DRIVE = {5: 5.0, 8: 2.5, 9: 2.5, 12: 2.0}
SYN_BOOST = {5: 2.0, 8: 1.5, 9: 1.5, 12: 1.35}
DELAY_BOOST = {1: 1.1, 3: 1.3}
DENSITY = 0.3

# The kept indices (tests/test_feature_fuzz_host.py re-derives the list): random draws, then the fill pass.
KEPT = (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
        32, 33, 35, 36, 37, 38, 39, 40, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 53, 54, 56, 57, 58, 59, 60, 61, 62, 63,
        64, 65, 66, 67, 68, 69, 70, 71, 72, 74, 75, 76, 77, 78, 79, 81, 82, 83, 84, 85, 87, 88, 89, 90, 91, 92, 93, 94,
        95, 1160, 1208, 1504, 2176, 2232)


# ------------------------------------------------------------------------------------------------ axes and refusals
def axis_values(cfg):
    """{axis: "axis=value"} of a configuration: the coverage axes and bias (which takes part in one refusal)."""
    return {"kind": f"kind={cfg['kind']}", "norm": f"norm={cfg['normalization']}",
            "dirs": f"dirs={2 if cfg['bidirectional'] else 1}", "dropout": f"dropout={cfg['dropout']}",
            "surrogate": f"surrogate={cfg['surrogate'][0] if cfg['surrogate'] else 'boxcar'}",
            "layout": f"layout={cfg['layout']}", "delay": f"delay={cfg['delay']}", "synapse": f"synapse={cfg['synapse']}",
            "output": f"output={cfg['output']}", "bias": f"bias={cfg['use_bias']}"}


def refusal(values):
    """The words of the refusal a set of axis values meets, or None."""
    values = set(values)
    for combo, words in REFUSED.items():
        if set(combo) <= values:
            return words
    return None


@functools.lru_cache(maxsize=None)
def required_pairs():
    """Every pair the coverage condition names, in a fixed order: two values of two different new axes, or a new-axis
    value with a value of an old axis."""
    new = [(a, f"{a}={v}") for a, vs in NEW_AXES.items() for v in vs]
    old = [(a, f"{a}={v}") for a, vs in OLD_AXES.items() for v in vs]
    pairs = [(u, v) for k, (a, u) in enumerate(new) for (b, v) in new[k + 1:] if a != b]
    pairs += [(u, v) for (_, u) in new for (_, v) in old]
    return tuple(pairs)


def pairs_of(cfg):
    v = axis_values(cfg)
    return {p for p in required_pairs() if p[0] in v.values() and p[1] in v.values()}


def coverage(indices):
    """(pairs covered by the cases, pairs refused, pairs missing)."""
    covered = set()
    for i in indices:
        covered |= pairs_of(draw(i))
    refused = {p for p in required_pairs() if refusal(p)}
    return covered, refused, [p for p in required_pairs() if p not in covered and p not in refused]


# ------------------------------------------------------------------------------------------------ configurations
def _finish(cfg):
    """The derived entries of a configuration."""
    out = cfg["output"]
    cfg["use_readout_layer"] = out != "none"
    cfg["per_step"] = out if out in ("prob", "sum") else None
    cfg["readout"] = out if out in ("softmax_mean", "u_max", "u_mean", "u_last") else "softmax_sum"
    cfg["learn_delays"], cfg["learn_synapse"] = cfg["delay"] in ("all", "hidden"), cfg["synapse"] in ("all", "hidden")
    if cfg["delay"] == "off":
        cfg["max_delay"] = 0
    return cfg


def draw(i):
    """The configuration of index i."""
    if i == WIDE:       # 66 pieces of four columns per sequence (tests/synapse_cases.py WIDE_H), three sequences
        return _finish(dict(index=WIDE, kind="adLIF", B=3, T=9, C=8, sizes=[264, 5], normalization="batchnorm",
                            bidirectional=False, use_bias=False, training=True, threshold=1.0, input="binary",
                            real_weights=False, dropout=0.0, regulariser=True, surrogate=None, layout="lengths",
                            lengths=[9, 1, 4], delay="off", max_delay=0, delay_layers="all", synapse="all",
                            synapse_layers="all", output="softmax_sum"))
    if i == DX_PLANES:  # functional._use_dx_planes sees a spike-fed layer with K = 2 x 128, H = 256, B T = 256
        lengths = [8, 1] + [int(v) for v in np.random.default_rng(DRAW_SEED).integers(1, 9, 30)]
        return _finish(dict(index=DX_PLANES, kind="RLIF", B=32, T=8, C=36, sizes=[128, 256, 20],
                            normalization="batchnorm", bidirectional=True, use_bias=False, training=True, threshold=1.0,
                            input="binary", real_weights=False, dropout=0.0, regulariser=True, surrogate=None,
                            layout="lengths", lengths=lengths, delay="all", max_delay=3, delay_layers="all",
                            synapse="off", synapse_layers="all", output="softmax_sum"))
    forced = {}
    if i >= FILL_BASE:
        forced = dict(v.split("=") for v in required_pairs()[(i - FILL_BASE) // FILL_TRIES])
    rng = np.random.default_rng([DRAW_SEED, i])

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    while True:
        a = {axis: str(pick(vs)) for axis, vs in list(OLD_AXES.items()) + list(NEW_AXES.items())}
        a.update(forced)
        B, T, C = pick(BATCHES), pick(STEPS), pick(CHANNELS)
        n_hidden = pick((1, 2))
        widths, classes = [pick(WIDTHS) for _ in range(2)], pick(CLASSES)
        bias, training, theta = bool(rng.integers(2)), bool(rng.integers(4)), pick((1.0, 0.75))
        inp, real_w, reg = pick(INPUTS), not rng.integers(4), bool(rng.integers(2))
        D, fixed_delay_layers, fixed_syn_layers = pick(MAX_DELAYS), pick(("all", "hidden")), pick(("all", "hidden"))
        tail = [int(v) for v in rng.integers(1, T + 1, B)]
        order = rng.permutation(B)
        bidir, drop = a["dirs"] == "2", float(a["dropout"])
        delay_layers = fixed_delay_layers if a["delay"] == "fixed" else a["delay"] if a["delay"] != "off" else "all"
        syn_layers = fixed_syn_layers if a["synapse"] == "fixed" else a["synapse"] if a["synapse"] != "off" else "all"
        if "hidden" in (delay_layers if a["delay"] != "off" else "", syn_layers if a["synapse"] != "off" else ""):
            n_hidden = 2            # (a "hidden" scope leaves the first layer out: the second has the feature)
        if drop > 0 and "dropout" in forced:
            training = True
        if drop > 0 and bidir and (a["layout"] != "dense" or a["synapse"] != "off"):    # (module docstring)
            if "dropout" in forced:
                bidir = False
            else:
                drop = 0.0
        if not training:
            drop = 0.0
        lengths = None
        if a["layout"] != "dense":
            lens = ([1, T] + tail)[:B]
            lengths = [lens[j] for j in order]
        name = a["surrogate"]
        cfg = _finish(dict(
            index=i, kind=a["kind"], B=B, T=T, C=C, sizes=widths[:n_hidden] + ([classes] if a["output"] != "none" else []),
            normalization=a["norm"], bidirectional=bidir, use_bias=bias, training=training, threshold=theta, input=inp,
            real_weights=bool(real_w), dropout=drop, regulariser=reg,
            surrogate=None if name == "boxcar" else (name, sg.TEST_SCALE[name]), layout=a["layout"], lengths=lengths,
            delay=a["delay"], max_delay=D, delay_layers=delay_layers, synapse=a["synapse"], synapse_layers=syn_layers,
            output=a["output"]))
        if refusal(axis_values(cfg).values()) is None:
            assert all(axis_values(cfg)[k] == f"{k}={v}" for k, v in forced.items()), (i, forced, cfg)
            return cfg


def label(cfg):
    """The configuration as a test id."""
    n = {"batchnorm": "bn", "layernorm": "ln", "none": "none"}[cfg["normalization"]]
    head = {WIDE: "wide", DX_PLANES: "dxplanes"}.get(cfg["index"], str(cfg["index"]))
    parts = [head, cfg["kind"], n, f"B{cfg['B']}T{cfg['T']}C{cfg['C']}", "x".join(map(str, cfg["sizes"])),
             "2dir" if cfg["bidirectional"] else "1dir", "train" if cfg["training"] else "eval", cfg["layout"],
             cfg["output"]]
    if cfg["delay"] != "off":
        parts.append(f"delay_{cfg['delay']}{cfg['max_delay']}")
    if cfg["synapse"] != "off":
        parts.append(f"syn_{cfg['synapse']}")
    parts += [k for k, on in (("bias", cfg["use_bias"]), ("th75", cfg["threshold"] != 1.0), ("realw", cfg["real_weights"]),
                              ("drop", cfg["dropout"] > 0), ("reg", cfg["regulariser"]), (cfg["input"], True)) if on]
    if cfg["surrogate"]:
        parts.append(cfg["surrogate"][0])
    return "-".join(parts)


def n_hidden(cfg):
    return len(cfg["sizes"]) - 1 if cfg["use_readout_layer"] else len(cfg["sizes"])


def has_delay(cfg, k):
    return cfg["delay"] != "off" and not (k == 0 and cfg["delay_layers"] == "hidden")


def has_synapse(cfg, k):
    return cfg["synapse"] != "off" and k < n_hidden(cfg) and not (k == 0 and cfg["synapse_layers"] == "hidden")


def dropout_seeds(cfg):
    return [SEED + 7919 * k for k in range(n_hidden(cfg))]


# ------------------------------------------------------------------------------------------------ tensors
def _parameters(cfg, g):
    """tests/network_cases.py _parameters at this file's drive tables, plus `delay` (0, the ties 2.5 and 3.5, a negative,
    one above the cap, then random ones over a little more than [0, D]) and `gamma` (a negative, one above hi, hi, 0, then
    random ones in (0.1, 0.7)) for the layers that have them."""
    kind, norm, T, dirs = cfg["kind"], cfg["normalization"], cfg["T"], 2 if cfg["bidirectional"] else 1
    p, fan, density = {}, cfg["C"], DENSITY * {"binary": 1.0, "counts": 2.0, "real": 1.0}[cfg["input"]]
    for k, H in enumerate(cfg["sizes"]):
        pre, hidden = f"snn.{k}.", k < n_hidden(cfg)
        boost = (SYN_BOOST[T] if has_synapse(cfg, k) else 1.0) * (DELAY_BOOST[cfg["max_delay"]] if has_delay(cfg, k) else 1.0)
        W = (torch.rand(H, fan, generator=g) * 2 - 1) / math.sqrt(fan) * 4
        W = W + (PLAIN_DRIVE[T] * boost / (density * fan) if norm == "none" and hidden else 0.25)
        p[pre + "W.weight"] = W if cfg["real_weights"] else _grid(W, 64)
        if cfg["use_bias"]:
            b = (torch.rand(H, generator=g) * 2 - 1) / math.sqrt(fan)
            p[pre + "W.bias"] = b if cfg["real_weights"] else _grid(b, 64)
        if hidden and orc.RECURRENT[kind]:
            V = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g)
            p[pre + "V.weight"] = V if cfg["real_weights"] else _grid(V, 64)
        lo, hi = orc.ALPHA_LIM
        p[pre + "alpha"] = torch.rand(H, generator=g) * (hi - lo + 0.02) + lo - 0.01
        if hidden and orc.ADAPTIVE[kind]:
            lo, hi = orc.BETA_LIM
            p[pre + "beta"] = torch.rand(H, generator=g) * (hi - lo + 0.004) + lo - 0.002
            p[pre + "a"] = torch.rand(H, generator=g) * 2.1 - 1.05
            p[pre + "b"] = torch.rand(H, generator=g) * 2.1 - 0.05
        if norm in ("batchnorm", "layernorm"):
            gain = AFFINE_GAIN[T] * boost if hidden else 1.0
            p[pre + "norm.weight"] = _grid((torch.rand(H, generator=g) + 1.0) * gain, 16)
            p[pre + "norm.bias"] = _grid((torch.rand(H, generator=g) * 0.5 + 0.25) * gain, 16)
        if norm == "batchnorm":
            p[pre + "norm.running_mean"] = torch.rand(H, generator=g) - 0.5
            p[pre + "norm.running_var"] = torch.rand(H, generator=g) * 0.75 + 0.25
            p[pre + "norm.num_batches_tracked"] = torch.tensor(3 + k)
        if has_delay(cfg, k):
            D = cfg["max_delay"]
            th = torch.rand(fan, generator=g) * (D + 1.0) - 0.5
            head = torch.tensor([0.0, 2.5, 3.5, -0.75, D + 0.5])[:fan]
            th[:len(head)] = head
            p[pre + "delay"] = th
        if has_synapse(cfg, k):
            gm = torch.rand(H, generator=g) * 0.6 + 0.1
            head = torch.tensor([SYN_LIMITS[0] - 0.125, SYN_LIMITS[1] + 0.0625, SYN_LIMITS[1], SYN_LIMITS[0]])[:H]
            gm[:len(head)] = head
            p[pre + "gamma"] = gm
        fan, density = H * dirs, 0.25
    if not cfg["real_weights"]:     # what the bf16 operand mode relies on
        assert all(torch.equal(v, v.bfloat16().float()) for k, v in p.items() if k.endswith(("W.weight", "V.weight")))
    return p


def _eval_statistics(cfg, c, g):
    """tests/network_cases.py _eval_statistics on this file's oracle run: the running statistics an eval-mode case
    normalises with lie near the batch's own."""
    start = dict(c["params"])
    for k in start:
        if k.endswith("running_mean"):
            start[k] = torch.zeros_like(start[k])
        if k.endswith("running_var"):
            start[k] = torch.ones_like(start[k])
    stats = oracle_run(dict(c, params=start, cfg=dict(cfg, training=True, dropout=0.0), masks=None), torch.float64,
                       backward=False)["stats"]
    for k in sorted(stats):
        v = stats[k].float()
        if k.endswith("running_mean"):
            mean = v / orc.BN_MOMENTUM
            var = (stats[k[:-4] + "var"].float() - (1 - orc.BN_MOMENTUM)) / orc.BN_MOMENTUM
            c["params"][k] = mean + (torch.rand(v.shape, generator=g) * 0.4 - 0.2) * var.sqrt()
            c["params"][k[:-4] + "var"] = var * (torch.rand(v.shape, generator=g) * 0.45 + 0.8)


def drop_masks(cfg):
    """The hidden layers' dropout multipliers (B, T, H * dirs), made on the host (module docstring)."""
    if cfg["dropout"] <= 0:
        return None
    B, T, dirs, nh = cfg["B"], cfg["T"], 2 if cfg["bidirectional"] else 1, n_hidden(cfg)
    rec = orc.RECURRENT[cfg["kind"]]
    run = [(H + 3) // 4 * 4 if rec else H for H in cfg["sizes"][:nh]]   # (a recurrent cell runs at its width padded to 4)
    assert dirs == 1 or (cfg["layout"] == "dense" and cfg["synapse"] == "off")
    if cfg["layout"] == "pack":
        return pc.packed_drop_masks(cfg["lengths"], cfg["dropout"], dropout_seeds(cfg), cfg["sizes"][:nh], T, run)
    return [torch.from_numpy(dn.keep_mask_padded(s, B, T, dirs, H, Hp, cfg["dropout"]))
            for s, H, Hp in zip(dropout_seeds(cfg), cfg["sizes"][:nh], run)]


@functools.lru_cache(maxsize=None)
def case(i):
    """draw(i) and the tensors of the case (CPU, fp32; the counts input as uint8 too)."""
    return case_of(draw(i), 7100 + (i if i >= 0 else 99991 - i + 1000 * FIXED_SEEDS[i]))


def case_of(cfg, seed):
    """The tensors of a configuration at a data seed (the host test makes configurations of its own)."""
    B, T, C, dirs = cfg["B"], cfg["T"], cfg["C"], 2 if cfg["bidirectional"] else 1
    g = torch.Generator().manual_seed(seed)
    c = dict(cfg=cfg, params=_parameters(cfg, g))
    on = torch.rand(B, T, C, generator=g) < DENSITY
    if cfg["input"] == "binary":
        x = on.float()
    elif cfg["input"] == "counts":
        x = on.float() * torch.randint(1, 4, (B, T, C), generator=g).float()
    else:
        x = on.float() * torch.rand(B, T, C, generator=g) * 2
    if cfg["lengths"] is not None:
        x = x * rag.valid_mask(cfg["lengths"], T)[:, :, None]
    c["x"] = x
    c["counts"] = x.to(torch.uint8) if cfg["input"] == "counts" else None
    nh, last = n_hidden(cfg), cfg["sizes"][-1]
    c["y"], c["gout"], c["gseq"] = None, None, None
    if cfg["use_readout_layer"]:
        c["y"], c["gout"] = torch.randint(0, last, (B,), generator=g), torch.randn(B, last, generator=g)
        if cfg["per_step"]:
            c["gseq"] = torch.randn(B, T, last, generator=g) / T
    init = []
    for k, H in enumerate(cfg["sizes"]):
        names = (("u0", "w0", "s0") if orc.ADAPTIVE[cfg["kind"]] else ("u0", "s0")) if k < nh else ("u0",)
        rows = B * dirs if k < nh else B
        init.append({n: torch.floor(torch.rand(rows, H, generator=g) * 16) / 16 for n in names})
    c["init"] = init
    c["masks"] = drop_masks(cfg)
    if cfg["normalization"] == "batchnorm" and not cfg["training"]:
        _eval_statistics(cfg, c, g)
    return c


# ------------------------------------------------------------------------------------------------ the two sides
def net_kwargs(cfg):
    """What SNN's constructor takes from a configuration."""
    name, scale = cfg["surrogate"] or ("boxcar", None)
    kw = dict(neuron_type=cfg["kind"], threshold=cfg["threshold"], dropout=cfg["dropout"],
              normalization=cfg["normalization"], use_bias=cfg["use_bias"], bidirectional=cfg["bidirectional"],
              use_readout_layer=cfg["use_readout_layer"], surrogate=name, surrogate_scale=scale, readout=cfg["readout"])
    if cfg["delay"] != "off":
        kw.update(max_delay=cfg["max_delay"], delay_init="uniform", learn_delays=cfg["learn_delays"],
                  delay_layers=cfg["delay_layers"])
    if cfg["synapse"] != "off":
        kw.update(synapse=SYN_LIMITS, learn_synapse=cfg["learn_synapse"], synapse_layers=cfg["synapse_layers"])
    return kw


def forward_kwargs(cfg):
    """What SNN.forward takes from a configuration, beside x."""
    kw = {}
    if cfg["layout"] != "dense":
        kw["lengths"] = torch.tensor(cfg["lengths"])
    if cfg["layout"] == "pack":
        kw["pack"] = True
    if cfg["per_step"]:
        kw["per_step"] = cfg["per_step"]
    return kw


def build(sp, cfg):
    """(the package's SNN on the CPU with the case's parameters loaded and its dropout seeds pinned, the parameters)."""
    params = case(cfg["index"])["params"]
    net = sp.SNN((cfg["B"], None, cfg["C"]), cfg["sizes"], **net_kwargs(cfg))
    res = net.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for lay, seed in zip(list(net.snn)[:n_hidden(cfg)], dropout_seeds(cfg)):
        lay._dropout_seed = lambda device, seed=seed: seed
    return net, params


def loss_of(cfg, out, rates, y, gout, seq=None, gseq=None):
    """The scalar both sides differentiate: tests/network_cases.py loss_of, and with per_step a random cotangent on seq
    beside it (the loss uses seq as well as out)."""
    if cfg["use_readout_layer"]:
        if cfg["regulariser"]:
            loss = orc.train_step_loss(out, rates, y, use_regularizers=True, reg_fmin=REG_F, reg_fmax=REG_F)
        else:
            loss = (out * gout).sum()
        if seq is not None:
            loss = loss + (seq * gseq).sum()
        return loss
    loss = (out * out).mean()
    if cfg["regulariser"]:
        loss = loss + 0.5 * (F.relu(REG_F - rates).sum() + F.relu(rates - REG_F).sum())
    return loss


def learnable(cfg, key):
    """Whether a floating-point entry of the state_dict gets a gradient."""
    if "running" in key:
        return False
    if key.endswith("delay"):
        return cfg["learn_delays"]
    if key.endswith("gamma"):
        return cfg["learn_synapse"]
    return True


def oracle_run(c, dtype, backward=True):
    """One oracle step of case c in dtype: out, rates, seq (None without per_step), every hidden layer's spike train
    (after dropout and the validity mask), loss, every gradient, the running statistics, and u - theta of every hidden
    layer as (rows, T, H)."""
    cfg = c["cfg"]

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    p = {k: cast(v).clone().requires_grad_(v.is_floating_point() and learnable(cfg, k))
         for k, v in c["params"].items() if "num_batches" not in k}
    init = [{k: cast(v) for k, v in st.items()} for st in c["init"]]
    masks = None if c["masks"] is None else [cast(m) for m in c["masks"]]
    rec, spikes, stats = [], [], {}

    def step(d):
        rec.append(d.detach())
        if cfg["surrogate"]:
            from sparch_amd.snns import SpikeFunctionSurrogate
            return SpikeFunctionSurrogate.apply(d, *cfg["surrogate"])
        return _Step.apply(d)

    old, orc.spike = orc.spike, step
    try:
        res = fo.snn_forward(cast(c["x"]), p, neuron_type=cfg["kind"], num_layers=len(cfg["sizes"]), init_states=init,
                             lengths=cfg["lengths"], normalization=cfg["normalization"],
                             bidirectional=cfg["bidirectional"], use_readout_layer=cfg["use_readout_layer"],
                             training=cfg["training"], theta=cfg["threshold"], stats=stats, drop_masks=masks,
                             spikes_out=spikes, max_delay=cfg["max_delay"],
                             synapse=SYN_LIMITS_F32 if cfg["synapse"] != "off" else None, readout=cfg["readout"],
                             per_step=cfg["per_step"])
    finally:
        orc.spike = old
    out, rates, seq = res if cfg["per_step"] else (*res, None)
    T = cfg["T"]
    assert len(rec) == n_hidden(cfg) * T
    r = dict(out=out.detach(), rates=rates.detach(), seq=None if seq is None else seq.detach(),
             spikes=[s.detach() for s in spikes], stats=stats,
             diffs=[torch.stack(rec[k * T:(k + 1) * T], dim=1) for k in range(n_hidden(cfg))])
    if backward:
        loss = loss_of(cfg, out, rates, c["y"], None if c["gout"] is None else cast(c["gout"]), seq,
                       None if c["gseq"] is None else cast(c["gseq"]))
        loss.backward()
        r.update(loss=loss.detach(), grads={k: v.grad for k, v in p.items() if v.requires_grad})
    return r


@functools.lru_cache(maxsize=None)
def runs(i):
    """(the fp64 run, the fp32 run) of case i."""
    return oracle_run(case(i), torch.float64), oracle_run(case(i), torch.float32)


def valid_rows(cfg):
    """(rows, T, 1) bool: the steps of a cell's rows that count (all of them without lengths)."""
    dirs = 2 if cfg["bidirectional"] else 1
    if cfg["lengths"] is None:
        return torch.ones(cfg["B"] * dirs, cfg["T"], 1, dtype=torch.bool)
    m = rag.valid_mask(cfg["lengths"], cfg["T"])
    return torch.cat([m] * dirs, dim=0)[:, :, None]


def role_of(key):
    return key if key in ("out", "loss", "seq") else key.split(".", 2)[2]


def compared(run):
    """The tensors held to `bounds`: out, seq where present, loss and every parameter gradient."""
    res = dict(out=run["out"], loss=run["loss"], **run["grads"])
    if run["seq"] is not None:
        res["seq"] = run["seq"]
    return res


def relative_errors(i):
    """|fp32 run - fp64 run| over the fp64 run's max-abs, per compared tensor (the loss: over max(1, |loss|))."""
    r64, r32 = runs(i)
    a, b = compared(r64), compared(r32)
    return {k: maxabs(b[k].double() - a[k]) / (max(1.0, maxabs(a[k])) if k == "loss" else maxabs(a[k]) + 1e-300)
            for k in a if not residue(case(i)["cfg"], k)}


def verdict(i, slack=1.0):
    """(kept, reason): the keep rule of tests/network_cases.py verdict, unchanged, on this file's oracle runs of case i
    (slack: as there)."""
    cfg = case(i)["cfg"]
    r64, r32 = runs(i)
    m = valid_rows(cfg)
    # (a) decidable
    for s64, s32 in zip(r64["spikes"], r32["spikes"]):
        if not torch.equal(s64.float(), s32) and slack >= 1.0:
            return False, "a: the spike trains of the fp32 and fp64 runs differ"
    margin = min(float(d[m.expand_as(d)].abs().min()) for d in r64["diffs"])
    err = max(float((d32.double() - d64)[m.expand_as(d64)].abs().max()) for d64, d32 in zip(r64["diffs"], r32["diffs"]))
    if not margin >= MARGIN * slack * err or margin == 0.0:
        return False, f"a: margin {margin:.2e} under {MARGIN * slack:g} x {err:.2e}"
    if cfg["regulariser"]:      # the regulariser's hinge is a decision too: no rate within fp32 rounding of it
        if float((r64["rates"] - REG_F).abs().min()) < 1e-5:
            return False, "a: a firing rate on the regulariser's hinge"
    # (b) alive
    for d in r64["diffs"]:
        rate = float((d > 0)[m.expand_as(d)].double().mean())
        if not RATE_WINDOW[0] <= rate <= RATE_WINDOW[1]:
            return False, f"b: firing rate {rate:.3f}"
    for k, v in r64["grads"].items():
        if not residue(cfg, k) and not bool(v.any()):
            return False, f"b: the gradient of {k} is identically zero"
    # (c) well-conditioned
    for k, e in relative_errors(i).items():
        cap = OUT_RTOL if k in ("out", "seq") else LOSS_RTOL if k == "loss" else GRAD_RTOL
        if not e <= cap / slack:
            return False, f"c: {k} {e:.2e}"
    return True, ""


def fill_index(pair, attempt=0):
    return FILL_BASE + required_pairs().index(pair) * FILL_TRIES + attempt


def derive_kept(n_random=N_RANDOM):
    """(KEPT as the rule gives it, every index tried, {rejected index: reason}): the random indices, then for every
    required pair the kept ones so far leave uncovered the first kept attempt of the fill pass."""
    kept, tried, rejected = [], [], {}

    def take(i):
        tried.append(i)
        ok, why = verdict(i)
        if ok:
            kept.append(i)
        else:
            rejected[i] = why
        return ok

    for i in range(n_random):
        take(i)
    while True:
        missing = coverage(kept)[2]
        missing = [p for p in missing if fill_index(p, FILL_TRIES - 1) not in tried]
        if not missing:
            break
        for attempt in range(FILL_TRIES):
            if take(fill_index(missing[0], attempt)):
                break
    return kept, tried, rejected


def tried_indices(kept=None):
    """Every index the derivation looks at on the way to `kept`: the random ones, and of each fill pair in it the attempts
    up to the kept one."""
    kept = KEPT if kept is None else kept
    tried = list(range(N_RANDOM))
    for i in kept:
        if i >= FILL_BASE:
            first = FILL_BASE + (i - FILL_BASE) // FILL_TRIES * FILL_TRIES
            tried += list(range(first, i + 1))
    return tried


@functools.lru_cache(maxsize=None)
def role_errors():
    """r_role: the worst relative fp32 error of each role over all kept cases (tests/network_cases.py role_errors)."""
    worst = {r: 0.0 for r in ROLES}
    for i in KEPT:
        for k, e in relative_errors(i).items():
            worst[role_of(k)] = max(worst[role_of(k)], e)
    return worst


def bounds(i):
    """{tensor: bound}, bound = 4 x max(|fp32 oracle - fp64 oracle| of this case, r_role x max-abs of the reference),
    each asserted to stay under the project's whole-network bars (seq takes out's).  W.bias under train-mode BatchNorm has
    no entry."""
    cfg = case(i)["cfg"]
    r64, r32 = runs(i)
    a, b = compared(r64), compared(r32)
    pool, res = role_errors(), {}
    for k in a:
        if residue(cfg, k):
            continue
        top = max(1.0, maxabs(a[k])) if k == "loss" else maxabs(a[k])
        res[k] = 4.0 * max(maxabs(b[k].double() - a[k]), pool[role_of(k)] * top)
        cap = OUT_CAP if k in ("out", "seq") else LOSS_CAP if k == "loss" else GRAD_CAP
        assert res[k] <= cap * top * (1 + 1e-9), (k, res[k], cap * top)
    return res


def bf16_cases():
    """The first 16 kept cases whose operands are bf16-exact: grid weights, a 0/1 or count input, the box-car."""
    ok = [i for i in KEPT if not draw(i)["real_weights"] and draw(i)["input"] != "real" and not draw(i)["surrogate"]]
    return ok[:16]


def other_layout(cfg):
    """A ragged configuration in the other ragged layout, or None where that one is refused."""
    if cfg["layout"] == "dense":
        return None
    other = dict(cfg, layout="pack" if cfg["layout"] == "lengths" else "lengths")
    return None if refusal(axis_values(other).values()) else other


def device_run(sp, c, backward=True, grad=True, **over):
    """One step of case c on the HIP path: dict(net, out, rates, seq, loss, spikes {layer: (B,T,F) train}, x).  The spike
    trains are recorded around forward_with_rate, so the layers still hand each other placeholders and bf16 planes (a
    packed layer's train is unpacked on the host, tests/packed_numpy.py).  grad=False: the forward alone under
    torch.no_grad().  over: entries of the configuration replaced for this run (layout, training)."""
    from sparch_amd import functional as Fn
    from sparch_amd import snns as snn_mod
    cfg = dict(c["cfg"], **over)
    net, _ = build(sp, cfg)
    net = net.to(DEV).train(cfg["training"])
    rec = {}
    for k, lay in enumerate(list(net.snn)[:n_hidden(cfg)]):
        def wrapped(inp, states=None, orig=lay.forward_with_rate, k=k, **kw):
            s, r = orig(inp, states=states, **kw)
            rec[k] = snn_mod.materialize_spikes(s).detach()
            return s, r
        lay.forward_with_rate = wrapped
    if cfg["input"] == "counts":
        x = Fn.input_from_counts(c["counts"].to(DEV))
    else:
        x = c["x"].to(DEV)
        if cfg["lengths"] is not None and grad:
            x.requires_grad_(True)
    with torch.set_grad_enabled(grad), injected_states(c):
        res = net(x, **forward_kwargs(cfg))
        Fn.check_status()
        out, rates, seq = res if cfg["per_step"] else (*res, None)
        loss = None
        if backward and grad:
            on = lambda t: None if t is None else t.to(DEV)  # noqa: E731
            loss = loss_of(cfg, out, rates, on(c["y"]), on(c["gout"]), seq, on(c["gseq"]))
            loss.backward()
            Fn.check_status()
    dirs = 2 if cfg["bidirectional"] else 1
    for k, s in rec.items():
        width = cfg["sizes"][k] * dirs
        s = s.float().reshape(-1, width)
        if cfg["layout"] == "pack":
            torch.cuda.synchronize()
            s = torch.from_numpy(pn.unpack(s.cpu().numpy(), cfg["lengths"], cfg["T"]))
        rec[k] = s.reshape(cfg["B"], cfg["T"], width)
    return dict(net=net, out=out, rates=rates, seq=seq, loss=loss, spikes=rec, x=x)

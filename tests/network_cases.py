"""
Whole spiking networks drawn at random, with a normalisation, for tests/test_network_fuzz_host.py (the keep rule, the
oracle's consistency, what the bound resolves) and tests/test_network_fuzz_gpu.py (the HIP path against the oracle).

draw(i)          the configuration of index i, a pure function of i (PLANES: the one fixed case that reaches the bf16
                 planes of dx, functional._use_dx_planes).
case(i)          draw(i) plus every tensor of the case, generated from seeds on the CPU: parameters under the
                 reference's state_dict keys, input, labels / cotangent, initial states on a 2^-4 grid, dropout masks
                 (tests/dropout_numpy.py), lengths.  Made once, never written to.
build(sp, cfg)   the SNN of the package with those parameters loaded and its dropout seeds pinned.
oracle_run(c, dtype)  oracle.snn_oracle.snn_forward (tests.ragged_oracle.snn_forward with lengths) in `dtype`, with
                 orc.spike replaced for the call by a step that keeps the input's dtype and records u - theta.
verdict(i)       the keep rule, on the oracle's fp32 and fp64 runs alone.  KEPT: the first N_KEPT kept indices, a
                 literal that tests/test_network_fuzz_host.py re-derives.
bounds(i)        the acceptance bound of every compared tensor, from the oracle alone.
device_run(sp, c)  one step of the case on the HIP path, the initial states injected.

The drive is tuned toward the firing-rate window, not the window toward the drive: the affine parameters of the
normalisation grow as the sequence gets shorter (a membrane potential that starts in [0, 1) and integrates
(1 - alpha) * drive for 4 steps reaches the threshold only under a drive of several units), and without a normalisation
the weights' offset is set from the fan-in and the input density.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc
from tests import dropout_numpy as dn
from tests import ragged_oracle as rag
from tests import surrogate_numpy as sg
from tests.kit import DEV, SEED

KINDS = ("LIF", "adLIF", "RLIF", "RadLIF")
BATCHES, STEPS, CHANNELS = (2, 5, 17, 33), (4, 7, 19), (3, 20, 33, 70)
WIDTHS, CLASSES = (3, 5, 12, 30, 33, 64, 66, 100, 130), (3, 20, 35, 130)
NORMS = ("batchnorm",) * 3 + ("layernorm",) * 2 + ("none",)
INPUTS = ("binary", "counts", "real")
SMOOTH = ("triangle", "fast_sigmoid", "atan")
P_DROP = 0.25
REG_F = 0.21            # fmin = fmax of the regulariser: one of its two hinges is live for every unit
N_KEPT = 64
PLANES = -1             # draw(PLANES): two directions, BatchNorm, a spike-fed layer with K = 2 x 128, H = 256, B T = 256
DRAW_SEED = 24          # of the seeds 0 .. 39 the one whose kept cases spread most evenly over the axes (the cap below)
PLANES_SEED = 15        # the first data seed at which the planes case's margin is 32 x the fp32 error (4 x the rule's)
MARGIN = 8.0            # condition (a): smallest |u - theta| over largest fp32-vs-fp64 difference of u - theta
RATE_WINDOW = (0.02, 0.7)
GRAD_RTOL, OUT_RTOL, LOSS_RTOL = 1e-4, 2.5e-5, 2.5e-6     # condition (c): a quarter of the caps below
GRAD_CAP, OUT_CAP, LOSS_CAP = 5e-4, 1e-4, 1e-5            # the project's whole-network bars
ROLES = ("W.weight", "W.bias", "V.weight", "alpha", "beta", "a", "b", "norm.weight", "norm.bias", "out", "loss")

# the affine gain of the normalised drive and the mean drive without a normalisation, per sequence length
AFFINE_GAIN = {4: 5.0, 7: 3.0, 8: 2.0, 19: 1.25}
PLAIN_DRIVE = {4: 6.0, 7: 3.5, 8: 2.5, 19: 1.5}
DENSITY = 0.3

# The first N_KEPT indices that verdict() keeps (tests/test_network_fuzz_host.py re-derives the list).
KEPT = (0, 1, 2, 4, 6, 7, 8, 10, 12, 13, 15, 17, 19, 20, 21, 23, 24, 26, 28, 29, 30, 31, 32, 34, 35, 36, 37, 38, 40,
        41, 42, 43, 44, 45, 47, 48, 50, 51, 52, 53, 54, 55, 56, 58, 59, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71,
        72, 73, 74, 75, 76, 77, 78, 79)


def draw(i):
    """The configuration of index i."""
    if i == PLANES:
        return dict(index=PLANES, kind="RLIF", B=32, T=8, C=33, sizes=[128, 256, 20], normalization="batchnorm",
                    bidirectional=True, use_bias=False, use_readout_layer=True, training=True, threshold=1.0,
                    input="binary", real_weights=False, dropout=0.0, regulariser=True, lengths=None, surrogate=None)
    rng = np.random.default_rng([DRAW_SEED, i])

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    B, T, C, nl = pick(BATCHES), pick(STEPS), pick(CHANNELS), pick((2, 3))
    widths, classes = [pick(WIDTHS) for _ in range(3)], pick(CLASSES)
    norm, bidir, bias = pick(NORMS), bool(rng.integers(2)), bool(rng.integers(2))
    readout, training, theta = bool(rng.integers(4)), bool(rng.integers(4)), pick((1.0, 0.75))
    inp, real_w, drop, reg = pick(INPUTS), not rng.integers(4), not rng.integers(4), bool(rng.integers(2))
    ragged, smooth, name = not rng.integers(3), not rng.integers(4), pick(SMOOTH)
    tail = [int(v) for v in rng.integers(1, T + 1, B)]
    sizes = widths[:nl - 1] + [classes if readout else widths[2]]
    eligible = not bidir and readout and not (norm == "batchnorm" and bias)
    lengths = ([1, T] + tail)[:B] if (ragged and eligible) else None
    return dict(index=i, kind=KINDS[i % 4], B=B, T=T, C=C, sizes=sizes, normalization=norm, bidirectional=bidir,
                use_bias=bias, use_readout_layer=readout, training=training, threshold=theta, input=inp,
                real_weights=bool(real_w), dropout=P_DROP if (drop and training) else 0.0, regulariser=reg,
                lengths=lengths, surrogate=(name, sg.TEST_SCALE[name]) if smooth else None)


def label(cfg):
    """The configuration as a test id."""
    if cfg["index"] == PLANES:
        return "planes-RLIF-bn-B32T8C33-128x256x20-2dir-train-binary-reg"
    n = {"batchnorm": "bn", "layernorm": "ln", "none": "none"}[cfg["normalization"]]
    parts = [str(cfg["index"]), cfg["kind"], n, f"B{cfg['B']}T{cfg['T']}C{cfg['C']}", "x".join(map(str, cfg["sizes"])),
             "2dir" if cfg["bidirectional"] else "1dir", "train" if cfg["training"] else "eval", cfg["input"]]
    parts += [k for k, on in (("bias", cfg["use_bias"]), ("noreadout", not cfg["use_readout_layer"]),
                              ("th75", cfg["threshold"] != 1.0), ("realw", cfg["real_weights"]),
                              ("drop", cfg["dropout"] > 0), ("reg", cfg["regulariser"]),
                              ("len", cfg["lengths"] is not None)) if on]
    if cfg["surrogate"]:
        parts.append(cfg["surrogate"][0])
    return "-".join(parts)


def axis_values(cfg):
    """The axis values a case stands for, as the tallies of the cap count them."""
    return [f"kind={cfg['kind']}", f"norm={cfg['normalization']}", f"dirs={2 if cfg['bidirectional'] else 1}",
            f"bias={cfg['use_bias']}", f"readout={cfg['use_readout_layer']}", f"train={cfg['training']}",
            f"threshold={cfg['threshold']}", f"input={cfg['input']}", f"real_weights={cfg['real_weights']}",
            f"dropout={cfg['dropout']}", f"regulariser={cfg['regulariser']}", f"lengths={cfg['lengths'] is not None}",
            f"smooth={cfg['surrogate'] is not None}"]


def n_hidden(cfg):
    return len(cfg["sizes"]) - 1 if cfg["use_readout_layer"] else len(cfg["sizes"])


def dropout_seeds(cfg):
    return [SEED + 7919 * k for k in range(n_hidden(cfg))]


def _grid(t, steps):
    """On the 2^-k grid and in 8 significant bits (a large entry lands on a coarser grid): exact as a bf16 operand."""
    return (torch.round(t * steps) / steps).bfloat16().float()


def _parameters(cfg, g):
    """Every parameter under the reference's state_dict keys: W at nn.Linear's initialisation times 4 plus a positive
    offset and V orthogonal, both on the 2^-6 grid unless the case has real-valued weights; the affine of the
    normalisation on a 2^-4 grid; running statistics drawn, not left at 0 / 1; a few neuron parameters outside their
    clamp ranges."""
    kind, norm, T, dirs = cfg["kind"], cfg["normalization"], cfg["T"], 2 if cfg["bidirectional"] else 1
    p, fan, density = {}, cfg["C"], DENSITY * {"binary": 1.0, "counts": 2.0, "real": 1.0}[cfg["input"]]
    for k, H in enumerate(cfg["sizes"]):
        pre, hidden = f"snn.{k}.", k < n_hidden(cfg)
        W = (torch.rand(H, fan, generator=g) * 2 - 1) / math.sqrt(fan) * 4
        # without a normalisation the offset carries the mean drive; under one it is removed, make_net's 0.25 stays
        W = W + (PLAIN_DRIVE[T] / (density * fan) if norm == "none" and hidden else 0.25)
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
            gain = AFFINE_GAIN[T] if hidden else 1.0
            p[pre + "norm.weight"] = _grid((torch.rand(H, generator=g) + 1.0) * gain, 16)
            p[pre + "norm.bias"] = _grid((torch.rand(H, generator=g) * 0.5 + 0.25) * gain, 16)
        if norm == "batchnorm":
            p[pre + "norm.running_mean"] = torch.rand(H, generator=g) - 0.5
            p[pre + "norm.running_var"] = torch.rand(H, generator=g) * 0.75 + 0.25
            p[pre + "norm.num_batches_tracked"] = torch.tensor(3 + k)
        fan, density = H * dirs, 0.25
    if not cfg["real_weights"]:     # what the bf16 operand mode relies on
        assert all(torch.equal(v, v.bfloat16().float()) for k, v in p.items() if k.endswith(("W.weight", "V.weight")))
    return p


def _eval_statistics(cfg, c, g):
    """Eval mode normalises with the running statistics, so they have to lie near the batch's for the network to fire:
    the batch statistics of the oracle's own train-mode fp64 pass (running_mean 0 and running_var 1 going in), the mean
    moved by up to 0.2 standard deviations and the variance scaled by 0.8 .. 1.25.  Nothing of the package enters."""
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


@functools.lru_cache(maxsize=None)
def case(i):
    """draw(i) and the tensors of the case (CPU, fp32; the counts input as uint8 too)."""
    cfg = draw(i)
    B, T, C, dirs = cfg["B"], cfg["T"], cfg["C"], 2 if cfg["bidirectional"] else 1
    g = torch.Generator().manual_seed(7000 + (i if i >= 0 else 99991 + PLANES_SEED))
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
    if cfg["use_readout_layer"]:
        c["y"], c["gout"] = torch.randint(0, last, (B,), generator=g), torch.randn(B, last, generator=g)
    else:
        c["y"], c["gout"] = None, None
    init = []
    for k, H in enumerate(cfg["sizes"]):
        names = (("u0", "w0", "s0") if orc.ADAPTIVE[cfg["kind"]] else ("u0", "s0")) if k < nh else ("u0",)
        rows = B * dirs if k < nh else B
        init.append({n: torch.floor(torch.rand(rows, H, generator=g) * 16) / 16 for n in names})
    c["init"] = init
    c["masks"] = None
    if cfg["dropout"] > 0:      # (a recurrent cell runs at its width padded to 4: the mask index is that tensor's)
        rec = orc.RECURRENT[cfg["kind"]]
        c["masks"] = [torch.from_numpy(dn.keep_mask_padded(s, B, T, dirs, H, (H + 3) // 4 * 4 if rec else H,
                                                             cfg["dropout"]))
                      for s, H in zip(dropout_seeds(cfg), cfg["sizes"][:nh])]
    if cfg["normalization"] == "batchnorm" and not cfg["training"]:
        _eval_statistics(cfg, c, g)
    return c


def build(sp, cfg):
    """(the package's SNN on the CPU with the case's parameters loaded and its dropout seeds pinned, the parameters)."""
    params = case(cfg["index"])["params"]
    name, scale = cfg["surrogate"] or ("boxcar", None)
    net = sp.SNN((cfg["B"], None, cfg["C"]), cfg["sizes"], neuron_type=cfg["kind"], threshold=cfg["threshold"],
                 dropout=cfg["dropout"], normalization=cfg["normalization"], use_bias=cfg["use_bias"],
                 bidirectional=cfg["bidirectional"], use_readout_layer=cfg["use_readout_layer"], surrogate=name,
                 surrogate_scale=scale)
    res = net.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for lay, seed in zip(list(net.snn)[:n_hidden(cfg)], dropout_seeds(cfg)):
        lay._dropout_seed = lambda device, seed=seed: seed
    return net, params


class _Step(torch.autograd.Function):
    """oracle._Boxcar in the input's own dtype: the same comparison and the same assignments, the result not cast to
    float32."""

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


def loss_of(cfg, out, rates, y, gout):
    """The scalar both sides differentiate.  With a readout: the train step's loss with the regulariser, or a random
    cotangent; without one (out * out).mean(), plus the regulariser's term in the same half of the cases."""
    if cfg["use_readout_layer"]:
        if cfg["regulariser"]:
            return orc.train_step_loss(out, rates, y, use_regularizers=True, reg_fmin=REG_F, reg_fmax=REG_F)
        return (out * gout).sum()
    loss = (out * out).mean()
    if cfg["regulariser"]:
        loss = loss + 0.5 * (F.relu(REG_F - rates).sum() + F.relu(rates - REG_F).sum())
    return loss


def oracle_run(c, dtype, backward=True, rates_edit=None):
    """One oracle step of case c in dtype: out, rates, every hidden layer's spike train (after dropout and the validity
    mask), loss, every gradient, the running statistics, and u - theta of every hidden layer as (rows, T, H)."""
    cfg = c["cfg"]

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    p = {k: cast(v).clone().requires_grad_(v.is_floating_point() and "running" not in k)
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

    kw = dict(neuron_type=cfg["kind"], num_layers=len(cfg["sizes"]), init_states=init,
              normalization=cfg["normalization"], training=cfg["training"], theta=cfg["threshold"], stats=stats,
              drop_masks=masks, spikes_out=spikes)
    old, orc.spike = orc.spike, step
    try:
        if cfg["lengths"] is None:
            out, rates = orc.snn_forward(cast(c["x"]), p, bidirectional=cfg["bidirectional"],
                                         use_readout_layer=cfg["use_readout_layer"], **kw)
        else:
            out, rates = rag.snn_forward(cast(c["x"]), cfg["lengths"], p, **kw)
    finally:
        orc.spike = old
    T = cfg["T"]
    assert len(rec) == n_hidden(cfg) * T
    r = dict(out=out.detach(), rates=rates.detach(), spikes=[s.detach() for s in spikes], stats=stats,
             diffs=[torch.stack(rec[k * T:(k + 1) * T], dim=1) for k in range(n_hidden(cfg))])
    if backward:
        if rates_edit is not None:
            rates = rates_edit(rates)
        loss = loss_of(cfg, out, rates, c["y"], None if c["gout"] is None else cast(c["gout"]))
        loss.backward()
        r.update(loss=loss.detach(), grads={k: v.grad for k, v in p.items() if v.requires_grad})
        r["rates"] = rates.detach()
    return r


@functools.lru_cache(maxsize=None)
def runs(i):
    """(the fp64 run, the fp32 run) of case i."""
    return oracle_run(case(i), torch.float64), oracle_run(case(i), torch.float32)


def valid_rows(cfg):
    """(rows, T, 1) bool: the steps of a cell's rows that count (all of them without lengths)."""
    rows = cfg["B"] * (2 if cfg["bidirectional"] else 1)
    if cfg["lengths"] is None:
        return torch.ones(rows, cfg["T"], 1, dtype=torch.bool)
    return rag.valid_mask(cfg["lengths"], cfg["T"])[:, :, None]


def maxabs(t):
    return float(t.detach().abs().max())


def role_of(key):
    return key if key in ("out", "loss") else key.split(".", 2)[2]


def residue(cfg, key):
    """W.bias under train-mode BatchNorm: the gradient is zero in real arithmetic and rounding residue in every
    implementation."""
    return key.endswith("W.bias") and cfg["normalization"] == "batchnorm" and cfg["training"]


def compared(run):
    """The tensors held to `bounds`: out, loss and every parameter gradient."""
    return dict(out=run["out"], loss=run["loss"], **run["grads"])


def relative_errors(i):
    """|fp32 run - fp64 run| over the fp64 run's max-abs, per compared tensor (the loss: over max(1, |loss|))."""
    r64, r32 = runs(i)
    a, b = compared(r64), compared(r32)
    return {k: maxabs(b[k].double() - a[k]) / (max(1.0, maxabs(a[k])) if k == "loss" else maxabs(a[k]) + 1e-300)
            for k in a if not residue(case(i)["cfg"], k)}


def verdict(i, slack=1.0):
    """(kept, reason): the keep rule on the oracle's fp32 and fp64 runs of case i.  slack: the factor by which the two
    thresholds that are held against the fp32 run's error are tightened (> 1) or relaxed (< 1).  That error is a sample
    of fp32 rounding and moves by up to a factor of 1.5 from one CPU to the next (another BLAS path), so the host test
    re-derives KEPT with a band: what passes at slack 2 must be in KEPT, what fails at slack 0.5 must not be."""
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
        cap = OUT_RTOL if k == "out" else LOSS_RTOL if k == "loss" else GRAD_RTOL
        if not e <= cap / slack:
            return False, f"c: {k} {e:.2e}"
    return True, ""


def derive_kept(n=N_KEPT):
    """(the first n kept indices, {rejected index: reason})."""
    kept, rejected, i = [], {}, 0
    while len(kept) < n:
        ok, why = verdict(i)
        if ok:
            kept.append(i)
        else:
            rejected[i] = why
        i += 1
    return kept, rejected


@functools.lru_cache(maxsize=None)
def role_errors():
    """r_role: the worst relative fp32 error of each parameter role over all kept cases.  One tensor's own fp32 run is
    a small sample of what correct fp32 arithmetic does to it (tests/test_ragged_gpu.py pooled_relative_error)."""
    worst = {r: 0.0 for r in ROLES}
    for i in KEPT:
        for k, e in relative_errors(i).items():
            worst[role_of(k)] = max(worst[role_of(k)], e)
    return worst


def bounds(i):
    """{tensor: bound}, bound = 4 x max(|fp32 oracle - fp64 oracle| of this case, r_role x max-abs of the reference),
    each asserted to stay under the project's whole-network bars.  W.bias under BatchNorm has no entry."""
    cfg = case(i)["cfg"]
    r64, r32 = runs(i)
    a, b = compared(r64), compared(r32)
    pool, res = role_errors(), {}
    for k in a:
        if residue(cfg, k):
            continue
        top = max(1.0, maxabs(a[k])) if k == "loss" else maxabs(a[k])
        res[k] = 4.0 * max(maxabs(b[k].double() - a[k]), pool[role_of(k)] * top)
        cap = OUT_CAP if k == "out" else LOSS_CAP if k == "loss" else GRAD_CAP
        assert res[k] <= cap * top * (1 + 1e-9), (k, res[k], cap * top)
    return res


def bf16_cases():
    """The first 16 kept cases whose operands are bf16-exact: grid weights, a 0/1 or count input, the box-car."""
    ok = [i for i in KEPT if not draw(i)["real_weights"] and draw(i)["input"] != "real" and not draw(i)["surrogate"]]
    return ok[:16]


class injected_states:
    """The initial states of case c handed to the network's draws, in the reference's order."""

    def __init__(self, c):
        self.order = [st[k] for st in c["init"] for k in ("u0", "w0", "s0") if k in st]

    def __enter__(self):
        from sparch_amd import snns as snn_mod
        it = iter(self.order)
        self.mod, self.old = snn_mod, snn_mod._rand_to

        def next_state(rows, cols, device):
            t = next(it)
            assert tuple(t.shape) == (rows, cols)
            return t.to(device)

        snn_mod._rand_to = next_state

    def __exit__(self, *exc):
        self.mod._rand_to = self.old


def device_run(sp, c, backward=True, grad=True):
    """One step of case c on the HIP path: dict(net, out, rates, loss, spikes {layer: train}, x).  The spike trains are
    recorded as tests/spiking_cases.py run_dyadic records them: around forward_with_rate, so the layers still hand each
    other placeholders and bf16 planes.  grad=False: the forward alone under torch.no_grad()."""
    from sparch_amd import functional as Fn
    from sparch_amd import snns as snn_mod
    cfg = c["cfg"]
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
    kw = {} if cfg["lengths"] is None else {"lengths": torch.tensor(cfg["lengths"])}
    with torch.set_grad_enabled(grad), injected_states(c):
        out, rates = net(x, **kw)
        Fn.check_status()
        loss = None
        if backward and grad:
            loss = loss_of(cfg, out, rates, None if c["y"] is None else c["y"].to(DEV),
                           None if c["gout"] is None else c["gout"].to(DEV))
            loss.backward()
            Fn.check_status()
    return dict(net=net, out=out, rates=rates, loss=loss, spikes=rec, x=x)

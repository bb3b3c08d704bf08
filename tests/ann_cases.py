"""
Whole non-spiking baseline networks (sparch_amd/anns.py: MLP, RNN, LiGRU, GRU, ReadoutLayerANN) drawn at random, for
tests/test_ann_fuzz_host.py (the keep rule, the coverage, what the bound resolves) and tests/test_ann_fuzz_gpu.py (the
HIP path against the oracle in float64).  The structure is tests/network_cases.py's, and so are the margin, the keep
thresholds and the caps, imported from there.

draw(i)          the configuration of index i, a pure function of i.  0 <= i < FILL_BASE: a random draw.  i >= FILL_BASE:
                 the fill pass — pair (i - FILL_BASE) // FILL_TRIES of required_pairs() forced, the rest drawn.
                 RNN_WIDE, GRU_TILE: the two fixed cases.
case(i)          draw(i) plus every tensor of the case, generated from seeds on the CPU: parameters under the reference's
                 state_dict keys, input, labels / cotangent, dropout masks (tests/dropout_numpy.py).  Never written to.
build(sp, cfg)   the ANN of the package with those parameters loaded and its dropout seeds pinned.
oracle_run(c, dtype)   tests/ann_net_oracle.py in `dtype`: out, loss, every gradient (the input's too), the running
                 statistics after the step, every hidden layer's undropped output, every LiGRU relu argument.
verdict(i)       the keep rule, on the oracle's fp32 and fp64 runs alone:
                   a  LiGRU: the smallest |relu argument| is at least MARGIN x the largest fp32-vs-fp64 difference of those
                      arguments (a flipped relu' is a decision no bound covers)
                   b  no compared gradient is identically zero
                   c  the fp32 oracle is within a quarter of the caps
KEPT             the first N_KEPT kept random indices, then what the fill pass adds; a literal that the host test
                 re-derives with network_cases.verdict's slack band.
bounds(i)        4 x max(|fp32 oracle - fp64 oracle| of the case, r_role x max-abs of the fp64 run) per compared tensor,
                 asserted under the caps; never fitted to a device result.
device_run(sp, c)   one step of the case on the HIP path.

The launch path of a case (default / step / chunk) is an axis of the draw, but only tests/test_ann_fuzz_gpu.py acts on
it (PATH_ENV, through monkeypatch.setenv): the oracle never sees it.

What was changed, and why.  The axes are the issue's.  A single step (T = 1) leaves V*.weight, and the GRU's Wr, Vr
and normr, with a gradient that is exactly zero in every arithmetic (structural_zero): condition b would reject every
recurrent T = 1 draw (the kept share was 0.71), so these are no subject of it and the GPU test asserts them exactly zero
instead.  DRAW_SEED was chosen among 0 .. 39 (see there).  With eval mode, dropout, the grid and 4-D inputs and the loss
threshold in, the rule keeps 66 of the 70 indices tried (tests/test_ann_fuzz_host.py prints the share and the rejects).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import ann_net_oracle as ano
from tests import dropout_numpy as dn
from tests.kit import DEV, SEED
from tests.network_cases import GRAD_CAP, GRAD_RTOL, LOSS_CAP, LOSS_RTOL, MARGIN, OUT_CAP, OUT_RTOL  # noqa: F401

KINDS = ("MLP", "RNN", "LiGRU", "GRU")
BATCHES, STEPS, CHANNELS = (4, 9, 17, 33), (1, 4, 7, 19), (3, 20, 33, 70)
WIDTHS, CLASSES = (3, 5, 12, 30, 32, 33, 64, 66, 96, 130), (3, 20, 35, 130)
NORMS = ("batchnorm",) * 3 + ("layernorm",) * 2 + ("none",)
INPUTS = ("real", "grid", "4d")
PATHS = ("default", "step", "chunk")
P_DROP = 0.25
N_KEPT = 64
DRAW_SEED = 20          # of the seeds 0 .. 39 the one whose kept list is the same on one CPU thread and on eight and whose
                        # worst fp32 errors stay furthest below the thresholds of condition c on both (2.4e-5, 6.5e-6, 1.0e-6)
FILL_BASE, FILL_TRIES = 1000, 8
RNN_WIDE, GRU_TILE = -1, -2     # RNN [1028, 20]: above 1024, one launch per step.  GRU 2 x [96, 64] + 35 classes: a
FIXED = (RNN_WIDE, GRU_TILE)    # direction boundary inside a row tile on the persistent kernels, a readout fed by 128 columns
ROLES = ("W.weight", "W.bias", "V.weight", "norm.weight", "norm.bias", "x", "out", "loss")

# what the GPU test sets for a launch path, per kind (sparch_amd/functional.py reads them at every forward)
PATH_ENV = {
    "default": {},
    "step": {"MLP": {}, "RNN": {"SPARCH_REC_STEP_PATH": "1"}, "LiGRU": {"SPARCH_LIGRU_PERSISTENT": "0"},
             "GRU": {"SPARCH_GRU_PERSISTENT": "0"}},
    "chunk": {"SPARCH_REC_STEPS_PER_LAUNCH": "3"},
}

AXES = {"kind": KINDS, "norm": ("batchnorm", "layernorm", "none"), "dirs": (1, 2), "readout": (True, False),
        "train": (True, False), "dropout": (0.0, P_DROP), "input": INPUTS, "path": PATHS, "padded": (True, False)}
# the combinations of axis values no configuration has, each with its reason
REFUSED = {
    ("kind=MLP", "dirs=2"): "ANN refuses a bidirectional MLP (ValueError: MLP cannot be bidirectional)",
    ("train=False", f"dropout={P_DROP}"): "dropout is the identity in eval mode: an eval case has no mask to check",
}

# The kept indices (tests/test_ann_fuzz_host.py re-derives the list): the first N_KEPT kept random draws, then the fill pass.
KEPT = (0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33,
        34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63,
        64, 65, 66, 67, 1384, 2648)


# ------------------------------------------------------------------------------------------------ axes and coverage
def axis_values(cfg):
    """{axis: "axis=value"} of a configuration."""
    return {"kind": f"kind={cfg['kind']}", "norm": f"norm={cfg['normalization']}",
            "dirs": f"dirs={2 if cfg['bidirectional'] else 1}", "readout": f"readout={cfg['use_readout_layer']}",
            "train": f"train={cfg['training']}", "dropout": f"dropout={cfg['dropout']}", "input": f"input={cfg['input']}",
            "path": f"path={cfg['path']}", "padded": f"padded={any(h % 4 for h in hidden_sizes(cfg))}"}


def refusal(values):
    values = set(values)
    for combo, words in REFUSED.items():
        if set(combo) <= values:
            return words
    return None


@functools.lru_cache(maxsize=None)
def required_pairs():
    """Every pair of values of two different axes, in a fixed order."""
    vals = [(a, f"{a}={v}") for a, vs in AXES.items() for v in vs]
    return tuple((u, v) for k, (a, u) in enumerate(vals) for (b, v) in vals[k + 1:] if a != b)


def pairs_of(cfg):
    v = set(axis_values(cfg).values())
    return {p for p in required_pairs() if p[0] in v and p[1] in v}


def coverage(indices):
    """(pairs covered by the cases, pairs refused, pairs missing)."""
    covered = set()
    for i in indices:
        covered |= pairs_of(draw(i))
    refused = {p for p in required_pairs() if refusal(p)}
    return covered, refused, [p for p in required_pairs() if p not in covered and p not in refused]


# ------------------------------------------------------------------------------------------------ configurations
def n_hidden(cfg):
    return len(cfg["sizes"]) - 1 if cfg["use_readout_layer"] else len(cfg["sizes"])


def hidden_sizes(cfg):
    return cfg["sizes"][:n_hidden(cfg)]


def draw(i):
    """The configuration of index i."""
    base = dict(use_bias=False, use_readout_layer=True, training=True, input="real", path="default")
    if i == RNN_WIDE:
        return dict(base, index=i, kind="RNN", B=4, T=4, C=20, sizes=[1028, 20], normalization="layernorm",
                    bidirectional=False, dropout=0.0)
    if i == GRU_TILE:
        return dict(base, index=i, kind="GRU", B=17, T=7, C=33, sizes=[96, 64, 35], normalization="batchnorm",
                    bidirectional=True, dropout=P_DROP)
    forced = set()
    if i >= FILL_BASE:
        forced = set(required_pairs()[(i - FILL_BASE) // FILL_TRIES])
    kind = KINDS[i % 4]
    for v in forced:
        if v.startswith("kind="):
            kind = v[len("kind="):]
    rng = np.random.default_rng([DRAW_SEED, i])

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    while True:
        B, T, C, nl = pick(BATCHES), pick(STEPS), pick(CHANNELS), pick((2, 3))
        widths, classes = [pick(WIDTHS) for _ in range(3)], pick(CLASSES)
        norm, bidir, bias = pick(NORMS), bool(rng.integers(2)) and kind != "MLP", bool(rng.integers(2))
        readout, training, drop = bool(rng.integers(4)), bool(rng.integers(4)), not rng.integers(4)
        inp, path = pick(INPUTS), pick(PATHS)
        if f"dropout={P_DROP}" in forced:
            drop = True
        cfg = dict(index=i, kind=kind, B=B, T=T, C=C, sizes=widths[:nl - 1] + [classes if readout else widths[2]],
                   normalization=norm, bidirectional=bidir, use_bias=bias, use_readout_layer=readout, training=training,
                   dropout=P_DROP if (drop and training) else 0.0, input=inp, path=path)
        if forced <= set(axis_values(cfg).values()):
            return cfg


def label(cfg):
    """The configuration as a test id."""
    n = {"batchnorm": "bn", "layernorm": "ln", "none": "none"}[cfg["normalization"]]
    head = {RNN_WIDE: "wide", GRU_TILE: "tile"}.get(cfg["index"], str(cfg["index"]))
    parts = [head, cfg["kind"], n, f"B{cfg['B']}T{cfg['T']}C{cfg['C']}", "x".join(map(str, cfg["sizes"])),
             "2dir" if cfg["bidirectional"] else "1dir", "train" if cfg["training"] else "eval", cfg["input"], cfg["path"]]
    parts += [k for k, on in (("bias", cfg["use_bias"]), ("noreadout", not cfg["use_readout_layer"]),
                              ("drop", cfg["dropout"] > 0)) if on]
    return "-".join(parts)


def oracle_cfg(cfg):
    return dict(ann_type=cfg["kind"], layer_sizes=cfg["sizes"], use_readout_layer=cfg["use_readout_layer"],
                normalization=cfg["normalization"], bidirectional=cfg["bidirectional"])


def dropout_seeds(cfg):
    return [SEED + 7919 * k for k in range(n_hidden(cfg))]


def drop_masks(cfg, padded=True):
    """One (B, T, dirs * H) mask per hidden layer, or None.  All four kinds run at Hp = 4 * ceil(H / 4) per direction
    (anns.py pads MLP layers too), and the mask's element index is that tensor's.  padded=False: the index of the
    unpadded tensor, a wrong network of tests/test_ann_fuzz_host.py."""
    if cfg["dropout"] <= 0:
        return None
    dirs = 2 if cfg["bidirectional"] else 1
    return [torch.from_numpy(dn.keep_mask_padded(s, cfg["B"], cfg["T"], dirs, H, (H + 3) // 4 * 4 if padded else H,
                                                 cfg["dropout"]))
            for s, H in zip(dropout_seeds(cfg), hidden_sizes(cfg))]


def _parameters(cfg, g):
    """Every parameter under the reference's state_dict keys: W (and its bias) at nn.Linear's scale, V orthogonal, the
    affine weight in [0.7, 1.3] and bias in [-0.2, 0.2], running statistics drawn (mean in +-0.5, variance in
    [0.25, 1]) and num_batches_tracked = 3 + k."""
    kind, norm, dirs = cfg["kind"], cfg["normalization"], 2 if cfg["bidirectional"] else 1
    p, fan = {}, cfg["C"] * (2 if cfg["input"] == "4d" else 1)

    def normalisation(pre, H, k):
        if norm in ("batchnorm", "layernorm"):
            p[pre + ".weight"] = torch.rand(H, generator=g) * 0.6 + 0.7
            p[pre + ".bias"] = torch.rand(H, generator=g) * 0.4 - 0.2
        if norm == "batchnorm":
            p[pre + ".running_mean"] = torch.rand(H, generator=g) - 0.5
            p[pre + ".running_var"] = torch.rand(H, generator=g) * 0.75 + 0.25
            p[pre + ".num_batches_tracked"] = torch.tensor(3 + k)

    for k, H in enumerate(cfg["sizes"]):
        hidden = k < n_hidden(cfg)
        for gate in (ano.GATES[kind] if hidden else ("",)):
            pre = f"ann.{k}."
            p[pre + f"W{gate}.weight"] = (torch.rand(H, fan, generator=g) * 2 - 1) / math.sqrt(fan)
            if cfg["use_bias"]:
                p[pre + f"W{gate}.bias"] = (torch.rand(H, generator=g) * 2 - 1) / math.sqrt(fan)
            if hidden and ano.RECURRENT[kind]:
                p[pre + f"V{gate}.weight"] = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g)
            normalisation(pre + f"norm{gate}", H, k)
        fan = H * dirs
    return p


@functools.lru_cache(maxsize=None)
def case(i):
    """draw(i) and the tensors of the case (CPU, fp32)."""
    cfg = draw(i)
    B, T, C = cfg["B"], cfg["T"], cfg["C"]
    g = torch.Generator().manual_seed(9000 + (i if i >= 0 else 99991 - i))
    c = dict(cfg=cfg, params=_parameters(cfg, g))
    if cfg["input"] == "4d":
        x = torch.randn(B, T, C, 2, generator=g)
    else:
        x = torch.randn(B, T, C, generator=g)
        if cfg["input"] == "grid":          # on the 2^-4 grid and in 8 significant bits: exact as a bf16 operand
            x = (torch.round(x * 16) / 16).bfloat16().float()
    c["x"] = x
    last = cfg["sizes"][-1]
    if cfg["use_readout_layer"]:
        c["y"], c["gout"] = torch.randint(0, last, (B,), generator=g), None
    else:
        dirs = 2 if cfg["bidirectional"] else 1
        c["y"], c["gout"] = None, torch.randn(B, T, last * dirs, generator=g)
    c["masks"] = drop_masks(cfg)
    return c


def input_shape(cfg):
    return (cfg["B"], None, cfg["C"], 2) if cfg["input"] == "4d" else (cfg["B"], None, cfg["C"])


def build(sp, cfg):
    """(the package's ANN on the CPU with the case's parameters loaded and its dropout seeds pinned, the parameters)."""
    from sparch_amd.anns import ANN
    params = case(cfg["index"])["params"]
    net = ANN(input_shape(cfg), cfg["sizes"], ann_type=cfg["kind"], dropout=cfg["dropout"],
                 normalization=cfg["normalization"], use_bias=cfg["use_bias"], bidirectional=cfg["bidirectional"],
                 use_readout_layer=cfg["use_readout_layer"])
    res = net.load_state_dict(params, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for lay, seed in zip(list(net.ann)[:n_hidden(cfg)], dropout_seeds(cfg)):
        lay._dropout_seed = lambda device, seed=seed: seed
    return net, params


def loss_of(cfg, out, y, gout):
    """The scalar both sides differentiate: cross-entropy with a readout, a random cotangent without one."""
    return F.cross_entropy(out, y) if cfg["use_readout_layer"] else (out * gout).sum()


def oracle_run(c, dtype, masks="case"):
    """One oracle step of case c in dtype: out, loss, grads (parameters and "x"), stats (the running statistics after the
    step), hidden (every hidden layer's output before dropout), relu (every LiGRU relu argument).  masks: other masks
    than the case's (a wrong network)."""
    cfg = c["cfg"]

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    p = {k: cast(v).clone().requires_grad_("running" not in k) for k, v in c["params"].items() if "num_batches" not in k}
    running = {k: v.detach() for k, v in p.items() if "running" in k} or None
    masks = c["masks"] if isinstance(masks, str) else masks
    masks = None if masks is None else [cast(m) for m in masks]
    x = cast(c["x"]).clone().requires_grad_(True)
    record = {}
    out = ano.ann_forward(oracle_cfg(cfg), p, x, training=cfg["training"], running=running, masks=masks, record=record)
    loss = loss_of(cfg, out, c["y"], None if c["gout"] is None else cast(c["gout"]))
    loss.backward()
    grads = {k: v.grad for k, v in p.items() if v.requires_grad}
    grads["x"] = x.grad
    return dict(out=out.detach(), loss=loss.detach(), grads=grads, stats=running or {}, hidden=record["hidden"],
                relu=record["relu"])


@functools.lru_cache(maxsize=None)
def runs(i):
    """(the fp64 run, the fp32 run) of case i."""
    return oracle_run(case(i), torch.float64), oracle_run(case(i), torch.float32)


def maxabs(t):
    return float(t.detach().abs().max())


def role_of(key):
    """out, loss, x, or the parameter's role with the gate letter dropped: Wz.weight -> W.weight, normr.bias ->
    norm.bias."""
    if key in ("out", "loss", "x"):
        return key
    name, leaf = key.split(".", 2)[2].split(".")
    return name.rstrip("zr") + "." + leaf


def residue(cfg, key):
    """W*.bias under train-mode BatchNorm: the gradient is zero in real arithmetic and rounding residue in every
    implementation."""
    return role_of(key) == "W.bias" and cfg["normalization"] == "batchnorm" and cfg["training"]


def structural_zero(cfg, key):
    """What a single step leaves without a gradient: the cell starts from the zero state, so V*.weight multiplies zeros,
    and the GRU's reset gate scales that zero state, so nothing of Wr, Vr and normr reaches the output.  These gradients
    are exactly zero in every arithmetic.  They are not held to a relative bound (and are no subject of condition b):
    the GPU test asserts that every element is zero."""
    if cfg["T"] != 1 or key in ("out", "loss", "x"):
        return False
    name = key.split(".")[2]
    return name[0] == "V" or (cfg["kind"] == "GRU" and name in ("Wr", "normr") and int(key.split(".")[1]) < n_hidden(cfg))


def compared(run):
    """out, loss, every parameter gradient and the input's; `bounds` holds those that are neither residue nor
    structurally zero."""
    return dict(out=run["out"], loss=run["loss"], **run["grads"])


def unbounded(cfg, key):
    return residue(cfg, key) or structural_zero(cfg, key)


def relative_errors(i):
    """|fp32 run - fp64 run| over the fp64 run's max-abs, per compared tensor (the loss: over max(1, |loss|))."""
    r64, r32 = runs(i)
    a, b = compared(r64), compared(r32)
    return {k: maxabs(b[k].double() - a[k]) / (max(1.0, maxabs(a[k])) if k == "loss" else maxabs(a[k]) + 1e-300)
            for k in a if not unbounded(case(i)["cfg"], k)}


def verdict(i, slack=1.0):
    """(kept, reason): the keep rule on the oracle's fp32 and fp64 runs of case i.  slack tightens (> 1) or relaxes (< 1)
    the thresholds held against the fp32 run's error, as in network_cases.verdict."""
    cfg = case(i)["cfg"]
    r64, r32 = runs(i)
    # (a) decidable
    if r64["relu"]:
        margin = min(float(a.abs().min()) for a in r64["relu"])
        err = max(maxabs(a32.double() - a64) for a64, a32 in zip(r64["relu"], r32["relu"]))
        if not margin >= MARGIN * slack * err or margin == 0.0:
            return False, f"a: margin {margin:.2e} under {MARGIN * slack:g} x {err:.2e}"
    # (b) alive
    for k, v in r64["grads"].items():
        if structural_zero(cfg, k):
            assert not bool(v.any()), k
        elif not residue(cfg, k) and not bool(v.any()):
            return False, f"b: the gradient of {k} is identically zero"
    # (c) well-conditioned
    for k, e in relative_errors(i).items():
        cap = OUT_RTOL if k == "out" else LOSS_RTOL if k == "loss" else GRAD_RTOL
        if not e <= cap / slack:
            return False, f"c: {k} {e:.2e}"
    return True, ""


def fill_index(pair, attempt=0):
    return FILL_BASE + required_pairs().index(pair) * FILL_TRIES + attempt


def derive_kept(n=N_KEPT):
    """(KEPT as the rule gives it, every index tried, {rejected index: reason}): random indices until n are kept, then for
    every required pair the kept ones leave uncovered the first kept attempt of the fill pass."""
    kept, tried, rejected = [], [], {}

    def take(i):
        tried.append(i)
        ok, why = verdict(i)
        if ok:
            kept.append(i)
        else:
            rejected[i] = why
        return ok

    i = 0
    while len(kept) < n:
        take(i)
        i += 1
    while True:
        missing = [p for p in coverage(kept)[2] if fill_index(p, FILL_TRIES - 1) not in tried]
        if not missing:
            break
        for attempt in range(FILL_TRIES):
            if take(fill_index(missing[0], attempt)):
                break
    return kept, tried, rejected


def tried_indices(kept=None):
    """Every index the derivation looks at on the way to `kept`."""
    kept = KEPT if kept is None else kept
    tried = list(range(max(i for i in kept if i < FILL_BASE) + 1))
    for i in kept:
        if i >= FILL_BASE:
            first = FILL_BASE + (i - FILL_BASE) // FILL_TRIES * FILL_TRIES
            tried += list(range(first, i + 1))
    return tried


@functools.lru_cache(maxsize=None)
def role_errors():
    """r_role: the worst relative fp32 error of each role over all kept and fixed cases."""
    worst = {r: 0.0 for r in ROLES}
    for i in KEPT + FIXED:
        for k, e in relative_errors(i).items():
            worst[role_of(k)] = max(worst[role_of(k)], e)
    return worst


def bounds(i):
    """{tensor: bound}, bound = 4 x max(|fp32 oracle - fp64 oracle| of this case, r_role x max-abs of the fp64 run), each
    asserted to stay under the project's whole-network bars.  W*.bias under train-mode BatchNorm has no entry."""
    cfg = case(i)["cfg"]
    r64, r32 = runs(i)
    a, b = compared(r64), compared(r32)
    pool, res = role_errors(), {}
    for k in a:
        if unbounded(cfg, k):
            continue
        top = max(1.0, maxabs(a[k])) if k == "loss" else maxabs(a[k])
        res[k] = 4.0 * max(maxabs(b[k].double() - a[k]), pool[role_of(k)] * top)
        cap = OUT_CAP if k == "out" else LOSS_CAP if k == "loss" else GRAD_CAP
        assert res[k] <= cap * top * (1 + 1e-9), (k, res[k], cap * top)
    return res


def device_run(sp, c, backward=True, grad=True):
    """One step of case c on the HIP path: dict(net, out, loss, x, hidden [every hidden layer's output, after dropout,
    from a forward hook]).  grad=False: the forward alone under torch.no_grad()."""
    from sparch_amd import functional as Fn
    cfg = c["cfg"]
    net, _ = build(sp, cfg)
    net = net.to(DEV).train(cfg["training"])
    hidden, hooks = {}, []
    for k, lay in enumerate(list(net.ann)[:n_hidden(cfg)]):
        hooks.append(lay.register_forward_hook(lambda mod, args, out, k=k: hidden.__setitem__(k, out.detach())))
    x = c["x"].to(DEV)
    if grad:
        x.requires_grad_(True)
    with torch.set_grad_enabled(grad):
        out, none = net(x)
        Fn.check_status()
        assert none is None
        loss = None
        if backward and grad:
            loss = loss_of(cfg, out, None if c["y"] is None else c["y"].to(DEV),
                           None if c["gout"] is None else c["gout"].to(DEV))
            loss.backward()
            Fn.check_status()
    for h in hooks:
        h.remove()
    return dict(net=net, out=out, loss=loss, x=x, hidden=[hidden[k] for k in range(n_hidden(cfg))])

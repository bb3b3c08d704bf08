"""
Shared cases of the spiking kernels' GPU tests: the inputs of tests/spiking_numpy.py on the device, the kernels' forward
on them, and the dyadic cells and networks that test_hip_parity, test_dropout_rate_backward_gpu and the streaming tests
run.  The lru_cache'd builders hold device tensors: each is ONE object, imported by every test module that needs it, so
a GPU session keeps one copy of a case.  Nothing here touches the GPU at import.
"""
import functools

import torch

from oracle import snn_oracle as orc
from tests import spiking_numpy as sn
from tests.golden_io import snn_case
from tests.kit import DEV, F32, SEED, D, N
from tests.kit import Fn as _Fn


# ------------------------------------------------------------------------------------------------ recurrent kernels
@functools.lru_cache(maxsize=4)
def rec_case(kind, B, dirs, T, H, regime):
    """Inputs of one case on the host and on the device, made once and never written to."""
    c = sn.make_inputs(kind, B, dirs, T, H, sn.case_seed(kind, B, dirs, T, H), regime, affine_in=(dirs == 2))
    c["dev"] = {k: D(c[k]) for k in ("Wx", "scale", "shift", "u0", "w0", "s0", "g_out", "g_rate")}
    c["dev"]["p"] = {k: D(v) for k, v in c["p"].items()}
    return c


def rec_forward(c, spl):
    Fn, d = _Fn(), c["dev"]
    assert not Fn.SAVE_BF16
    s_out, count, saved, s16 = Fn.cell_forward(c["kind"], d["Wx"], d["scale"], d["shift"], d["p"], d["u0"], d["w0"], d["s0"],
                                               B=c["B"], dirs=c["dirs"], theta=c["theta"], p_drop=0.0, seed=0,
                                               steps_per_launch=spl)
    Fn.check_status()
    torch.cuda.synchronize()
    return s_out, count, saved, s16


# ------------------------------------------------------------------------------------------------ scan kernels
@functools.lru_cache(maxsize=2)
def scan_case(kind, B, dirs, T, H):
    """Inputs of one case on the host and on the device, made once and never written to; the conditions, asserted on
    the fp32 restatement's own free run."""
    c = sn.scan_case(kind, B, dirs, T, H)
    c["dev"] = {k: D(c[k]) for k in ("Wx", "scale", "shift", "u0", "w0", "s0", "g_out", "g_rate")}
    c["dev"]["p"] = {k: D(v) for k, v in c["p"].items()}
    c["dev"]["bn"] = tuple(D(v) for v in c["bn"])
    c["keep"] = sn.scan_keep(c, SEED)
    free = sn.forward(kind, F32, c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], B=B, dirs=dirs,
                      theta=c["theta"])
    c["spikes"], c["box"] = sn.scan_conditions(c, free["u_save"], c["keep"])
    # V4 takes four neurons per thread, everything else one (launch_cell of cell.hip)
    assert (B * dirs * H >= 524288 and H % 4 == 0) == ((B, dirs, H) == sn.V4)
    return c


def scan_forward(c, p_drop, save16=False, **kw):
    Fn, d = _Fn(), c["dev"]
    prev = Fn.SAVE_BF16
    Fn.SAVE_BF16 = save16
    try:
        res = Fn.cell_forward(c["kind"], d["Wx"], d["scale"], d["shift"], d["p"], d["u0"], d["w0"], d["s0"], B=c["B"],
                              dirs=c["dirs"], theta=c["theta"], p_drop=p_drop, seed=SEED, **kw)
    finally:
        Fn.SAVE_BF16 = prev
    Fn.check_status()
    torch.cuda.synchronize()
    return res


GEOM = {"V4": sn.V4 + (sn.T_V4,), "V1": sn.V1 + (sn.T_V1,), "V1big": sn.V1BIG + (sn.T_V4,), "V1odd": sn.V1ODD + (sn.T_V1,)}


def scan_case_of(kind, geom, T=None):
    B, dirs, H, T0 = GEOM[geom]
    return scan_case(kind, B, dirs, T0 if T is None else T, H)


def collect(dWx, grads, with_bn):
    """What cell_backward returned as numpy arrays, the BatchNorm sums under their own names."""
    got = {"dWx": N(dWx)}
    got.update({k: N(v) for k, v in grads.items() if k != "bn_sums"})
    if with_bn:
        got["bn_dy"], got["bn_dyx"] = N(grads["bn_sums"][0]), N(grads["bn_sums"][1])
    return got


# ------------------------------------------------------------------------------------------------ dyadic cells, networks
def dyadic_cell_case(kind, Bp, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    V = torch.randint(-24, 25, (H, H), generator=g).float() / 64.0
    Wx = torch.randn(Bp, T, H, generator=g) * 1.5 + 0.4
    p = {"alpha": torch.rand(H, generator=g) * 0.2 + 0.78, "V": V}
    if kind == "RadLIF":
        p.update(beta=torch.rand(H, generator=g) * 0.05 + 0.95, a=torch.rand(H, generator=g) * 2.4 - 1.2,
                 b=torch.rand(H, generator=g) * 2.4 - 0.2)
    u0 = torch.rand(Bp, H, generator=g)
    w0 = torch.rand(Bp, H, generator=g) if kind == "RadLIF" else None
    s0 = (torch.rand(Bp, H, generator=g) < 0.3).float()
    g_s = torch.randn(Bp, T, H, generator=g)
    return Wx, p, u0, w0, s0, g_s


def dyadic_cell_case_fwd(kind, Bp, T, H, seed):
    """dyadic_cell_case without the output gradient (its last draw): what a forward-only test takes."""
    return dyadic_cell_case(kind, Bp, T, H, seed)[:5]


def build_snn(sp, cfg, params, dropout=0.0):
    net = sp.SNN((cfg["B"], None, cfg["C"]), cfg["layer_sizes"], neuron_type=cfg["neuron_type"], dropout=dropout,
                 normalization=cfg["normalization"], use_bias=cfg["use_bias"], bidirectional=cfg["bidirectional"],
                 use_readout_layer=cfg["use_readout_layer"])
    missing = net.load_state_dict(params, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return net.to(DEV)


def run_dyadic(sp, name, monkeypatch, dropout=0.0, seeds=None, loss_kw=None):
    """One training step of a dyadic fixture's network on the HIP path, fed the fixture's initial states in
    the reference's draw order.  Returns (cfg, z, per-layer spikes, out, loss, net).  With dropout, `seeds[k]` is
    the dropout seed hidden layer k hands its kernels; `loss_kw` goes to oracle.train_step_loss (the regulariser)."""
    Fn = _Fn()
    cfg, x, y, params, init, z = snn_case(name)
    net = build_snn(sp, cfg, params, dropout).train()
    if seeds is not None:
        for lay, seed in zip(list(net.snn)[:-1], seeds):
            lay._dropout_seed = lambda device, seed=seed: seed
    order = []
    for st in init:
        order += [st[k] for k in ("u0", "w0", "s0") if k in st]
    states = iter(order)

    def next_state(rows, cols, device):
        t = next(states)
        assert tuple(t.shape) == (rows, cols)
        return t.to(device)

    from sparch_amd import snns as snn_mod
    monkeypatch.setattr(snn_mod, "_rand_to", next_state)
    rec = {}
    for k, lay in enumerate(list(net.snn)[:-1]):
        def wrapped(inp, states=None, orig=lay.forward_with_rate, k=k, **kw):
            s, r = orig(inp, states=states, **kw)
            rec[k] = snn_mod.materialize_spikes(s).detach()  # between the network's layers: the bf16 plane
            return s, r
        lay.forward_with_rate = wrapped
    out, rates = net(x.to(DEV))
    Fn.check_status()
    loss = orc.train_step_loss(out, rates, y.to(DEV), **(loss_kw or {}))
    loss.backward()
    Fn.check_status()
    return cfg, z, rec, out, loss, net

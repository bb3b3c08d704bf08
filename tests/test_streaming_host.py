"""CPU: what streaming inference (sparch_amd/streaming.py) rests on and what it refuses, without a device.

* the premise: a cell's step needs (u, w, s) of the step before and nothing else, so the oracle run in chunks with
  that state carried equals the oracle run over the whole sequence, bit for bit, on real-valued parameters;
* the constructor's refusals (bidirectional, training mode) come before any device use;
* the new entry points validate their arguments and return SPARCH_EINVAL without launching;
* StreamingFbank's frame arithmetic (a pure host helper) over random chunkings.
"""
import numpy as np
import pytest
import torch

from oracle import bptt_numpy as bp
from tests.golden_io import CELL_KINDS

CHUNKS = [1, 7, 1, 21, 7]


@pytest.mark.parametrize("kind", CELL_KINDS)
def test_oracle_in_chunks_with_carried_state_equals_whole_run(kind):
    B, T, H = 6, sum(CHUNKS), 48
    g = torch.Generator().manual_seed(1000 + len(kind))
    p = {"alpha": (torch.rand(H, generator=g) * 0.14 + 0.82).numpy()}
    if kind in ("adLIF", "RadLIF"):
        p.update(beta=(torch.rand(H, generator=g) * 0.024 + 0.967).numpy(), a=(torch.rand(H, generator=g) * 2 - 1).numpy(),
                 b=(torch.rand(H, generator=g) * 2).numpy())
    if kind in ("RLIF", "RadLIF"):
        p["V"] = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g).numpy()
    Wx = (torch.randn(B, T, H, generator=g) * 1.5 + 0.5).numpy()
    u0, s0 = torch.rand(B, H, generator=g).numpy(), torch.rand(B, H, generator=g).numpy()
    w0 = torch.rand(B, H, generator=g).numpy() if kind in ("adLIF", "RadLIF") else None
    S, U, W = bp.cell_forward(kind, Wx, p, u0, w0, s0)
    assert S.mean() > 0.003
    u, w, s, t0 = u0, w0, s0, 0
    for n in CHUNKS:
        Sc, Uc, Wc = bp.cell_forward(kind, Wx[:, t0:t0 + n], p, u, w, s)
        assert np.array_equal(Sc, S[:, t0:t0 + n]) and np.array_equal(Uc, U[:, t0:t0 + n]), (kind, t0)
        if W is not None:
            assert np.array_equal(Wc, W[:, t0:t0 + n]), (kind, t0)
        u, s, w = Uc[:, -1], Sc[:, -1], (None if Wc is None else Wc[:, -1])
        t0 += n
    assert t0 == T


def test_constructor_refuses_bidirectional_and_training_mode_before_any_device_use():
    import sparch_amd
    from sparch_amd import anns

    torch.manual_seed(3)
    net = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="RadLIF", dropout=0.1, bidirectional=True).eval()
    with pytest.raises(ValueError, match="not causal"):
        sparch_amd.StreamingSNN(net, 4)
    net = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="adLIF", dropout=0.1)
    assert net.training
    with pytest.raises(ValueError, match="training mode"):
        sparch_amd.StreamingSNN(net, 4)
    st = sparch_amd.StreamingSNN(net.eval(), 4, graph=True)     # CPU parameters: fine until the first use
    assert st.steps_seen == 0 and st.batch_size == 4
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.reset()
    ann = anns.ANN((4, None, 12), [16, 5], ann_type="MLP").eval()
    with pytest.raises(ValueError):
        sparch_amd.StreamingSNN(ann, 4)


def test_stream_entry_points_validate_without_launching():
    from sparch_amd._capi import lib
    P = 16   # any non-NULL, 16-byte aligned value: nothing is dereferenced before the checks

    def cell(kind=1, dirs=1, p_drop=0.0, u=P, w=P, s=P):
        return lib.sparch_cell_stream_fwd(kind, 2, dirs, 3, 8, P, None, None, P, P, P, P, u, w, s, 1.0, p_drop, P,
                                          None, None, None)

    assert cell(dirs=2) == -1 and cell(kind=2) == -1 and cell(kind=3) == -1 and cell(p_drop=0.1) == -1
    assert cell(u=None) == -1 and cell(s=None) == -1 and cell(w=None) == -1

    def rec(kind=3, dirs=1, p_drop=0.0, u=P, w=P, s=P, s16=P, prec=0):
        return lib.sparch_rec_cell_stream_fwd(kind, 2, dirs, 3, 8, P, None, None, P, P, P, P, P, P, u, w, s, s16, 1.0,
                                              p_drop, P, None, None, P, 1 << 20, P, 3, None, prec)

    assert rec(dirs=2) == -1 and rec(kind=0) == -1 and rec(kind=1) == -1 and rec(p_drop=0.5) == -1
    assert rec(u=None) == -1 and rec(s=None) == -1 and rec(w=None) == -1 and rec(s16=None) == -1 and rec(prec=7) == -1

    def rstep(kind=3, dirs=1, p_drop=0.0, u=P, w=P, s=P, s16=P, t=0):
        return lib.sparch_rec_cell_step_stream_fwd(kind, 2, dirs, 3, 8, t, P, None, None, P, P, P, P, P, u, w, s, s16,
                                                   1.0, p_drop, P, None, None, None)

    assert rstep(dirs=2) == -1 and rstep(kind=1) == -1 and rstep(p_drop=0.5) == -1 and rstep(t=3) == -1
    assert rstep(u=None) == -1 and rstep(s=None) == -1 and rstep(w=None) == -1 and rstep(s16=None) == -1

    def ro(C=5, u=P, out=P):
        return lib.sparch_readout_stream_fwd(2, 3, C, P, None, None, P, u, out, None)

    assert ro(C=257) == -1 and ro(u=None) == -1 and ro(out=None) == -1
    assert lib.sparch_abi_version() == 5        # additive: the ABI version stays


@pytest.mark.parametrize("N", [399, 400, 16000, 16001])
def test_fbank_stream_plan_over_random_chunkings(N):
    from sparch_amd._capi import lib
    from sparch_amd.streaming import fbank_stream_plan

    rng = np.random.default_rng(N)
    for trial in range(50):
        cuts, left = [], N
        while left > 0:
            n = int(min(left, rng.integers(1, [7, 161, 401, 1000, 5000][trial % 5])))
            cuts.append(n)
            left -= n
        tail, total, made = 0, 0, False
        for n in cuts:
            frames, keep = fbank_stream_plan(tail, n)
            assert 0 <= keep <= 399 and frames >= 0
            assert keep == tail + n - 160 * frames          # every sample is consumed exactly once
            made = made or frames > 0
            if made:
                assert 240 <= keep <= 399
            tail, total = keep, total + frames
        assert total == lib.sparch_fbank_frames(N), (N, cuts[:8])

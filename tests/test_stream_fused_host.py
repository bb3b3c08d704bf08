"""CPU: the fused streaming step (csrc/streamstep.hip, StreamingSNN(fused=True)) — what it refuses, without a device.

* both entry points return SPARCH_EINVAL for every bad argument before anything is dereferenced or launched (the
  pointer value 16, as in test_stream_entry_points_validate_without_launching), are bound in `_capi.PROTOTYPES`, and
  leave the ABI version alone;
* StreamingSNN(fused=True) constructs on CPU parameters and still has no CPU fallback; LayerNorm is refused at
  construction, bidirectional networks and training mode as before.
"""
import pytest
import torch

P = 16   # any non-NULL, 16-byte aligned value: nothing is dereferenced before the checks
Q = 32   # another one


def test_step_entry_points_validate_without_launching():
    from sparch_amd import _capi
    lib = _capi.lib
    assert "sparch_stream_step_fwd" in _capi.PROTOTYPES and "sparch_stream_step_readout" in _capi.PROTOTYPES

    def step(kind=3, B=2, K=12, H=8, ld=8, in_dtype=0, x=P, ldx=12, W=P, scale=None, shift=None, alpha=P, beta=P,
             a=P, b=P, vmask_t=P, u=P, w=P, s_in=P, s_out=Q):
        return lib.sparch_stream_step_fwd(kind, B, K, H, ld, in_dtype, x, ldx, W, None, scale, shift, alpha, beta, a, b,
                                          vmask_t, u, w, s_in, s_out, None, 1.0, None, None)

    assert step(kind=4) == -1 and step(kind=-1) == -1                      # unknown kind
    assert step(in_dtype=2) == -1 and step(in_dtype=-1) == -1              # unknown input type
    for name in ("x", "W", "alpha", "u", "s_in", "s_out"):                 # a required pointer is NULL
        assert step(**{name: None}) == -1, name
    for kind in (1, 3):                                                     # adLIF / RadLIF without an adaptive pointer
        for name in ("beta", "a", "b", "w"):
            assert step(kind=kind, **{name: None}) == -1, (kind, name)
    for kind in (2, 3):                                                     # RLIF / RadLIF
        assert step(kind=kind, vmask_t=None) == -1                         # ... without the masked V
        assert step(kind=kind, s_out=P) == -1                              # ... writing the spikes it reads
    assert step(scale=P) == -1 and step(shift=P) == -1                     # half an affine map
    assert step(ld=7) == -1 and step(ldx=11) == -1                         # strides below the widths
    assert step(B=0) == -1 and step(K=0) == -1 and step(H=0) == -1
    assert step(u=24) == -2 and step(W=20) == -2 and step(s_out=40) == -2  # SPARCH_EALIGN, after every EINVAL check
    assert step(u=24, x=None) == -1

    def ro(B=2, K=12, C=5, x=P, ldx=12, W=P, scale=None, shift=None, alpha=P, u=P, out=P):
        return lib.sparch_stream_step_readout(B, K, C, x, ldx, W, None, scale, shift, alpha, u, out, None)

    assert ro(C=257) == -1 and ro(C=0) == -1 and ro(B=0) == -1 and ro(K=0) == -1 and ro(ldx=11) == -1
    for name in ("x", "W", "alpha", "u", "out"):
        assert ro(**{name: None}) == -1, name
    assert ro(scale=P) == -1 and ro(shift=P) == -1
    assert ro(W=20) == -2
    assert lib.sparch_abi_version() == 5        # additive: the ABI version stays


def test_fused_constructor_on_cpu_parameters_and_its_refusals():
    import sparch_amd

    torch.manual_seed(3)
    net = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="RadLIF", dropout=0.1)
    with pytest.raises(ValueError, match="training mode"):
        sparch_amd.StreamingSNN(net, 4, fused=True)
    for graph in (False, True):
        st = sparch_amd.StreamingSNN(net.eval(), 4, graph=graph, fused=True)     # CPU parameters: fine until the first use
        assert st.fused and st.fused_active and st.steps_seen == 0 and st.batch_size == 4
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            st.reset()
    plain = sparch_amd.StreamingSNN(net, 4)
    assert not plain.fused and not plain.fused_active
    with pytest.raises(AttributeError):
        plain.fused_active = True               # read-only
    ln = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="adLIF", dropout=0.1, normalization="layernorm").eval()
    with pytest.raises(ValueError, match="LayerNorm"):
        sparch_amd.StreamingSNN(ln, 4, fused=True)
    sparch_amd.StreamingSNN(ln, 4)              # (the chunk path takes it)
    bi = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="RadLIF", dropout=0.1, bidirectional=True).eval()
    with pytest.raises(ValueError, match="not causal"):
        sparch_amd.StreamingSNN(bi, 4, fused=True)

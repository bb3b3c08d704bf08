"""GPU: the fused streaming step — StreamingSNN(fused=True), sparch_stream_step_fwd / sparch_stream_step_readout.

1. whole networks against the REFERENCE's dyadic fixtures in chunks of 1, eager and as two alternately replayed graphs;
2. fused chunks of 1 == the eval forward net(x) with BatchNorm, RadLIF / adLIF / LIF;
3. the double buffer: fused and chunked steps mixed, set_state(get_state()) / refresh() behind an odd number of fused
   steps, reset(rows=...) mid-stream;
4. kernel geometries against the oracle on dyadic W and V (every sum exact in any order): smallest shape, a crossed
   row tile, the zero-padded state, H above the persistent kernels' limit, K beyond one staging piece, the headline
   layer; uint8 input; a padded layer feeding the next;
5. real-valued W and V, teacher-forced against the numpy oracle (the project's yardstick for real-valued products);
6. the readout kernel alone at the C ABI against gemm_nt + sparch_readout_stream_fwd;  7. three launches a step.
"""
import pytest
import torch

from tests import stream_cases as cases
from tests.golden_io import DYADIC_LONG
from tests.kit import DEV, sp  # noqa: F401  (sp: a fixture)
from tests.kit import Fn as _Fn
from tests.stream_cases import calls_of, dyadic_net

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ 1. reference-pinned
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["dyadic_RadLIF_none", "dyadic_RLIF_none_bias", DYADIC_LONG])
def test_fused_stream_equals_reference_fixture(sp, name, graph):
    cases.check_fused_stream_equals_reference_fixture(sp, name, graph)


# ------------------------------------------------------------------------------------------ 2. eval BatchNorm
@pytest.mark.parametrize("kind", ["RadLIF", "adLIF", "LIF"])
def test_fused_stream_equals_eval_forward_with_batchnorm(sp, kind):
    cases.check_fused_stream_equals_eval_forward_with_batchnorm(sp, kind)


# ------------------------------------------------------------------------------------------ 3. parity, path mixing
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_fused_and_chunked_steps_alternate_on_one_state(sp, graph):
    cases.check_fused_and_chunked_steps_alternate_on_one_state(sp, graph)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("how", ["set_state", "refresh"])
def test_stream_continues_behind_an_odd_number_of_fused_steps(sp, how, graph):
    cases.check_stream_continues_behind_an_odd_number_of_fused_steps(sp, how, graph)


def test_fused_reset_rows_mid_stream(sp):
    cases.check_fused_reset_rows_mid_stream(sp)


# ------------------------------------------------------------------------------------------ 4. geometry
# (kind, B, K, H, T, seed); the seed of the smallest shape is one at which two of its three neurons spike (five zero-mean
# weights rarely reach the threshold by themselves)
GEOMETRIES = [("LIF", 1, 5, 3, 12, 126), ("adLIF", 33, 70, 100, 12, 270), ("RLIF", 9, 48, 130, 12, 278),
              ("RadLIF", 5, 96, 1536, 12, 1732), ("RadLIF", 2, 1030, 64, 12, 1194), ("RadLIF", 256, 700, 1024, 10, 1824)]


@pytest.mark.parametrize("kind,B,K,H,T,seed", GEOMETRIES)
def test_fused_step_geometries_vs_oracle(sp, kind, B, K, H, T, seed):
    x = (torch.rand(B, T, K, generator=torch.Generator().manual_seed(K)) < 0.3).float()
    cases.check_step_geometry_vs_oracle(sp, kind, B, K, H, T, seed, x)


def test_fused_step_reads_uint8_counts_like_their_fp32_twin(sp):
    cases.check_fused_step_reads_uint8_counts_like_their_fp32_twin(sp)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_padded_layer_feeds_the_next(sp, graph):
    cases.check_padded_layer_feeds_the_next(sp, graph)


# ------------------------------------------------------------------------------------------ 5. real-valued
@pytest.mark.parametrize("inp", ["binary", "real"])
@pytest.mark.parametrize("kind,B,T,K,H", [("RadLIF", 16, 40, 200, 256), ("RLIF", 7, 40, 100, 130),
                                          ("adLIF", 32, 30, 700, 96), ("LIF", 1, 200, 64, 64),
                                          ("RadLIF", 3, 24, 96, 1100)])
def test_fused_step_one_step_ahead_vs_oracle_trajectory(sp, kind, B, T, K, H, inp):
    cases.check_fused_step_one_step_ahead_vs_oracle_trajectory(sp, kind, B, T, K, H, inp)


# ------------------------------------------------------------------------------------------ 6. readout at the C ABI
@pytest.mark.parametrize("B,K,C", [(1, 5, 5), (33, 130, 35), (4, 1024, 256)])
def test_readout_step_kernel_equals_gemm_and_readout_stream_kernel(B, K, C):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    g = torch.Generator().manual_seed(B + K + C)
    W = (torch.randint(-24, 25, (C, K), generator=g).float() / 64.0).to(DEV)
    bias = (torch.randint(-24, 25, (C,), generator=g).float() / 64.0).to(DEV)
    alpha = (torch.rand(C, generator=g) * 0.14 + 0.82).to(DEV)
    scale, shift = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) * 0.2).to(DEV)
    u0 = torch.rand(B, C, generator=g).to(DEV)
    xs = [(torch.rand(B, K, generator=g) < 0.3).float().to(DEV) for _ in range(9)]
    for with_bias, with_affine in ((False, False), (True, True)):
        bs, sc, sh = (bias if with_bias else None), (scale if with_affine else None), (shift if with_affine else None)
        u_ref, out_ref = u0.clone(), torch.zeros(B, C, device=DEV)
        u, out = u0.clone(), torch.zeros(B, C, device=DEV)
        for x in xs:
            Wx, _ = Fn.gemm_nt(x, W, bs)
            check(lib.sparch_readout_stream_fwd(B, 1, C, ptr(Wx), ptr(sc), ptr(sh), ptr(alpha), ptr(u_ref), ptr(out_ref),
                                                Fn._stream()), "sparch_readout_stream_fwd")
            check(lib.sparch_stream_step_readout(B, K, C, ptr(x), K, ptr(W), ptr(bs), ptr(sc), ptr(sh), ptr(alpha),
                                                 ptr(u), ptr(out), Fn._stream()), "sparch_stream_step_readout")
        assert torch.equal(u, u_ref) and torch.equal(out, out_ref)
        assert abs(float(out.sum()) - B * len(xs)) <= 1e-3 * B * len(xs)


# ------------------------------------------------------------------------------------------ 7. launches
def test_fused_step_is_one_library_call_per_layer(sp):
    net, init = dyadic_net(sp, "RadLIF", 4, 64, [64, 64, 20], "none", 13)
    x = (torch.rand(4, 3, 64, generator=torch.Generator().manual_seed(2)) < 0.3).float().to(DEV)
    fused, plain = sp.StreamingSNN(net, 4, fused=True), sp.StreamingSNN(net, 4)
    for st in (fused, plain):
        st.reset(states=init)
        st.step(x[:, 0:1])
    got = calls_of(lambda: fused.step(x[:, 1:2]))
    assert got == ["sparch_stream_step_fwd", "sparch_stream_step_fwd", "sparch_stream_step_readout"], got
    assert len(calls_of(lambda: plain.step(x[:, 1:2]))) > 3
    assert torch.equal(fused.step(x[:, 2:3]), plain.step(x[:, 2:3]))

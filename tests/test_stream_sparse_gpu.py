"""GPU: the event-driven fused streaming step — StreamingSNN(fused=True, sparse=True), sparch_stream_step_sparse_fwd /
sparch_stream_step_sparse_readout (csrc/streamsparse.hip).

The scenarios and assertions are those of tests/test_stream_fused_gpu.py (the check_* bodies of tests/stream_cases.py,
which both files call), run on a module stand-in whose StreamingSNN(fused=True) is StreamingSNN(fused=True,
sparse=True): the reference's dyadic fixtures in chunks of 1 (eager and as two alternately replayed graphs), eval-mode BatchNorm, fused and chunked steps mixed on one state, set_state /
refresh behind an odd number of steps, reset(rows=...) mid-stream (real-valued fresh rows beside binary rows in one
row tile), uint8 counts, a padded layer feeding the next, and the teacher-forced real-valued cases with their bars
unchanged.  Every such test also asserts that the sparse entry points, and not the dense fused ones, were called.
Of its own: the kernel geometries against the oracle on dyadic W and V with lists of every kind (shorter than the
waves, a full list beyond one piece, empty / full / 5 % rows in one row tile, a step without any input), the readout
kernel against its dense twin at the C ABI, and the library calls of one step.
"""
import pytest
import torch

from tests import stream_cases as cases
from tests.golden_io import DYADIC_LONG
from tests.kit import DEV, sp  # noqa: F401  (sp: a fixture)
from tests.kit import Fn as _Fn
from tests.stream_cases import calls_of, dyadic_net, recorded_calls

pytestmark = pytest.mark.gpu

SPARSE = ("sparch_stream_step_sparse_fwd", "sparch_stream_step_sparse_readout")
DENSE = ("sparch_stream_step_fwd", "sparch_stream_step_readout")


class SparseModule:
    """sparch_amd, except that StreamingSNN(fused=True) is the event-driven form (an unfused stream stays as it is)."""

    def __init__(self, sp):
        self._sp, self.made = sp, []

    def __getattr__(self, name):
        return getattr(self._sp, name)

    def StreamingSNN(self, net, batch_size, graph=False, fused=False):
        st = self._sp.StreamingSNN(net, batch_size, graph=graph, fused=fused, sparse=fused)
        if fused:
            self.made.append(st)
        return st


@pytest.fixture
def spx(sp):
    """The stand-in module; behind the test: every fused stream was sparse, and only the sparse entry points ran."""
    mod = SparseModule(sp)
    with recorded_calls(SPARSE + DENSE) as seen:
        yield mod
    assert mod.made and all(st.sparse and st.sparse_active for st in mod.made)
    assert seen and all(n in SPARSE for n in seen), sorted(set(seen))


# ------------------------------------------------------------------------------------------ 1. reference-pinned
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", ["dyadic_RadLIF_none", "dyadic_RLIF_none_bias", DYADIC_LONG])
def test_sparse_stream_equals_reference_fixture(spx, name, graph):
    cases.check_fused_stream_equals_reference_fixture(spx, name, graph)   # (asserts both parities captured and replayed)


# ------------------------------------------------------------------------------------------ 2. eval BatchNorm
@pytest.mark.parametrize("kind", ["RadLIF", "adLIF", "LIF"])
def test_sparse_stream_equals_eval_forward_with_batchnorm(spx, kind):
    cases.check_fused_stream_equals_eval_forward_with_batchnorm(spx, kind)


# ------------------------------------------------------------------------------------------ 3. parity, path mixing
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_sparse_and_chunked_steps_alternate_on_one_state(spx, graph):
    cases.check_fused_and_chunked_steps_alternate_on_one_state(spx, graph)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("how", ["set_state", "refresh"])
def test_stream_continues_behind_an_odd_number_of_sparse_steps(spx, how, graph):
    cases.check_stream_continues_behind_an_odd_number_of_fused_steps(spx, how, graph)


def test_sparse_reset_rows_mid_stream(spx):
    cases.check_fused_reset_rows_mid_stream(spx)


# ------------------------------------------------------------------------------------------ 4. geometry
def _x(B, T, K, density):
    return (torch.rand(B, T, K, generator=torch.Generator().manual_seed(K)) < density).float()


def _x_mixed_rows(B, T, K):
    """One row tile holding an all-zero input row, an all-ones row and a 5 % row."""
    x = (torch.rand(B, T, K, generator=torch.Generator().manual_seed(K)) < 0.05).float()
    x[0], x[1] = 0.0, 1.0
    assert x[2].sum() > 0 and x[2].mean() < 0.1
    return x


def _x_silent_step(B, T, K):
    """Density 0.3, and at t = 4 no input at all, for every row."""
    x = _x(B, T, K, 0.3)
    x[:, 4] = 0.0
    return x


# (kind, B, K, H, T, seed, input); the first six are the shapes (and seeds) of the dense fused test: one partial column
# tile and a list shorter than the waves, a crossed row tile, the padded state and a partial last column tile, H above
# the persistent kernels' limit, a FULL list beyond one piece (density 1.0), the headline layer
GEOMETRIES = [("LIF", 1, 5, 3, 12, 126, 0.3), ("adLIF", 33, 70, 100, 12, 270, 0.3), ("RLIF", 9, 48, 130, 12, 278, 0.3),
              ("RadLIF", 5, 96, 1536, 12, 1732, 0.3), ("RadLIF", 2, 1030, 64, 12, 1194, 1.0),
              ("RadLIF", 256, 700, 1024, 6, 1824, 0.3), ("RadLIF", 3, 200, 70, 12, 31, _x_mixed_rows),
              ("RadLIF", 4, 96, 128, 12, 33, _x_silent_step)]


@pytest.mark.parametrize("kind,B,K,H,T,seed,inp", GEOMETRIES,
                         ids=[f"{g[0]}-{g[1]}-{g[2]}-{g[3]}-{g[6] if isinstance(g[6], float) else g[6].__name__[3:]}"
                              for g in GEOMETRIES])
def test_sparse_step_geometries_vs_oracle(spx, kind, B, K, H, T, seed, inp):
    x = _x(B, T, K, inp) if isinstance(inp, float) else inp(B, T, K)
    cases.check_step_geometry_vs_oracle(spx, kind, B, K, H, T, seed, x)


# ------------------------------------------------------------------------------------------ 5. uint8, 6. padded layers
def test_sparse_step_reads_uint8_counts_like_their_fp32_twin(spx):
    cases.check_fused_step_reads_uint8_counts_like_their_fp32_twin(spx)       # (counts up to 3; equal to the oracle too)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_sparse_padded_layer_feeds_the_next(spx, graph):
    cases.check_padded_layer_feeds_the_next(spx, graph)


# ------------------------------------------------------------------------------------------ 7. real-valued
@pytest.mark.parametrize("inp", ["binary", "real"])
@pytest.mark.parametrize("kind,B,T,K,H", [("RadLIF", 16, 40, 200, 256), ("RLIF", 7, 40, 100, 130),
                                          ("adLIF", 32, 30, 700, 96), ("LIF", 1, 200, 64, 64),
                                          ("RadLIF", 3, 24, 96, 1100)])
def test_sparse_step_one_step_ahead_vs_oracle_trajectory(spx, kind, B, T, K, H, inp):
    """The dense fused test's cases and bars, unchanged: a spike may differ only where the oracle's |u - 1| <= 1e-4;
    flips <= 1e-4 N + 2; oracle rate > 0.003."""
    cases.check_fused_step_one_step_ahead_vs_oracle_trajectory(spx, kind, B, T, K, H, inp)


# ------------------------------------------------------------------------------------------ 8. readout at the C ABI
@pytest.mark.parametrize("B,K,C", [(1, 5, 5), (33, 130, 35), (4, 1024, 256)])
def test_sparse_readout_kernel_equals_the_dense_readout_step(B, K, C):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    g = torch.Generator().manual_seed(B + K + C)
    W = (torch.randint(-24, 25, (C, K), generator=g).float() / 64.0).to(DEV)
    ldc = (C + 3) // 4 * 4
    Wt = torch.nn.functional.pad(W.t(), (0, ldc - C)).contiguous()
    bias = (torch.randint(-24, 25, (C,), generator=g).float() / 64.0).to(DEV)
    alpha = (torch.rand(C, generator=g) * 0.14 + 0.82).to(DEV)
    scale, shift = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) * 0.2).to(DEV)
    u0 = torch.rand(B, C, generator=g).to(DEV)
    xs = [(torch.rand(B, K, generator=g) < 0.3).float().to(DEV) for _ in range(9)]
    xs[3] = torch.zeros(B, K, device=DEV)                                  # a step without any input
    assert sum(float(x.sum()) for x in xs) > 0 and float(xs[3].sum()) == 0
    for with_bias, with_affine in ((False, False), (True, True)):
        bs, sc, sh = (bias if with_bias else None), (scale if with_affine else None), (shift if with_affine else None)
        u_ref, out_ref = u0.clone(), torch.zeros(B, C, device=DEV)
        u, out = u0.clone(), torch.zeros(B, C, device=DEV)
        for x in xs:
            check(lib.sparch_stream_step_readout(B, K, C, ptr(x), K, ptr(W), ptr(bs), ptr(sc), ptr(sh), ptr(alpha),
                                                 ptr(u_ref), ptr(out_ref), Fn._stream()), "sparch_stream_step_readout")
            check(lib.sparch_stream_step_sparse_readout(B, K, C, ptr(x), K, ptr(Wt), ldc, ptr(bs), ptr(sc), ptr(sh),
                                                        ptr(alpha), ptr(u), ptr(out), Fn._stream()),
                  "sparch_stream_step_sparse_readout")
        Fn.check_status()
        assert torch.equal(u, u_ref) and torch.equal(out, out_ref)
        assert abs(float(out.sum()) - B * len(xs)) <= 1e-3 * B * len(xs)


# ------------------------------------------------------------------------------------------ 9. library calls
def test_sparse_step_is_one_library_call_per_layer(sp):
    net, init = dyadic_net(sp, "RadLIF", 4, 64, [64, 64, 20], "none", 13)
    x = (torch.rand(4, 3, 64, generator=torch.Generator().manual_seed(2)) < 0.3).float().to(DEV)
    sparse, dense = sp.StreamingSNN(net, 4, fused=True, sparse=True), sp.StreamingSNN(net, 4, fused=True)
    assert sparse.sparse_active and not dense.sparse_active
    for st in (sparse, dense):
        st.reset(states=init)
        st.step(x[:, 0:1])
    got = calls_of(lambda: sparse.step(x[:, 1:2]))
    assert got == ["sparch_stream_step_sparse_fwd", "sparch_stream_step_sparse_fwd",
                   "sparch_stream_step_sparse_readout"], got
    assert calls_of(lambda: dense.step(x[:, 1:2])) == ["sparch_stream_step_fwd", "sparch_stream_step_fwd",
                                                       "sparch_stream_step_readout"]
    out_s, out_d = sparse.step(x[:, 2:3]), dense.step(x[:, 2:3])
    assert float(out_s.sum()) > 0 and torch.equal(out_s, out_d)

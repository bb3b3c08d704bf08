"""
The fp64 restatement of the axonal delays (tests/delay_numpy.py) checked against itself, without a GPU:
  * d = 0 is the identity; shifts compose inside T; g_x is the adjoint of y, exactly on integer data;
  * the rounding of the parameter (ties to even, clamp, NaN) and the gate;
  * the sign of the delay's gradient: one spike, a target d + 1 steps later, loss sum (y - y*)^2  =>  g_theta = -4,
    so gradient descent moves the delay towards the target;
  * the chunked form with a carried history equals the whole-sequence shift.
"""
import numpy as np
import pytest

from tests import delay_numpy as dn


def _ints(seed, *shape):
    return np.random.default_rng(seed).integers(-5, 6, shape).astype(np.float64)


def test_steps_round_half_to_even_and_clamp():
    theta = np.array([0.0, 0.5, 1.5, 2.5, 3.5, -0.2, -7.0, 4.49, 4.51, 9.0, np.nan, 255.5], np.float32)
    assert dn.steps(theta, 4).tolist() == [0, 0, 2, 2, 4, 0, 0, 4, 4, 4, 0, 4]
    assert dn.steps(theta, 255).tolist()[-3:] == [9, 0, 255]
    assert dn.gate(theta, 4).tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert dn.gate(np.array([4.0, 4.0001, -0.0], np.float32), 4).tolist() == [1, 0, 1]


@pytest.mark.parametrize("lengths", [None, [9, 1, 4]])
def test_zero_delay_is_the_identity(lengths):
    x = _ints(1, 3, 9, 5)
    mask = np.arange(9)[None, :, None] < np.asarray(lengths or [9] * 3)[:, None, None]
    for theta in (np.zeros(5), np.full(5, 0.5), np.full(5, -3.0)):
        assert np.array_equal(dn.forward(x, theta, 4, lengths), x * mask)
        assert np.array_equal(dn.backward_x(x, theta, 4, lengths), x * mask)


def test_shifts_compose_inside_T():
    x = _ints(2, 2, 12, 6)
    d1, d2 = np.array([0, 1, 2, 3, 5, 7.0]), np.array([4, 0, 3, 9, 6, 5.0])
    twice = dn.forward(dn.forward(x, d1, 12), d2, 12)
    assert np.array_equal(twice, dn.forward(x, d1 + d2, 24))
    assert not twice[:, :, 3].any() and not twice[:, :, 5].any()      # 3 + 9 and 7 + 5 reach T: whole columns are zero
    assert twice[:, :, 0].any()


@pytest.mark.parametrize("lengths", [None, [9, 1, 4]])
def test_gx_is_the_adjoint_of_y(lengths):
    theta = np.array([0, 1, 2.5, 3.5, 8, 11, -1, 4.2])
    x, g = _ints(3, 3, 9, 8), _ints(4, 3, 9, 8)
    lhs = float((dn.forward(x, theta, 11, lengths) * g).sum())
    rhs = float((x * dn.backward_x(g, theta, 11, lengths)).sum())
    assert lhs == rhs and lhs != 0.0


def test_gy_on_padded_steps_is_ignored():
    theta, lengths = np.array([1.0, 2.0, 0.0]), [5, 2]
    x, g = _ints(5, 2, 6, 3), _ints(6, 2, 6, 3)
    dirty = g.copy()
    dirty[0, 5:], dirty[1, 2:] = np.nan, 1e30
    assert np.array_equal(dn.backward_x(g, theta, 3, lengths), dn.backward_x(dirty, theta, 3, lengths))
    a, b = dn.backward_theta(g, x, theta, 3, lengths), dn.backward_theta(dirty, x, theta, 3, lengths)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("d,t0", [(0, 3), (2, 0), (3, 4)])
def test_sign_pin_one_spike_target_one_step_later(d, t0):
    """y = x delayed by d has its spike at t0 + d, the target at t0 + d + 1; L = sum (y - y*)^2, g_y = 2 (y - y*) is +2 at
    the spike and -2 one step later; g_theta = 2 * (0 - 1) + (-2) * (1 - 0) = -4: descent makes the delay larger."""
    T, D = 12, 5
    x = np.zeros((1, T, 1))
    x[0, t0, 0] = 1.0
    theta = np.array([float(d)])
    y, target = dn.forward(x, theta, D), dn.forward(x, theta + 1, D)
    assert y[0, t0 + d, 0] == 1 and target[0, t0 + d + 1, 0] == 1 and y.sum() == target.sum() == 1
    g_theta, mag = dn.backward_theta(2 * (y - target), x, theta, D)
    assert g_theta.tolist() == [-4.0] and mag.tolist() == [4.0]
    lr = 0.1
    assert abs((theta - lr * g_theta)[0] - (d + 1)) < abs(theta[0] - (d + 1))
    # the rule is a FORWARD difference, y(d + 1) - y(d): it is the exact change of the loss for one more step of delay
    loss = lambda y_: float(((y_ - target) ** 2).sum())  # noqa: E731
    assert loss(dn.forward(x, theta + 1, D)) - loss(y) == -2.0     # (the linearisation, -4, overshoots the quadratic)


def test_the_gate_zeroes_clamped_delays():
    x, g = _ints(7, 2, 7, 4) + 0.5, _ints(8, 2, 7, 4) + 0.5
    theta = np.array([-0.5, 0.0, 3.0, 3.5])
    g_theta, mag = dn.backward_theta(g, x, theta, 3)
    assert g_theta[0] == 0.0 and g_theta[3] == 0.0 and g_theta[1] != 0.0 and g_theta[2] != 0.0 and (mag > 0).all()


@pytest.mark.parametrize("sizes", [[1] * 9, [2, 2, 2, 2, 1], [5, 4], [9]])
def test_the_chunked_form_is_the_whole_sequence_shift(sizes):
    x = np.random.default_rng(9).integers(0, 2, (3, 9, 6)).astype(np.uint16)
    theta = np.array([0, 1, 2.5, 3.5, 4, 7.0])
    cuts = np.cumsum([0] + sizes)
    chunks = [x[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    got = np.concatenate(dn.stream(chunks, theta, 4), axis=1)
    assert got.dtype == x.dtype and np.array_equal(got, dn.forward(x, theta, 4))

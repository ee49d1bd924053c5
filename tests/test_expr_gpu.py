"""rxhip_expr_eval: the expression interpreter (csrc/expr.hpp) on the device, on its own — one program per opcode and three composites at 130 points
(two wavefronts and a ragged third).  Values (plain mode) within 4 ulp of numpy's, Jacobians (forward-mode duals) within 1e-12·max(1, |entry|) of
hand-written ones, a point outside sqrt's domain gives NaN at that point only."""
import numpy as np
import pytest

import nlssm_ref as R
import rxhip

pytestmark = pytest.mark.gpu

N = 130
RNG = np.random.default_rng(11)
X2 = RNG.uniform(0.2, 2.5, (N, 2))    # positive: every unary function is inside its domain

# name -> (f on tracers / numpy, hand-written Jacobian rows [[∂f0/∂x0, ∂f0/∂x1], [∂f1/∂x0, ∂f1/∂x1]])
OPS = {
    "add": (lambda x: [x[0] + x[1], x[1] + 1.5], lambda a, b: [[1, 1], [0, 1]]),
    "sub": (lambda x: [x[0] - x[1], 1.5 - x[1]], lambda a, b: [[1, -1], [0, -1]]),
    "mul": (lambda x: [x[0] * x[1], 3.0 * x[1]], lambda a, b: [[b, a], [0, 3]]),
    "div": (lambda x: [x[0] / x[1], 2.0 / x[0]], lambda a, b: [[1 / b, -a / b ** 2], [-2 / a ** 2, 0]]),
    "neg": (lambda x: [-x[0], -(x[0] * x[1])], lambda a, b: [[-1, 0], [-b, -a]]),
    "sqrt": (lambda x: [np.sqrt(x[0]), np.sqrt(x[0] * x[1])], lambda a, b: [[0.5 / np.sqrt(a), 0], [0.5 * b / np.sqrt(a * b), 0.5 * a / np.sqrt(a * b)]]),
    "exp": (lambda x: [np.exp(x[0]), np.exp(-x[1])], lambda a, b: [[np.exp(a), 0], [0, -np.exp(-b)]]),
    "log": (lambda x: [np.log(x[0]), np.log(x[0] * x[1])], lambda a, b: [[1 / a, 0], [1 / a, 1 / b]]),
    "sin": (lambda x: [np.sin(x[0]), np.sin(x[0] * x[1])], lambda a, b: [[np.cos(a), 0], [b * np.cos(a * b), a * np.cos(a * b)]]),
    "cos": (lambda x: [np.cos(x[0]), np.cos(x[0] + x[1])], lambda a, b: [[-np.sin(a), 0], [-np.sin(a + b), -np.sin(a + b)]]),
    "tanh": (lambda x: [np.tanh(x[0]), np.tanh(x[0] - x[1])], lambda a, b: [[1 - np.tanh(a) ** 2, 0], [1 - np.tanh(a - b) ** 2, -(1 - np.tanh(a - b) ** 2)]]),
    "const_var_out": (lambda x: [x[1], 2.25], lambda a, b: [[0, 1], [0, 0]]),
}


def hold(value, jac, want, want_jac):
    assert np.max(np.abs(value - want) / np.spacing(np.abs(want))) <= 4
    assert np.max(np.abs(jac - want_jac) / np.maximum(1.0, np.abs(want_jac))) < 1e-12


@pytest.mark.parametrize("name", list(OPS))
def test_one_program_per_op(name):
    f, jac = OPS[name]
    value, J = rxhip.expr_eval(rxhip.trace(f, 2), X2)
    want = np.array([np.asarray(f(list(p)), dtype=np.float64) for p in X2])
    want_jac = np.array([np.asarray(jac(*p), dtype=np.float64) for p in X2])
    hold(value, J, want, want_jac)


def positive_four(x, M=np):
    """DIV, SQRT and LOG on [1.5, 3]⁴, every term positive: a distance in ulp to numpy means something only where nothing cancels (two correct
    libms may differ by an ulp in a log, and a difference of two such terms shows that ulp magnified)"""
    return [M.sqrt(x[0]) / x[1], M.log(x[2]) * x[3], x[0] / M.sqrt(x[2] * x[3]), M.log(x[1] * x[0]) + M.sqrt(x[3])]


def positive_four_jac(x):
    a, b, c, e = x
    return np.array([[0.5 / (np.sqrt(a) * b), -np.sqrt(a) / b ** 2, 0, 0], [0, 0, e / c, np.log(c)],
                     [1 / np.sqrt(c * e), 0, -0.5 * a / (c * np.sqrt(c * e)), -0.5 * a / (e * np.sqrt(c * e))], [1 / a, 1 / b, 0, 0.5 / np.sqrt(e)]])


@pytest.mark.parametrize("name", ["pendulum", "coupled", "positive_four"])
def test_composites(name):
    if name == "positive_four":
        d, f, jac, x = 4, positive_four, positive_four_jac, RNG.uniform(1.5, 3.0, (N, 4))
    else:
        d, f, jac = R.FUNCS[name]
        x = RNG.uniform(-2.0, 2.0, (N, d))
    value, J = rxhip.expr_eval(rxhip.trace(lambda t: f(t, np), d), x)
    hold(value, J, np.array([f(p, np) for p in x]), np.array([jac(p) for p in x]))


def test_a_program_at_the_caps_runs_its_tangents_in_passes():
    """16 live slots at d = 4: 24 LDS rows leave 4 components per pass, so the 4 tangents need two passes and 9 sigma points would need three"""
    def wide(x):
        vs = [np.sin(x[i % 4] * float(i + 2)) for i in range(12)]
        acc = vs[0]
        for a, b in zip(vs[1:], vs[:-1]):
            acc = acc + a * b
        return [acc, x[1] * acc, x[2] + acc, np.cos(x[3])]
    p = rxhip.trace(wide, 4)
    assert p.n_slots >= 13
    x = RNG.uniform(-1.0, 1.0, (N, 4))
    value, J = rxhip.expr_eval(p, x)
    want = np.array([wide(list(q)) for q in x], dtype=np.float64)
    # a signed sum of 12 sines and 11 products of them, every term at most 1 in size: 35 operations of at most 2 ulp of 1 each, not ulp of the (cancelled) sum
    assert np.max(np.abs(value - want)) < 35 * 2 * np.spacing(13.0)   # (every output is below 13 in size)
    h = 1e-6   # central differences of the float64 program: the passes must agree on every column
    for k in range(4):
        e = np.zeros(4); e[k] = h
        fd = (np.array([wide(list(q + e)) for q in x], dtype=np.float64) - np.array([wide(list(q - e)) for q in x], dtype=np.float64)) / (2 * h)
        assert np.max(np.abs(J[:, :, k] - fd)) < 1e-7, k


def test_a_point_outside_the_domain_is_nan_at_that_point_only():
    x = X2.copy()
    x[[5, 64, 129], 0] = -1.0
    value, J = rxhip.expr_eval(rxhip.trace(lambda t: [np.sqrt(t[0]), t[1]], 2), x)
    bad = np.zeros(N, dtype=bool)
    bad[[5, 64, 129]] = True
    assert np.all(np.isnan(value[bad, 0])) and np.all(np.isnan(J[bad, 0, 0]))
    assert np.array_equal(value[~bad, 0], np.sqrt(x[~bad, 0])) and np.array_equal(value[:, 1], x[:, 1]) and np.all(np.isfinite(J[~bad]))
    assert np.array_equal(J[:, 1], np.tile([0.0, 1.0], (N, 1)))

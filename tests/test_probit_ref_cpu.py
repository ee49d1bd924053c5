"""The CPU restatement of the probit state-space engine (tests/probit_ref.py) against the reference's own known answer
(test/models/statespace/probit_tests.jl:33-78) and against itself: the message-passing form of the parallel-EP iteration is held to an
independent dense form (tridiagonal precision + diag(w), inverted), and the tilted moments to brute-force quadrature."""
import numpy as np
import pytest

import probit_ref as R

# probit_tests.jl:33-58 with StableRNG(123): sixteen 0s, then 1 0 1 0 1 0 1 1 0 1 0 1 1, then eleven 1s
REFERENCE_Y = [0] * 16 + [1, 0, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 1] + [1] * 11
# free energy after parallel-EP iterations 1 … 10 on that data (numpy restatement, dense form)
PER_ITERATION = [49.9782300505, 16.1765807194, 15.6498987462, 15.6462691376, 15.6462370819, 15.6462369750, 15.6462369651, 15.6462369673,
                 15.6462369672, 15.6462369672]


@pytest.fixture(scope="module")
def reference_run():
    _, y = R.reference_data()
    return y, R.run_messages(y, **R.REFERENCE_MODEL, iterations=10), R.run_dense(y, **R.REFERENCE_MODEL, iterations=10)


def test_reference_data_regenerates():
    x, y = R.reference_data()
    assert len(y) == 40 and x[0] == -2.0
    assert [int(v) for v in y] == REFERENCE_Y


def _hold(msg, dense):
    (m1, v1, f1), (m2, v2, f2) = msg, dense
    assert np.max(np.abs(m1 - m2) / np.maximum(np.abs(m2), np.sqrt(v2))) < 1e-10
    assert np.max(np.abs(v1 - v2) / v2) < 1e-10
    assert np.max(np.abs(f1 - f2) / np.abs(f2)) < 1e-10


def test_messages_equal_dense_on_the_reference_case(reference_run):
    _, msg, dense = reference_run
    _hold(msg, dense)


@pytest.mark.parametrize("seed", range(20))
def test_messages_equal_dense_on_random_small_models(seed):
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(1, 13))
    a, c, q, v0, m0 = rng.uniform(0.5, 1.1), rng.normal(0.0, 0.3), rng.uniform(0.05, 2.0), rng.uniform(0.2, 20.0), rng.normal(0.0, 1.0)
    y = (rng.random(T) < 0.5).astype(np.float64)
    y[rng.random(T) < 0.25] = np.nan
    if seed % 5 == 0:
        y[0] = y[-1] = np.nan
    if np.all(np.isnan(y)):   # a series without any observation has free energy exactly 0: a relative bound means nothing there
        y[T // 2] = 1.0
    iters = int(rng.integers(1, 6))
    _hold(R.run_messages(y, a, c, q, m0, v0, iters), R.run_dense(y, a, c, q, m0, v0, iters))


def test_free_energy_reaches_the_golden_value(reference_run):
    _, (_, _, fe), (_, _, fe_dense) = reference_run
    assert len(fe) == 10
    print("last free energy", repr(fe[-1]), "relative to golden", abs(fe[-1] - R.GOLDEN_FE) / R.GOLDEN_FE)
    assert abs(fe[-1] - R.GOLDEN_FE) < 1e-8 * R.GOLDEN_FE
    assert abs(fe_dense[-1] - R.GOLDEN_FE) < 1e-8 * R.GOLDEN_FE


def test_per_iteration_values(reference_run):
    _, (_, _, fe), _ = reference_run
    assert np.max(np.abs(fe - np.array(PER_ITERATION))) < 1e-9


def test_free_energy_never_rises_by_more_than_the_reference_allows(reference_run):
    _, (_, _, fe), _ = reference_run
    assert np.all(np.diff(fe) <= 1e-6)   # probit_tests.jl:76


def _quadrature(m, v, y):
    """Tilted mean / variance of N(x; m, v) Φ(s x) by the trapezoid rule on m ± (12 σ + |m|), weights in the log domain: meaningful in
    the far tail too (the tilted density moves at most |m| away from m, and log Φ is evaluated directly)."""
    s = 2.0 * y - 1.0
    x = m + (12.0 * np.sqrt(v) + abs(m)) * np.linspace(-1.0, 1.0, 400001)
    lw = -0.5 * (x - m) ** 2 / v + R.log_ndtr(s * x)
    w = np.exp(lw - lw.max())
    z = w.sum()
    mean = (w * x).sum() / z
    return mean, (w * (x - mean) ** 2).sum() / z


@pytest.mark.parametrize("y", [0.0, 1.0])
@pytest.mark.parametrize("v", [0.01, 0.5, 1.0, 7.0, 100.0])
@pytest.mark.parametrize("m", [-40.0, -6.0, -1.5, 0.0, 0.3, 2.0, 8.0, 40.0])
def test_tilted_moments_against_quadrature(m, v, y):
    mt, vt = R.tilted(m, v, y)
    xi, w = R.site_update(m, v, y)
    assert np.isfinite(mt) and np.isfinite(vt) and vt > 0 and np.isfinite(xi) and w > 0
    qm, qv = _quadrature(m, v, y)
    assert abs(mt - qm) < 1e-9 * max(1.0, abs(qm)), (mt, qm)
    assert abs(vt - qv) < 1e-9 * qv, (vt, qv)


def test_mills_ratio_is_finite_and_accurate_where_phi_underflows():
    r = float(R.mills(-40.0))
    # asymptotic series r(z) = |z| / (1 − 1/z² + 3/z⁴ − 15/z⁶ + 105/z⁸ …), |z| = 40: terms fall below 1e-16 at the fifth
    z2 = 1600.0
    assert abs(r - 40.0 / (1.0 - 1.0 / z2 + 3.0 / z2 ** 2 - 15.0 / z2 ** 3 + 105.0 / z2 ** 4)) < 1e-12 * r

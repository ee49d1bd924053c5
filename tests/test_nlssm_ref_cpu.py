"""The numpy restatement of the nonlinear state-space engine (tests/nlssm_ref.py) against its 50-digit twin (tests/nlssm_mp.py) on the grid the device
is tested on, against the project's oracle on a linear f, and the monotonicity of the unknown-noise free energy.  CPU only."""
import numpy as np
import pytest

import nlssm_mp as M
import nlssm_ref as R
import rxoracle


@pytest.fixture(scope="module")
def measured():
    return M.measure()


def test_restatement_stays_within_a_hundredth_of_the_contract_against_50_digits(measured):
    """the float64 restatement alone, over every series of every case of tests/test_nlssm_gpu.py (about ten CPU minutes of mpmath, spread over the
    CPUs): a hundredth of each contract bound, so that a device result within the contract of the restatement is within 1.01 contracts of the truth"""
    print("float64 restatement against 50 digits:", measured)
    for k, v in measured.items():
        assert v <= R.BOUNDS[k] / 100, (k, v)


def test_recorded_envelope_is_the_measured_one(measured):
    for k, v in measured.items():
        assert M.ENVELOPE[k] <= R.BOUNDS[k] / 100 and v <= 1.02 * M.ENVELOPE[k], (k, v, M.ENVELOPE[k])   # (recorded to two digits, rounded up)


def test_grid_covers_what_it_claims():
    grid = R.case_grid()
    ids = [g[0] for g in grid]
    assert len(set(ids)) == len(ids)
    ds = {R.FUNCS[c["name"]][0] for _, c, *_ in grid}
    assert ds == {1, 2, 4}
    assert {c["y"].shape[:2] for _, c, *_ in grid} == {(1, 1), (5, 3), (37, 70)}
    for method in ("linearization", "unscented"):
        mine = [(c, mode, it) for _, c, m, mode, it in grid if m == method]
        assert {bool(c["Q"].any()) for c, _, _ in mine} == {True, False}
        assert {c["per_series"] for c, _, _ in mine} == {True, False}
        assert {c["y"].shape[2] < R.FUNCS[c["name"]][0] for c, _, _ in mine} == {True, False}
        assert {(c["noise"] is not None, mode, it) for c, mode, it in mine} == {(False, "filter", 1), (False, "smooth", 1), (True, "filter", 1), (True, "filter", 5)}
    for _, c, *_ in grid:
        y = c["y"]
        assert np.isnan(y[0, 0]).all() and np.isnan(y[-1, 0]).all()
        if y.shape[1] > 1:
            assert np.isnan(y[:, 1]).all()
        if y.shape[0] == 37:
            assert 0.1 < np.isnan(y[:, 2:, 0]).mean() < 0.3


@pytest.mark.parametrize("name", ["linear2", "linear4"])
@pytest.mark.parametrize("method", ["linearization", "unscented"])
def test_linear_f_is_the_kalman_filter_and_the_rts_smoother(name, method):
    """f(x) = A x: both delta-node approximations are exact, so filter, smoother and free energy equal the oracle's (posteriors 1e-6 relative, −log p(y)
    1e-8 relative: the project's contract)"""
    A = R.LINEAR[name]
    d = A.shape[0]
    rng = np.random.default_rng(d)
    B, P, Q = np.eye(d)[:2] + 0.1 * rng.standard_normal((2, d)), R.spd(rng, d, 0.2), R.spd(rng, 2, 0.5)
    m0, V0 = rng.standard_normal(d), R.spd(rng, d, 1.0)
    y = rng.standard_normal((40, 2))
    rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    om, oc, nll = rxoracle.lgssm_kalman_rts(A, B, P, Q, m0, V0, y, prior_through_transition=True)
    sm = R.run_series(name, y, m0, V0, P, B, R=Q, method=method, mode="smooth")
    assert rel(sm["mean"], om) < 1e-6 and rel(sm["cov"], oc) < 1e-6 and abs(sm["fe"] - nll) < 1e-8 * abs(nll)
    fm, fc, _, _ = rxoracle.lgssm_filter(A, B, P, Q, m0, V0, y, prior_through_transition=True)
    fl = R.run_series(name, y, m0, V0, P, B, R=Q, method=method, mode="filter")
    assert rel(fl["mean"], fm) < 1e-6 and rel(fl["cov"], fc) < 1e-6 and abs(fl["fe"] - nll) < 1e-8 * abs(nll)


@pytest.mark.parametrize("method", ["linearization", "unscented"])
def test_unknown_noise_free_energy_does_not_increase_over_the_iterations_of_a_step(method):
    """every iteration of a step is a pair of exact coordinate updates of q(x_t) and q(τ) on the step's own free energy"""
    case = R.make_case(7, "pendulum", 37, 3, 1, False, True, False)
    out = R.run_case(case, method, "filter", 8)
    fe = out["fe_iter"]                      # [T][series][iterations]
    obs = ~np.isnan(case["y"][:, :, 0])
    assert obs.sum() > 40
    steps = np.diff(fe[obs], axis=1)
    assert np.all(steps <= 1e-12 * np.maximum(1.0, np.abs(fe[obs][:, :-1]))), steps.max()
    assert np.all(fe[~obs] == 0.0)

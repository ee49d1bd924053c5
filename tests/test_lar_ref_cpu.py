"""The CPU restatement of the latent autoregressive engine (tests/lar_ref.py) held to what does not depend on it: its dense form (numpy's inverse
of the whole Λ) against its banded form (the device's recursions in plain Python), the reference's known answers on its regenerated data, the
monotone free energy, and the C oracle's Kalman/RTS smoother on the companion-form chain when θ and γ are pinned."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lar_ref as R
import rxoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _non_increasing(fe):
    return bool(np.all(np.diff(fe) <= 1e-9 * np.abs(fe[1:])))


@pytest.mark.parametrize("missing", [0.0, 0.25])
@pytest.mark.parametrize("p", range(1, 9))
def test_dense_equals_banded(p, missing):
    for T in sorted({1, 2, p, p + 1, 23}):
        y, m = R.random_case(1000 + 10 * p + T, T, 2, p, missing)
        dense = R.run_batch(y, **m, iterations=3, want_cond=True)
        band = R.run_batch(y, **m, iterations=3, banded=True)
        assert dense["cond"] <= 1e8
        e = R.contract_errors(band, dense)
        zs = np.sqrt(dense["band"][..., 0])
        ez = float(np.max(np.abs(band["z_mean"] - dense["z_mean"]) / zs))
        assert max(e["mean"], e["par"], e["fe"], ez) < 1e-10, (T, e, ez)
        assert _non_increasing(dense["fe"]) and _non_increasing(band["fe"])


@pytest.fixture(scope="module")
def golden_runs():
    y, z = R.reference_data()
    return y, z, {p: R.run(y, 15, **R.model(p, 5.0)) for p in R.RECORDED_FE}


def test_golden_file_equals_a_fresh_regeneration(tmp_path):
    y, z = R.reference_data()
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_lar_golden
    finally:
        sys.path.pop(0)
    yy, zz = make_lar_golden.lar()
    assert np.array_equal(yy, y) and np.array_equal(zz, z) and y.shape == (500,)
    assert np.allclose(y[:4], [0.67220215, 1.73669239, 0.63298751, -0.4117014], atol=5e-9) and y[499] == 0.30362488134838256


def test_recorded_and_golden_free_energies(golden_runs):
    _, _, runs = golden_runs
    for p, (first, last) in R.RECORDED_FE.items():
        fe = runs[p]["fe"]
        print(p, repr(float(fe[0])), repr(float(fe[-1])))
        assert abs(fe[0] - first) < 1e-8 * first and abs(fe[-1] - last) < 1e-8 * last
        assert np.all(np.diff(fe) < 0)                                            # strictly down over the 15 iterations
    for p, want in R.GOLDEN_FE.items():                                           # lar_tests.jl:171, :202
        assert abs(runs[p]["fe"][-1] - want) < 0.01


def test_every_random_case_is_well_conditioned_and_its_free_energy_never_rises():
    n = 0
    for group in R.CASES.values():
        for spec in group:
            y, m, iters, shared = R.case(spec)
            r = R.run_batch(y, **m, iterations=iters, share_parameters=shared, want_cond=True)
            assert r["cond"] <= 1e8, (spec, r["cond"])
            assert _non_increasing(r["fe"]), (spec, r["fe"])
            n += 1
    assert n == sum(len(g) for g in R.CASES.values())


def test_shared_parameters_with_one_series_is_the_unshared_run():
    y, m = R.random_case(7, 12, 1, 3)
    a = R.run_batch(y, **m, iterations=4)
    b = R.run_batch(y, **m, iterations=4, share_parameters=True)
    for k in ("x_mean", "x_cov", "theta_mean", "theta_cov", "gamma_shape", "gamma_rate"):
        assert np.array_equal(a[k], b[k])
    assert np.allclose(a["fe"], b["fe"], rtol=1e-13)


@pytest.mark.parametrize("p,T", [(1, 30), (2, 25), (4, 20), (8, 15)])
def test_pinned_parameters_give_the_kalman_smoother(p, T):
    """θ pinned by a prior precision of 1e12 and γ by Gamma(1e12, 1e12/γ): the state marginals of the first iteration are those of the linear
    Gaussian chain x[t] = A x[t-1] + w, A = companion(θ), state noise diag(1/γ, 1e-12 …), y[t] = x[t]₁ + v — computed by the C oracle's Kalman/RTS smoother,
    which shares no code with the restatement.  1e-6 standard deviations."""
    rng = np.random.default_rng(300 + p)
    theta = 0.5 * rng.standard_normal(p) / p
    gamma, tau = 3.0, 5.0
    a_ = rng.standard_normal((p, p))
    w0 = a_ @ a_.T / p + np.eye(p)
    m0 = rng.standard_normal(p)
    y = rng.standard_normal(T)
    m = R.model(p, tau, prior_theta=(theta, 1e12 * np.eye(p)), prior_gamma=(1e12, 1e12 / gamma), prior_x0=(m0, w0))
    A = np.zeros((p, p))
    A[0] = theta
    A[1:, :-1] = np.eye(p - 1)
    Q = np.diag([1.0 / gamma] + [1e-12] * (p - 1))
    B = np.zeros((1, p))
    B[0, 0] = 1.0
    om, oc, _ = rxoracle.lgssm_kalman_rts(A, B, Q, np.array([[1.0 / tau]]), m0, np.linalg.inv(w0), y[:, None], prior_through_transition=True)
    for banded in (False, True):
        r = R.run(y, 1, banded=banded, **m)
        sd = np.sqrt(np.einsum("tii->ti", oc))
        em = float(np.max(np.abs(r["x_mean"] - om) / sd))
        ec = float(np.max(np.abs(r["x_cov"] - oc) / (sd[:, :, None] * sd[:, None, :])))
        print(f"p = {p}: mean {em:.2e} sd, cov {ec:.2e}")
        assert em < 1e-6 and ec < 1e-6

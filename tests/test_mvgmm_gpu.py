"""GPU parity tests of the multivariate Gaussian mixture engine (MvNormal components, Wishart precisions) against the
oracle, every iteration; model and driver shaped after test/models/mixtures/gmm_multivariate_tests.jl.
The contract is mvgmm_ref.hold: per (iteration, component), means 1e-6 posterior standard deviations (and 1e-6 of the largest mean), cov and
V 1e-6 relative to √(ref_aa · ref_bb), nu and alpha 1e-6 relative, free energy 1e-8 relative, responsibilities 1e-9 absolute.  The cases
are mvgmm_ref.CASES["lane"]; the edges of the lane path have a file of their own, tests/test_mvgmm_lane_gpu.py."""
import numpy as np
import pytest

import rxhip
import rxoracle

import mvgmm_ref
from mvgmm_ref import CASES, Case, contract_errors, hold, setup

pytestmark = pytest.mark.gpu


def run_engine(y, pri, init, iters, resp=True):
    """one run of a fresh engine, as the dict hold() takes (with the raw history under "raw")"""
    with rxhip.MvGMMEngine(y.shape[0], *pri, *init, materialize_responsibilities=resp) as eng:
        eng.set_data(y)
        eng.run(iters, True)
        return dict(eng.history(), fe=eng.free_energy(), resp=eng.responsibilities() if resp else None)


@pytest.mark.parametrize("d,K,N,iters", [c[:4] for c in CASES["lane"]])
def test_matches_oracle_every_iteration(d, K, N, iters):
    c = Case(d, K, N, iters)
    y, pri, init, ref = mvgmm_ref.case(c)
    got = run_engine(y, pri, init, iters)
    hold(got, mvgmm_ref.oracle(c), f"lane vs oracle {c[:4]}")
    hold(got, ref, f"lane vs restatement {c[:4]}")
    fe = got["fe"]
    assert np.all(np.diff(fe) < 1e-6 * np.abs(fe[-1]))  # free energy non-increasing (gmm_multivariate_tests.jl:139)


def test_reference_shaped_run_recovers_the_clusters():
    """K = 3, d = 2, N = 500, 25 iterations (gmm_multivariate_tests.jl:80-149): estimated means point at the true ones."""
    rng = np.random.default_rng(43)
    ang = 2 * np.pi / 3 * np.arange(3)
    means = 50.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    rot = [np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) for a in ang]
    covs = [R @ np.diag([10.0, 20.0]) @ R.T for R in rot]
    y = np.stack([rng.multivariate_normal(means[k], covs[k]) for k in rng.integers(0, 3, 500)])
    mu0, S0, nu0, V0, al0 = setup(3, 2, means, seed=42)
    spec = rxhip.multivariate_gaussian_mixture(mu0, S0, nu0, V0)
    res = rxhip.infer(model=spec, data={"y": y}, iterations=25, free_energy=True,
                      initialization={"m": rxhip.MvNormalMeanCovariance(mu0, S0), "w": rxhip.Wishart(nu0, V0), "s": rxhip.Dirichlet(np.ones(3))})
    assert res.free_energy.shape == (25,) and np.all(np.diff(res.free_energy) < 1e-6 * abs(res.free_energy[-1]))
    em = res.posteriors["m"].mean[-1]
    for k in range(3):
        assert np.linalg.norm(em[k] / np.linalg.norm(em[k]) - means[k] / np.linalg.norm(means[k])) < 0.1
    ohist, ofe, _ = rxoracle.mvgmm_vmp(y, mu0, S0, nu0, V0, al0, rxoracle.mvgmm_pack(mu0, S0, nu0, V0, np.ones(3)), 25)
    assert abs(res.free_energy[-1] - ofe[-1]) < 1e-8 * abs(ofe[-1])


def test_univariate_engine_agrees_for_d1():
    """Wishart(ν, V) in one dimension is Gamma(ν/2, 1/(2V)): the two device engines give the same answers."""
    rng = np.random.default_rng(8)
    N, K = 5000, 4
    mus = np.array([-9.0, -2.0, 3.0, 11.0])
    y = mus[rng.integers(0, K, N)] + rng.standard_normal(N)
    mu0, v0, a0, b0, al0 = mus + 1.0, np.full(K, 1e2), np.full(K, 0.5), np.full(K, 0.25), np.ones(K)
    with rxhip.GMMEngine(N, mu0, v0, a0, b0, al0, mu0, np.ones(K), np.ones(K), np.ones(K), np.ones(K)) as e1:
        e1.set_data(y); e1.run(7, True)
        h1, f1 = e1.history(), e1.free_energy()
    with rxhip.MvGMMEngine(N, mu0[:, None], v0[:, None, None], 2 * a0, (1 / (2 * b0))[:, None, None], al0, mu0[:, None],
                           np.ones((K, 1, 1)), 2 * np.ones(K), 0.5 * np.ones((K, 1, 1)), np.ones(K)) as e2:
        e2.set_data(y[:, None]); e2.run(7, True)
        h2, f2 = e2.history(), e2.free_energy()
    assert np.max(np.abs(f1 - f2) / np.abs(f1)) < 1e-9
    # the univariate history [it][mean m, var m, shape, rate, alpha][K] in the multivariate layout
    as1 = dict(mean=h1[:, 0][..., None], cov=h1[:, 1][..., None, None], nu=2 * h1[:, 2], V=(1 / (2 * h1[:, 3]))[..., None, None], alpha=h1[:, 4])
    e = contract_errors(h2, as1)
    print(" ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["mean_global"] < 1e-9 and e["nu"] < 1e-9 and e["V"] < 1e-8   # V per (iteration, component): at d = 1 that is the rate, element-wise


def test_error_paths():
    I = np.eye(2)
    K = 2
    args = (np.zeros((K, 2)), np.tile(I, (K, 1, 1)), np.full(K, 3.0), np.tile(I, (K, 1, 1)), np.ones(K))
    with pytest.raises(rxhip.RxHipError) as ei:  # Wishart degrees of freedom must exceed d − 1
        rxhip.MvGMMEngine(10, args[0], args[1], np.full(K, 0.5), args[3], args[4], *args)
    assert ei.value.status == 3
    bad = np.tile(np.array([[1.0, 2.0], [2.0, 1.0]]), (K, 1, 1))
    with pytest.raises(rxhip.RxHipError) as ei:  # indefinite prior covariance
        rxhip.MvGMMEngine(10, args[0], bad, args[2], args[3], args[4], *args)
    assert ei.value.status == 3
    with pytest.raises(rxhip.RxHipError) as ei:  # d = 3 with more than 8 components has no device schedule
        rxhip.MvGMMEngine(10, np.zeros((9, 3)), np.tile(np.eye(3), (9, 1, 1)), np.full(9, 4.0), np.tile(np.eye(3), (9, 1, 1)), np.ones(9),
                          np.zeros((9, 3)), np.tile(np.eye(3), (9, 1, 1)), np.full(9, 4.0), np.tile(np.eye(3), (9, 1, 1)), np.ones(9))
    assert ei.value.status == 2

"""The nonlinear state-space engine (include/rxhip.h rxhip_nlssm_desc, csrc/nlssm_kernels.hpp, csrc/expr.hpp) on the device against its CPU
restatement tests/nlssm_ref.py, itself held to 50 digits on these cases (tests/test_nlssm_ref_cpu.py): d ∈ {1, 2, 4}, T ∈ {1, 5, 37}, series ∈
{1, 3, 70}, both methods, Q = 0 and Q > 0, d_y < d and d_y = d, 20 % missing, a series with nothing observed, first and last step missing, shared
and per-series priors, FILTER with known and unknown noise at 1 and 5 iterations, SMOOTH, both layouts, a second run bit for bit.  Contract: means
1e-6 posterior sd, covariances 1e-6·√(V_ii V_jj), Gamma shape and rate 1e-6 relative, free energy 1e-8·max(1, |F|) per series."""
import os

import numpy as np
import pytest

import nlssm_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu

GRID = R.case_grid()


def engine(case, method, mode, **kw):
    d, f, _ = R.FUNCS[case["name"]]
    T, S, _ = case["y"].shape
    noise = case["noise"]
    return rxhip.NonlinearSSMEngine(lambda x: f(x, np), d, T, case["m0"], case["V0"], case["H"], R=None if noise else case["R"], Q=case["Q"], noise_prior=noise,
                                    method=method, mode=mode, n_series=S, per_series=case["per_series"], **kw)


def results(eng, unknown, layout="time_chain"):
    mean, cov = eng.marginals(layout=layout)
    out = dict(mean=mean, cov=cov, fe=eng.free_energy_per_chain())
    if unknown:
        out["shape"], out["rate"] = eng.noise()
    return out


@pytest.mark.parametrize("cid, case, method, mode, iterations", GRID, ids=[g[0] for g in GRID])
def test_engine_equals_the_restatement(cid, case, method, mode, iterations):
    unknown = case["noise"] is not None
    ref = R.run_case(case, method, mode, iterations)
    with engine(case, method, mode) as eng:
        eng.set_data(case["y"])
        eng.run(iterations=iterations, free_energy=True)
        got = results(eng, unknown)
        err = R.errors(got, ref, unknown)
        print(cid, err)
        for k, v in err.items():
            assert v < R.BOUNDS[k], (k, v)
        total = eng.free_energy()
        assert np.all(total == total[-1]) and abs(total[-1] - ref["fe"].sum()) < 1e-8 * max(1.0, np.abs(ref["fe"]).sum())
        if case["y"].shape[1] > 1:
            assert got["fe"][1] == 0.0                       # series 1 observes nothing
        # the other layout: data in and marginals out as [series][T]
        eng.set_data(np.ascontiguousarray(case["y"].transpose(1, 0, 2)), layout="chain_time")
        eng.run(iterations=iterations, free_energy=True)     # … which is also the second run on the handle: bit for bit
        again = results(eng, unknown)
        for k in got:
            assert np.array_equal(again[k], got[k]), k
        mean_ct, cov_ct = eng.marginals(layout="chain_time")
        assert np.array_equal(mean_ct, got["mean"].transpose(1, 0, 2)) and np.array_equal(cov_ct, got["cov"].transpose(1, 0, 2, 3))
        eng.run(iterations=iterations, free_energy=False)    # without the free energy: the same posteriors
        assert np.array_equal(eng.marginals()[0], got["mean"])


@pytest.mark.parametrize("name", ["linear2", "linear4"])
@pytest.mark.parametrize("method", ["linearization", "unscented"])
def test_linear_f_equals_the_linear_gaussian_engine(name, method):
    A = R.LINEAR[name]
    d = A.shape[0]
    rng = np.random.default_rng(d)
    B, P, Q = np.eye(d)[:2] + 0.1 * rng.standard_normal((2, d)), R.spd(rng, d, 0.2), R.spd(rng, 2, 0.5)
    m0, V0 = rng.standard_normal(d), R.spd(rng, d, 1.0)
    T, C = 37, 70
    y = rng.standard_normal((T, C, 2))
    f = R.FUNCS[name][1]
    with rxhip.LGSSMEngine(A, B, P, Q, m0, V0, T=T, n_chains=C, prior_through_transition=True) as lin:
        lin.set_data(y)
        for mode in ("smooth", "filter"):
            if mode == "smooth":
                lin.run(iterations=1, free_energy=True)
            else:
                lin.run_filter(free_energy=True)
            lm, lc = lin.marginals()
            lfe = lin.free_energy_per_chain()
            with rxhip.NonlinearSSMEngine(lambda x: f(x, np), d, T, m0, V0, B, R=Q, Q=P, method=method, mode=mode, n_series=C) as eng:
                eng.set_data(y)
                eng.run(free_energy=True)
                got = results(eng, False)
                want_fe = lfe if mode == "smooth" else fe_smooth        # the filter's −log p(y) is the smoother's
                err = R.errors(got, dict(mean=lm, cov=lc, fe=want_fe), False)
                print(name, method, mode, err)
                assert err["mean"] < 1e-6 and err["cov"] < 1e-6 and err["fe"] < 1e-8
            if mode == "smooth":
                fe_smooth = lfe


def test_a_value_that_is_not_finite_is_a_status_with_the_step_and_series():
    """f = sqrt(x0) − 1.5: series 1 of 3 starts at 9 → 1.5 → −0.275, so the third application (step 2, counted from 0) is outside sqrt's domain; the
    others start at 1e6 and stay inside for T = 4.  The run is refused with a text, nothing faults, and the handle then answers good data."""
    f = lambda x: [np.sqrt(x[0]) - 1.5]
    y = np.full((4, 3, 1), np.nan)
    for method, mode in (("linearization", "filter"), ("unscented", "filter"), ("linearization", "smooth"), ("unscented", "smooth")):
        with rxhip.NonlinearSSMEngine(f, 1, 4, np.array([[1e6], [9.0], [1e6]]), np.full((3, 1, 1), 1e-4), [1.0], R=[[1.0]], method=method, mode=mode, n_series=3,
                                      per_series=True) as eng:
            eng.set_data(y)
            for _ in range(2):                               # SMOOTH: a fresh record buffer the first time, the stopped lane's stale records the second
                with pytest.raises(rxhip.RxHipError) as ei:
                    eng.run(free_energy=True)
                assert ei.value.status == _lib.ERR_NONFINITE_FE and "nlssm" in str(ei.value) and "step 2 of series 1" in str(ei.value), (method, mode, str(ei.value))
                eng.sync()                                   # the status word was cleared: nothing is left pending


def test_the_handle_answers_good_data_after_a_refused_run():
    R.FUNCS["_sqrt"] = (1, lambda x, M=np: [M.sqrt(x[0]) - 1.5], lambda x: np.array([[0.5 / np.sqrt(x[0])]]))
    try:
        # with these observations the filter is pulled toward 400 and stays in the domain (means 203 … 699, variances 0.5: unit Q, R and V0 keep the
        # update well conditioned); with nothing observed series 1 leaves the domain at step 2
        case = dict(name="_sqrt", y=np.full((4, 3, 1), 400.0), m0=np.array([[1e6], [9.0], [1e6]]), V0=np.full((3, 1, 1), 1.0), Q=np.ones((1, 1)),
                    H=np.ones((1, 1)), R=np.ones((1, 1)), noise=None, per_series=True)
        with engine(case, "linearization", "filter") as eng:
            eng.set_data(np.full((4, 3, 1), np.nan))
            with pytest.raises(rxhip.RxHipError, match="step 2 of series 1"):
                eng.run()
            eng.set_data(case["y"])
            eng.run()
            err = R.errors(results(eng, False), R.run_case(case, "linearization", "filter", 1), False)
            assert all(v < R.BOUNDS[k] for k, v in err.items()), err
    finally:
        del R.FUNCS["_sqrt"]


def test_a_singular_prediction_is_the_non_spd_status_in_the_smoother():
    with rxhip.NonlinearSSMEngine(lambda x: [x[0], x[0]], 2, 4, np.zeros(2), np.eye(2), [1.0, 0.0], R=[[1.0]], mode="smooth") as eng:
        eng.set_data(np.zeros((4, 1, 1)))
        with pytest.raises(rxhip.RxHipError) as ei:
            eng.run()
        assert ei.value.status == _lib.ERR_NOT_POSDEF
    with rxhip.NonlinearSSMEngine(lambda x: [x[0], x[0]], 2, 4, np.zeros(2), np.eye(2), [1.0, 0.0], R=[[1.0]], mode="filter") as eng:
        eng.set_data(np.zeros((4, 1, 1)))
        eng.run()                                            # the extended filter itself needs no inverse of P
        assert np.all(np.isfinite(eng.marginals()[0]))


PEND = lambda x: [x[0] + R.DT * x[1], x[1] - R.G * R.DT * np.sin(x[0])]


@pytest.mark.parametrize("method", [rxhip.Linearization(), rxhip.Unscented()])
def test_infer_equals_the_engine_class(method):
    rng = np.random.default_rng(5)
    T, S = 50, 2
    y = 0.5 + rng.standard_normal((S, T))
    name = "unscented" if isinstance(method, rxhip.Unscented) else "linearization"
    m0, V0, H = np.array([0.5, 0.0]), 0.01 * np.eye(2), np.array([[1.0, 0.0]])
    known = rxhip.nonlinear_ssm(PEND, 2, m0, V0, process_cov=1e-4 * np.eye(2), obs_matrix=H, obs_cov=[[1.0]], method=method)
    res = rxhip.infer(model=known, data={"y": y[..., None]}, free_energy=True)
    with rxhip.NonlinearSSMEngine(PEND, 2, T, m0, V0, H, R=[[1.0]], Q=1e-4 * np.eye(2), method=name, mode="smooth", n_series=S) as eng:
        eng.set_data(y[..., None], layout="chain_time")
        eng.run(free_energy=True)
        mean, cov = eng.marginals(layout="chain_time")
        assert np.array_equal(res.posteriors["x"].mean, mean) and np.array_equal(res.posteriors["x"].cov, cov) and np.array_equal(res.free_energy, eng.free_energy())
    unknown = rxhip.nonlinear_ssm(PEND, 2, m0, V0, obs_matrix=H, obs_precision_prior=rxhip.GammaShapeScale(1.0, 100.0), method=method)
    res = rxhip.infer(model=unknown, data={"y": y[..., None]}, autoupdates=True, keephistory=T, iterations=5, free_energy=True)
    with rxhip.NonlinearSSMEngine(PEND, 2, T, m0, V0, H, noise_prior=(1.0, 0.01), method=name, mode="filter", n_series=S) as eng:
        eng.set_data(y[..., None], layout="chain_time")
        eng.run(iterations=5, free_energy=True)
        mean, cov = eng.marginals(layout="chain_time")
        shape, rate = eng.noise()
        assert np.array_equal(res.history["x"].mean, mean) and np.array_equal(res.history["x"].cov, cov)
        assert np.array_equal(res.history["τ"].shape, shape.T) and np.array_equal(res.history["τ"].rate, rate.T)
        assert np.array_equal(res.free_energy_history, eng.free_energy()) and np.all(shape[-1] == 1.0 + 0.5 * T)
    one = rxhip.infer(model=unknown, data={"y": y[0]}, autoupdates=True, iterations=5)
    assert one.history["x"].mean.shape == (T, 2) and np.array_equal(one.history["x"].mean, mean[0]) and np.array_equal(one.history["τ"].rate, rate[:, 0])
    with pytest.raises(rxhip.RxHipError, match="smoothing with unknown observation noise"):
        rxhip.infer(model=unknown, data={"y": y[0]})
    with pytest.raises(ValueError, match="keephistory must be 50"):
        rxhip.infer(model=unknown, data={"y": y[0]}, autoupdates=True, keephistory=3)


@pytest.mark.parametrize("method", ["linearization", "unscented"])
def test_the_papers_pendulum_is_tracked(method):
    """the regenerated data set of the reference's example (tests/golden/pendulum_stablerng42.npz), streamed as there: 5 iterations per observation,
    q(τ) from Gamma(shape 1, scale 100).  The device equals the restatement, and at least 95 % of the true angles lie within 3 posterior sd."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pendulum_stablerng42.npz"))
    y, truth = g["y"][1:, None, None], g["states"][1:]          # the reference's first observation is a placeholder, not a draw
    case = dict(name="pendulum", y=y, m0=np.array([0.5, 0.0]), V0=0.01 * np.eye(2), Q=np.zeros((2, 2)), H=np.array([[1.0, 0.0]]), R=None, noise=(1.0, 0.01),
                per_series=False)
    ref = R.run_case(case, method, "filter", 5)
    with engine(case, method, "filter") as eng:
        eng.set_data(y)
        eng.run(iterations=5, free_energy=True)
        got = results(eng, True)
    err = R.errors(got, ref, True)
    print(method, err)
    # the contract itself for both methods (unscented: 999 steps at Q = 0 take the float64 restatement past a HUNDREDTH of the contract against 50 digits,
    # tests/nlssm_mp.py — 1.3e-8 sd after 300 steps — so device and restatement may each sit that far from the truth, far inside the contract)
    assert all(v < R.BOUNDS[k] for k, v in err.items()), err
    for out in (ref, got):
        inside = np.abs(out["mean"][:, 0, 0] - truth[:, 0]) < 3.0 * np.sqrt(out["cov"][:, 0, 0, 0])
        assert inside.mean() >= 0.95

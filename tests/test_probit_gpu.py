"""The probit state-space engine (include/rxhip.h rxhip_probit_desc, csrc/probit_kernels.hpp) against its CPU restatement tests/probit_ref.py.
The project's contract: posterior means within 1e-6 posterior standard deviations, variances within 1e-6 relative, free energy within 1e-8
relative — per iteration and per series."""
import numpy as np
import pytest

import probit_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu


def _hold(mean, var, ref_mean, ref_var):
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
    em = float(np.max(np.abs(mean - ref_mean) / np.sqrt(ref_var)))
    ev = float(np.max(np.abs(var - ref_var) / ref_var))
    print(f"mean err {em:.3e} sd, var rel {ev:.3e}")
    assert em < 1e-6 and ev < 1e-6, (em, ev)


def _hold_fe(fe, ref):
    ef = float(np.max(np.abs(fe - ref) / np.abs(ref)))
    print(f"fe rel {ef:.3e}")
    assert np.all(np.isfinite(fe)) and ef < 1e-8, ef


def _fe_per_series_and_iteration(make, y, iters, layout="time_chain"):
    """The ABI returns per-series values of the LAST iteration: one run per iteration count gives every (iteration, series)."""
    out = []
    for n in range(1, iters + 1):
        with make() as eng:
            eng.set_data(y if layout == "time_chain" else np.ascontiguousarray(y.T), layout=layout)
            eng.run(n, True)
            out.append(eng.free_energy_per_chain())
    return np.array(out)


@pytest.fixture(scope="module")
def reference_case():
    _, y = R.reference_data()
    return y, R.run_messages(y, **R.REFERENCE_MODEL, iterations=10)


def test_reference_case(reference_case):
    y, (rm, rv, rfe) = reference_case
    p = R.REFERENCE_MODEL
    with rxhip.ProbitEngine(40, p["a"], p["c"], p["q"], p["m0"], p["v0"]) as eng:
        eng.set_data(y[:, None])
        eng.run(10, True)
        mean, var = eng.marginals()
        fe, fes = eng.free_energy(), eng.free_energy_per_chain()
        counters = eng.counters()
    assert mean.shape == (41, 1) and fe.shape == (10,)
    _hold(mean[:, 0], var[:, 0], rm, rv)
    _hold_fe(fe, rfe)
    assert fes[0] == fe[-1]
    print("last free energy", repr(fe[-1]))
    assert abs(fe[-1] - R.GOLDEN_FE) < 1e-8 * R.GOLDEN_FE   # probit_tests.jl:77
    assert np.all(np.diff(fe) <= 1e-6)                       # probit_tests.jl:76
    assert all(counters[k] > 0 for k in ("rule_calls", "products", "marginals"))


@pytest.fixture(scope="module")
def batch_case():
    rng = np.random.default_rng(20)
    T, C, iters = 37, 130, 6
    a, c, q, m0, v0 = float(rng.uniform(0.7, 1.0)), float(rng.normal(0, 0.2)), float(rng.uniform(0.02, 0.5)), float(rng.normal()), float(rng.uniform(0.5, 20))
    y = (rng.random((T, C)) < 0.5).astype(np.float64)
    y[rng.random((T, C)) < 0.05] = np.nan
    y[:, 0] = 0.0                      # all 0
    y[:, 1] = 1.0                      # all 1
    y[:, 2] = np.arange(T) % 2         # alternating
    miss = rng.random(T) < 0.3         # 30 % missing, the first and the last step among them
    miss[0] = miss[-1] = True
    y[:, 3] = np.where(miss, np.nan, (rng.random(T) < 0.5).astype(np.float64))
    mean, var, _ = R.run_batch(y, a, c, q, m0, v0, iters)
    fe = np.array([R.run_batch(y, a, c, q, m0, v0, n)[2][-1] for n in range(1, iters + 1)])   # [iteration][series] (the n-th iterate's last value)
    return (T, C, iters, a, c, q, m0, v0), y, mean, var, fe


@pytest.mark.parametrize("layout", ["time_chain", "chain_time"])
def test_batch_of_130_series(batch_case, layout):
    (T, C, iters, a, c, q, m0, v0), y, rm, rv, rfe = batch_case
    make = lambda: rxhip.ProbitEngine(T, a, c, q, m0, v0, n_series=C)
    with make() as eng:
        eng.set_data(y if layout == "time_chain" else np.ascontiguousarray(y.T), layout=layout)
        eng.run(iters, True)
        mean, var = eng.marginals(layout=layout)
        fe_tot, fe_last = eng.free_energy(), eng.free_energy_per_chain()
    if layout == "chain_time":
        mean, var = mean.T, var.T
    _hold(mean, var, rm, rv)
    _hold_fe(fe_last, rfe[-1])
    _hold_fe(fe_tot, rfe.sum(axis=1))
    _hold_fe(_fe_per_series_and_iteration(make, y, iters, layout), rfe)   # per iteration AND per series


@pytest.mark.parametrize("T", [1, 2])
def test_shortest_chains(T):
    rng = np.random.default_rng(T)
    y = (rng.random((T, 3)) < 0.5).astype(np.float64)
    y[0, 2] = np.nan
    rm, rv, rfe = R.run_batch(y, 0.9, 0.2, 0.3, -0.5, 2.0, 4)
    make = lambda: rxhip.ProbitEngine(T, 0.9, 0.2, 0.3, -0.5, 2.0, n_series=3)
    with make() as eng:
        eng.set_data(y)
        eng.run(4, True)
        mean, var = eng.marginals()
    _hold(mean, var, rm, rv)
    fe = _fe_per_series_and_iteration(make, y, 4)
    obs = ~np.all(np.isnan(y), axis=0)   # (T = 1 with its only step missing: the free energy is exactly 0, nothing to be relative to)
    _hold_fe(fe[:, obs], rfe[:, obs])
    assert np.max(np.abs(fe[:, ~obs])) < 1e-12 if np.any(~obs) else True


def test_lower_tail():
    y = np.ones((5, 1))
    rm, rv, rfe = R.run_messages(y[:, 0], 1.0, 0.0, 1e-4, -40.0, 0.01, 5)
    with rxhip.ProbitEngine(5, 1.0, 0.0, 1e-4, -40.0, 0.01) as eng:
        eng.set_data(y)
        eng.run(5, True)
        mean, var = eng.marginals()
        fe = eng.free_energy()
    _hold(mean[:, 0], var[:, 0], rm, rv)
    _hold_fe(fe, rfe)


def test_n_iterations_in_one_run_is_the_nth_iterate_and_free_energy_does_not_touch_the_posteriors(reference_case):
    y, _ = reference_case
    p = R.REFERENCE_MODEL
    for n in (1, 3):
        rm, rv, rfe = R.run_messages(y, **p, iterations=n)
        with rxhip.ProbitEngine(40, p["a"], p["c"], p["q"], p["m0"], p["v0"]) as eng:
            eng.set_data(y[:, None])
            eng.run(n, True)
            mean, var = eng.marginals()
            fe = eng.free_energy()
            eng.run(n, False)
            mean0, var0 = eng.marginals()
        _hold(mean[:, 0], var[:, 0], rm, rv)
        _hold_fe(fe, rfe)
        assert np.array_equal(mean, mean0) and np.array_equal(var, var0)   # bit for bit


def test_infer_end_to_end(reference_case):
    y, (rm, rv, rfe) = reference_case
    res = rxhip.infer(model=rxhip.probit_ssm(1.0, 0.1, 0.01, 0.0, 100.0), data={"y": y}, iterations=10, free_energy=True)
    assert res.error is None and res.posteriors["x"].mean.shape == (41,) and res.free_energy.shape == (10,)
    _hold(res.posteriors["x"].mean, res.posteriors["x"].var, rm, rv)
    _hold_fe(res.free_energy, rfe)
    assert abs(res.free_energy[-1] - R.GOLDEN_FE) < 1e-8 * R.GOLDEN_FE
    # a batch: [T, n_series]
    res2 = rxhip.infer(model=rxhip.probit_ssm(1.0, 0.1, 0.01, 0.0, 100.0), data={"y": np.stack([y, 1.0 - y], axis=1)}, iterations=2, free_energy=True)
    assert res2.posteriors["x"].mean.shape == (41, 2) and res2.free_energy.shape == (2,)


@pytest.mark.parametrize("kw,word", [(dict(q=0.0), "variance q"), (dict(q=-1.0), "variance q"), (dict(v0=0.0), "variance v0"), (dict(n_gh=0), "n_gh"), (dict(n_gh=33), "n_gh")])
def test_bad_descriptor_is_a_status_with_a_text(kw, word):
    args = dict(a=1.0, c=0.0, q=0.1, m0=0.0, v0=1.0, n_gh=32)
    args.update(kw)
    with pytest.raises(rxhip.RxHipError) as ei:
        rxhip.ProbitEngine(4, **args)
    assert ei.value.status == _lib.ERR_BADARG and word in str(ei.value)


@pytest.mark.parametrize("bad", [0.5, 2.0, -1.0, np.inf])
def test_bad_observation_is_a_status_with_a_text(bad):
    y = np.array([[0.0], [1.0], [bad], [np.nan]])
    with rxhip.ProbitEngine(4, 1.0, 0.0, 0.1, 0.0, 1.0) as eng:
        with pytest.raises(rxhip.RxHipError) as ei:
            eng.set_data(y)
        assert ei.value.status == _lib.ERR_BADARG and "neither 0, 1 nor NaN" in str(ei.value)
        with pytest.raises(rxhip.RxHipError) as ei:   # … and the refused data is not run on
            eng.run(1, True)
        assert ei.value.status == _lib.ERR_STATE
        eng.set_data(np.array([[0.0], [1.0], [1.0], [np.nan]]))   # the engine stays usable
        eng.run(2, True)
        assert np.all(np.isfinite(eng.free_energy()))

"""The binomial regression engine (include/rxhip.h rxhip_binreg_desc, csrc/binreg_kernels.hpp) against its CPU restatement tests/binreg_ref.py: q(β) and
the free energy of every iteration and problem — at the project's contract (binreg_ref.hold: means 1e-6 posterior standard deviations, covariances
1e-6 relative to √(v_i v_j), free energy 1e-8 relative).  Every random case keeps cond W ≤ 1e8 (asserted in tests/test_binreg_ref_cpu.py), so the
contract has two decades over cond·ε; the host build of the same arithmetic sits near 1e-12 (tests/test_binreg_host.py).
Shapes: d = 1, 2, 4 on the lane path and 5 (first MFMA dimension), 16 (a full tile), 17 (first with a second column tile), 32 (the last) on the
matrix cores; N = 1, a tile of points − 1, a tile, a tile + 1, and chunk cap × tile + 1, at which the first workgroup runs its grid-stride loop
twice (the constants come from rxhip_binreg_schedule and are asserted against binreg_ref's)."""
import numpy as np
import pytest

import binreg_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu

DIMS = (1, 2, 4, 5, 16, 17, 32)


def _run(X, y, n, m, iters, fe=True, parts=("X", "n", "y")):
    C, N, d = X.shape
    with rxhip.BinomialRegressionEngine(N, d, m["prior_xi"], m["prior_precision"], m["init"], n_problems=C) as eng:
        for p in parts:
            {"X": eng.set_regressors, "n": eng.set_trials, "y": eng.set_observations}[p]({"X": X, "n": n, "y": y}[p])
        eng.run(iters, fe)
        mean, cov, fep = eng.parameters()
        return dict(mean=mean, cov=cov, fe=fep, total=eng.free_energy() if fe else None, last=eng.free_energy_per_chain() if fe else None)


def _non_increasing(fe):
    return bool(np.all(np.diff(fe, axis=0) <= 1e-9 * np.abs(fe[1:])))


def _check(X, y, n, m, iters):
    ref = R.run_batch(X, y, n, **m, iterations=iters)
    got = _run(X, y, n, m, iters)
    e = R.hold(got, ref)
    tot = ref["fe"].sum(axis=1)
    et = float(np.max(np.abs(got["total"] - tot) / np.maximum(1.0, np.abs(tot))))      # rxhip_get_free_energy: per iteration, summed over the problems
    assert et < 1e-8, et
    assert np.array_equal(got["last"], got["fe"][-1])                                  # rxhip_get_free_energy_per_chain: per problem, last iteration
    assert _non_increasing(got["fe"]) and _non_increasing(got["total"][:, None]), got["fe"]
    return got, e


def _same(a, b, keys=("mean", "cov")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- 1. dimensions and sizes ---------------------------------------------------------------------------------------------------------------------------
def test_schedule_constants():
    for d, (tile, cap) in [(1, (R.SMALL_TILE, R.SMALL_CAP)), (4, (R.SMALL_TILE, R.SMALL_CAP)), (5, (R.MFMA_TILE, R.MFMA_CAP)), (32, (R.MFMA_TILE, R.MFMA_CAP))]:
        assert rxhip.BinomialRegressionEngine.schedule(tile * cap, d) == (tile, cap)
        assert rxhip.BinomialRegressionEngine.schedule(tile * cap + 1, d) == (tile, cap)         # one tile more than workgroups: the first takes two
        assert rxhip.BinomialRegressionEngine.schedule(tile + 1, d) == (tile, 2)
        assert rxhip.BinomialRegressionEngine.schedule(1, d) == (tile, 1)
    assert rxhip.BinomialRegressionEngine.schedule(10, 33) == (0, 0)


@pytest.mark.parametrize("d", DIMS)
def test_sizes_around_a_tile(d):
    """N = 1, tile − 1, tile, tile + 1"""
    for N in R.sizes_for(d)[:4]:
        _check(*R.size_case(d, N))


@pytest.mark.parametrize("d", [4, 16, 32])
def test_a_workgroup_strides_over_two_tiles(d):
    """N = cap·tile + 1: workgroup 0 of each kernel family (lane path, one column tile, two) takes a second tile; 16.8 MB of X at d = 4 and d = 32"""
    N = R.sizes_for(d)[4]
    tile, chunks = rxhip.BinomialRegressionEngine.schedule(N, d)
    assert (N + tile - 1) // tile == chunks + 1
    _check(*R.size_case(d, N))


# ---- 2. degenerate rows, missing values, batches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", R.CASES["degenerate"], ids=lambda s: f"d{s[3]}")
def test_degenerate_rows_on_the_device(spec):
    """problem 0 holds an all-zero row (c = 0), a row scaled by 1e-9, a row scaled to c ≈ 1500, a missing y and n_i = 0"""
    X, y, n, m, iters = R.case(spec)
    assert not X[0, 0].any() and np.isnan(y[0, 3]) and n[0, 4] == 0.0
    _check(X, y, n, m, iters)


@pytest.mark.parametrize("spec", R.CASES["batch"], ids=lambda s: f"d{s[3]}")
def test_a_problem_in_a_batch_has_the_bits_of_the_problem_alone(spec):
    X, y, n, m, iters = R.case(spec)
    assert X.shape[0] == 5
    got, _ = _check(X, y, n, m, iters)
    alone = _run(X[2:3], y[2:3], n[2:3], m, iters)
    for k in ("mean", "cov", "fe"):
        assert np.array_equal(got[k][:, 2], alone[k][:, 0]), k


@pytest.mark.parametrize("spec", R.CASES["batch"], ids=lambda s: f"d{s[3]}")
def test_two_runs_and_runs_without_the_free_energy_give_the_same_bits(spec):
    X, y, n, m, iters = R.case(spec)
    a, b, c = _run(X, y, n, m, iters), _run(X, y, n, m, iters, parts=("y", "X", "n")), _run(X, y, n, m, iters, fe=False)
    assert _same(a, b, ("mean", "cov", "fe", "total")) and _same(a, c)
    C, N, d = X.shape
    with rxhip.BinomialRegressionEngine(N, d, m["prior_xi"], m["prior_precision"], m["init"], n_problems=C) as eng:   # a second run of one engine starts over
        eng.set_data(X, y, n)
        eng.run(2, False)
        eng.run(iters, True)
        mean, cov, fe = eng.parameters()
        assert np.array_equal(mean, a["mean"]) and np.array_equal(cov, a["cov"]) and np.array_equal(fe, a["fe"])
        assert eng.counters() == dict(rule_calls=iters * C * (N + 1), products=iters * C * N, marginals=iters * C * (N + 1))


def test_custom_initial_q():
    X, y, n, m, iters = R.case((360, 150, 2, 5, 0.1, False, 4))
    r = np.random.default_rng(9)
    A = r.standard_normal((5, 5))
    m = dict(m, init=(r.standard_normal(5), 0.3 * np.eye(5) + 0.1 * A @ A.T))
    _check(X, y, n, m, iters)


# ---- 3. the reference's test through infer -------------------------------------------------------------------------------------------------------------
def test_reference_test_through_infer():
    """binomialreg_tests.jl:97-106: the 20 simulations as one batch, 100 iterations; F_end < F_first per problem, coverage ≥ 0.8 per feature"""
    X, y, n = R.reference_batch()
    res = rxhip.infer(model=rxhip.binomial_regression(np.zeros(2), np.eye(2)), data={"X": X, "y": y, "n_trials": n}, iterations=100, free_energy=True)
    mean, cov = res.posteriors["β"]
    fe = res.free_energy
    assert mean.shape == (100, 20, 2) and cov.shape == (100, 20, 2, 2) and fe.shape == (100, 20)
    assert np.all(fe[-1] < fe[0]) and _non_increasing(fe)
    cover = R.coverage(mean[-1], cov[-1])
    print("coverage", cover)
    assert np.all(cover >= 0.8)
    R.hold(dict(mean=mean, cov=cov, fe=fe), R.run_batch(X, y, n, **R.model(2), iterations=100))


def test_golden_data_through_infer():
    X, y, n = R.golden_data()
    res = rxhip.infer(model=rxhip.binomial_regression(np.zeros(2), np.eye(2)), data={"X": X, "y": y, "n_trials": n}, iterations=100, free_energy=True)
    mean, cov = res.posteriors["β"]
    assert mean.shape == (100, 2) and cov.shape == (100, 2, 2) and res.free_energy.shape == (100,)
    print("F after iterations 1 and 100:", repr(res.free_energy[0]), repr(res.free_energy[-1]))
    for got, want in zip((res.free_energy[0], res.free_energy[-1]), R.RECORDED_FE):
        assert abs(got - want) < 1e-8 * want


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _status(fn):
    with pytest.raises(rxhip.RxHipError) as ei:
        fn()
    assert str(ei.value)
    return ei.value.status


def test_refusals():
    I2 = np.eye(2)
    assert _status(lambda: rxhip.BinomialRegressionEngine(10, 33, np.zeros(33), np.eye(33))) == _lib.ERR_BADARG
    assert _status(lambda: rxhip.BinomialRegressionEngine(0, 2, np.zeros(2), I2)) == _lib.ERR_BADARG
    assert _status(lambda: rxhip.BinomialRegressionEngine(10, 2, np.zeros(2), I2, n_problems=0)) == _lib.ERR_BADARG
    assert _status(lambda: rxhip.BinomialRegressionEngine(10, 2, np.zeros(2), np.array([[1.0, 2.0], [2.0, 1.0]]))) == _lib.ERR_BADARG      # not positive definite
    assert _status(lambda: rxhip.BinomialRegressionEngine(10, 2, np.zeros(2), np.array([[1.0, 0.5], [0.0, 1.0]]))) == _lib.ERR_BADARG      # not symmetric
    assert _status(lambda: rxhip.BinomialRegressionEngine(10, 2, np.zeros(2), I2, init=(np.zeros(2), -I2))) == _lib.ERR_BADARG
    assert _status(lambda: rxhip.BinomialRegressionEngine(10, 2, np.array([0.0, np.inf]), I2)) == _lib.ERR_BADARG
    X, y, n, m, _ = R.case((361, 10, 1, 2, 0.0, False, 1))
    n = np.maximum(n, 1.0)
    y = np.minimum(y, n)
    with rxhip.BinomialRegressionEngine(10, 2, m["prior_xi"], m["prior_precision"]) as eng:
        assert _status(lambda: eng.run(1)) == _lib.ERR_STATE                       # nothing set
        eng.set_regressors(X)
        eng.set_observations(y)
        assert _status(lambda: eng.run(1)) == _lib.ERR_STATE                       # n_trials missing
        bad = y.copy()
        bad[0, 3] = n[0, 3] + 1.0
        eng.set_observations(bad)                                                  # (nothing to hold it against yet)
        assert _status(lambda: eng.set_trials(n)) == _lib.ERR_BADARG               # y > n
        assert _status(lambda: eng.run(1)) == _lib.ERR_STATE                       # the refused array counts as not set
        eng.set_trials(np.maximum(n, bad))
        eng.run(1)
        assert _status(lambda: eng.set_trials(n)) == _lib.ERR_BADARG               # … n below the y in place
        assert _status(lambda: eng.run(1)) == _lib.ERR_STATE
        eng.set_observations(y)
        eng.set_trials(n)
        for k, v in ((0, np.inf), (5, -np.inf), (7, np.nan)):
            Xb = X.copy()
            Xb.ravel()[k] = v
            assert _status(lambda: eng.set_regressors(Xb)) == _lib.ERR_BADARG      # Inf / NaN in X
        assert _status(lambda: eng.run(1)) == _lib.ERR_STATE
        eng.set_regressors(X)
        nb = n.copy()
        nb[0, 2] = -1.0
        assert _status(lambda: eng.set_trials(nb)) == _lib.ERR_BADARG              # n < 0
        yb = y.copy()
        yb[0, 1] = np.inf
        assert _status(lambda: eng.set_observations(yb)) == _lib.ERR_BADARG        # Inf in y
        yb[0, 1] = -1.0
        eng.set_trials(n)
        assert _status(lambda: eng.set_observations(yb)) == _lib.ERR_BADARG        # y < 0
        eng.set_observations(y)
        eng.run(2, False)
        assert _status(lambda: eng.free_energy()) == _lib.ERR_STATE                # not asked for
        ref = R.run_batch(X, y, n, m["prior_xi"], m["prior_precision"], R.model(2, m["prior_xi"], m["prior_precision"])["init"], 2)
        mean, cov, _ = eng.parameters()
        R.hold(dict(mean=mean, cov=cov), ref)

"""The regression / autoregression engine (include/rxhip.h rxhip_arreg_desc, csrc/arreg_kernels.hpp) against its CPU restatement tests/arreg_ref.py:
q(θ), q(γ) and the free energy of every iteration and series at the project's contract (arreg_ref.hold: θ means 1e-6 posterior standard deviations,
covariances 1e-6 relative to √(v_i v_j), γ shape exact, γ rate 1e-6 relative, F 1e-8 relative with denominator max(1, |F|)).  Every case keeps
R/s ≥ 1e-6 and cond Λ ≤ 1e8 (asserted in tests/test_arreg_ref_cpu.py); the host build of the same arithmetic sits near 1e-14 (tests/test_arreg_host.py).
Shapes: d = 1 … 4 on the lane path, 5, 16 (a full tile), 17 (first with a second column tile), 32 on the matrix cores; N = 1, tile − 1, tile,
tile + 1 and (2·cap + 1) tiles, at which workgroup 0 strides over three; lagged mode at p = 1, 4, 5, 8, 17, 32 with T = p, p + 1, tile ± 1 + p and NaN
at index 0, T − 1 and on both sides of a tile boundary; 1, 3 and 300 series; 1, 15 and 40 iterations (40 is above every initial capacity); shared
parameters.  The statistics of the pass alone are held to long-double sums at |G_ij − ref| ≤ 2Nε √(G_ii G_jj), the bound of a sum of N products."""
import ctypes

import numpy as np
import pytest

import arreg_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _collect(eng, iters, fe):
    eng.run(iters, fe)
    tm, tc, ga, gb, f = eng.parameters()
    return dict(mean=tm, cov=tc, a=ga, b=gb, fe=f, total=eng.free_energy() if fe else None, last=eng.free_energy_per_chain() if fe else None)


def _run_reg(X, y, m, iters, fe=True, shared=False, stats=False, order=("X", "y")):
    C, N, d = X.shape
    with rxhip.ARRegressionEngine(N, d, **m, n_series=C, share_parameters=shared) as eng:
        for part in order:
            {"X": eng.set_regressors, "y": eng.set_observations}[part]({"X": X, "y": y}[part])
        st = eng.statistics() if stats else None
        return dict(_collect(eng, iters, fe), stats=st)


def _run_lag(z, p, m, iters, fe=True, shared=False, stats=False, layout="time_chain"):
    T, C = z.shape
    with rxhip.ARRegressionEngine(T, p, **m, n_series=C, lagged=True, share_parameters=shared) as eng:
        eng.set_data(z if layout == "time_chain" else np.ascontiguousarray(z.T), layout=layout)
        st = eng.statistics() if stats else None
        return dict(_collect(eng, iters, fe), stats=st)


def _hold_statistics(st, X, y):
    """the pass alone against long-double sums: 2Nε √(G_ii G_jj) for G, the same with s for h and s; n exact"""
    G, h, s, n = st
    for c in range(X.shape[0]):
        Gr, hr, sr, nr = R.statistics(X[c], y[c], np.longdouble)
        assert n[c] == nr
        N = max(nr, 1.0)
        dg = np.sqrt(np.diag(Gr).astype(np.float64))
        assert np.all(np.abs(G[c] - Gr.astype(np.float64)) <= 2.0 * N * EPS * np.outer(dg, dg) + 1e-300), (c, np.max(np.abs(G[c] - Gr.astype(np.float64))))
        assert np.array_equal(G[c], G[c].T)
        assert np.all(np.abs(h[c] - hr.astype(np.float64)) <= 2.0 * N * EPS * dg * np.sqrt(float(sr)) + 1e-300)
        assert abs(s[c] - float(sr)) <= 2.0 * N * EPS * float(sr)


def _check(got, ref, shared=False):
    e = R.hold(got, ref)
    tot = ref["fe"].sum(axis=1)
    et = float(np.max(np.abs(got["total"] - tot) / np.maximum(1.0, np.abs(tot))))        # rxhip_get_free_energy: per iteration, summed over the groups
    assert et < 1e-8, et
    G = ref["fe"].shape[1]
    assert np.array_equal(got["last"][:G], got["fe"][-1]) and not got["last"][G:].any()      # rxhip_get_free_energy_per_chain: last iteration
    assert R.non_increasing(got["fe"]), got["fe"]
    return e


def _same(a, b, keys=("mean", "cov", "a", "b")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- 1. schedule, dimensions and sizes ------------------------------------------------------------------------------------------------------------------
def test_schedule_constants():
    S = rxhip.ARRegressionEngine.schedule
    for d, (tile, cap) in [(1, (R.SMALL_TILE, R.SMALL_CAP)), (4, (R.SMALL_TILE, R.SMALL_CAP)), (5, (R.MFMA_TILE, R.MFMA_CAP)), (32, (R.MFMA_TILE, R.MFMA_CAP))]:
        assert S(tile * cap, d) == (tile, cap) and S(tile * cap + 1, d) == (tile, cap) and S(tile + 1, d) == (tile, 2) and S(1, d) == (tile, 1)
        assert S(0, d) == (tile, 1)                                                            # a lagged series with T ≤ p: one workgroup, a zero partial
        assert S(R.stride_rows(d), d) == (tile, cap) and R.stride_rows(d) // tile == 2 * cap + 1   # workgroup 0 takes tiles 0, cap and 2·cap
        for rows in (1, tile + 1, R.stride_rows(d)):
            assert S(rows, d) == (R.tile_rows(d), R.chunks(rows, d))
    assert S(10, 33) == (0, 0) and S(10, 0) == (0, 0) and S(-1, 2) == (0, 0)


_SIZE = {}


def _size_cases():
    if not _SIZE:
        for X, y, m, iters in R.size_cases():
            _SIZE.setdefault(X.shape[2], []).append((X, y, m, iters))
    return _SIZE


@pytest.mark.parametrize("d", R.DIMS)
def test_sizes_around_a_tile(d):
    """N = 1, tile − 1, tile, tile + 1; every fifth y missing"""
    for X, y, m, iters in _size_cases()[d]:
        got = _run_reg(X, y, m, iters, stats=True)
        _check(got, R.run_batch(X, y, **m, iterations=iters))
        _hold_statistics(got["stats"], X, y)


@pytest.mark.parametrize("p", R.LAGS)
def test_lagged_sizes_and_nan_windows(p):
    """T = p (no row), p + 1 (one), tile − 1 + p, tile + 1 + p; then NaN at 0, T − 1 and on both sides of the tile boundary: the halo carries it"""
    for z, pp, m, iters in R.lag_cases():
        if pp != p:
            continue
        ref = R.run_lagged(z, p, **m, iterations=iters)
        for layout in ("time_chain", "chain_time"):
            got = _run_lag(z, p, m, iters, stats=True, layout=layout)
            _check(got, ref)
            X, y = R.lag_rows(z[:, 0], p)
            _hold_statistics(got["stats"], X[None], y[None])
        if z.shape[0] <= p:
            # n = 0: the posterior is the prior (m = Λ0⁻¹(Λ0 m0): to rounding times cond Λ0 ≤ 164, far inside 1e-12 prior standard deviations) and F = 0
            sd0 = np.sqrt(np.diag(np.linalg.inv(m["prior_theta"][1])))
            assert got["stats"][3][0] == 0.0 and np.all(np.abs(got["mean"][-1, 0] - m["prior_theta"][0]) < 1e-12 * sd0) and abs(got["fe"][-1, 0]) < 1e-12
            assert got["a"][-1, 0] == m["prior_gamma"][0] and got["b"][-1, 0] == m["prior_gamma"][1]


@pytest.mark.parametrize("k", range(5), ids=["d4", "d16", "d32", "lag4", "lag32"])
def test_a_workgroup_strides_over_three_tiles(k):
    case = R.stride_case(k)
    if case[0] == "reg":
        _, X, y, m, iters = case
        got = _run_reg(X, y, m, iters, stats=True)
        _check(got, R.run_batch(X, y, **m, iterations=iters))
        _hold_statistics(got["stats"], X, y)
    else:
        _, z, p, m, iters = case
        got = _run_lag(z, p, m, iters, stats=True)
        _check(got, R.run_lagged(z, p, **m, iterations=iters))
        X, y = R.lag_rows(z[:, 0], p)
        _hold_statistics(got["stats"], X[None], y[None])


# ---- 2. batches, shared parameters, iteration counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_batches_of_regressions(k):
    X, y, m, iters, shared = R.batch_cases()[k]
    _check(_run_reg(X, y, m, iters, shared=shared), R.run_batch(X, y, **m, iterations=iters, shared=shared), shared)


@pytest.mark.parametrize("k", range(4))
def test_batches_of_series(k):
    z, p, m, iters, shared = R.lag_batch_cases()[k]
    _check(_run_lag(z, p, m, iters, shared=shared), R.run_lagged(z, p, **m, iterations=iters, shared=shared), shared)


@pytest.mark.parametrize("p", (2, 5, 17))
def test_lagged_mode_equals_regressor_mode(p):
    z, m = R.series_case(5000 + p, 700, 3, p, (0, 300, 699))
    rows = [R.lag_rows(z[:, c], p) for c in range(3)]
    X, y = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    a, b = _run_lag(z, p, m, 15, stats=True), _run_reg(X, y, m, 15, stats=True)
    assert np.array_equal(a["stats"][3], b["stats"][3])                                           # n exactly
    R.hold(a, b)
    R.hold(a, R.run_lagged(z, p, **m, iterations=15))


# ---- 3. bit identity ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d", [("reg", 3), ("reg", 17), ("lag", 4), ("lag", 8)])
def test_bit_identity(mode, d):
    if mode == "reg":
        X, y, m = R.regression_case(6000 + d, 300, 300, d, missing=0.05)
        run = lambda sel, iters, fe=True, **kw: _run_reg(X[sel], y[sel], m, iters, fe, **kw)
    else:
        z, m = R.series_case(6100 + d, 400, 300, d, (9, 200))
        run = lambda sel, iters, fe=True, **kw: _run_lag(np.ascontiguousarray(z[:, sel]), d, m, iters, fe, **kw)
    whole = slice(None)
    a, b, c = run(whole, 40), run(whole, 40), run(whole, 40, fe=False)
    assert _same(a, b, ("mean", "cov", "a", "b", "fe", "total")) and _same(a, c)                   # two runs; with and without the free energy
    short = run(whole, 2)
    assert all(np.array_equal(short[k], a[k][:2]) for k in ("mean", "cov", "a", "b", "fe", "total"))   # a 40-iteration run repeats a 2-iteration run's entries
    for member in (0, 150, 299):                                                                   # a series alone has the bits it has inside the batch
        alone = run(slice(member, member + 1), 40)
        for k in ("mean", "cov", "a", "b", "fe"):
            assert np.array_equal(a[k][:, member], alone[k][:, 0]), (k, member)


def test_a_second_run_keeps_the_statistics_and_starts_over():
    X, y, m = R.regression_case(6200, 500, 3, 5)
    ref = R.run_batch(X, y, **m, iterations=15)
    with rxhip.ARRegressionEngine(500, 5, **m, n_series=3) as eng:
        eng.set_observations(y)
        eng.set_regressors(X)
        first = _collect(eng, 2, False)
        again = _collect(eng, 15, True)
        R.hold(again, ref)
        assert _same(first, {k: again[k][:2] for k in ("mean", "cov", "a", "b")})
        assert eng.counters() == dict(rule_calls=15 * 3 * (2 * 500 + 2), products=15 * 3 * 2 * 500, marginals=15 * 3 * 2)
        eng.set_observations(2.0 * y)                                                              # new data: new statistics
        R.hold(_collect(eng, 3, True), R.run_batch(X, 2.0 * y, **m, iterations=3))


# ---- 4. the reference's data ---------------------------------------------------------------------------------------------------------------------------
def test_golden_data_through_infer():
    series, bench = R.golden()
    for order in range(1, 6):
        res = rxhip.infer(model=rxhip.autoregression(order), data={"y": series[order - 1]}, iterations=15, free_energy=True)
        (tm, tc), (ga, gb), fe = res.posteriors["θ"], res.posteriors["γ"], res.free_energy
        assert tm.shape == (15, order) and tc.shape == (15, order, order) and ga.shape == (15,) and gb.shape == (15,) and fe.shape == (15,)
        assert R.reference_checks(fe, len(ga), len(tm)), fe                                       # ar_tests.jl:61-65
        print(order, repr(float(fe[0])), repr(float(fe[-1])))
        for got, want in zip((fe[0], fe[-1]), R.RECORDED_FE[order]):
            assert abs(got - want) < 1e-8 * abs(want), (order, got, want)
        ref = R.run_lagged(series[order - 1][:, None], order, **R.model(order), iterations=15)
        R.hold(dict(mean=tm[:, None], cov=tc[:, None], a=ga[:, None], b=gb[:, None], fe=fe[:, None]), ref)
    fe = rxhip.infer(model=rxhip.autoregression(5), data={"y": bench}, iterations=15, free_energy=True).free_energy
    for got, want in zip((fe[0], fe[-1]), R.RECORDED_FE["bench"]):
        assert abs(got - want) < 1e-8 * abs(want)


def test_gaussian_regression_through_infer():
    X, y, m = R.regression_case(6300, 200, 4, 6, missing=0.1)
    mdl = rxhip.gaussian_regression(*m["prior_theta"], prior_gamma=m["prior_gamma"], init_gamma=m["init_gamma"])
    res = rxhip.infer(model=mdl, data={"x": X, "y": y}, iterations=15, free_energy=True)
    ref = R.run_batch(X, y, **m, iterations=15)
    (tm, tc), (ga, gb) = res.posteriors["θ"], res.posteriors["γ"]
    assert tm.shape == (15, 4, 6) and res.free_energy.shape == (15,)
    R.hold(dict(mean=tm, cov=tc, a=ga, b=gb), ref)
    assert np.all(np.abs(res.free_energy - ref["fe"].sum(axis=1)) < 1e-8 * np.abs(ref["fe"].sum(axis=1)))
    one = rxhip.infer(model=mdl, data={"x": X[1], "y": y[1]}, iterations=15, free_energy=True)
    assert np.array_equal(one.posteriors["θ"][0], tm[:, 1]) and np.array_equal(one.posteriors["γ"][1], gb[:, 1])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _refused(fn, status, text=None):
    with pytest.raises(rxhip.RxHipError) as ei:
        fn()
    assert ei.value.status == status and str(ei.value), str(ei.value)
    if text is not None:
        assert text in str(ei.value), str(ei.value)


NO_DATA = "run: no observations (call rxhip_set_data first)"
INF = "set_data: an observation is infinite (finite values and NaN = missing are accepted)"


def test_refused_creates():
    E, I2 = rxhip.ARRegressionEngine, np.eye(2)
    _refused(lambda: E(10, 33), _lib.ERR_BADARG, "arreg: d must be 1 … 32 (got 33)")
    _refused(lambda: E(10, 0), _lib.ERR_BADARG, "arreg: d must be 1 … 32 (got 0)")
    _refused(lambda: E(0, 2), _lib.ERR_BADARG, "arreg: N must be at least 1 (got 0)")
    _refused(lambda: E(10, 2, n_series=0), _lib.ERR_BADARG, "arreg: n_series must be at least 1 (got 0)")
    for pg in ((0.0, 1.0), (1.0, -1.0), (np.inf, 1.0), (1.0, np.nan)):
        _refused(lambda: E(10, 2, prior_gamma=pg), _lib.ERR_BADARG, "arreg: prior_gamma shape and rate must be positive and finite")
    _refused(lambda: E(10, 2, init_gamma=(1.0, 0.0)), _lib.ERR_BADARG, "arreg: init_gamma shape and rate must be positive and finite")
    for bad in (np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[1.0, 0.5], [0.0, 1.0]]), -I2, np.array([[np.inf, 0.0], [0.0, 1.0]])):
        _refused(lambda: E(10, 2, prior_theta=(np.zeros(2), bad)), _lib.ERR_BADARG, "arreg: prior_theta_precision is not symmetric positive definite")
    _refused(lambda: E(10, 2, prior_theta=(np.array([0.0, np.nan]), I2)), _lib.ERR_BADARG, "arreg: prior_theta_mean must be finite")
    L = _lib.lib()                                                                               # a refused create leaves a handle that destroys cleanly
    h = ctypes.c_void_p()
    assert L.rxhip_arreg_create(ctypes.byref(_lib.ArregDesc(N=8, n_series=1, d=0, prior_gamma_shape=1.0, prior_gamma_rate=1.0, device=-1)), ctypes.byref(h)) == _lib.ERR_BADARG
    assert h.value and L.rxhip_last_error(h).decode() == "arreg: d must be 1 … 32 (got 0)" and L.rxhip_destroy(h) == _lib.OK


def test_refusals_of_the_lagged_engine():
    L, dp = _lib.lib(), ctypes.POINTER(ctypes.c_double)
    z, m = R.series_case(6400, 50, 2, 3)
    ref = R.run_lagged(z, 3, **m, iterations=2)
    with rxhip.ARRegressionEngine(50, 3, **m, n_series=2, lagged=True) as eng:
        _refused(lambda: eng.run(1), _lib.ERR_STATE, NO_DATA)                                   # run before data
        _refused(lambda: eng.statistics(), _lib.ERR_STATE, "arreg_get_statistics: no observations")
        eng.set_data(z)
        _refused(lambda: eng.run(0), _lib.ERR_BADARG, "run: iterations must be positive")
        _refused(lambda: eng.run(-3), _lib.ERR_BADARG, "run: iterations must be positive")
        assert L.rxhip_run_filter(eng._h, 1) == _lib.ERR_BADARG and "run_filter: not a state-space engine" in L.rxhip_last_error(eng._h).decode()
        eng.run(2, False)
        _refused(lambda: eng.free_energy(), _lib.ERR_STATE)                                     # not asked for
        buf = np.empty(50 * 2 * 3)
        assert L.rxhip_get_marginals(eng._h, _lib.VAR_X, buf.ctypes.data_as(dp), None, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG
        assert L.rxhip_last_error(eng._h).decode() == "get_marginals: variable 1 is not random"
        assert L.rxhip_set_data(eng._h, _lib.VAR_REGRESSORS, buf.ctypes.data_as(dp), buf.size, 0) == _lib.ERR_BADARG   # the lagged mode has no X
        for v in (np.inf, -np.inf):
            zb = z.copy()
            zb[17, 1] = v
            _refused(lambda: eng.set_data(zb), _lib.ERR_BADARG, INF)
            _refused(lambda: eng.run(1), _lib.ERR_STATE, NO_DATA)                               # a refused array counts as not set
        _refused(lambda: eng.set_data(z[:-1]), _lib.ERR_BADARG, "set_data: expected 100 doubles, got 98")
        eng.set_data(z)
        host = _collect(eng, 2, True)
        R.hold(host, ref)


def test_device_data_equals_host_data_bit_for_bit():
    hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    z, m = R.series_case(6500, 600, 3, 5, (0, 133, 134, 599))
    host = _run_lag(z, 5, m, 15)
    for layout in ("time_chain", "chain_time"):
        a = np.ascontiguousarray(z if layout == "time_chain" else z.T)
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        with rxhip.ARRegressionEngine(600, 5, **m, n_series=3, lagged=True) as eng:
            eng.set_data_device(p.value, a.size, layout=layout)
            dev = _collect(eng, 15, True)
        assert hip.hipFree(p) == 0
        assert _same(host, dev, ("mean", "cov", "a", "b", "fe", "total"))
    bad = z.copy()
    bad[3, 0] = np.inf
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), bad.nbytes) == 0 and hip.hipMemcpy(p, bad.ctypes.data, bad.nbytes, 1) == 0
    with rxhip.ARRegressionEngine(600, 5, **m, n_series=3, lagged=True) as eng:
        _refused(lambda: eng.set_data_device(p.value, bad.size), _lib.ERR_BADARG, INF)
        _refused(lambda: eng.run(1), _lib.ERR_STATE, NO_DATA)
    assert hip.hipFree(p) == 0


def test_refusals_of_the_regressor_engine():
    X, y, m = R.regression_case(6600, 40, 2, 3)
    need = "run: the regression engine needs RXHIP_VAR_REGRESSORS and RXHIP_VAR_Y"
    with rxhip.ARRegressionEngine(40, 3, **m, n_series=2) as eng:
        _refused(lambda: eng.run(1), _lib.ERR_STATE, need + " (missing: regressors y)")
        eng.set_regressors(X)
        _refused(lambda: eng.run(1), _lib.ERR_STATE, need + " (missing: y)")
        eng.set_observations(y)
        eng.run(1)
        for k, v in ((0, np.inf), (5, -np.inf), (7, np.nan)):
            Xb = X.copy()
            Xb.ravel()[k] = v
            _refused(lambda: eng.set_regressors(Xb), _lib.ERR_BADARG, "set_data: regressor %d is not finite" % k)   # NaN in X is refused
            _refused(lambda: eng.run(1), _lib.ERR_STATE, need + " (missing: regressors)")                           # a refused array counts as not set
        eng.set_regressors(X)
        yb = y.copy()
        yb[1, 2] = np.inf
        _refused(lambda: eng.set_observations(yb), _lib.ERR_BADARG, "set_data: observation 42 is infinite")
        _refused(lambda: eng.run(1), _lib.ERR_STATE, need + " (missing: y)")
        _refused(lambda: eng.set_data_device(0, 80), _lib.ERR_BADARG, "set_data_device: the regression engine checks X and y on the host")
        eng.set_observations(y)
        R.hold(_collect(eng, 3, True), R.run_batch(X, y, **m, iterations=3))

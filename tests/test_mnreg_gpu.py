"""The multinomial regression engine (include/rxhip.h rxhip_mnreg_desc, csrc/mnreg_kernels.hpp) against its CPU restatement tests/mnreg_ref.py: q(ψ) and
the free energy of every iteration (offline) or step (online) and problem — at the project's contract (mnreg_ref.hold: means 1e-6 posterior standard
deviations, covariances and variances 1e-6 relative to √(v_i v_j), free energy 1e-8 relative with denominator max(1, |F|)).  Every random case keeps
cond W ≤ 1e8 (asserted in tests/test_mnreg_ref_cpu.py).
Shapes: K = 2, 3, 5, 6, 17, 18, 33 (d = 32, the last of the mvd_chol_inv class), 34 (d = 33, the first of the second class), 65; N = 1, a tile of rows − 1,
a tile, a tile + 1, and chunk cap × tile + 1, at which the first workgroup of the statistics pass runs its grid-stride loop twice (the constants come
from rxhip_mnreg_schedule and are asserted against mnreg_ref's)."""
import ctypes
import math

import numpy as np
import pytest

import binreg_ref
import mnreg_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu


def _run(Y, m, iters, fe=True, online=False, keep_cov=False, n_trials=None):
    C, N, K = Y.shape
    with rxhip.MultinomialRegressionEngine(N, K, m["prior_xi"], m["prior_precision"], n_trials=n_trials, init=None if online else m["init"], n_problems=C,
                                           online=online, keep_cov_history=keep_cov) as eng:
        eng.set_data(Y)
        eng.run(iters, fe)
        out = dict(total=eng.free_energy() if fe else None, last=eng.free_energy_per_chain() if fe else None)
        if online:
            out["mean"], out["var"], out["cov"], out["fe"] = eng.history()
            out["final"] = eng.parameters()
        else:
            out["mean"], out["cov"], out["fe"] = eng.parameters()
        return out


def _non_increasing(fe, d=64):
    return R.does_not_rise(fe, d)


def _check(Y, m, iters):
    ref = R.run_batch(Y, **m, iterations=iters)
    got = _run(Y, m, iters)
    e = R.hold(got, ref)
    tot = ref["fe"].sum(axis=1)
    et = float(np.max(np.abs(got["total"] - tot) / np.maximum(1.0, np.abs(tot))))      # rxhip_get_free_energy: per iteration, summed over the problems
    assert et < 1e-8, et
    assert np.array_equal(got["last"], got["fe"][-1])                                  # rxhip_get_free_energy_per_chain: per problem, last iteration
    assert _non_increasing(got["fe"], Y.shape[-1] - 1), got["fe"]
    return got, e


def _same(a, b, keys=("mean", "cov")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _counts(seed, C, N, K, top=7):
    """plain integer counts, vectorised (the large sizes)"""
    return np.random.default_rng(seed).integers(0, top, (C, N, K)).astype(np.float64)


# ---- 1. dimensions and sizes ---------------------------------------------------------------------------------------------------------------------------
def test_schedule_constants():
    for K in (2, 3, 8, 9, 16, 17, 18, 32, 33, 65):
        tile, cap = R.tile_rows(K), R.CHUNKS_CAP
        assert rxhip.MultinomialRegressionEngine.schedule(tile * cap, K) == (tile, cap)
        assert rxhip.MultinomialRegressionEngine.schedule(tile * cap + 1, K) == (tile, cap)        # one tile more than workgroups: the first takes two
        assert rxhip.MultinomialRegressionEngine.schedule(tile + 1, K) == (tile, 2)
        assert rxhip.MultinomialRegressionEngine.schedule(1, K) == (tile, 1)
    assert rxhip.MultinomialRegressionEngine.schedule(10, 66) == (0, 0) and rxhip.MultinomialRegressionEngine.schedule(10, 1) == (0, 0)


@pytest.mark.parametrize("spec", R.CASES["dims"] + R.CASES["small"], ids=lambda s: f"K{s[3]}-N{s[1]}")
def test_dimensions(spec):
    _check(*R.case(spec))


def _statistics_check(Y):
    C, N, K = Y.shape
    with rxhip.MultinomialRegressionEngine(N, K, np.zeros(K - 1), np.eye(K - 1), n_problems=C) as eng:
        eng.set_data(Y)
        Yc, S, lc, n = eng.statistics()
    for c in range(C):
        obs = R.observed(Y[c])
        Yi = Y[c][obs].astype(np.int64)
        col = Yi.sum(axis=0)
        assert np.array_equal(Yc[c], col.astype(np.float64)) and n[c] == float(obs.sum())                  # bit-equal to int64 sums
        assert np.array_equal(S[c], R.remainders(Yi).sum(axis=0).astype(np.float64))                       # … and to the per-row remainders
        terms = np.concatenate([R._lgamma(Yi.sum(axis=1) + 1.0), -R._lgamma(Yi.astype(np.float64) + 1.0).reshape(-1)]).astype(np.longdouble)
        bound = 2.0 * max(float(obs.sum()), 1.0) * K * np.finfo(np.float64).eps * float(np.sum(np.abs(terms)))
        assert abs(lc[c] - float(np.sum(terms))) <= bound, (lc[c], float(np.sum(terms)), bound)


@pytest.mark.parametrize("K", [3, 18])
def test_sizes_around_a_tile(K):
    """N = 1, tile − 1, tile, tile + 1: statistics bit-equal to integer sums, the iterations at the contract"""
    for N in R.sizes_for(K)[:4]:
        Y = _counts(500 + K + N, 1, N, K)
        if N > 2:
            Y[0, N // 2, 0] = np.nan
        _statistics_check(Y)
        _check(Y, R.model(K), 3)


@pytest.mark.parametrize("K", [3, 18])
def test_a_workgroup_strides_over_two_tiles(K):
    N = R.sizes_for(K)[4]
    tile, chunks = rxhip.MultinomialRegressionEngine.schedule(N, K)
    assert (N + tile - 1) // tile == chunks + 1
    Y = _counts(510 + K, 1, N, K, top=4)
    Y[0, 5, 1] = np.nan
    Y[0, N - 1, :] = np.nan
    _statistics_check(Y)
    _check(Y, R.model(K), 2)


# ---- 2. edge rows and priors ---------------------------------------------------------------------------------------------------------------------------
def test_edge_rows():
    K = 5
    Y, m, _ = R.case((520, 30, 2, K, 0.0, 4))
    Y[0, 0, :] = 0.0                           # N_i = 0
    Y[0, 1, :] = [9.0, 0.0, 0.0, 0.0, 0.0]     # all mass in category 1: every later remainder 0
    Y[0, :, 3:] = 0.0                          # the last two categories never observed: S_4 = 0, ψ_4 keeps the prior's conditional
    Y[1, :, :] = np.nan                        # a fully missing problem
    got, _ = _check(Y, m, 4)
    V0 = np.linalg.inv(m["prior_precision"])
    prior = dict(mean=np.tile(V0 @ m["prior_xi"], (4, 1)), cov=np.tile(V0, (4, 1, 1)), fe=np.zeros(4))
    R.hold(dict(mean=got["mean"][:, 1], cov=got["cov"][:, 1], fe=got["fe"][:, 1]), prior)
    with rxhip.MultinomialRegressionEngine(30, K, m["prior_xi"], m["prior_precision"], n_problems=2) as eng:
        eng.set_data(Y)
        _, S, _, n = eng.statistics()
        assert S[0, 3] == 0.0 and n[1] == 0.0 and not S[1].any()


@pytest.mark.parametrize("K", [4, 34])
def test_edge_priors(K):
    d = K - 1
    Y, _, _ = R.case((530 + K, 40, 1, K, 0.1, 4))
    tiny = R.model(K, np.zeros(d), 1e12 * np.eye(d))                       # c = 1e-6: the series branch of ω̄
    got, _ = _check(Y, tiny, 4)
    huge = R.model(K, 1500.0 * (-1.0) ** np.arange(d), np.eye(d))          # c ≈ 1500
    got, _ = _check(Y, huge, 4)
    assert np.all(np.isfinite(got["fe"]))


@pytest.mark.parametrize("K", [3, 10, 33])
def test_against_the_binomial_engine_on_the_expanded_problem(K):
    """rows x = e_k, n = N_ik, y = y_ik: the two implementations share only point_term and mvd_chol_inv"""
    Y, m, iters = R.case((540 + K, 60, 1, K, 0.1, 5))
    X, y, n = R.expanded(Y[0])
    with rxhip.BinomialRegressionEngine(len(y), K - 1, m["prior_xi"], m["prior_precision"], m["init"]) as eng:
        eng.set_data(X, y, n)
        eng.run(iters, True)
        bm, bc, bf = eng.parameters()
    got = _run(Y, m, iters)
    R.hold(got, dict(mean=bm, cov=bc, fe=bf))


def test_custom_initial_q():
    Y, m, iters = R.case((550, 70, 2, 6, 0.1, 4))
    r = np.random.default_rng(9)
    A = r.standard_normal((5, 5))
    _check(Y, dict(m, init=(r.standard_normal(5), 0.3 * np.eye(5) + 0.1 * A @ A.T)), iters)


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------------------------------
def test_bits():
    Y, m, iters = R.case(R.CASES["batch"][0])
    assert Y.shape == (300, 50, 10)
    a, b, c = _run(Y, m, iters), _run(Y, m, iters), _run(Y, m, iters, fe=False)
    assert _same(a, b, ("mean", "cov", "fe", "total")) and _same(a, c)                       # two runs; with and without the free energy
    for k in (0, 150, 299):                                                                  # a problem alone and as a member of the batch
        alone = _run(Y[k:k + 1], m, iters)
        for q in ("mean", "cov", "fe"):
            assert np.array_equal(a[q][:, k], alone[q][:, 0]), (k, q)
    ref = R.run_batch(Y[:4], **m, iterations=iters)
    R.hold({q: a[q][:, :4] for q in ("mean", "cov", "fe")}, ref)


def test_a_second_run_launches_no_statistics_kernel_and_longer_runs_grow_the_buffers():
    Y, m, _ = R.case((560, 90, 3, 10, 0.1, 2))
    C, N, K = Y.shape
    with rxhip.MultinomialRegressionEngine(N, K, m["prior_xi"], m["prior_precision"], init=m["init"], n_problems=C) as eng:
        eng.set_profiling(True)
        eng.set_data(Y)
        eng.run(2, True)
        m2, c2, f2 = eng.parameters()
        t2 = eng.free_energy()
        eng.run(40, True)                                                                    # past the 32 entries the buffers start with
        m40, c40, f40 = eng.parameters()
        t40 = eng.free_energy()
        eng.sync()
        kt = eng.kernel_times()
        assert kt["k_gmm_pass"]["launches"] == 1 and kt["k_gmm_update"]["launches"] == 2, kt   # ONE statistics pass per data set, ONE resident kernel per run
        assert np.array_equal(m40[:2], m2) and np.array_equal(c40[:2], c2) and np.array_equal(f40[:2], f2) and np.array_equal(t40[:2], t2)
        assert t40.shape == (40,) and _non_increasing(f40, K - 1)
        assert np.array_equal(eng.free_energy_per_chain(), f40[-1])
        eng.set_data(Y[::-1].copy())                                                         # new data, new statistics
        eng.run(2, True)
        eng.sync()
        assert eng.kernel_times()["k_gmm_pass"]["launches"] == 2
        R.hold(dict(zip(("mean", "cov", "fe"), eng.parameters())), R.run_batch(Y[::-1], **m, iterations=2))


# ---- 4. online -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", R.CASES["online"], ids=lambda s: f"K{s[3]}-T{s[1]}-it{s[5]}")
def test_online_history(spec):
    Y, m, iters = R.case(spec)
    C, T, K = Y.shape
    Y[0, 0, :] = np.nan                      # missing rows at t = 1, in the middle and at T
    Y[1, T // 2, 0] = np.nan
    Y[2, T - 1, K - 1] = np.nan
    ref = R.online_batch(Y, m["prior_xi"], m["prior_precision"], iters)
    got = _run(Y, m, iters, online=True, keep_cov=True)
    R.hold({k: got[k] for k in ("mean", "var", "cov", "fe")}, ref)
    assert np.array_equal(got["var"], np.einsum("tcii->tci", got["cov"]))
    fm, fc, ff = got["final"]
    assert np.array_equal(fm, got["mean"][-1]) and np.array_equal(fc, got["cov"][-1]) and np.array_equal(ff, got["fe"][-1])
    assert got["fe"][0, 0] == 0.0 and np.array_equal(got["mean"][T - 1, 2], got["mean"][T - 2, 2]) if T > 1 else True
    tot = ref["fe_it"].sum(axis=1)
    assert float(np.max(np.abs(got["total"] - tot) / np.maximum(1.0, np.abs(tot)))) < 1e-8
    per = ref["fe"].sum(axis=0)
    assert float(np.max(np.abs(got["last"] - per) / np.maximum(1.0, np.abs(per)))) < 1e-8
    off = _run(Y, m, iters, online=True, keep_cov=False)                                     # the covariance history changes nothing else
    assert off["cov"] is None and _same(got, off, ("mean", "var", "fe", "total", "last"))
    assert all(np.array_equal(x, y) for x, y in zip(got["final"], off["final"]))
    nofe = _run(Y, m, iters, fe=False, online=True)
    assert _same(got, nofe, ("mean", "var"))


@pytest.mark.parametrize("K", [3, 34])
def test_online_is_the_offline_engine_chained(K):
    """T = 5 steps on the device ≡ the OFFLINE engine called T times on one row with the previous posterior as prior"""
    Y, m, _ = R.case((570 + K, 5, 1, K, 0.0, 1))
    for iters in (1, 3):
        got = _run(Y, m, iters, online=True, keep_cov=True)
        xi, W = m["prior_xi"], m["prior_precision"]
        means, covs, fes = [], [], []
        for t in range(5):
            step = _run(Y[:, t:t + 1], R.model(K, xi, W), iters)
            mean, cov = step["mean"][-1, 0], step["cov"][-1, 0]
            W = np.linalg.inv(cov)
            W = 0.5 * (W + W.T)
            xi = W @ mean
            means.append(mean), covs.append(cov), fes.append(step["fe"][-1, 0])
        R.hold(dict(mean=got["mean"][:, 0], cov=got["cov"][:, 0], fe=got["fe"][:, 0]), dict(mean=np.array(means), cov=np.array(covs), fe=np.array(fes)))


# ---- 5. the common entry points and the refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("online", [False, True])
def test_common_entry_points(online):
    L = rxhip.lib()
    Y, m, _ = R.case((580, 6, 2, 4, 0.0, 1))
    with rxhip.MultinomialRegressionEngine(6, 4, m["prior_xi"], m["prior_precision"], n_problems=2, online=online) as eng:
        with pytest.raises(rxhip.RxHipError) as ei:                                          # a run without data
            eng.run(1, True)
        assert ei.value.status == _lib.ERR_STATE
        buf = np.zeros(2 * 6 * 4)
        assert L.rxhip_set_data_device(eng._h, _lib.VAR_Y, None, buf.size, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG
        assert b"mnreg" in L.rxhip_last_error(eng._h)
        for bad, what in ((np.inf, "infinite"), (-1.0, "non-negative"), (0.5, "non-negative"), (2.0 ** 31 + 1.0, "2^31")):
            Z = Y.copy()
            Z[1, 2, 1] = bad
            with pytest.raises(rxhip.RxHipError) as ei:
                eng.set_data(Z)
            assert ei.value.status == _lib.ERR_BADARG and "mnreg" in str(ei.value) and what in str(ei.value), str(ei.value)
            with pytest.raises(rxhip.RxHipError) as ei:                                      # a refused array counts as not set
                eng.run(1, True)
            assert ei.value.status == _lib.ERR_STATE
        eng.set_data(Y)
        eng.run(2, True)
        assert eng.free_energy().shape == (2,) and eng.free_energy_per_chain().shape == (2,)
        eng.run(35, True)                                                                    # capacity growth on a longer second run
        assert eng.free_energy().shape == (35,) and np.all(np.isfinite(eng.free_energy()))
        out = np.zeros(64)
        assert L.rxhip_get_marginals(eng._h, _lib.VAR_X, out.ctypes.data_as(_lib.c_double_p), None, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG
        assert L.rxhip_run_filter(eng._h, 0) == _lib.ERR_BADARG
        if not online:
            with pytest.raises(rxhip.RxHipError):
                eng.history()
    with rxhip.MultinomialRegressionEngine(6, 4, m["prior_xi"], m["prior_precision"], n_trials=int(np.nansum(Y[0, 0])) + 1, n_problems=2, online=online) as eng:
        with pytest.raises(rxhip.RxHipError) as ei:
            eng.set_data(Y)
        assert ei.value.status == _lib.ERR_BADARG and "n_trials" in str(ei.value) and "mnreg" in str(ei.value)
    desc = _lib.MnregDesc()                                                                  # a refused create leaves a handle that destroys cleanly
    desc.N, desc.n_problems, desc.K, desc.mode = 5, 1, 66, int(online)
    h = ctypes.c_void_p()
    assert L.rxhip_mnreg_create(ctypes.byref(desc), ctypes.byref(h)) == _lib.ERR_BADARG and h.value
    assert b"mnreg" in L.rxhip_last_error(h) and L.rxhip_destroy(h) == _lib.OK


# ---- 6. the reference's workloads through infer --------------------------------------------------------------------------------------------------------
def test_reference_offline_workload_through_infer():
    """multinomialreg_tests.jl:11-55 on the golden draw: MSE < 2e-5, F falls, |F₉₉ − F₁₀₀| < 1e-8; RECORDED_FE at 1e-8.
    The reference's `F[end] <= F[end − 1]` is held to the resolution of fp64 at |F| (mnreg_ref.fe_resolution): in the 50-digit statement
    (tests/mnreg_mp.py) the iteration has converged by then, F₉₉ − F₁₀₀ = 2.7e-21 at F = 13540.6 (one ulp: 1.8e-12), so the sign of the difference of
    two fp64 evaluations is rounding.  Measured on an MI355X: F₉₉ one ulp below the 50-digit value, F₁₀₀ one ulp above, F₁₀₀ − F₉₉ = +3.6e-12 (two
    ulps); the numpy restatement has −4.0e-11 with errors of +2.8e-11 and −1.2e-11 against the same 50-digit values."""
    Y, p, W0, N = R.golden()
    K = Y.shape[1]
    res = rxhip.infer(model=rxhip.multinomial_regression(np.zeros(K - 1), W0, n_trials=N), data={"y": Y}, iterations=100, free_energy=True)
    mean, cov = res.posteriors["ψ"]
    fe = res.free_energy
    assert mean.shape == (100, K - 1) and cov.shape == (100, K - 1, K - 1) and fe.shape == (100,)
    mse = float(np.mean((rxhip.logistic_stick_breaking(mean[-1]) - p) ** 2))
    print("mse", mse, "F", fe[0], fe[-1], abs(fe[-2] - fe[-1]))
    assert mse < 2e-5 and fe[-1] < fe[0] and R.does_not_rise(fe[-2:], K - 1) and abs(fe[-2] - fe[-1]) < 1e-8
    assert abs(fe[0] - R.RECORDED_FE[0]) < 1e-8 * R.RECORDED_FE[0] and abs(fe[-1] - R.RECORDED_FE[1]) < 1e-8 * R.RECORDED_FE[1]
    batch = rxhip.infer(model=rxhip.multinomial_regression(np.zeros(K - 1), W0), data={"y": np.stack([Y, Y[::-1]])}, iterations=3, free_energy=True)
    assert batch.posteriors["ψ"][0].shape == (3, 2, K - 1) and batch.free_energy.shape == (3, 2)
    assert np.array_equal(batch.posteriors["ψ"][0][:, 0], mean[:3])


def test_reference_online_workload_through_infer():
    """multinomialreg_tests.jl:57-116 on the first 200 rows of the golden draw (the whole of it belongs to scripts/bench_mnreg.py): history against
    the restatement, F_1 as recorded, F_1 > F_T"""
    Y, p, W0, N = R.golden("mnreg_online_seed1")
    Y = Y[:200]
    K = Y.shape[1]
    res = rxhip.infer(model=rxhip.multinomial_regression(np.zeros(K - 1), W0, n_trials=N), data={"y": Y}, iterations=1, free_energy=True, autoupdates=True,
                      keephistory=len(Y), historyvars=("ψ", "ψ_cov"))
    hm, hv = res.history["ψ"]
    assert hm.shape == (200, K - 1) and hv.shape == (200, K - 1) and res.history["ψ_cov"].shape == (200, K - 1, K - 1) and res.free_energy.shape == (200,)
    ref = R.online(Y, np.zeros(K - 1), W0, 1)
    R.hold(dict(mean=hm, var=hv, cov=res.history["ψ_cov"], fe=res.free_energy), ref)
    assert np.array_equal(res.posteriors["ψ"][0], hm[-1]) and res.posteriors["ψ"][1].shape == (K - 1, K - 1)
    assert abs(res.free_energy[0] - R.RECORDED_FE_ONLINE[0]) < 1e-8 * R.RECORDED_FE_ONLINE[0] and res.free_energy[-1] < res.free_energy[0]

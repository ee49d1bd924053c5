"""What pins tests/arreg_ref.py (the CPU restatement of the regression / autoregression engine) independently of the engine:
(a) a 60-digit mpmath statement of statistics, iteration and free energy on 24 regressor and lag cases, held at 1e-10 of the contract's denominators;
(b) F written as a function of free (m, V, a, b) rises when either block leaves its update, and does not rise between iterations;
(c) at d = 1 with γ held (a0, b0 → ∞ at a fixed ratio) q(θ) is the conjugate closed form;
(d) the lagged rows are ar_ssm_data's on a short series, written out by hand;
(e) on the regenerated data of the reference, orders 1 … 5 and 15 iterations, the reference's own assertions (ar_tests.jl:61-65) and RECORDED_FE;
(f) the numerical envelope — R/s ≥ 1e-6 and cond Λ ≤ 1e8 at every iteration — on every case any test uses, no seed passed over."""
import os
import sys

import mpmath as mp
import numpy as np
import pytest

import arreg_ref as R

mp.mp.dps = 60


def mp_run(X, y, m, iterations):
    """the model's iteration in 60-digit arithmetic, from the data"""
    (m0, L0), (a0, b0) = m["prior_theta"], m["prior_gamma"]
    ia, ib = m["prior_gamma"] if m["init_gamma"] is None else m["init_gamma"]
    d = X.shape[1]
    keep = [i for i in range(len(y)) if not np.isnan(y[i])]
    Xm = mp.matrix([[mp.mpf(float(X[i, j])) for j in range(d)] for i in keep]) if keep else mp.zeros(0, d)
    ym = mp.matrix([mp.mpf(float(y[i])) for i in keep]) if keep else mp.zeros(0, 1)
    G = Xm.T * Xm if keep else mp.zeros(d, d)
    h = Xm.T * ym if keep else mp.zeros(d, 1)
    s = (ym.T * ym)[0] if keep else mp.mpf(0)
    n = mp.mpf(len(keep))
    L0m, m0m = mp.matrix(L0.tolist()), mp.matrix(m0.tolist())
    a0, b0 = mp.mpf(a0), mp.mpf(b0)
    gbar = mp.mpf(ia) / mp.mpf(ib)
    logdet_l0 = mp.log(mp.det(L0m))
    out = dict(mean=[], cov=[], a=[], b=[], fe=[])
    for _ in range(iterations):
        L = L0m + gbar * G
        V = mp.inverse(L)
        mm = V * (L0m * m0m + gbar * h)
        R_ = s - 2 * (mm.T * h)[0] + sum((V[i, j] + mm[i] * mm[j]) * G[i, j] for i in range(d) for j in range(d))    # tr((V + m mᵀ) G), G symmetric
        a, b = a0 + n / 2, b0 + R_ / 2
        dm = mm - m0m
        kl_t = (sum(L0m[i, j] * V[j, i] for i in range(d) for j in range(d)) + (dm.T * L0m * dm)[0] - d - logdet_l0 + mp.log(mp.det(L))) / 2   # ln det V = −ln det Λ
        kl_g = (a - a0) * mp.digamma(a) - mp.loggamma(a) + mp.loggamma(a0) + a0 * (mp.log(b) - mp.log(b0)) + a * (b0 - b) / b
        F = -(n / 2 * (mp.digamma(a) - mp.log(b) - mp.log(2 * mp.pi)) - (a / b) * R_ / 2) + kl_t + kl_g
        out["mean"].append([float(v) for v in mm]), out["cov"].append([[float(V[i, j]) for j in range(d)] for i in range(d)])
        out["a"].append(float(a)), out["b"].append(float(b)), out["fe"].append(float(F))
        gbar = a / b
    return {k: np.array(v)[:, None] for k, v in out.items()}


def mp_cases():
    """24 cases: 12 regressor (d = 1 … 32, some with missing y, one with N = 1) and 12 lagged (p = 1 … 32, NaN inside, T = p and T = p + 1)"""
    out = []
    for k, (d, N) in enumerate(((1, 1), (1, 40), (2, 30), (3, 50), (4, 60), (5, 40), (8, 64), (16, 80), (17, 70), (24, 90), (32, 100), (32, 33))):
        X, y, m = R.regression_case(500 + k, N, 1, d, missing=0.1 if k % 2 else 0.0)
        out.append((X[0], y[0], m, 3 if d > 8 else 6))
    for k, (p, T) in enumerate(((1, 1), (1, 2), (1, 50), (2, 40), (4, 60), (5, 5), (5, 70), (8, 90), (17, 18), (17, 100), (32, 120), (32, 40))):
        z, m = R.series_case(600 + k, T, 1, p, (T // 2,) if k % 3 == 2 else ())
        X, y = R.lag_rows(z[:, 0], p)
        out.append((X, y, m, 3 if p > 8 else 6))
    return out


def test_a_mpmath_statement_at_60_digits():
    worst = {}
    cases = mp_cases()
    assert len(cases) == 24
    for X, y, m, iters in cases:
        ref = mp_run(X, y, m, iters)
        got = R.run_batch(X[None], y[None], **m, iterations=iters)
        assert np.array_equal(got["a"], ref["a"])
        e = R.contract_errors(got, ref)
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(e.values()) < 1e-10, (X.shape, e)
    print("worst against mpmath:", worst)


def test_b_f_rises_when_a_block_leaves_its_update():
    r = np.random.default_rng(77)
    for k in range(40):
        d = int(r.integers(1, 33))
        X, y, m = R.regression_case(700 + k, int(r.integers(d + 2, 200)), 1, d, missing=0.05)
        G, h, s, n = R.statistics(X[0], y[0])
        (m0, L0), (a0, b0) = m["prior_theta"], m["prior_gamma"]
        out = R.run_stats(G, h, s, n, **m, iterations=8)
        assert R.non_increasing(out["fe"]), out["fe"]
        # the θ block at fixed q(γ) = the init: its update is the minimiser
        ia, ib = m["init_gamma"]
        mm, V, _ = R.theta_update(G, h, m0, L0, ia / ib)
        f0 = R.free_energy_of(G, h, s, n, m0, L0, a0, b0, mm, V, ia, ib)
        for _ in range(4):
            dm = 0.1 * r.standard_normal(d) * np.sqrt(np.diag(V))
            assert R.free_energy_of(G, h, s, n, m0, L0, a0, b0, mm + dm, V, ia, ib) > f0
            assert R.free_energy_of(G, h, s, n, m0, L0, a0, b0, mm, V * (1.0 + 0.2 * r.random() + 0.01), ia, ib) > f0
            assert R.free_energy_of(G, h, s, n, m0, L0, a0, b0, mm, V * (1.0 - 0.2 * r.random() - 0.01), ia, ib) > f0
        # the γ block at that q(θ)
        a, b = a0 + 0.5 * n, b0 + 0.5 * R.residual(G, h, s, mm, V)
        f1 = R.free_energy_of(G, h, s, n, m0, L0, a0, b0, mm, V, a, b)
        assert f1 <= f0 + 1e-9 * max(1.0, abs(f0))
        for fa, fb in ((1.05, 1.0), (0.95, 1.0), (1.0, 1.05), (1.0, 0.95), (1.03, 0.98)):
            assert R.free_energy_of(G, h, s, n, m0, L0, a0, b0, mm, V, a * fa, b * fb) > f1


def test_c_one_regressor_with_gamma_held_is_the_conjugate_closed_form():
    r = np.random.default_rng(5)
    x, g, lam0, mu0 = r.standard_normal(60), 2.5, 0.7, 0.3
    y = 0.8 * x + r.standard_normal(60) / np.sqrt(g)
    big = 1e13
    out = R.run_batch(x[None, :, None], y[None], (np.array([mu0]), np.array([[lam0]])), (g * big, big), None, 5)
    v = 1.0 / (lam0 + g * (x @ x))
    mean = v * (lam0 * mu0 + g * (x @ y))
    assert np.all(np.abs(out["cov"][:, 0, 0, 0] - v) < 1e-9 * v) and np.all(np.abs(out["mean"][:, 0, 0] - mean) < 1e-9 * np.sqrt(v))


def test_d_lagged_rows_are_ar_ssm_data_by_hand():
    X, y = R.lag_rows(np.array([1.0, 2.0, 3.0, 4.0, 5.0]), 2)     # inputs [2, 1], [3, 2], [4, 3]; outputs 3, 4, 5
    assert X.tolist() == [[2.0, 1.0], [3.0, 2.0], [4.0, 3.0]] and y.tolist() == [3.0, 4.0, 5.0]
    X, y = R.lag_rows(np.array([1.0, 2.0, 3.0, 4.0]), 1)
    assert X.tolist() == [[1.0], [2.0], [3.0]] and y.tolist() == [2.0, 3.0, 4.0]
    X, y = R.lag_rows(np.array([1.0, np.nan, 3.0, 4.0, 5.0, 6.0]), 2)   # the NaN drops rows t = 2 (regressor) and t = 3 (regressor); t = 1 is no row
    assert np.isnan(y).tolist() == [True, True, False, False] and X[2:].tolist() == [[4.0, 3.0], [5.0, 4.0]]
    assert R.lag_rows(np.array([1.0, 2.0]), 2)[0].shape == (0, 2) and R.lag_rows(np.array([1.0]), 3)[1].shape == (0,)
    out = R.run_lagged(np.array([[1.0], [2.0]]), 2, **R.model(2), iterations=2)       # T ≤ p: n = 0, the posterior is the prior, F = 0
    assert np.array_equal(out["mean"], np.zeros((2, 1, 2))) and np.array_equal(out["cov"][0, 0], np.eye(2)) and np.all(out["a"] == 1.0) and np.all(out["b"] == 1.0)
    assert np.all(np.abs(out["fe"]) < 1e-14)


def test_e_reference_data_and_its_own_assertions():
    sys.path.insert(0, os.path.join(R.HERE, "golden"))
    import make_ar_golden
    series, bench = R.golden()
    assert np.array_equal(series, make_ar_golden.draws(1234, 1000, 5)) and np.array_equal(bench, make_ar_golden.draws(32, 1000)[0])
    assert series.shape == (5, 1000) and bench.shape == (1000,)
    for order in range(1, 6):
        out = R.run_lagged(series[order - 1][:, None], order, **R.model(order), iterations=15)
        fe = out["fe"][:, 0]
        assert R.reference_checks(fe, len(out["a"]), len(out["mean"])), (order, fe)
        print(order, repr(float(fe[0])), repr(float(fe[-1])))
        assert fe[0] == pytest.approx(R.RECORDED_FE[order][0], rel=1e-13) and fe[-1] == pytest.approx(R.RECORDED_FE[order][1], rel=1e-13)
    fe = R.run_lagged(bench[:, None], 5, **R.model(5), iterations=15)["fe"][:, 0]
    assert fe[0] == pytest.approx(R.RECORDED_FE["bench"][0], rel=1e-13) and fe[-1] == pytest.approx(R.RECORDED_FE["bench"][1], rel=1e-13)


def _envelope(out, what):
    assert float(out["rs"].min()) >= 1e-6 and float(out["cond"].max()) <= 1e8, (what, float(out["rs"].min()), float(out["cond"].max()))
    return float(out["rs"].min()), float(out["cond"].max())


def test_f_numerical_envelope_of_every_case():
    worst = [1.0, 1.0]

    def fold(v):
        worst[0], worst[1] = min(worst[0], v[0]), max(worst[1], v[1])
    for X, y, m, iters in mp_cases():
        fold(_envelope(R.run_batch(X[None], y[None], **m, iterations=iters), "mp"))
    for X, y, m, iters in R.size_cases():
        fold(_envelope(R.run_batch(X, y, **m, iterations=iters), ("size", X.shape)))
    for z, p, m, iters in R.lag_cases():
        fold(_envelope(R.run_lagged(z, p, **m, iterations=iters), ("lag", z.shape, p)))
    for X, y, m, iters, shared in R.batch_cases():
        fold(_envelope(R.run_batch(X, y, **m, iterations=iters, shared=shared), ("batch", X.shape)))
    for z, p, m, iters, shared in R.lag_batch_cases():
        fold(_envelope(R.run_lagged(z, p, **m, iterations=iters, shared=shared), ("lag batch", z.shape, p)))
    for case in R.stride_cases():
        if case[0] == "reg":
            fold(_envelope(R.run_batch(case[1], case[2], **case[3], iterations=case[4]), ("stride", case[1].shape)))
        else:
            fold(_envelope(R.run_lagged(case[1], case[2], **case[3], iterations=case[4]), ("stride lag", case[1].shape, case[2])))
    series, bench = R.golden()
    for order in range(1, 6):
        fold(_envelope(R.run_lagged(series[order - 1][:, None], order, **R.model(order), iterations=15), ("golden", order)))
    print("smallest R/s %.3g, largest cond %.3g" % tuple(worst))

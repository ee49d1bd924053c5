"""What pins tests/mnreg_ref.py (the CPU restatement the GPU tests of the multinomial regression engine compare against), independently of the engine:
the 50-digit statement tests/mnreg_mp.py, the binomial restatement tests/binreg_ref.py on the expanded problem, the suffix-sum identity against the
per-row remainders, F as a function of free (m, V, c), the online recursion as chained one-row problems, and the reference's assertions on the golden
draws (tests/golden/make_mnreg_golden.py)."""
import numpy as np
import pytest

import binreg_ref
import mnreg_mp
import mnreg_ref as R

MP_CASES = [(600 + i, N, K, miss, it) for i, (N, K, miss, it) in enumerate([(12, 2, 0.0, 3), (9, 3, 0.2, 3), (10, 5, 0.0, 3), (7, 6, 0.2, 3), (6, 17, 0.0, 2),
                                                                             (5, 18, 0.2, 2), (4, 33, 0.0, 1), (4, 34, 0.2, 1), (3, 65, 0.0, 1), (1, 3, 0.0, 3),
                                                                             (1, 34, 0.0, 1), (20, 10, 0.1, 4)])]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))


@pytest.mark.parametrize("spec", MP_CASES, ids=lambda s: f"K{s[2]}-N{s[1]}")
def test_against_the_50_digit_statement(spec):
    seed, N, K, miss, iters = spec
    Y, m = R.random_case(seed, N, 1, K, miss)
    got, ref = R.run(Y[0], **m, iterations=iters), mnreg_mp.run(Y[0], **m, iterations=iters)
    assert max(_rel(got[k], ref[k]) for k in ("mean", "cov", "fe")) < 1e-10
    if K in (3, 6) or (K == 34 and N == 1):
        T = min(N, 4)
        got, ref = R.online(Y[0][:T], m["prior_xi"], m["prior_precision"], 2), mnreg_mp.online(Y[0][:T], m["prior_xi"], m["prior_precision"], 2)
        assert max(_rel(got[k], ref[k]) for k in ("mean", "cov", "fe")) < 1e-10


@pytest.mark.parametrize("K", [2, 3, 10, 33, 65])
def test_against_the_binomial_restatement_on_the_expanded_problem(K):
    Y, m = R.random_case(620 + K, 40, 1, K, 0.1)
    X, y, n = R.expanded(Y[0])
    got, ref = R.run(Y[0], **m, iterations=5), binreg_ref.run(X, y, n, m["prior_xi"], m["prior_precision"], m["init"], 5)
    assert max(_rel(got[k], ref[k]) for k in ("mean", "cov", "fe")) < 1e-12


@pytest.mark.parametrize("K", [2, 7, 34, 65])
def test_suffix_sums_are_the_summed_remainders_exactly(K):
    Y, _ = R.random_case(630 + K, 200, 1, K, 0.1)
    st = R.statistics(Y[0])
    Yi = Y[0][R.observed(Y[0])].astype(np.int64)
    rem = np.stack([Yi.sum(axis=1) - Yi[:, :k].sum(axis=1) for k in range(K)], axis=1)      # N_ik = N_i − Σ_{j<k} y_ij
    assert np.array_equal(rem, R.remainders(Yi))
    assert np.array_equal(st["S"], rem.sum(axis=0).astype(np.float64)) and np.array_equal(st["Y"], Yi.sum(axis=0).astype(np.float64))
    assert st["n"] == len(Yi)
    lc2 = float(np.sum(R._lgamma(rem[:, :-1] + 1.0) - R._lgamma(Yi[:, :-1] + 1.0) - R._lgamma(rem[:, :-1] - Yi[:, :-1] + 1.0)))   # Σ ln C(N_ik, y_ik)
    assert abs(st["lc"] - lc2) < 1e-10 * max(1.0, abs(lc2))


def test_each_block_update_minimises_the_free_energy():
    """F(m, V, c) at the iteration's own point is below F with either block moved away from its update (40 random cases)"""
    for i in range(40):
        K = (2, 3, 5, 9, 18, 34)[i % 6]
        Y, m = R.random_case(640 + i, 25, 1, K, 0.1)
        st = R.statistics(Y[0])
        S = st["S"][:-1]
        kappa = st["Y"][:-1] - 0.5 * S
        r = R.iterate(S, kappa, st["lc"], m["prior_xi"], m["prior_precision"], m["init"], 3)
        mm, V, c = r["mean"][-1], r["cov"][-1], r["c"]
        F = lambda m_, V_, c_: R.free_energy_of(S, kappa, st["lc"], m["prior_xi"], m["prior_precision"], m_, V_, c_)
        F0 = F(mm, V, c)
        assert abs(F0 - r["fe"][-1]) < 1e-9 * max(1.0, abs(F0))
        rng = np.random.default_rng(i)
        for _ in range(3):
            assert F(mm + 0.05 * rng.standard_normal(K - 1), V, c) > F0                    # q(ψ) is optimal for this q(ω)
            assert F(mm, V * (1.0 + 0.05 * rng.random()), c) > F0
        c_opt = np.sqrt(mm * mm + np.diag(V))                                              # q(ω) optimal for this q(ψ): the next iteration's step 1
        Fopt = F(mm, V, c_opt)
        assert Fopt <= F0 + 1e-9 * max(1.0, abs(F0))
        for _ in range(3):
            assert F(mm, V, c_opt * (1.0 + 0.1 * rng.random(K - 1) + 0.01)) >= Fopt - 1e-9 * max(1.0, abs(Fopt))


ALL_CASES = [(g, s) for g, specs in R.CASES.items() for s in specs]


@pytest.mark.parametrize("group,spec", ALL_CASES, ids=lambda v: v if isinstance(v, str) else f"K{v[3]}-N{v[1]}-s{v[0]}")
def test_cases_are_well_conditioned_and_the_free_energy_falls(group, spec):
    Y, m, iters = R.case(spec)
    if group == "online":
        for k in range(len(Y)):
            r = R.online(Y[k], m["prior_xi"], m["prior_precision"], iters, want_cond=True)
            assert r["cond"].max() <= 1e8 and np.all(np.isfinite(r["fe"]))
        return
    r = R.run_batch(Y, **m, iterations=iters, want_cond=True)
    assert r["cond"].max() <= 1e8, r["cond"].max()
    assert R.does_not_rise(r["fe"], Y.shape[-1] - 1)


@pytest.mark.parametrize("K", [3, 10, 34])
def test_online_is_a_chain_of_one_row_offline_problems(K):
    Y, m = R.random_case(660 + K, 12, 1, K, 0.15)
    for iters in (1, 3):
        on = R.online(Y[0], m["prior_xi"], m["prior_precision"], iters)
        xi, W = m["prior_xi"], m["prior_precision"]
        for t in range(12):
            r = R.run(Y[0][t:t + 1], **R.model(K, xi, W), iterations=iters)
            mean, cov = r["mean"][-1], r["cov"][-1]
            missing = np.isnan(Y[0][t]).any()
            assert _rel(on["mean"][t], mean) < 1e-11 and _rel(on["cov"][t], cov) < 1e-11
            assert on["fe"][t] == 0.0 if missing else abs(on["fe"][t] - r["fe"][-1]) < 1e-10 * max(1.0, abs(r["fe"][-1]))
            W = np.linalg.inv(cov)                                                        # the posterior in weighted-mean / precision form
            W = 0.5 * (W + W.T)
            xi = W @ mean


def test_reference_assertions_on_the_golden_draws():
    """multinomialreg_tests.jl:48-54 and :107-114 on tests/golden/mnreg_seed1.npz and mnreg_online_seed1.npz (seed 1 of the recipe: seeds 2 and 3 do not
    reach |F₉₉ − F₁₀₀| < 1e-8 in 100 iterations).  `F[end] <= F[end − 1]` to the resolution of fp64 at |F| (mnreg_ref.fe_resolution): in 50 digits
    F₉₉ − F₁₀₀ = 2.7e-21."""
    Y, p, W0, N = R.golden()
    assert Y.shape == (1000, 10) and np.all(Y.sum(axis=1) == N) and N == 20
    Yr, pr, W0r = R.recipe(1, 20, 10, 1000)
    assert np.array_equal(Y, Yr) and np.array_equal(p, pr) and np.array_equal(W0, W0r)
    m = R.model(10, None, W0)
    r = R.run(Y, **m, iterations=100, want_cond=True)
    fe = r["fe"]
    mse = float(np.mean((R.logistic_stick_breaking(r["mean"][-1]) - p) ** 2))
    assert mse < 2e-5 and fe[-1] < fe[0] and R.does_not_rise(fe[-2:], 9) and abs(fe[-2] - fe[-1]) < 1e-8
    assert abs(fe[0] - R.RECORDED_FE[0]) < 1e-9 * fe[0] and abs(fe[-1] - R.RECORDED_FE[1]) < 1e-9 * fe[-1]
    assert abs(fe[0] - 16164.787492) < 1e-5 and abs(fe[-1] - 13540.5956155703) < 1e-9 * fe[-1]      # the figures of the issue's prototype
    assert r["cond"].max() <= 1e8
    Y, p, W0, N = R.golden("mnreg_online_seed1")
    assert Y.shape == (5000, 40) and np.all(Y.sum(axis=1) == N) and N == 50
    o = R.online(Y, np.zeros(39), W0, 1)
    mse = float(np.mean((R.logistic_stick_breaking(o["mean"][-1]) - p) ** 2))
    assert mse < 1e-3 and o["fe"][-1] < o["fe"][0]
    assert abs(o["fe"][0] - R.RECORDED_FE_ONLINE[0]) < 1e-9 * o["fe"][0] and abs(o["fe"][-1] - R.RECORDED_FE_ONLINE[1]) < 1e-9 * o["fe"][-1]
    assert abs(o["fe"][0] - 369.858) < 1e-3 and abs(o["fe"][-1] - 47.846) < 1e-3


def test_stick_breaking_map():
    import rxhip
    m = np.random.default_rng(3).standard_normal(9)
    p = R.logistic_stick_breaking(m)
    assert abs(p.sum() - 1.0) < 1e-15 and np.all(p > 0) and np.allclose(rxhip.logistic_stick_breaking(m), p, rtol=1e-13, atol=1e-15)
    assert np.allclose(R.logistic_stick_breaking(np.zeros(3)), [0.5, 0.25, 0.125, 0.125])

"""What pins tests/binreg_ref.py (the CPU restatement of the binomial regression engine) independently of the engine:
(a) with n_i = 1 its F is minus the Jaakkola–Jordan bound as Bishop writes it (10.164); (b) at d = 1 its F is an upper bound of −ln p(y) by
quadrature over β; (c) ω̄ is minus the derivative of the Pólya-Gamma Laplace transform at 0; (d) F written as a function of free (m, V, c) rises
when any block leaves its update, and does not rise between iterations; (e) the reference's own assertions on data drawn by its recipe;
(f) every random case any test uses keeps cond W ≤ 1e8 at every iteration."""
import math

import numpy as np
import pytest

import binreg_ref as R


def test_a_bernoulli_case_is_minus_the_jaakkola_jordan_bound():
    """Bishop (10.164) with ξ_n = c_n, λ(ξ) = tanh(ξ/2)/(4ξ), t_n = y_n:
    L = ½ ln(|V_N|/|V_0|) + ½ m_Nᵀ V_N⁻¹ m_N − ½ m_0ᵀ V_0⁻¹ m_0 + Σ_n [ln σ(ξ_n) − ½ ξ_n + λ(ξ_n) ξ_n²], which is the bound at q(β) = N(m_N, V_N) computed
    from the SAME ξ: the restatement's F after one iteration started at (m, V) uses c from (m, V), exactly this."""
    r = np.random.default_rng(5)
    N, d = 200, 3
    X = r.standard_normal((N, d))
    y = (r.random(N) < 0.5).astype(np.float64)
    n = np.ones(N)
    W0 = 0.5 * np.eye(d) + 0.1
    xi0 = np.array([0.1, -0.2, 0.3])
    for iters in (1, 3, 40):
        out = R.run(X, y, n, xi0, W0, R.model(d, xi0, W0)["init"], iters)
        m, V, c = out["mean"][-1], out["cov"][-1], out["c"]
        lam = np.tanh(0.5 * c) / (4.0 * c)
        m0 = np.linalg.solve(W0, xi0)
        L = (0.5 * (np.linalg.slogdet(V)[1] + np.linalg.slogdet(W0)[1]) + 0.5 * m @ np.linalg.solve(V, m) - 0.5 * m0 @ W0 @ m0
             + np.sum(-np.logaddexp(0.0, -c) - 0.5 * c + lam * c * c))
        assert abs(out["fe"][-1] + L) < 1e-10 * max(1.0, abs(L)), (iters, out["fe"][-1], -L)


def test_b_one_feature_bounds_the_evidence_by_quadrature():
    X, y, n = R.reference_recipe(3, N=30, beta=np.array([0.7]))
    xi0, W0 = np.array([0.3]), np.array([[2.0]])
    out = R.run(X, y, n, xi0, W0, R.model(1, xi0, W0)["init"], 200)
    b = np.linspace(-6.0, 6.0, 200001)
    m0 = xi0[0] / W0[0, 0]
    lp = -0.5 * W0[0, 0] * (b - m0) ** 2 + 0.5 * math.log(W0[0, 0] / (2.0 * math.pi))
    ps = X[:, 0][:, None] * b[None, :]
    lchoose = R._lgamma(n + 1.0) - R._lgamma(y + 1.0) - R._lgamma(n - y + 1.0)
    ll = np.sum(lchoose[:, None] + y[:, None] * ps - n[:, None] * np.logaddexp(0.0, ps), axis=0)
    t = lp + ll
    logev = t.max() + math.log(np.sum(np.exp(t - t.max())) * (b[1] - b[0]))
    gap = out["fe"][-1] + logev
    print("F", out["fe"][-1], "-ln p(y)", -logev, "gap", gap)
    assert 0.0 <= gap < 0.5          # a bound, and a tight one: the gap is the KL of the factorised q to the posterior


def test_c_pg_mean_is_the_derivative_of_the_laplace_transform():
    """E[exp(−tω)] = coshⁿ(c/2) / coshⁿ(√(c² + 2t)/2) for ω ~ PG(n, c): ω̄ = −d/dt at t = 0, by a central difference in logs"""
    for n in (1.0, 7.0, 20.0):
        for c in (0.03, 0.5, 2.0, 9.0, 40.0):              # (2h < c²: the root stays real)
            h = 1e-5 * max(c * c, 1.0)
            f = lambda t: -n * (R.log_2cosh_half(math.sqrt(c * c + 2.0 * t)) - R.log_2cosh_half(c))   # ln E[exp(−tω)]
            num = -(f(h) - f(-h)) / (2.0 * h)
            assert abs(num - R.pg_mean(n, c)) < 1e-6 * R.pg_mean(n, c), (n, c, num, R.pg_mean(n, c))
    assert R.pg_mean(8.0, 0.0) == 2.0


def test_d_each_block_minimises_F_and_F_does_not_rise():
    X, y, n, mdl = R.random_case(77, 60, 1, 3, 0.1)
    X, y, n = X[0], y[0], n[0]
    xi0, W0 = mdl["prior_xi"], mdl["prior_precision"]
    out = R.run(X, y, n, xi0, W0, mdl["init"], 6)
    assert np.all(np.diff(out["fe"]) <= 1e-10 * np.abs(out["fe"][1:]))
    r = np.random.default_rng(1)
    for it in (1, 5):
        m, V, c = out["mean"][it], out["cov"][it], out["c"] if it == 5 else R.run(X, y, n, xi0, W0, mdl["init"], it + 1)["c"]
        F = R.free_energy_of(X, y, n, xi0, W0, m, V, c)
        assert abs(F - out["fe"][it]) < 1e-10 * abs(F)                     # the iteration's F is this function at its own point
        for _ in range(5):                                                  # q(β) is at ITS minimum given c: any other (m, V) is worse
            dm = 1e-2 * r.standard_normal(3)
            A = 1e-2 * r.standard_normal((3, 3))
            assert R.free_energy_of(X, y, n, xi0, W0, m + dm, V, c) > F
            assert R.free_energy_of(X, y, n, xi0, W0, m, V + A @ A.T, c) > F
            assert R.free_energy_of(X, y, n, xi0, W0, m, 0.97 * V, c) > F
        c_new = np.sqrt(np.einsum("ij,jk,ik->i", X, V + np.outer(m, m), X))  # q(ω) at its minimum given q(β): c_i² = x_iᵀSx_i, any other c is worse
        F_new = R.free_energy_of(X, y, n, xi0, W0, m, V, c_new)
        assert F_new <= F + 1e-12 * abs(F)
        for _ in range(5):
            assert R.free_energy_of(X, y, n, xi0, W0, m, V, c_new * np.exp(0.05 * r.standard_normal(len(c_new)))) > F_new


@pytest.fixture(scope="module")
def reference_run():
    X, y, n = R.reference_batch()
    return R.run_batch(X, y, n, np.zeros(2), np.eye(2), R.model(2)["init"], 100, want_cond=True)


def test_e_the_references_own_assertions(reference_run):
    """binomialreg_tests.jl:97-106 on 20 data sets of its recipe"""
    fe = reference_run["fe"]
    assert fe.shape == (100, 20)
    assert np.all(fe[-1] < fe[0])
    assert np.all(np.diff(fe, axis=0) <= 1e-10 * np.abs(fe[1:]))
    cov = R.coverage(reference_run["mean"][-1], reference_run["cov"][-1])
    print("coverage", cov)
    assert np.all(cov >= 0.8)
    assert np.all(reference_run["cond"] <= 1e8)


def test_e_golden_data_and_recorded_free_energies():
    X, y, n = R.golden_data()
    assert X.shape == (1000, 2) and y.shape == (1000,) and n.shape == (1000,)
    assert np.all((n >= 5) & (n <= 20) & (y >= 0) & (y <= n))
    out = R.run(X, y, n, np.zeros(2), np.eye(2), R.model(2)["init"], 100, want_cond=True)
    print("F after iterations 1 and 100:", repr(out["fe"][0]), repr(out["fe"][-1]))
    for got, want in zip((out["fe"][0], out["fe"][-1]), R.RECORDED_FE):
        assert abs(got - want) < 1e-8 * abs(want)
    assert out["fe"][-1] < out["fe"][0] and np.all(out["cond"] <= 1e8)
    assert np.all(R.coverage(out["mean"][-1][None], out["cov"][-1][None]) == 1.0)


def all_random_cases():
    cases = [R.case(spec) for group in R.CASES.values() for spec in group]
    cases += [R.size_case(d, N) for d in (1, 2, 4, 5, 16, 17, 32) for N in R.sizes_for(d)[:4]]
    cases += [R.size_case(d, R.sizes_for(d)[4]) for d in (4, 16, 32)]
    return cases


def test_f_every_random_case_is_well_conditioned():
    worst = 0.0
    for X, y, n, mdl, iters in all_random_cases():
        out = R.run_batch(X, y, n, **mdl, iterations=iters, want_cond=True)
        worst = max(worst, float(out["cond"].max()))
        assert np.all(np.isfinite(out["fe"]))
        assert np.all(np.diff(out["fe"], axis=0) <= 1e-9 * np.abs(out["fe"][1:]))
    print("worst cond W:", worst)
    assert worst <= 1e8

"""CPU restatement of the binomial regression engine (include/rxhip.h rxhip_binreg_desc, csrc/binreg_kernels.hpp), reference model
test/models/regression/binomialreg_tests.jl: `β ~ MvNormalWeightedMeanPrecision(ξ0, W0); y[i] ~ BinomialPolya(X[i], n_trials[i], β)`, coordinate-ascent VMP
under Pólya-Gamma augmentation with q(β, ω) = q(β) Π q(ω_i).  Plain numpy, nothing of the engine.

One iteration, from q(β) = N(m, V):  S = V + m mᵀ, c_i² = x_iᵀ S x_i, ω̄_i = n_i tanh(c_i/2)/(2 c_i), G = Σ_obs ω̄_i x_i x_iᵀ,
P = Σ_obs(−n_i ln(2 cosh(c_i/2)) + ½ c_i² ω̄_i);  W = W0 + G, V = W⁻¹, m = V ξ with ξ = ξ0 + Σ_obs (y_i − n_i/2) x_i;
F = −[lc + mᵀ(ξ − ξ0) − ½ tr((V + m mᵀ) G) + P] + KL(N(m, V) ‖ N(W0⁻¹ξ0, W0⁻¹)), lc = Σ_obs ln C(n_i, y_i).  A NaN y_i is missing.

What pins it, independently of the engine: tests/test_binreg_ref_cpu.py (the Jaakkola–Jordan bound at n_i = 1, the evidence by quadrature at d = 1,
ω̄ against the Pólya-Gamma Laplace transform, F as a function of free (m, V, c), the reference's own assertions)."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TRUE_BETA = np.array([-1.0, 0.6])     # binomialreg_tests.jl:28
# this iteration on tests/golden/binreg_seed1.npz (zero ξ0, unit W0): F after iterations 1 and 100
RECORDED_FE = (1885.1305316532219, 1793.2285605678721)

_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def log_2cosh_half(c):
    """ln(2 cosh(c/2)), c ≥ 0"""
    c = np.abs(c)
    return 0.5 * c + np.log1p(np.exp(-c))


def pg_mean(n, c):
    """E[ω], ω ~ PG(n, c): n tanh(c/2)/(2c), n/4 at c = 0"""
    c = np.asarray(c, dtype=np.float64)
    safe = np.where(c > 1e-6, c, 1.0)
    return np.where(c > 1e-6, n * np.tanh(0.5 * safe) / (2.0 * safe), 0.25 * n * (1.0 - c * c / 12.0))


def model(d, prior_xi=None, prior_precision=None, init=None):
    """The engine's arguments with the defaults filled in: zero ξ0, unit W0; an init of None = the prior's W0⁻¹ξ0, W0⁻¹"""
    xi0 = np.zeros(d) if prior_xi is None else np.array(prior_xi, dtype=np.float64).reshape(d)
    W0 = np.eye(d) if prior_precision is None else np.array(prior_precision, dtype=np.float64).reshape(d, d)
    if init is None:
        V = np.linalg.inv(W0)
        init = (V @ xi0, V)
    return dict(prior_xi=xi0, prior_precision=W0, init=(np.array(init[0], dtype=np.float64), np.array(init[1], dtype=np.float64)))


def data_terms(X, y, n, xi0):
    """observed mask, ξ, lc"""
    obs = ~np.isnan(y)
    yo, no = y[obs], n[obs]
    xi = xi0 + X[obs].T @ (yo - 0.5 * no)
    lc = float(np.sum(_lgamma(no + 1.0) - _lgamma(yo + 1.0) - _lgamma(no - yo + 1.0)))
    return obs, xi, lc


def kl_to_prior(m, V, xi0, W0):
    d = len(m)
    m0 = np.linalg.solve(W0, xi0)
    return 0.5 * (np.trace(W0 @ V) + (m - m0) @ W0 @ (m - m0) - d - np.linalg.slogdet(W0)[1] - np.linalg.slogdet(V)[1])


def free_energy_of(X, y, n, xi0, W0, m, V, c):
    """F as a function of FREE q(β) = N(m, V) and q(ω_i) = PG(n_i, c_i) (c [N]; entries at missing points are not read):
    −Σ_obs E[ln p(y_i, ω_i | β)/q(ω_i)] + KL(q(β) ‖ p(β)) with E_q(β)[(x_iᵀβ)²] = x_iᵀ(V + m mᵀ)x_i.  The iteration's F is this at its own c and (m, V)."""
    obs, xi, lc = data_terms(X, y, n, xi0)
    Xo, no, co = X[obs], n[obs], np.asarray(c, dtype=np.float64)[obs]
    w = pg_mean(no, co)
    q2 = np.sum((Xo @ (V + np.outer(m, m))) * Xo, axis=1)
    like = lc + m @ (xi - xi0) - 0.5 * np.sum(w * q2) + np.sum(-no * log_2cosh_half(co) + 0.5 * co * co * w)
    return -like + kl_to_prior(m, V, xi0, W0)


def run(X, y, n, prior_xi, prior_precision, init, iterations, want_cond=False):
    """One problem.  dict(mean [it][d], cov [it][d][d], fe [it], c [N] of the last iteration's step 1 (, cond [it] of W))"""
    X, y, n = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(n, dtype=np.float64)
    xi0, W0 = prior_xi, prior_precision
    obs, xi, lc = data_terms(X, y, n, xi0)
    Xo, no = X[obs], n[obs]
    m, V = init
    means, covs, fes, conds = [], [], [], []
    c = np.zeros(len(y))
    for _ in range(iterations):
        S = V + np.outer(m, m)
        c2 = np.maximum(np.sum((Xo @ S) * Xo, axis=1), 0.0)
        co = np.sqrt(c2)
        w = pg_mean(no, co)
        G = (Xo * w[:, None]).T @ Xo
        P = np.sum(-no * log_2cosh_half(co) + 0.5 * c2 * w)
        W = W0 + G
        V = np.linalg.inv(W)
        V = 0.5 * (V + V.T)
        m = V @ xi
        F = -(lc + m @ (xi - xi0) - 0.5 * np.trace((V + np.outer(m, m)) @ G) + P) + kl_to_prior(m, V, xi0, W0)
        means.append(m)
        covs.append(V)
        fes.append(F)
        conds.append(np.linalg.cond(W))
        c = np.zeros(len(y))
        c[obs] = co
    out = dict(mean=np.array(means), cov=np.array(covs), fe=np.array(fes), c=c)
    if want_cond:
        out["cond"] = np.array(conds)
    return out


def run_batch(X, y, n, prior_xi, prior_precision, init, iterations, want_cond=False):
    """X [C][N][d], y, n [C][N] -> mean [it][C][d], cov [it][C][d][d], fe [it][C] (, cond [it][C])"""
    rs = [run(X[k], y[k], n[k], prior_xi, prior_precision, init, iterations, want_cond) for k in range(len(X))]
    out = dict(mean=np.stack([r["mean"] for r in rs], 1), cov=np.stack([r["cov"] for r in rs], 1), fe=np.stack([r["fe"] for r in rs], 1))
    if want_cond:
        out["cond"] = np.stack([r["cond"] for r in rs], 1)
    return out


def contract_errors(got, ref):
    """means in posterior standard deviations, covariances relative to √(v_i v_j), F relative with denominator max(1, |F|)"""
    sd = np.sqrt(np.einsum("...ii->...i", ref["cov"]))
    e = dict(mean=float(np.max(np.abs(got["mean"] - ref["mean"]) / sd)),
             cov=float(np.max(np.abs(got["cov"] - ref["cov"]) / np.sqrt(sd[..., :, None] * sd[..., None, :] * sd[..., :, None] * sd[..., None, :]))))
    if got.get("fe") is not None:
        e["fe"] = float(np.max(np.abs(got["fe"] - ref["fe"]) / np.maximum(1.0, np.abs(ref["fe"]))))
    return e


def hold(got, ref):
    """asserts the contract: means 1e-6 posterior standard deviations, covariances 1e-6 relative to √(v_i v_j), F 1e-8 relative; returns the errors"""
    for k in ("mean", "cov", "fe"):
        if got.get(k) is not None:
            assert np.shape(got[k]) == np.shape(ref[k]), (k, np.shape(got[k]), np.shape(ref[k]))
            assert np.all(np.isfinite(got[k])), k
    e = contract_errors(got, ref)
    print("  ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["mean"] < 1e-6 and e["cov"] < 1e-6 and e.get("fe", 0.0) < 1e-8, e
    return e


def reference_recipe(seed, N=1000, beta=TRUE_BETA):
    """generate_synthetic_binomial_data (binomialreg_tests.jl:6-25) with numpy's default_rng(seed) in place of StableRNG(seed): X ~ N(0, 1),
    n_trials uniform on 5 … 20, y_i ~ Binomial(n_i, σ(x_iᵀβ)).  The recipe, not the reference's bits."""
    r = np.random.default_rng(seed)
    X = r.standard_normal((N, len(beta)))
    n = r.integers(5, 21, N).astype(np.float64)
    y = r.binomial(n.astype(np.int64), 1.0 / (1.0 + np.exp(-X @ beta))).astype(np.float64)
    return X, y, n


def reference_batch():
    """the 20 simulations of binomialreg_tests.jl:60-91 as one batch: X [20][1000][2], y, n [20][1000]"""
    sims = [reference_recipe(s) for s in range(1, 21)]
    return tuple(np.stack([s[k] for s in sims]) for k in range(3))


def coverage(mean, cov, beta=TRUE_BETA):
    """fraction of problems whose 95 % credible interval of each feature holds the true β (binomialreg_tests.jl:82-106); mean [C][d], cov [C][d][d]"""
    sd = np.sqrt(np.einsum("...ii->...i", cov))
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)((beta - mean) / (sd * math.sqrt(2.0))))
    return np.mean((cdf >= 0.025) & (cdf <= 0.975), axis=0)


def golden_data():
    """(X [1000][2], y [1000], n_trials [1000]) of tests/golden/binreg_seed1.npz (tests/golden/make_binreg_golden.py)"""
    g = np.load(os.path.join(HERE, "golden", "binreg_seed1.npz"))
    return g["X"].astype(np.float64), g["y"].astype(np.float64), g["n_trials"].astype(np.float64)


def random_case(seed, N, C, d, missing=0.0, degenerate=False):
    """X ~ N(0, 1/d), β ~ N(0, 4), n_i uniform on 0 … 20 (n_i = 0 occurs), a random SPD prior precision and a nonzero ξ0; `missing`: the fraction of
    y set to NaN; `degenerate`: problem 0 gets an all-zero row (c = 0), a row scaled by 1e-9, a row scaled by 1e3 and then to c ≈ 1500 under the
    initial q(β), a missing y and an n_i = 0 (as many of them as N allows, in this order)."""
    r = np.random.default_rng(seed)
    X = r.standard_normal((C, N, d)) / math.sqrt(d)
    bt = 2.0 * r.standard_normal((C, d))
    n = r.integers(0, 21, (C, N)).astype(np.float64)
    A = r.standard_normal((d, d)) / math.sqrt(d)
    W0 = np.eye(d) + 0.5 * A @ A.T
    xi0 = 0.3 * r.standard_normal(d)
    if degenerate:
        S0 = np.linalg.inv(W0)
        S0 = S0 + np.outer(S0 @ xi0, S0 @ xi0)
        rows = list(range(min(N, 5)))
        if len(rows) > 0:
            X[0, rows[0]] = 0.0
        if len(rows) > 1:
            X[0, rows[1]] *= 1e-9
        if len(rows) > 2:
            X[0, rows[2]] *= 1500.0 / math.sqrt(X[0, rows[2]] @ S0 @ X[0, rows[2]])
            n[0, rows[2]] = 7.0
        if len(rows) > 4:
            n[0, rows[4]] = 0.0
    y = r.binomial(n.astype(np.int64), 0.5 * (1.0 + np.tanh(0.5 * np.einsum("cnd,cd->cn", X, bt)))).astype(np.float64)
    if missing:
        y[r.random((C, N)) < missing] = np.nan
    if degenerate and N > 3:
        y[0, 3] = np.nan
    return X, y, n, model(d, xi0, W0)


# Every random case of the host and GPU tests, by group: (seed, N, problems, d, missing, degenerate, iterations).  tests/test_binreg_ref_cpu.py
# asserts cond W ≤ 1e8 at every iteration of each, which leaves the contract two decades over cond·ε.  Seeds passed over because they broke that
# condition: none.  The N of the "sizes" group are filled in from the schedule (tile − 1, tile, tile + 1, and one N at which a workgroup takes two
# tiles) by sizes_for().
CASES = dict(
    host=[(300 + i, N, C, d, 0.1, True, 4) for i, (N, C, d) in enumerate([(40, 2, 1), (33, 1, 2), (17, 2, 3), (29, 1, 4), (50, 2, 5), (70, 1, 16), (90, 1, 17),
                                                                            (120, 2, 32), (1, 1, 2), (1, 1, 7), (3, 1, 32)])],
    degenerate=[(330 + d, 300, 2, d, 0.1, True, 4) for d in (1, 2, 4, 5, 16, 17, 32)],
    batch=[(340, 700, 5, 2, 0.05, False, 5), (341, 700, 5, 17, 0.05, False, 5)],
)
SMALL_TILE, SMALL_CAP, MFMA_TILE, MFMA_CAP = 256, 2048, 128, 512   # csrc/binreg_kernels.hpp breg::kSmallTile …; tests/test_binreg_gpu.py asserts them against the library


def sizes_for(d):
    """the N of the size tests at d features: 1, tile − 1, tile, tile + 1, and cap·tile + 1 (one workgroup runs its grid-stride loop twice)"""
    tile, cap = (SMALL_TILE, SMALL_CAP) if d <= 4 else (MFMA_TILE, MFMA_CAP)
    return [1, tile - 1, tile, tile + 1, cap * tile + 1]


def size_case(d, N):
    return random_case(350 + d, N, 1, d, 0.02, False) + (3,)


def case(spec):
    """(X, y, n, model, iterations) of a CASES entry"""
    seed, N, C, d, missing, degenerate, iters = spec
    return random_case(seed, N, C, d, missing, degenerate) + (iters,)

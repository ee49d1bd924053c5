"""CPU restatement of the multinomial regression engine (include/rxhip.h rxhip_mnreg_desc, csrc/mnreg_kernels.hpp), reference model
test/models/regression/multinomialreg_tests.jl: `ψ ~ MvNormalWeightedMeanPrecision(ξ0, W0); y[i] ~ MultinomialPolya(N_i, ψ)`, coordinate-ascent VMP
under stick-breaking Pólya-Gamma augmentation with q(ψ, ω) = q(ψ) Π q(ω_ik).  Plain numpy, nothing of the engine.

Statistics over the observed rows (a row with any NaN is missing): Y_k = Σ_i y_ik, S_k = Σ_i N_ik with N_ik = Σ_{j≥k} y_ij, n = rows,
lc = Σ_i [lnΓ(N_i + 1) − Σ_k lnΓ(y_ik + 1)], κ_k = Y_k − S_k/2, ξ = ξ0 + κ.
One iteration, from q(ψ) = N(m, V):  c_k² = m_k² + V_kk, ω̄_k = S_k tanh(c_k/2)/(2 c_k), P = Σ_k(−S_k ln(2 cosh(c_k/2)) + ½ c_k² ω̄_k);
W = W0 + diag(ω̄), V = W⁻¹, m = V ξ;  F = −[lc + mᵀκ − ½ Σ_k (V_kk + m_k²) ω̄_k + P] + KL(N(m, V) ‖ N(W0⁻¹ξ0, W0⁻¹)).
Online: step t takes the current (ξ, W) as its prior, starts from N(W⁻¹ξ, W⁻¹), runs the iterations on row t alone, then ξ += κ_t,
W += diag(ω̄_t); F_t is the one-row free energy of the last iteration against the step's prior; a missing row changes nothing and has F_t = 0.

What pins it, independently of the engine: tests/test_mnreg_ref_cpu.py (the 50-digit statement tests/mnreg_mp.py, tests/binreg_ref.py on the
expanded problem, S against the per-row remainders, F as a function of free (m, V, c), online ≡ chained one-row problems, the reference's own
assertions on the golden sets)."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# this iteration on tests/golden/mnreg_seed1.npz: F after iterations 1 and 100; on mnreg_online_seed1.npz (one iteration per step): F_1 and F_T
RECORDED_FE = (16164.787492417712, 13540.595615570262)
RECORDED_FE_ONLINE = (369.8580151218972, 47.84587943786684)

# "F does not rise" between two fp64 evaluations is decided to fe_resolution(d) ulps of max(1, |F|): F is assembled from 4d + 4 terms (S_k ln 2cosh, ½c_k²ω̄_k,
# m_kκ_k, ½(V_kk + m_k²)ω̄_k per k; lc, the trace, the quadratic form and the log-determinants of the KL), each carrying at least one rounding of its
# own size, which on the golden set reaches 4|F| (Σ_k S_k ln 2cosh = 5.6e4 at F = 1.35e4), in two evaluations: 2 · 4 · (4d + 4) ulps.  At d = 9 that is
# 5.8e-10 at F = 13540.6, against the reference's own convergence tolerance of 1e-8 (and the 1e-9·|F| the binomial engine's tests allow).
def fe_resolution(d):
    return 8 * (4 * d + 4)


def does_not_rise(fe, d):
    """fe [iterations][...]: no entry above its predecessor by more than fe_resolution(d) ulps"""
    fe = np.asarray(fe)
    return bool(np.all(np.diff(fe, axis=0) <= fe_resolution(d) * np.spacing(np.maximum(1.0, np.abs(fe[1:])))))


_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def log_2cosh_half(c):
    c = np.abs(c)
    return 0.5 * c + np.log1p(np.exp(-c))


def pg_mean(n, c):
    """E[ω], ω ~ PG(n, c): n tanh(c/2)/(2c), n/4 at c = 0"""
    c = np.asarray(c, dtype=np.float64)
    safe = np.where(c > 1e-6, c, 1.0)
    return np.where(c > 1e-6, n * np.tanh(0.5 * safe) / (2.0 * safe), 0.25 * n * (1.0 - c * c / 12.0))


def logistic_stick_breaking(m):
    """p_k = σ(m_k)(1 − Σ_{j<k} p_j), p_K the remainder"""
    p = np.empty(len(m) + 1)
    for k, v in enumerate(m):
        p[k] = (1.0 - p[:k].sum()) / (1.0 + math.exp(-v))
    p[-1] = 1.0 - p[:-1].sum()
    return p


def model(K, prior_xi=None, prior_precision=None, init=None):
    """The engine's arguments with the defaults filled in: zero ξ0, unit W0; an init of None = the prior's W0⁻¹ξ0, W0⁻¹"""
    d = K - 1
    xi0 = np.zeros(d) if prior_xi is None else np.array(prior_xi, dtype=np.float64).reshape(d)
    W0 = np.eye(d) if prior_precision is None else np.array(prior_precision, dtype=np.float64).reshape(d, d)
    if init is None:
        V = np.linalg.inv(W0)
        init = (V @ xi0, V)
    return dict(prior_xi=xi0, prior_precision=W0, init=(np.array(init[0], dtype=np.float64), np.array(init[1], dtype=np.float64)))


def observed(Y):
    return ~np.isnan(Y).any(axis=-1)


def remainders(Y):
    """N_ik = Σ_{j≥k} y_ij for every row, [rows][K]"""
    return np.cumsum(Y[..., ::-1], axis=-1)[..., ::-1]


def statistics(Y):
    """Y [N][K] -> dict(Y [K], S [K] (S_K = Y_K), n, lc): column sums over the observed rows, S from the identity S_k = Σ_{j≥k} Y_j"""
    Yo = np.asarray(Y, dtype=np.float64)[observed(Y)]
    col = Yo.sum(axis=0) if len(Yo) else np.zeros(Y.shape[-1])
    lc = float(np.sum(_lgamma(Yo.sum(axis=1) + 1.0)) - np.sum(_lgamma(Yo + 1.0))) if len(Yo) else 0.0
    return dict(Y=col, S=np.cumsum(col[::-1])[::-1].copy(), n=float(len(Yo)), lc=lc)


def kl(m, V, mp, Wp):
    d = len(m)
    return 0.5 * (np.trace(Wp @ V) + (m - mp) @ Wp @ (m - mp) - d - np.linalg.slogdet(Wp)[1] - np.linalg.slogdet(V)[1])


def free_energy_of(S, kappa, lc, xi0, W0, m, V, c):
    """F as a function of FREE q(ψ) = N(m, V) and q(ω_ik) = PG(N_ik, c_k) (S, kappa, c over k < K)"""
    w = pg_mean(S, c)
    like = lc + m @ kappa - 0.5 * np.sum((np.diag(V) + m * m) * w) + np.sum(-S * log_2cosh_half(c) + 0.5 * c * c * w)
    return -like + kl(m, V, np.linalg.solve(W0, xi0), W0)


def iterate(S, kappa, lc, xi0, W0, init, iterations, want_cond=False):
    """the iterations from the statistics (S, kappa over k < K) under the prior (ξ0, W0): dict(mean, cov, fe, w of the last, c of the last (, cond))"""
    m, V = init
    mp = np.linalg.solve(W0, xi0)
    means, covs, fes, conds = [], [], [], []
    w = np.zeros_like(S)
    c = np.zeros_like(S)
    for _ in range(iterations):
        c2 = m * m + np.diag(V)
        c = np.sqrt(c2)
        w = pg_mean(S, c)
        P = np.sum(-S * log_2cosh_half(c) + 0.5 * c2 * w)
        W = W0 + np.diag(w)
        V = np.linalg.inv(W)
        V = 0.5 * (V + V.T)
        m = V @ (xi0 + kappa)
        F = -(lc + m @ kappa - 0.5 * np.sum((np.diag(V) + m * m) * w) + P) + kl(m, V, mp, W0)
        means.append(m)
        covs.append(V)
        fes.append(F)
        conds.append(np.linalg.cond(W))
    out = dict(mean=np.array(means), cov=np.array(covs), fe=np.array(fes), w=w, c=c)
    if want_cond:
        out["cond"] = np.array(conds)
    return out


def run(Y, prior_xi, prior_precision, init, iterations, want_cond=False):
    """One problem, Y [N][K].  dict(mean [it][d], cov [it][d][d], fe [it] (, cond [it] of W))"""
    st = statistics(Y)
    S = st["S"][:-1]
    kappa = st["Y"][:-1] - 0.5 * S
    return iterate(S, kappa, st["lc"], prior_xi, prior_precision, init, iterations, want_cond)


def run_batch(Y, prior_xi, prior_precision, init, iterations, want_cond=False):
    """Y [C][N][K] -> mean [it][C][d], cov [it][C][d][d], fe [it][C] (, cond [it][C])"""
    rs = [run(Y[k], prior_xi, prior_precision, init, iterations, want_cond) for k in range(len(Y))]
    out = dict(mean=np.stack([r["mean"] for r in rs], 1), cov=np.stack([r["cov"] for r in rs], 1), fe=np.stack([r["fe"] for r in rs], 1))
    if want_cond:
        out["cond"] = np.stack([r["cond"] for r in rs], 1)
    return out


def online(Y, prior_xi, prior_precision, iterations=1, want_cond=False):
    """One series, Y [T][K].  dict(mean [T][d], var [T][d], cov [T][d][d], fe [T] (F_t), fe_it [iterations] (Σ_t of the step's F after that many
    iterations) (, cond [T]))"""
    xi, W = np.array(prior_xi, dtype=np.float64), np.array(prior_precision, dtype=np.float64)
    T, K = Y.shape
    d = K - 1
    V = np.linalg.inv(W)
    V = 0.5 * (V + V.T)
    m = V @ xi
    means, covs, fes, conds = [], [], [], []
    fe_it = np.zeros(iterations)
    for t in range(T):
        if np.isnan(Y[t]).any():
            means.append(m)
            covs.append(V)
            fes.append(0.0)
            conds.append(np.linalg.cond(W))
            continue
        st = statistics(Y[t:t + 1])
        S = st["S"][:-1]
        kappa = st["Y"][:-1] - 0.5 * S
        r = iterate(S, kappa, st["lc"], xi, W, (m, V), iterations, want_cond=True)
        m, V = r["mean"][-1], r["cov"][-1]
        fe_it += r["fe"]
        xi = xi + kappa
        W = W + np.diag(r["w"])
        means.append(m)
        covs.append(V)
        fes.append(r["fe"][-1])
        conds.append(r["cond"].max())
    covs = np.array(covs)
    out = dict(mean=np.array(means), cov=covs, var=np.einsum("tii->ti", covs).copy(), fe=np.array(fes), fe_it=fe_it)
    if want_cond:
        out["cond"] = np.array(conds)
    return out


def online_batch(Y, prior_xi, prior_precision, iterations=1):
    """Y [C][T][K] -> mean, var [T][C][d], cov [T][C][d][d], fe [T][C], fe_it [iterations][C]"""
    rs = [online(Y[k], prior_xi, prior_precision, iterations) for k in range(len(Y))]
    return {k: np.stack([r[k] for r in rs], 1) for k in ("mean", "var", "cov", "fe", "fe_it")}


def expanded(Y):
    """the binomial regression problem this model is: per observed row and k < K a row x = e_k, n = N_ik, y = y_ik -> (X, y, n)"""
    Yo = np.asarray(Y, dtype=np.float64)[observed(Y)]
    K = Y.shape[-1]
    R = remainders(Yo)
    X = np.tile(np.eye(K - 1), (len(Yo), 1))
    return X, Yo[:, :-1].reshape(-1).copy(), R[:, :-1].reshape(-1).copy()


def contract_errors(got, ref):
    """means in posterior standard deviations, covariances (or variances) relative to √(v_i v_j), F relative with denominator max(1, |F|)"""
    if "cov" in ref:
        sd = np.sqrt(np.einsum("...ii->...i", ref["cov"]))
    else:
        sd = np.sqrt(ref["var"])
    e = dict(mean=float(np.max(np.abs(got["mean"] - ref["mean"]) / sd)))
    if got.get("cov") is not None:
        e["cov"] = float(np.max(np.abs(got["cov"] - ref["cov"]) / (sd[..., :, None] * sd[..., None, :])))
    if got.get("var") is not None:
        e["var"] = float(np.max(np.abs(got["var"] - ref["var"]) / (sd * sd)))
    if got.get("fe") is not None:
        e["fe"] = float(np.max(np.abs(got["fe"] - ref["fe"]) / np.maximum(1.0, np.abs(ref["fe"]))))
    return e


def hold(got, ref):
    """asserts the contract: means 1e-6 posterior standard deviations, covariances and variances 1e-6 relative to √(v_i v_j), F 1e-8 relative;
    returns the errors"""
    for k in ("mean", "cov", "var", "fe"):
        if got.get(k) is not None:
            assert np.shape(got[k]) == np.shape(ref[k]), (k, np.shape(got[k]), np.shape(ref[k]))
            assert np.all(np.isfinite(got[k])), k
    e = contract_errors(got, ref)
    print("  ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["mean"] < 1e-6 and e.get("cov", 0.0) < 1e-6 and e.get("var", 0.0) < 1e-6 and e.get("fe", 0.0) < 1e-8, e
    return e


def recipe(seed, N, K, nsamples):
    """generate_multinomial_data (test/utiltests.jl) and the Wishart(K, I) prior precision of multinomialreg_tests.jl with numpy's
    default_rng(seed) in place of StableRNG: in this order ψ = standard_normal(K), p = softmax(ψ), Y = multinomial(N, p, nsamples),
    A = standard_normal((K, K − 1)), W0 = AᵀA.  The recipe, not the reference's bits.  -> (Y int64 [nsamples][K], p [K], W0)"""
    r = np.random.default_rng(seed)
    psi = r.standard_normal(K)
    p = np.exp(psi - psi.max())
    p /= p.sum()
    Y = r.multinomial(N, p, nsamples)
    A = r.standard_normal((K, K - 1))
    return Y, p, A.T @ A


def golden(name="mnreg_seed1"):
    """(Y [nsamples][K] float64, p [K], W0, N) of tests/golden/<name>.npz (tests/golden/make_mnreg_golden.py)"""
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    return g["Y"].astype(np.float64), g["p"], g["W0"], int(g["N"])


def random_case(seed, N, C, K, missing=0.0):
    """row totals uniform on 0 … 20 (0 occurs), the split of a row multinomial under a random ψ ~ N(0, 1) per problem, W0 = I + ½AAᵀ/d, a nonzero
    ξ0; `missing`: the fraction of rows with a NaN (in one random entry, or all of them).  -> (Y [C][N][K], model)"""
    r = np.random.default_rng(seed)
    d = K - 1
    Y = np.empty((C, N, K))
    for c in range(C):
        psi = r.standard_normal(K)
        p = np.exp(psi - psi.max())
        p /= p.sum()
        tot = r.integers(0, 21, N)
        Y[c] = np.array([r.multinomial(t, p) for t in tot], dtype=np.float64).reshape(N, K)
    A = r.standard_normal((d, d))
    W0 = np.eye(d) + 0.5 * A @ A.T / d
    xi0 = 0.3 * r.standard_normal(d)
    if missing:
        rows = r.random((C, N)) < missing
        whole = r.random((C, N)) < 0.5
        col = r.integers(0, K, (C, N))
        for c, i in zip(*np.nonzero(rows)):
            if whole[c, i]:
                Y[c, i, :] = np.nan
            else:
                Y[c, i, col[c, i]] = np.nan
    return Y, model(K, xi0, W0)


# Every random case of the CPU and GPU tests, by group: (seed, N, problems, K, missing, iterations).  tests/test_mnreg_ref_cpu.py asserts
# cond W ≤ 1e8 at every iteration of each, which leaves the contract two decades over cond·ε.  Seeds passed over because they broke that condition: none.
CASES = dict(
    dims=[(400 + K, N, 2, K, 0.1, it) for K, N, it in [(2, 40, 4), (3, 57, 5), (5, 64, 6), (6, 71, 4), (17, 80, 5), (18, 93, 6), (33, 100, 4), (34, 111, 5),
                                                        (65, 120, 6)]],
    small=[(470 + i, N, C, K, 0.1, 4) for i, (N, C, K) in enumerate([(1, 1, 2), (1, 2, 7), (3, 1, 65), (2, 3, 34)])],
    batch=[(480, 50, 300, 10, 0.05, 3)],
    online=[(490 + K + T, T, 8, K, 0.1, it) for K in (3, 10, 34) for T, it in ((1, 1), (2, 3), (50, 1))] + [(499, 50, 8, 10, 0.1, 3)],
)
CHUNKS_CAP = 1024   # csrc/mnreg_kernels.hpp mnreg::kChunksCap; tests/test_mnreg_gpu.py asserts it and tile_rows against the library


def tile_rows(K):
    return 512 if K <= 8 else 256 if K <= 16 else 128 if K <= 32 else 64


def sizes_for(K):
    """the N of the size tests at K categories: 1, tile − 1, tile, tile + 1, and cap·tile + 1 (one workgroup runs its grid-stride loop twice)"""
    t = tile_rows(K)
    return [1, t - 1, t, t + 1, CHUNKS_CAP * t + 1]


def case(spec):
    """(Y, model, iterations) of a CASES entry"""
    seed, N, C, K, missing, iters = spec
    return random_case(seed, N, C, K, missing) + (iters,)

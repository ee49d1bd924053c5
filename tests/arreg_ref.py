"""CPU restatement (numpy, fp64) of the regression / autoregression engine's iteration (include/rxhip.h rxhip_arreg_desc, csrc/arreg_kernels.hpp), the
case generator of its tests and the contract they hold.

Model (test/models/autoregressive/ar_tests.jl:17-46): γ ~ Gamma(a0, b0), θ ~ N(m0, Λ0⁻¹), y_i ~ N(x_iᵀθ, γ⁻¹), q(γ, θ) = q(γ)q(θ).  Statistics
G = Σ x xᵀ, h = Σ y x, s = Σ y², n over the rows that count (a NaN y drops the row; in lagged mode a NaN z_t drops every row it appears in).
One iteration from q(γ) = Gamma(a, b), ḡ = a/b:  Λ = Λ0 + ḡ G, V = Λ⁻¹, m = V(Λ0 m0 + ḡ h);  a = a0 + n/2, b = b0 + R/2,
R = s − 2 mᵀh + tr((V + m mᵀ) G);  F = −[n/2 (ψ(a) − ln b − ln 2π) − ½ (a/b) R] + KL(N(m, V) ‖ N(m0, Λ0⁻¹)) + KL(Gamma(a, b) ‖ Gamma(a0, b0)).

tests/test_arreg_ref_cpu.py pins this file to a 60-digit mpmath statement, to the conjugate closed form, to the reference's own assertions on its
own data, and asserts the numerical envelope (R/s ≥ 1e-6, cond Λ ≤ 1e8 at every iteration) on every case the other tests use."""
import os

import numpy as np
from scipy.signal import lfilter
from scipy.special import digamma, gammaln

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_TILE, SMALL_CAP, MFMA_TILE, MFMA_CAP, SMALL_MAX_D = 256, 2048, 128, 512, 4   # csrc/arreg_kernels.hpp
# F after iterations 1 and 15 on the regenerated series of ar_tests.jl:48-53 (orders 1 … 5, priors and initial q(γ) of the reference), this file's
# values; the last pair is the benchmark series of :69 at order 5
RECORDED_FE = {
    1: (1432.8721941461902, 1432.8721103150529),
    2: (1455.7503820386016, 1455.748559592009),
    3: (1434.9901984144833, 1434.9899954702717),
    4: (1429.9910971577053, 1429.9910851732266),
    5: (1441.79146230053, 1441.7907483938282),
    "bench": (1443.0819807960647, 1443.0811067959507),
}


def tile_rows(d):
    return SMALL_TILE if d <= SMALL_MAX_D else MFMA_TILE


def chunks(rows, d):
    tp = tile_rows(d)
    return max(1, min((rows + tp - 1) // tp, SMALL_CAP if d <= SMALL_MAX_D else MFMA_CAP))


def model(d, prior_theta=None, prior_gamma=(1.0, 1.0), init_gamma=None):
    m0, L0 = (np.zeros(d), np.eye(d)) if prior_theta is None else (np.asarray(prior_theta[0], float), np.asarray(prior_theta[1], float))
    return dict(prior_theta=(m0, L0), prior_gamma=(float(prior_gamma[0]), float(prior_gamma[1])),
                init_gamma=None if init_gamma is None else (float(init_gamma[0]), float(init_gamma[1])))


def lag_rows(z, p):
    """ar_ssm_data (ar_tests.jl:7-15): row t = p … T−1 has y = z_t, x = (z_{t−1}, …, z_{t−p}); a row that holds a NaN gets y = NaN (dropped), x = 0"""
    z = np.asarray(z, float)
    T = len(z)
    if T <= p:
        return np.zeros((0, p)), np.zeros(0)
    W = np.lib.stride_tricks.sliding_window_view(z, p + 1)       # W[i] = z[i … i + p], row i is time t = i + p
    X, y = W[:, :p][:, ::-1].copy(), W[:, p].copy()
    bad = np.isnan(W).any(axis=1)
    X[bad], y[bad] = 0.0, np.nan
    return X, y


def statistics(X, y, dtype=np.float64):
    """G, h, s, n over the rows whose y is not NaN; dtype=np.longdouble for the bound of the statistics test"""
    keep = ~np.isnan(y)
    Xk, yk = np.asarray(X, dtype)[keep], np.asarray(y, dtype)[keep]
    return Xk.T @ Xk, Xk.T @ yk, yk @ yk, float(keep.sum())


def kl_normal(m, V, m0, L0):
    d = len(m)
    dm = m - m0
    return 0.5 * (np.trace(L0 @ V) + dm @ L0 @ dm - d - np.linalg.slogdet(L0)[1] - np.linalg.slogdet(V)[1])


def kl_gamma(a, b, a0, b0):
    return float((a - a0) * digamma(a) - gammaln(a) + gammaln(a0) + a0 * (np.log(b) - np.log(b0)) + a * (b0 - b) / b)


def residual(G, h, s, m, V):
    return s - 2.0 * (m @ h) + np.trace((V + np.outer(m, m)) @ G)


def free_energy_of(G, h, s, n, m0, L0, a0, b0, m, V, a, b):
    """F of ANY q(θ) = N(m, V), q(γ) = Gamma(a, b): the exact variational free energy"""
    R = residual(G, h, s, m, V)
    return float(-(0.5 * n * (digamma(a) - np.log(b) - np.log(2.0 * np.pi)) - 0.5 * (a / b) * R) + kl_normal(m, V, m0, L0) + kl_gamma(a, b, a0, b0))


def theta_update(G, h, m0, L0, gbar):
    L = L0 + gbar * G
    V = np.linalg.inv(L)
    V = 0.5 * (V + V.T)
    return V @ (L0 @ m0 + gbar * h), V, L


def run_stats(G, h, s, n, prior_theta, prior_gamma, init_gamma, iterations):
    """→ dict(mean [it][d], cov [it][d][d], a [it], b [it], fe [it], cond [it] of Λ, rs [it] = R/s)"""
    (m0, L0), (a0, b0) = prior_theta, prior_gamma
    ia, ib = prior_gamma if init_gamma is None else init_gamma
    gbar = ia / ib
    out = dict(mean=[], cov=[], a=[], b=[], fe=[], cond=[], rs=[])
    for _ in range(iterations):
        m, V, L = theta_update(G, h, m0, L0, gbar)
        R = residual(G, h, s, m, V)
        a, b = a0 + 0.5 * n, b0 + 0.5 * R
        out["mean"].append(m), out["cov"].append(V), out["a"].append(a), out["b"].append(b)
        out["fe"].append(free_energy_of(G, h, s, n, m0, L0, a0, b0, m, V, a, b))
        out["cond"].append(np.linalg.cond(L)), out["rs"].append(R / s if s > 0 else 1.0)
        gbar = a / b
    return {k: np.array(v) for k, v in out.items()}


def run_batch(X, y, prior_theta, prior_gamma, init_gamma, iterations, shared=False):
    """X [C][N][d], y [C][N] → arrays [iterations][G][…], G = C or 1 (shared: the statistics added over the series in ascending order)"""
    st = [statistics(X[c], y[c]) for c in range(len(X))]
    if shared:
        tot = st[0]
        for nxt in st[1:]:
            tot = tuple(a + b for a, b in zip(tot, nxt))
        st = [tot]
    runs = [run_stats(*s4, prior_theta, prior_gamma, init_gamma, iterations) for s4 in st]
    return {k: np.stack([r[k] for r in runs], axis=1) for k in runs[0]}


def run_lagged(z, p, prior_theta, prior_gamma, init_gamma, iterations, shared=False):
    """z [T][C]: the raw series"""
    z = np.asarray(z, float)
    rows = [lag_rows(z[:, c], p) for c in range(z.shape[1])]
    return run_batch(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), prior_theta, prior_gamma, init_gamma, iterations, shared)


def contract_errors(got, ref):
    """θ means in posterior standard deviations, covariances relative to √(v_i v_j), γ shape exact, γ rate relative, F relative with denominator max(1, |F|)"""
    sd = np.sqrt(np.einsum("...ii->...i", ref["cov"]))
    e = dict(mean=float(np.max(np.abs(got["mean"] - ref["mean"]) / sd)),
             cov=float(np.max(np.abs(got["cov"] - ref["cov"]) / (sd[..., :, None] * sd[..., None, :]))),
             a=float(np.max(np.abs(got["a"] - ref["a"]))), b=float(np.max(np.abs(got["b"] - ref["b"]) / np.abs(ref["b"]))))
    if got.get("fe") is not None:
        e["fe"] = float(np.max(np.abs(got["fe"] - ref["fe"]) / np.maximum(1.0, np.abs(ref["fe"]))))
    return e


def hold(got, ref):
    """asserts the contract: means 1e-6 sd, covariances 1e-6, γ shape exact, γ rate 1e-6 relative, F 1e-8 relative; returns the errors"""
    for k in ("mean", "cov", "a", "b", "fe"):
        if got.get(k) is not None:
            assert np.shape(got[k]) == np.shape(ref[k]), (k, np.shape(got[k]), np.shape(ref[k]))
            assert np.all(np.isfinite(got[k])), k
    e = contract_errors(got, ref)
    print("  ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["mean"] < 1e-6 and e["cov"] < 1e-6 and e["a"] == 0.0 and e["b"] < 1e-6 and e.get("fe", 0.0) < 1e-8, e
    return e


def non_increasing(fe):
    return bool(np.all(np.diff(fe, axis=0) <= 1e-9 * np.maximum(1.0, np.abs(fe[1:]))))


def reference_checks(fe, n_gamma, n_theta):
    """ar_tests.jl:61-65"""
    d = np.diff(fe)
    return n_gamma == 15 and n_theta == 15 and len(fe) == 15 and fe[-1] < fe[0] and bool(np.all(d[np.abs(d) > 1e-3] < 0))


def golden():
    z = np.load(os.path.join(HERE, "golden", "ar_stablerng1234.npz"))
    return z["series"], z["bench"]


# ---- the case generator -------------------------------------------------------------------------------------------------------------------------------
def random_model(rng, d):
    A = rng.standard_normal((d, d))
    return model(d, (0.3 * rng.standard_normal(d), np.eye(d) + 0.2 * A @ A.T / d), (1.0 + rng.random(), 0.5 + rng.random()),
                 (0.5 + rng.random(), 0.5 + rng.random()))


def regression_case(seed, N, C, d, missing=0.0):
    """X [C][N][d] standard normal, y = Xθ + noise of standard deviation 0.5 … 1 (so R/s stays well above 1e-6), NaN in y at rate `missing`"""
    rng = np.random.default_rng(seed)
    m = random_model(rng, d)
    X = rng.standard_normal((C, N, d))
    theta = rng.standard_normal((C, d)) / np.sqrt(d)
    y = np.einsum("cnd,cd->cn", X, theta) + (0.5 + 0.5 * rng.random((C, 1))) * rng.standard_normal((C, N))
    if missing > 0.0:
        y[rng.random((C, N)) < missing] = np.nan
    return X, y, m


def series_case(seed, T, C, p, nan_at=()):
    """z [T][C]: a stable AR(1)-like series with unit driving noise (far from a perfect fit), NaN at the given time indices of every series"""
    rng = np.random.default_rng(seed)
    m = random_model(rng, p)
    z = lfilter([1.0], [1.0, -0.6], rng.standard_normal((T, C)), axis=0)          # z_t = 0.6 z_{t−1} + e_t
    for t in nan_at:
        if 0 <= t < T:
            z[t] = np.nan
    return z, m


DIMS = (1, 2, 3, 4, 5, 16, 17, 32)
LAGS = (1, 4, 5, 8, 17, 32)


def sizes_for(d):
    """N = 1, tile − 1, tile, tile + 1"""
    t = tile_rows(d)
    return [1, t - 1, t, t + 1]


def nan_positions(T, p):
    """index 0, T − 1, and both sides of the first tile boundary of the rows (row i is time i + p; rows tile − 1 and tile)"""
    t = tile_rows(p)
    return sorted({0, T - 1, t - 1 + p, t + p} & set(range(T)))


# ---- the cases of the tests (tests/test_arreg_gpu.py, tests/test_arreg_host.py); tests/test_arreg_ref_cpu.py asserts the envelope on every one ----------
def stride_rows(d):
    """rows at which workgroup 0 strides over three tiles: (2·cap + 1) tiles"""
    return (2 * (SMALL_CAP if d <= SMALL_MAX_D else MFMA_CAP) + 1) * tile_rows(d)


def size_cases():
    """(X, y, model, iterations): d × N around a tile, one series, 3 iterations; every fifth y missing where there are at least 5 rows"""
    out = []
    for d in DIMS:
        for k, N in enumerate(sizes_for(d)):
            X, y, m = regression_case(1000 + 10 * d + k, N, 1, d)
            if N >= 5:
                y[0, 3::5] = np.nan
            out.append((X, y, m, 3))
    return out


def lag_cases():
    """(z, p, model, iterations): p × T ∈ {p, p + 1, tile − 1 + p, tile + 1 + p}, and T = tile + 1 + p with NaN at 0, T − 1 and both sides of the tile boundary"""
    out = []
    for p in LAGS:
        t = tile_rows(p)
        for k, T in enumerate((p, p + 1, t - 1 + p, t + 1 + p)):
            z, m = series_case(2000 + 10 * p + k, T, 1, p)
            out.append((z, p, m, 3))
        T = t + 1 + 2 * p
        z, m = series_case(2900 + p, T, 1, p, nan_positions(T, p))
        out.append((z, p, m, 3))
    return out


def batch_cases():
    """(X, y, model, iterations, shared): n_series 1, 3, 300; 1, 15 and 40 iterations; shared parameters at 3 series; missing y"""
    out = []
    for seed, C, d, iters, shared in ((3001, 1, 2, 1, False), (3002, 3, 5, 15, False), (3003, 300, 3, 40, False), (3004, 300, 17, 15, False),
                                      (3005, 3, 4, 40, True), (3006, 3, 16, 15, True)):
        X, y, m = regression_case(seed, 300, C, d, missing=0.05)
        out.append((X, y, m, iters, shared))
    return out


def lag_batch_cases():
    """(z, p, model, iterations, shared)"""
    out = []
    for seed, C, p, iters, shared in ((3101, 3, 2, 15, False), (3102, 300, 5, 40, False), (3103, 3, 8, 15, True), (3104, 300, 32, 2, False)):
        z, m = series_case(seed, 400, C, p, (7, 150))
        out.append((z, p, m, iters, shared))
    return out


def stride_case(k):
    """regressor mode at d = 4, 16, 32 (k = 0, 1, 2) and lagged mode at p = 4, 32 (k = 3, 4): workgroup 0 takes three tiles; (kind, data…, model, iterations)"""
    if k < 3:
        d = (4, 16, 32)[k]
        X, y, m = regression_case(4000 + d, stride_rows(d), 1, d)
        return ("reg", X, y, m, 2)
    p = (4, 32)[k - 3]
    z, m = series_case(4100 + p, stride_rows(p) + p, 1, p, (5, stride_rows(p) // 2))
    return ("lag", z, p, m, 2)


def stride_cases():
    return [stride_case(k) for k in range(5)]

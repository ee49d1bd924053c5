"""CPU restatement (numpy, float64) of the nonlinear state-space engine (include/rxhip.h rxhip_nlssm_desc, csrc/nlssm_kernels.hpp): the delta node
under Linearization and Unscented, the Kalman / VMP filter, the extended / unscented RTS smoother and the engine's free energy, written from the
definitions in the header with numpy's linear algebra (general inverses and log-determinants, not the kernels' closed forms).  The test functions
carry hand-written Jacobians; `f(x, M)` takes its elementary functions from the module M (numpy here, mpmath in tests/nlssm_mp.py, and numpy again
on tracer objects for rxhip.trace), so that every side evaluates the same formula."""
import math

import numpy as np
from scipy.special import digamma, gammaln

LOG2PI = math.log(2.0 * math.pi)
DT, G = 0.01, 9.81   # the pendulum of the reference's paper/example.jl

A2 = np.array([[0.95, 0.1], [-0.2, 0.9]])
A4 = np.array([[0.9, 0.1, 0.0, 0.05], [-0.1, 0.85, 0.1, 0.0], [0.0, -0.05, 0.9, 0.1], [0.05, 0.0, -0.1, 0.8]])


def _lin(A):
    return lambda x, M=np: [sum(float(A[i, j]) * x[j] for j in range(A.shape[1])) for i in range(A.shape[0])]


# name -> (d, f(x, M), hand-written Jacobian J(x) [d][d] in numpy).  None of them contracts strongly: with Q = 0 a contracting map shrinks the posterior
# width geometrically (0.7³⁷ ≈ 2e-6) while the mean stays of order one, which leaves the unscented envelope (|m|/sd ≤ 1e3, include/rxhip.h) within a few steps.
FUNCS = {
    "pendulum": (2, lambda x, M=np: [x[0] + DT * x[1], x[1] - G * DT * M.sin(x[0])],
                 lambda x: np.array([[1.0, DT], [-G * DT * np.cos(x[0]), 1.0]])),
    "scalar": (1, lambda x, M=np: [x[0] + 0.05 * M.sin(x[0])], lambda x: np.array([[1.0 + 0.05 * np.cos(x[0])]])),
    "coupled": (2, lambda x, M=np: [x[0] + 0.1 * x[1] * M.cos(x[0]), x[1] * M.exp(-0.1 * x[0] * x[0]) + M.tanh(x[1])],
                lambda x: np.array([[1.0 - 0.1 * x[1] * np.sin(x[0]), 0.1 * np.cos(x[0])],
                                    [-0.2 * x[0] * x[1] * np.exp(-0.1 * x[0] ** 2), np.exp(-0.1 * x[0] ** 2) + 1.0 - np.tanh(x[1]) ** 2]])),
    "four": (4, lambda x, M=np: [0.99 * x[0] + 0.1 * M.sqrt(1.0 + x[1] * x[1]), 0.98 * x[1] + 0.1 * M.log(2.0 + x[2] * x[2]),
                                 0.97 * x[2] + 0.2 * x[3] / (1.0 + x[0] * x[0]), 0.99 * x[3] + 0.1 * M.sin(x[0])],
             lambda x: np.array([[0.99, 0.1 * x[1] / np.sqrt(1.0 + x[1] ** 2), 0.0, 0.0],
                                 [0.0, 0.98, 0.2 * x[2] / (2.0 + x[2] ** 2), 0.0],
                                 [-0.4 * x[3] * x[0] / (1.0 + x[0] ** 2) ** 2, 0.0, 0.97, 0.2 / (1.0 + x[0] ** 2)],
                                 [0.1 * np.cos(x[0]), 0.0, 0.0, 0.99]])),
    "linear2": (2, _lin(A2), lambda x: A2.copy()),
    "linear4": (4, _lin(A4), lambda x: A4.copy()),
}
LINEAR = {"linear2": A2, "linear4": A4}


def unscented_weights(d, alpha=1e-3, beta=2.0, kappa=0.0):
    """(d + λ, Wm0, Wc0, Wi)"""
    sc = alpha * alpha * (d + kappa)
    wm0 = (sc - d) / sc
    return sc, wm0, wm0 + 1.0 - alpha * alpha + beta, 0.5 / sc


def delta(name, method, m, V, unscented=(1e-3, 2.0, 0.0)):
    """(m̃, Ṽ, C̃) of N(m, V) through the function `name`; method 'linearization' | 'unscented'"""
    d, f, jac = FUNCS[name]
    if method == "linearization":
        J = jac(m)
        mt = np.array(f(m), dtype=np.float64)
        Ct = V @ J.T
        Vt = J @ Ct
    else:
        sc, wm0, wc0, wi = unscented_weights(d, *unscented)
        L = np.linalg.cholesky(sc * V)
        X = [m] + [m + L[:, k] for k in range(d)] + [m - L[:, k] for k in range(d)]
        Y = [np.array(f(x), dtype=np.float64) for x in X]
        wm = [wm0] + [wi] * (2 * d)
        wc = [wc0] + [wi] * (2 * d)
        mt = sum(w * y for w, y in zip(wm, Y))
        Vt = sum(w * np.outer(y - mt, y - mt) for w, y in zip(wc, Y))
        Ct = sum(w * np.outer(x - m, y - mt) for w, x, y in zip(wc, X, Y))
    return mt, 0.5 * (Vt + Vt.T), Ct


def gauss_kl(m1, V1, m0, V0):
    """KL(N(m1, V1) ‖ N(m0, V0))"""
    d = len(m1)
    P0 = np.linalg.inv(V0)
    dm = m1 - m0
    return 0.5 * (np.trace(P0 @ V1) + dm @ P0 @ dm - d + np.linalg.slogdet(V0)[1] - np.linalg.slogdet(V1)[1])


def gamma_kl(a1, b1, a0, b0):
    """KL(Gamma(a1, b1) ‖ Gamma(a0, b0)), shape and rate"""
    return (a1 - a0) * digamma(a1) - gammaln(a1) + gammaln(a0) + a0 * (math.log(b1) - math.log(b0)) + a1 * (b0 - b1) / b1


def noise_step(mt, P, a, b, c, y, iterations):
    """the VMP iterations of one observation with unknown precision: (m′, V′, a′, b′, F per iteration)"""
    E = a / b
    fes = []
    for _ in range(iterations):
        k = P @ c
        s = c @ k
        g = E / (1.0 + E * s)
        mn = mt + k * g * (y - c @ mt)
        Vn = P - g * np.outer(k, k)
        an = a + 0.5
        e2 = (y - c @ mn) ** 2 + c @ Vn @ c
        bn = b + 0.5 * e2
        E = an / bn
        fes.append(gauss_kl(mn, Vn, mt, P) + gamma_kl(an, bn, a, b) + 0.5 * (LOG2PI - (digamma(an) - math.log(bn)) + (an / bn) * e2))
    return mn, 0.5 * (Vn + Vn.T), an, bn, fes


def run_series(name, y, m0, V0, Q, H, R=None, noise=None, method="linearization", mode="filter", iterations=1, unscented=(1e-3, 2.0, 0.0)):
    """One series, y [T][dy] (NaN = missing).  Returns dict(mean [T][d], cov [T][d][d], shape [T], rate [T], fe, fe_iter [T][iterations])."""
    d = FUNCS[name][0]
    T = y.shape[0]
    H = np.atleast_2d(H)
    m, V = np.array(m0, dtype=np.float64), np.array(V0, dtype=np.float64)
    a, b = noise if noise is not None else (1.0, 1.0)
    fm, fV, pm, pP, pC = [], [], [], [], []
    shape, rate, fe, fe_iter = np.zeros(T), np.zeros(T), 0.0, np.zeros((T, iterations))
    for t in range(T):
        mt, Vt, Ct = delta(name, method, m, V, unscented)
        P = Vt + Q
        pm.append(mt); pP.append(P); pC.append(Ct)
        if np.any(np.isnan(y[t])):
            m, V = mt, P
        elif noise is not None:
            m, V, a, b, fes = noise_step(mt, P, a, b, H[0], y[t, 0], iterations)
            fe += fes[-1]
            fe_iter[t] = fes
        else:
            S = H @ P @ H.T + R
            r = y[t] - H @ mt
            K = P @ H.T @ np.linalg.inv(S)
            m = mt + K @ r
            V = P - K @ S @ K.T
            V = 0.5 * (V + V.T)
            fe += 0.5 * (len(r) * LOG2PI + np.linalg.slogdet(S)[1] + r @ np.linalg.solve(S, r))
        fm.append(m); fV.append(V)
        shape[t], rate[t] = a, b
    mean, cov = np.array(fm), np.array(fV)
    if mode == "smooth":
        for t in range(T - 2, -1, -1):
            Gn = pC[t + 1] @ np.linalg.inv(pP[t + 1])
            mean[t] = fm[t] + Gn @ (mean[t + 1] - pm[t + 1])
            Vs = fV[t] + Gn @ (cov[t + 1] - pP[t + 1]) @ Gn.T
            cov[t] = 0.5 * (Vs + Vs.T)
    return dict(mean=mean, cov=cov, shape=shape, rate=rate, fe=fe, fe_iter=fe_iter)


def run_batch(name, y, m0, V0, Q, H, per_series=False, **kw):
    """y [T][S][dy]; per_series: m0 [S][d], V0 [S][d][d].  Arrays with the series axis second, as the engine returns them."""
    S = y.shape[1]
    outs = [run_series(name, y[:, s], m0[s] if per_series else m0, V0[s] if per_series else V0, Q, H, **kw) for s in range(S)]
    return dict(mean=np.stack([o["mean"] for o in outs], 1), cov=np.stack([o["cov"] for o in outs], 1), shape=np.stack([o["shape"] for o in outs], 1),
                rate=np.stack([o["rate"] for o in outs], 1), fe=np.array([o["fe"] for o in outs]), fe_iter=np.stack([o["fe_iter"] for o in outs], 1))


# ---- the cases the host build and the device are held to (tests/test_nlssm_host.py, tests/test_nlssm_gpu.py) -----------------------------------
def spd(rng, n, scale=1.0):
    a = rng.standard_normal((n, n))
    return scale * (a @ a.T / n + 0.5 * np.eye(n))


def make_case(seed, name, T, S, dy, q_zero, unknown, per_series):
    """model and data of one case: a prior of moderate |m|/sd (inside the unscented envelope), data simulated from the model, 20 % of the
    observations missing, series 1 (if any) with nothing observed, the first and last step of series 0 missing"""
    rng = np.random.default_rng(seed)
    d, f, _ = FUNCS[name]
    H = np.eye(d)[:dy] + (0.1 * rng.standard_normal((dy, d)) if d > 1 else 0.0)
    R = spd(rng, dy, 2.0)
    Q = np.zeros((d, d)) if q_zero else spd(rng, d, 0.05)
    # unknown noise: states of a few tenths.  The unscented mean carries an absolute error of about 1e6·ε·|f| (include/rxhip.h, envelope), which enters
    # the free energy of a step undamped; a short series has |F| of order one, so |f| of order one would use up the hundredth of the bound
    lim = 0.3 if unknown else 1.0
    if per_series:
        m0 = rng.uniform(-lim, lim, (S, d))
        V0 = np.stack([spd(rng, d, 0.5) for _ in range(S)])
    else:
        m0, V0 = rng.uniform(-lim, lim, d), spd(rng, d, 0.5)
    y = np.empty((T, S, dy))
    Lq = np.linalg.cholesky(Q + 1e-300 * np.eye(d)) if not q_zero else np.zeros((d, d))
    for s in range(S):
        x = (m0[s] if per_series else m0) + 0.3 * lim * rng.standard_normal(d)
        for t in range(T):
            x = np.array(f(x)) + Lq @ rng.standard_normal(d)
            y[t, s] = H @ x + (1.5 * rng.standard_normal(dy) if unknown else np.linalg.cholesky(R) @ rng.standard_normal(dy))
    y[rng.random((T, S)) < 0.2] = np.nan
    if S > 1:
        y[:, 1] = np.nan
    y[0, 0] = y[-1, 0] = np.nan
    return dict(name=name, y=y, m0=m0, V0=V0, Q=Q, H=H, R=R, noise=(2.0, 0.5) if unknown else None, per_series=per_series)


def case_grid():
    """(id, case, method, mode, iterations): d ∈ {1, 2, 4}, T ∈ {1, 5, 37}, series ∈ {1, 3, 70}, both methods, Q = 0 and Q > 0, d_y < d and
    d_y = d, shared and per-series priors, FILTER with known and unknown noise at 1 and 5 iterations, SMOOTH"""
    out = []
    # (`coupled` is for the interpreter's tests only: unobserved, its mean and width run off to 1e5 within 20 steps, where no two fp64 evaluations agree)
    shapes = [("scalar", 1, 1), ("pendulum", 1, 2), ("pendulum", 2, 2), ("four", 2, 4), ("four", 4, 4)]
    sizes = [(1, 1), (5, 3), (37, 70)]
    k = 0
    for name, dy, d in shapes:
        for T, S in sizes:
            for method in ("linearization", "unscented"):
                k += 1
                q_zero, per_series = (k // 2) % 2 == 0, k % 3 == 0
                known = make_case(100 + k, name, T, S, dy, q_zero, False, per_series)
                out.append((f"{name}-dy{dy}-T{T}-S{S}-{method}-filter", known, method, "filter", 1))
                out.append((f"{name}-dy{dy}-T{T}-S{S}-{method}-smooth", known, method, "smooth", 1))
                if dy == 1:
                    unknown = make_case(200 + k, name, T, S, 1, q_zero, True, per_series)
                    for it in (1, 5):
                        out.append((f"{name}-T{T}-S{S}-{method}-noise-it{it}", unknown, method, "filter", it))
    return out


def run_case(case, method, mode, iterations):
    kw = dict(method=method, mode=mode, iterations=iterations, per_series=case["per_series"])
    if case["noise"] is not None:
        kw["noise"] = case["noise"]
    else:
        kw["R"] = case["R"]
    return run_batch(case["name"], case["y"], case["m0"], case["V0"], case["Q"], case["H"], **kw)


def errors(got, ref, unknown):
    """the contract's gauges: mean error in posterior standard deviations, covariance error over √(V_ii V_jj), relative Gamma error, free-energy
    error over max(1, |F|) per series"""
    sd = np.sqrt(np.einsum("...ii->...i", ref["cov"]))
    e = dict(mean=float(np.max(np.abs(got["mean"] - ref["mean"]) / sd)),
             cov=float(np.max(np.abs(got["cov"] - ref["cov"]) / (sd[..., :, None] * sd[..., None, :]))),
             fe=float(np.max(np.abs(got["fe"] - ref["fe"]) / np.maximum(1.0, np.abs(ref["fe"])))))
    if unknown:
        e["gamma"] = float(max(np.max(np.abs(got["shape"] - ref["shape"]) / ref["shape"]), np.max(np.abs(got["rate"] - ref["rate"]) / ref["rate"])))
    return e


BOUNDS = dict(mean=1e-6, cov=1e-6, gamma=1e-6, fe=1e-8)

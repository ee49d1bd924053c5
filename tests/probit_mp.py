"""High-precision restatement of the probit state-space engine's iteration (one series), in mpmath at 60 digits.  Written from the model
and the textbook (parallel expectation propagation on a Gaussian chain), it shares no code with tests/probit_ref.py or with
csrc/probit_kernels.hpp: it pins the arithmetic of probit_ref.run_messages (tests/test_probit_contract_cpu.py), which in turn is what the
engine is held to (tests/test_probit_contract_gpu.py).

    x[0] ~ Normal(m0, v0);  x[k] ~ Normal(a x[k-1] + c, q);  y[k-1] ~ Probit(x[k])    k = 1 … T,  y ∈ {0, 1, NaN = missing}

One iteration: smooth the chain with the current Gaussian sites; the cavity of an observed step is its marginal without its own site; every
observed step gets a new site (ξ, w) = (m̃/ṽ − m/v, max(1/ṽ − 1/v, 1e-12)) from the moments (m̃, ṽ) of cavity × Φ(s x), all from that one
smoothing pass.  The posteriors and the free energy of iteration i are those of the Gaussian q given the sites after i updates.

The smoother is the moment form: a Kalman filter with the sites as pseudo-observations (gain form), backward likelihood messages, and the pair
covariance from conditioning the joint prediction of (x[k-1], x[k]) on what x[k] hears.  The Bethe free energy is the literal sum over factors
and variables from means, variances and pair covariances; its cancellation (small q: nearly singular pairs) costs at most ~25 of the 60 digits
at the corners of the contract grid.  The Probit energy uses the double-precision Gauss–Hermite nodes and weights of numpy, the same rule
as probit_ref.gauss_hermite: only the arithmetic differs."""
import math

import numpy as np
from mpmath import mp, mpf

DIGITS = 60

# The parameter grid of the contract (tests/test_probit_contract_gpu.py holds the engine to probit_ref.run_messages on it;
# tests/test_probit_contract_cpu.py pins run_messages to `run` at every one of its points): a point is (a, q, v0, m0, c).
GRID_A = (0.0, -0.9, 0.5, 1.0, 1.05)
GRID_Q = (1e-8, 1e-4, 1e-2, 1.0, 1e3)
GRID_V0 = (1e-4, 1.0, 1e6)
GRID_M0_C = ((0.0, 0.0), (3.0, -0.5), (-8.0, 0.3), (40.0, 0.0))
GRID = tuple((a, q, v0, m0, c) for a in GRID_A for q in GRID_Q for v0 in GRID_V0 for m0, c in GRID_M0_C)


def _log_ncdf(x):
    return mp.log(mp.ncdf(x)) if x <= 0 else mp.log1p(-mp.ncdf(-x))


def _smooth(T, a, c, q, m0, v0, xi, w):
    """Marginals, cavities (marginal without the own site) and pair covariances of the chain with sites (ξ, w) on x[1 … T]."""
    fm, fv, pm, pv = [None] * (T + 1), [None] * (T + 1), [None] * (T + 1), [None] * (T + 1)
    pm[0], pv[0] = m0, v0
    for k in range(T + 1):
        if w[k] > 0:   # pseudo-observation ξ/w with variance 1/w
            gain = pv[k] / (pv[k] + 1 / w[k])
            fm[k], fv[k] = pm[k] + gain * (xi[k] / w[k] - pm[k]), (1 - gain) * pv[k]
        else:
            fm[k], fv[k] = pm[k], pv[k]
        if k < T:
            pm[k + 1], pv[k + 1] = a * fm[k] + c, a * a * fv[k] + q
    # backward likelihood of x[k] from the steps after it, as weighted mean and precision
    bxi, bw = [mpf(0)] * (T + 1), [mpf(0)] * (T + 1)
    pair = [None] * T
    for k in range(T, 0, -1):
        lxi, lw = bxi[k] + xi[k], bw[k] + w[k]
        # N(x_k; a x + c, q) × exp(lξ x_k − ½ lw x_k²), integrated over x_k, as a function of x = x[k-1]
        bxi[k - 1], bw[k - 1] = a * (lxi - c * lw) / (1 + q * lw), a * a * lw / (1 + q * lw)
        pair[k - 1] = a * fv[k - 1] / (1 + lw * pv[k])   # cov(x[k-1], x[k]): the joint prediction conditioned on (lξ, lw)
    mean, var, cav = [None] * (T + 1), [None] * (T + 1), [None] * (T + 1)
    for k in range(T + 1):
        cp = 1 / pv[k] + bw[k]
        cav[k] = ((pm[k] / pv[k] + bxi[k]) / cp, 1 / cp)
        var[k] = 1 / (cp + w[k])
        mean[k] = (pm[k] / pv[k] + bxi[k] + xi[k]) * var[k]
    return mean, var, cav, pair


def _free_energy(y, T, a, c, q, m0, v0, mean, var, pair, gx, gw):
    l2pi = mp.log(2 * mp.pi)
    H = lambda v: (l2pi + 1 + mp.log(v)) / 2
    fe = (l2pi + mp.log(v0)) / 2 + ((mean[0] - m0) ** 2 + var[0]) / (2 * v0) - H(var[0])
    for k in range(1, T + 1):
        e2 = (mean[k] - a * mean[k - 1] - c) ** 2 + var[k] - 2 * a * pair[k - 1] + a * a * var[k - 1]
        fe += (l2pi + mp.log(q)) / 2 + e2 / (2 * q) - (l2pi + 1 + mp.log(var[k - 1] * var[k] - pair[k - 1] ** 2) / 2)
    for k in range(T + 1):
        observed = k >= 1 and not math.isnan(y[k - 1])
        degree = 1 + (1 if k < T else 0) + (1 if observed else 0)
        if observed:
            s = 1 if y[k - 1] > 0.5 else -1
            sd = mp.sqrt(2 * var[k])
            fe += -sum(wi * _log_ncdf(s * (mean[k] + sd * xi)) for xi, wi in zip(gx, gw)) - H(var[k])
        fe += (degree - 1) * H(var[k])
    return fe


def run(y, a, c, q, m0, v0, iterations, n_gh=32):
    """mean [T+1], var [T+1] after the last iteration and the free energy of every iteration, as lists of mpf."""
    with mp.workdps(DIGITS):
        y = [float(v) for v in y]
        T = len(y)
        a, c, q, m0, v0 = (mpf(float(v)) for v in (a, c, q, m0, v0))
        gx, gw = np.polynomial.hermite.hermgauss(n_gh)
        gw = gw / np.sqrt(np.pi)
        gx, gw = [mpf(float(v)) for v in gx], [mpf(float(v)) for v in gw]
        floor = mpf(1e-12)
        xi, w = [mpf(0)] * (T + 1), [mpf(0)] * (T + 1)
        fes = []
        for it in range(iterations + 1):
            mean, var, cav, pair = _smooth(T, a, c, q, m0, v0, xi, w)
            if it > 0:
                fes.append(_free_energy(y, T, a, c, q, m0, v0, mean, var, pair, gx, gw))
            if it == iterations:
                return mean, var, fes
            nxi, nw = list(xi), list(w)
            for k in range(1, T + 1):
                if math.isnan(y[k - 1]):
                    continue
                s = 1 if y[k - 1] > 0.5 else -1
                m, v = cav[k]
                z = s * m / mp.sqrt(1 + v)
                r = mp.npdf(z) / mp.ncdf(z)
                mt = m + s * v * r / mp.sqrt(1 + v)
                vt = v - v * v * r * (z + r) / (1 + v)
                nxi[k], nw[k] = mt / vt - m / v, max(1 / vt - 1 / v, floor)
            xi, w = nxi, nw


def errors(got, ref):
    """(mean error in posterior standard deviations, relative variance error, free-energy error over max(1, |F|) per iteration) of
    double-precision results against `run`'s, the differences taken at 60 digits."""
    (gm, gv, gf), (rm, rv, rf) = got, ref
    with mp.workdps(DIGITS):
        em = max(abs(mpf(float(g)) - r) / mp.sqrt(v) for g, r, v in zip(gm, rm, rv))
        ev = max(abs(mpf(float(g)) - r) / r for g, r in zip(gv, rv))
        ef = max(abs(mpf(float(g)) - r) / max(1, abs(r)) for g, r in zip(gf, rf))
        return float(em), float(ev), float(ef)

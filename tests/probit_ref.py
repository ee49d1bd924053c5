"""CPU restatement of the probit state-space engine (include/rxhip.h rxhip_probit_desc; reference model
test/models/statespace/probit_tests.jl:11-18), numpy + scipy, one series at a time:

    x[0] ~ Normal(m0, v0);  x[k] ~ Normal(a x[k-1] + c, q);  y[k-1] ~ Probit(x[k])    k = 1 … T,  y ∈ {0, 1, NaN = missing}

Two forms of the same parallel-EP iteration.  `run_messages` is written with forward / backward messages, the way the kernels are
(but with the site update in the literal textbook form, not the kernels' rearranged one).  `run_dense` builds the tridiagonal precision
of the chain plus diag(w), inverts it, and reads every marginal, pair marginal and cavity from the inverse: nothing is shared between
the two but the tilted moments, the Gauss–Hermite rule and the closed form of a transition's free-energy term (_bethe), which each feeds
from its own pair precision.  tests/test_probit_ref_cpu.py holds the first to the second and both to the reference's golden free energy.

Pinned range.  tests/test_probit_contract_cpu.py holds `run_messages` — means, variances and the free energy of every iteration — to the
60-digit restatement tests/probit_mp.py at every point of probit_mp.GRID (a ∈ {0, −0.9, 0.5, 1, 1.05}, q from 1e-8 to 1e3, v0 from 1e-4 to 1e6,
m0 from −8 to +40), at 100× inside the engine's contract.  Outside that range it is not pinned.  `run_dense` is the independent second form
at ordinary parameters only (its Schur complements subtract numbers of size 1/q): it is not held at small q."""
import numpy as np
from scipy.special import erfcx, log_ndtr, ndtr

GOLDEN_FE = 15.646236967225065          # probit_tests.jl:77
REFERENCE_MODEL = dict(a=1.0, c=0.1, q=0.01, m0=0.0, v0=100.0)   # probit_tests.jl:12-15
LOG2PI = float(np.log(2.0 * np.pi))
SITE_FLOOR = 1e-12


def reference_data(n=40, seed=123):
    """generate_data of probit_tests.jl:33-58: per step one randn, then one rand."""
    from stable_rng import StableRNG
    rng = StableRNG(seed)
    x = np.zeros(n + 1)
    y = np.zeros(n)
    x[0] = -2.0
    for k in range(1, n + 1):
        x[k] = x[k - 1] + 0.1 + np.sqrt(0.01) * rng.randn()
        y[k - 1] = 1.0 if ndtr(x[k]) > rng.rand() else 0.0
    return x, y


def mills(z):
    """r(z) = φ(z) / Φ(z), finite and accurate in the lower tail (z = −40: Φ underflows, r ≈ 40.025)."""
    z = np.asarray(z, dtype=np.float64)
    neg = np.sqrt(2.0 / np.pi) / erfcx(-np.minimum(z, 0.0) / np.sqrt(2.0))
    pos = np.exp(-0.5 * np.maximum(z, 0.0) ** 2) / np.sqrt(2.0 * np.pi) / ndtr(np.maximum(z, 0.0))
    return np.where(z < 0.0, neg, pos)


def tilted(m, v, y):
    """Mean and variance of N(x; m, v) Φ(s x) / Z, s = 2y − 1."""
    s = 2.0 * y - 1.0
    z = s * m / np.sqrt(1.0 + v)
    r = mills(z)
    return m + s * v * r / np.sqrt(1.0 + v), v - v * v * r * (z + r) / (1.0 + v)


def site_update(m, v, y):
    """New site (ξ, w) of an observed step from its cavity N(m, v)."""
    mt, vt = tilted(m, v, y)
    return mt / vt - m / v, max(1.0 / vt - 1.0 / v, SITE_FLOOR)


def gauss_hermite(n):
    x, w = np.polynomial.hermite.hermgauss(n)
    return x, w / np.sqrt(np.pi)


def probit_energy(mean, var, y, gh):
    """E_{N(mean, var)}[−log Φ(s x)] by the Gauss–Hermite rule."""
    s = 2.0 * y - 1.0
    return float(-np.sum(gh[1] * log_ndtr(s * (mean + np.sqrt(2.0 * var) * gh[0]))))


def entropy(var):
    return 0.5 * (LOG2PI + 1.0 + np.log(var))


def _bethe(mean, var, pairs, y, a, c, q, m0, v0, gh):
    """Bethe free energy of a Gaussian q: mean / var of x[0 … T] and, per transition (k-1, k), pairs[k-1] = (fp, fξ, lξ, lw): the pair marginal
    of (x[k-1], x[k]) has precision [[fp + a²/q, −a/q], [−a/q, 1/q + lw]] and weighted mean (fξ − a c/q, lξ + c/q) — (fp, fξ) is what x[k-1] hears
    from everything but this transition, (lξ, lw) what x[k] does.  The residual x[k] − a x[k-1] − c and the pair entropy are read from that
    precision: with D = q·det = fp (1 + q lw) + a² lw the vector (−a, 1) times the inverse precision is (−a lw, fp) / det, so
        E[res] = q (fp (lξ − c lw) − a lw fξ) / D,   var[res] = q (fp + a² lw) / D,   H = log 2πe − ½ log(D / q),
    sums of products of one sign in the variance and the determinant.  (From covariances — var[k-1] var[k] − cov² and var[k] − 2a cov +
    a² var[k-1] — both cancel when the pair is nearly singular: NaN at q = 1e-8, v0 = 100.)"""
    T = len(y)
    obs = ~np.isnan(y)
    fe = 0.5 * (LOG2PI + np.log(v0)) + 0.5 * ((mean[0] - m0) ** 2 + var[0]) / v0 - entropy(var[0])      # prior node
    for k in range(1, T + 1):                                                                           # transitions
        fp, fxi, lxi, lw = pairs[k - 1]
        D = fp * (1.0 + q * lw) + a * a * lw
        res = q * (fp * (lxi - c * lw) - a * lw * fxi) / D
        e2 = res * res + q * (fp + a * a * lw) / D
        fe += 0.5 * (LOG2PI + np.log(q)) + 0.5 * e2 / q - (LOG2PI + 1.0 - 0.5 * (np.log(D) - np.log(q)))
    for k in range(1, T + 1):                                                                           # probit nodes
        if obs[k - 1]:
            fe += probit_energy(mean[k], var[k], y[k - 1], gh) - entropy(var[k])
    for k in range(T + 1):                                                                              # variables
        deg = (1 if k == 0 else 0) + (1 if k > 0 else 0) + (1 if k < T else 0) + (1 if k > 0 and obs[k - 1] else 0)
        fe += (deg - 1) * entropy(var[k])
    return float(fe)


def run_messages(y, a, c, q, m0, v0, iterations, n_gh=32):
    """Parallel EP with messages.  Returns mean [T+1], var [T+1] after the last iteration and the free energy of every iteration."""
    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    gh = gauss_hermite(n_gh)
    xi, w = np.zeros(T + 1), np.zeros(T + 1)      # sites of x[1 … T] (index 0 unused: x[0] has none)
    fes = []

    def sweep(update):
        pm, pv = np.zeros(T + 1), np.zeros(T + 1)   # forward predictive message at x[k]
        pm[0], pv[0] = m0, v0
        for k in range(1, T + 1):
            fp = 1.0 / pv[k - 1] + w[k - 1]
            fm = (pm[k - 1] / pv[k - 1] + xi[k - 1]) / fp
            pm[k], pv[k] = a * fm + c, a * a / fp + q
        mean, var, pairs = np.zeros(T + 1), np.zeros(T + 1), [None] * T
        bxi, bw = 0.0, 0.0                          # backward message at x[k]
        nxi, nw = xi.copy(), w.copy()
        for k in range(T, -1, -1):
            cp = 1.0 / pv[k] + bw                   # cavity
            cm = (pm[k] / pv[k] + bxi) / cp
            var[k] = 1.0 / (cp + w[k])
            mean[k] = (pm[k] / pv[k] + bxi + xi[k]) * var[k]
            if update and k >= 1 and not np.isnan(y[k - 1]):
                nxi[k], nw[k] = site_update(cm, 1.0 / cp, y[k - 1])
            if k >= 1:
                lxi, lw = bxi + xi[k], bw + w[k]    # everything x[k] hears from its observation and the future: the OLD site
                # filtered belief of x[k-1] (precision, weighted mean) and what x[k] hears: the pair marginal of (x[k-1], x[k]), see _bethe
                pairs[k - 1] = (1.0 / pv[k - 1] + w[k - 1], pm[k - 1] / pv[k - 1] + xi[k - 1], lxi, lw)
                bxi, bw = a * (lxi - c * lw) / (1.0 + q * lw), a * a * lw / (1.0 + q * lw)
        return mean, var, pairs, nxi, nw

    for it in range(iterations):
        mean, var, pc, nxi, nw = sweep(True)
        if it > 0:
            fes.append(_bethe(mean, var, pc, y, a, c, q, m0, v0, gh))
        xi, w = nxi, nw
    mean, var, pc, _, _ = sweep(False)
    fes.append(_bethe(mean, var, pc, y, a, c, q, m0, v0, gh))
    return mean, var, np.array(fes)


def _dense_pairs(L, h, xi, w, a, c, q, m0, v0):
    """_bethe's pair input from the dense precision L and weighted mean h: the states before x[k-1] and after x[k] are integrated out by
    Schur complements (dense inverses of the two blocks), and the transition's own entries are never added, so nothing of size a²/q is
    subtracted back out."""
    n = len(h)
    pairs = []
    for k in range(1, n):
        fp, fxi = (1.0 / v0, m0 / v0) if k == 1 else (1.0 / q + w[k - 1], c / q + xi[k - 1])
        if k >= 2:      # the past x[0 … k-2], coupled to x[k-1] by −a/q
            P = np.linalg.inv(L[:k - 1, :k - 1])
            fp -= (a / q) ** 2 * P[-1, -1]
            fxi += (a / q) * (P @ h[:k - 1])[-1]
        lxi, lw = xi[k], w[k]
        if k < n - 1:   # the future x[k+1 … T], coupled to x[k] by −a/q; the outgoing transition puts a²/q, −a c/q on x[k]
            F = np.linalg.inv(L[k + 1:, k + 1:])
            lw += (a * a / q) * (1.0 - F[0, 0] / q)
            lxi += -a * c / q + (a / q) * (F @ h[k + 1:])[0]
        pairs.append((fp, fxi, lxi, lw))
    return pairs


def run_dense(y, a, c, q, m0, v0, iterations, n_gh=32):
    """The same iteration from the dense posterior: precision = chain (tridiagonal) + diag(w), inverted."""
    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    n = T + 1
    gh = gauss_hermite(n_gh)
    L0 = np.zeros((n, n))
    h0 = np.zeros(n)
    L0[0, 0] += 1.0 / v0
    h0[0] += m0 / v0
    for k in range(1, n):       # −log N(x_k; a x_{k-1} + c, q)
        L0[k, k] += 1.0 / q
        L0[k - 1, k - 1] += a * a / q
        L0[k, k - 1] -= a / q
        L0[k - 1, k] -= a / q
        h0[k] += c / q
        h0[k - 1] -= a * c / q
    xi, w = np.zeros(n), np.zeros(n)
    fes = []
    for it in range(iterations + 1):
        S = np.linalg.inv(L0 + np.diag(w))
        mu = S @ (h0 + xi)
        var = np.diag(S).copy()
        if it > 0:
            fes.append(_bethe(mu, var, _dense_pairs(L0 + np.diag(w), h0 + xi, xi, w, a, c, q, m0, v0), y, a, c, q, m0, v0, gh))
        if it == iterations:
            return mu, var, np.array(fes)
        nxi, nw = xi.copy(), w.copy()
        for k in range(1, n):
            if np.isnan(y[k - 1]):
                continue
            cp = 1.0 / var[k] - w[k]               # the marginal with site k divided out
            cm = (mu[k] / var[k] - xi[k]) / cp
            nxi[k], nw[k] = site_update(cm, 1.0 / cp, y[k - 1])
        xi, w = nxi, nw


def run_batch(y, a, c, q, m0, v0, iterations, n_gh=32, run=run_messages):
    """y [T][series]; a, c, q, m0, v0 scalars.  Returns mean, var [T+1][series], fe [iterations][series]."""
    y = np.asarray(y, dtype=np.float64)
    T, C = y.shape
    mean, var, fe = np.zeros((T + 1, C)), np.zeros((T + 1, C)), np.zeros((iterations, C))
    for s in range(C):
        mean[:, s], var[:, s], fe[:, s] = run(y[:, s], a, c, q, m0, v0, iterations, n_gh)
    return mean, var, fe


def contract_series(T, seed=7):
    """The six series of the contract grid, y [T][6]: all 1; all 0; alternating; random with 15 % missing and the first and last steps
    missing; a single observed step; nothing observed (its free energy is exactly 0)."""
    rng = np.random.default_rng(seed)
    y = np.full((T, 6), np.nan)
    y[:, 0] = 1.0
    y[:, 1] = 0.0
    y[:, 2] = np.arange(T) % 2
    y[:, 3] = np.where(rng.random(T) < 0.15, np.nan, (rng.random(T) < 0.5).astype(np.float64))
    y[0, 3] = y[-1, 3] = np.nan
    y[T // 3, 4] = 1.0
    y.setflags(write=False)
    return y

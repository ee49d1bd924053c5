"""The latent autoregressive engine's iteration (include/rxhip.h rxhip_lar_desc) restated in mpmath at 50 digits, the grid of cases on which
tests/test_lar_contract_cpu.py, tests/test_lar_host.py and tests/test_lar_contract_gpu.py hold the engine to it, and the engine's numerical
envelope (ENVELOPE) with the scan it was read from.

`run` is the iteration of the header written out plainly — update order x, θ, γ; the old mγ in θ's update; the new θ in γ's; NaN = missing;
`share` = one q(θ), q(γ) and the KL terms once — in two forms.  "dense": Λ assembled whole and inverted whole (through its dense Cholesky factor, which also
gives ln det), every statistic read off Σ + m mᵀ; ψ and lnΓ from mpmath.  It shares nothing with the device's recursions and is the independent one.  "banded":
LDLᵀ, two solves and the selected inverse, O(T p²), which scales to T = 4096; tests/test_lar_contract_cpu.py holds it to the dense form at 1e-40
on every case with T + p ≤ 48, and it carries the rest.  Both return, beside the posteriors and free energies, the gauges of the envelope taken
over all iterations: the largest |m_i|/sd_i, the smallest R/Szz, the largest cond Λ (the last in fp64 from scipy's eigvals_banded: a gauge, not a
reference).

`GRID` and `SCAN` are lists of case specs; `case(spec)` builds a spec's inputs deterministically.  The results live in tests/golden/lar_long.npz
(tests/golden/make_lar_long_golden.py): per case the vector `pick` selects, as float64, a CRC of the inputs and the gauges."""
import collections
import zlib

import mpmath as mp
import numpy as np
from scipy.linalg import eigvals_banded

import lar_ref as R

DPS = 50

# The envelope of the engine, in the measured gauges (include/rxhip.h states it; DESIGN.md §3.5c has the scan table it was read from).  The error of
# a state mean is ε·|m_i| at best, so in standard deviations it grows with ratio = max_i |m_i|/sd_i: on SCAN the banded fp64 restatement, which
# walks the device's order, is between 2e-18 and 4e-16 of the ratio away from the 50-digit means; it stays within a TENTH of the contract (1e-7 sd)
# on every scan case up to ratio 2.1e9 and first leaves it at 8.4e9.  Neighbouring cases differ by that factor of ten, so the bound is put a decade
# under the last pass: ratio ≤ 1e8 (4e-16 · 1e8 = 4e-8).  cond Λ ≤ 1e8 is kept beside it: the scan itself stays below cond 20, and nothing beyond
# 1e8 is held to the contract.  One sweep from the initial θ never makes R small, so the second part of SCAN iterates three times on fully
# observed data with an offset: θ learns the level, R/Szz falls to 1.6e-8, and b and F — nothing else — follow ε·Szz/R: b 5e-16/(R/Szz), F
# 6e-17/(R/Szz), so F leaves the tenth of its contract (1e-9) near R/Szz = 6e-8 and b (1e-7) near 5e-9.  The floor is R/Szz ≥ 1e-6, what the
# autoregression engine's envelope states for the same reason; at the floor b is within 1e-9 and F within 1e-10.
ENVELOPE = dict(ratio=1e8, cond=1e8, r_over_szz=1e-6)
TENTH = dict(mean=1e-7, par=1e-7, a=0.0, fe=1e-9)
CONTRACT = dict(mean=1e-6, par=1e-6, a=0.0, fe=1e-8)

Spec = collections.namedtuple("Spec", "name seed T C p iterations share tau gamma gcentre scale theta missing wth w0 far offset")


def _spec(name, seed, T=64, C=2, p=2, iterations=3, share=False, tau=5.0, gamma=1.0, gcentre=1.0, scale=1.0, theta=None, missing=0.1, wth=None,
          w0=None, far=False, offset=0.0):
    return Spec(name, seed, T, C, p, iterations, share, tau, gamma, gcentre, scale, theta, missing, wth, w0, far, offset)


# Cases moved inward by the admission rule (tests/test_lar_contract_cpu.py `test_the_grid_is_admitted`); the restatement stayed within 1e-8 sd on
# all of them, it is cond Λ ≤ 1e8 that they broke.  (1) The data scale 1e4 became 1e3: with γ matching, the first sweep has mγ ~ 1/scale², the
# rows of x0 and of missing steps hold nothing else, observed rows hold τ = 5: cond Λ = 8e8 at 1e4 (4e8 with every step observed), 5e6 at 1e3.
# (2) The offsets were to be 1e7 and 1e6, which the ratio alone admits.  The initial θ explains nothing of data that large, so b is huge and
# mγ ~ 1e-6/offset², and a missing step's row of Λ holds nothing else: cond Λ = 1.5e13 and above 1e11 (1.5e9 at 1e5); observed at every step instead, θ learns the
# level and R/Szz falls to 2.5e-8, where F is 1.2e-9 off, outside the tenth of its contract.  1e4 is the largest offset inside all three gauges
# (cond Λ = 1.5e7, R/Szz = 4.8e-5).  No other case had to move; no seed was passed over.
def _grid():
    out = []
    add = lambda name, **kw: out.append(_spec(name, 1000 + len(out), **kw))
    for p in range(1, 9):                                                        # every order over many interior rows, 15 feedbacks
        add(f"orders p={p}", T=257, p=p, iterations=15)
    for p in (1, 8):                                                             # long; series 1 has 200 consecutive missing steps
        add(f"long p={p}", T=4096, C=3, p=p, iterations=2, missing="run")
    for p in (8, 5):                                                             # boundary shapes
        for T in (1, 2, p - 1, p, p + 1):
            add(f"boundary p={p} T={T}", T=T, p=p, missing=0.0, iterations=2)
    for tau in (1e-6, 1e-3, 1e3, 1e6):                                           # observation precision
        add(f"tau={tau:g}", tau=tau)
    for g in (1e-3, 1e3, 1e6):                                                   # driving-noise precision; the prior centred there or 3 decades off
        add(f"gamma={g:g} centred", gamma=g)
        add(f"gamma={g:g} prior {'above' if g < 1 else 'below'}", gamma=g, gcentre=1e3 if g < 1 else 1e-3)
    for s in (1e-4, 1e3):                                                        # scale of the data, γ matching
        add(f"scale={s:g}", scale=s)
    add("theta=0.999", theta=0.999)                                              # dynamics
    add("theta=1 random walk", theta=1.0)
    add("theta=1.02 all observed", theta=1.02, missing=0.0)
    add("p=8 last lag only", p=8, theta="last")
    for w in (1e-6, 1e6):                                                        # priors
        add(f"Wtheta0=W0={w:g}", wth=w, w0=w)
    add("priors cond 1e4", p=3, wth="cond", w0="cond")
    add("init q(theta) far", p=3, far=True)
    add("all missing", missing="all")                                            # missing
    for where in ("first", "middle", "last"):
        add(f"one observed step, {where}", p=3, T=33, missing=where)
    add("first p steps missing", p=3, T=33, missing="firstp")
    add("offset 1e4", offset=1e4)                                                # offset: the largest the envelope admits at this (γ, τ) and a decade below
    add("offset 1e3", offset=1e3)
    for C in (65, 70):                                                           # shared parameters, a ragged second wavefront, scales 1 … 1e2
        add(f"shared C={C}", T=33, C=C, p=3, share=True)
    return out


SCAN_OFFSETS = tuple(10.0 ** k for k in range(2, 9))
SCAN_R_OFFSETS = (1e2, 1e3, 1e4, 1e5, 1e6)
SCAN_PAIRS = ((1.0, 5.0), (1e4, 1e2), (1e6, 1e4))


def _scan():
    """One sweep at T = 40, p = 2 and p = 1, one series observed at every step: an AR(p) path of innovation precision γ seen at precision τ, on a
    common offset; the γ prior and the initial q(γ) centred on γ.  Then the same shape at p = 2, γ = 1, τ = 5 iterated three times."""
    out = []
    for p in (2, 1):
        for g, tau in SCAN_PAIRS:
            for off in SCAN_OFFSETS:
                out.append(_spec(f"scan p={p} gamma={g:g} tau={tau:g} offset={off:g}", 2000 + len(out), T=40, C=1, p=p, iterations=1, tau=tau, gamma=g,
                                 missing=0.0, offset=off))
    for off in SCAN_R_OFFSETS:                                                   # three iterations: θ learns the level and R/Szz falls
        out.append(_spec(f"scan R/Szz offset={off:g}", 2000 + len(out), T=40, C=1, p=2, iterations=3, missing=0.0, offset=off))
    return out


GRID = _grid()
SCAN = _scan()


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------
def _theta(spec):
    th = np.zeros(spec.p)
    if spec.theta == "last":
        th[-1] = 0.9
    else:
        th[0] = 0.7 if spec.theta is None else spec.theta
        if spec.name.startswith("scan") and spec.p == 2:
            th[:] = (0.5, 0.3)
    return th


def _matrix(rng, p, how, unit):
    """a prior precision: None = random SPD of unit scale (as lar_ref.random_case), a float = that multiple of I, "cond" = a non-diagonal SPD
    matrix with eigenvalues 1e-2 … 1e2; `unit` is the precision that one unit of the variable's scale corresponds to"""
    a = rng.standard_normal((p, p))
    if how is None:
        return unit * (a @ a.T / p + np.eye(p))
    if how == "cond":
        q = np.linalg.qr(a)[0]
        w = (q * np.logspace(-2.0, 2.0, p)) @ q.T
        return 0.5 * (w + w.T)
    return float(how) * np.eye(p)


def case(spec):
    """(y [T][C], model dict as lar_ref.model gives it, iterations, share) of a spec.  Series c is driven by default_rng([seed, c]): z from the AR
    recursion with the spec's θ and innovation precision γ (50 steps of burn-in from zero), seen with noise of precision τ, times the scale
    (shared cases: times 10^(2c/(C−1)) as well), plus the offset; then the missing steps.  The model's draws come from default_rng(seed)."""
    T, C, p = spec.T, spec.C, spec.p
    th, sd = _theta(spec), spec.gamma ** -0.5
    y = np.empty((T, C))
    for c in range(C):
        r = np.random.default_rng([spec.seed, c])
        e, v, u = r.standard_normal(T + 50 + p), r.standard_normal(T), r.random(T)
        z = np.zeros(T + 50 + p)
        for t in range(p, len(z)):
            z[t] = th @ z[t - p:t][::-1] + sd * e[t]
        yc = (z[-T:] + v / np.sqrt(spec.tau)) * spec.scale * (10.0 ** (2.0 * c / (C - 1)) if spec.share else 1.0) + spec.offset
        if spec.missing == "all":
            yc[:] = np.nan
        elif spec.missing in ("first", "middle", "last"):
            keep = {"first": 0, "middle": T // 2, "last": T - 1}[spec.missing]
            yc[np.arange(T) != keep] = np.nan
        elif spec.missing == "firstp":
            yc[:p] = np.nan
        else:
            yc[u < (0.1 if spec.missing == "run" else spec.missing)] = np.nan
            if spec.missing == "run" and c == 1:
                yc[1000:1200] = np.nan
        y[:, c] = yc
    rng = np.random.default_rng(spec.seed)
    level = spec.scale * sd
    g0 = spec.gcentre * spec.gamma / spec.scale ** 2

    def gam():
        shape = rng.uniform(1.0, 3.0)
        return shape, shape / g0

    pt = (0.3 * rng.standard_normal(p), _matrix(rng, p, spec.wth, 1.0))
    px = (spec.offset + level * rng.standard_normal(p), _matrix(rng, p, spec.w0, level ** -2.0))
    it = (0.3 * rng.standard_normal(p), _matrix(rng, p, None, 0.1))
    if spec.far:
        it = (2.0 * (-1.0) ** np.arange(p), 10.0 * np.eye(p))
    m = R.model(p, spec.tau, prior_theta=pt, prior_gamma=gam(), prior_x0=px, init_theta=it, init_gamma=gam())
    return y, m, spec.iterations, spec.share


def checksum(y, m):
    """CRC-32 of a case's inputs, to notice a generator that drifted"""
    parts = [y, [m["tau"]], m["prior_gamma"], m["init_gamma"], *m["prior_theta"], *m["prior_x0"], *m["init_theta"]]
    parts = [np.ascontiguousarray(v, dtype=np.float64) for v in parts]
    return zlib.crc32(b"".join(np.where(np.isnan(v), -1.0, v).tobytes() for v in parts))


# ---- the iteration at 50 digits ---------------------------------------------------------------------------------------------------------------------
def _f(v):
    return mp.mpf(float(v))


def _vec(a):
    return [_f(v) for v in np.asarray(a, dtype=np.float64).ravel()]


def _mat(a):
    return [[_f(v) for v in row] for row in np.asarray(a, dtype=np.float64)]


def _g_matrix(mth, vth):
    p = len(mth)
    g = [[mp.mpf(0)] * (p + 1) for _ in range(p + 1)]
    g[0][0] = mp.mpf(1)
    for a in range(p):
        g[0][a + 1] = g[a + 1][0] = -mth[a]
        for b in range(p):
            g[a + 1][b + 1] = mth[a] * mth[b] + vth[a][b]
    return g


def _lam_entry(i, j, n, p, g, mg, w0, tau_i):
    """Λ(i, j), j ≤ i ≤ j + p (lar_ref.lam_entry)"""
    k = i - j
    s = mp.fsum(g[ki][ki + k] for ki in range(max(0, p - i), min(p - k, n - 1 - i) + 1))
    v = mg * s
    if i < p:
        v += w0[p - 1 - i][p - 1 - j]
    if k == 0:
        v += tau_i
    return v


def _rows(y, p, tau, g, mg, m0, w0):
    """per row i: the band entries Λ(i, i − k), k = 0 … p (0 where i − k < 0), and h_i; interior rows share their entries"""
    T = len(y)
    n = T + p
    h0 = [mp.fsum(w0[a][b] * m0[b] for b in range(p)) for a in range(p)]
    inner = None
    for i in range(n):
        seen = i >= p and y[i - p] == y[i - p]
        if p <= i < T:
            if inner is None:
                inner = [_lam_entry(i, i - k, n, p, g, mg, w0, 0) for k in range(p + 1)]
            a = list(inner)
        else:
            a = [_lam_entry(i, i - k, n, p, g, mg, w0, 0) if i - k >= 0 else mp.mpf(0) for k in range(p + 1)]
        if seen:
            a[0] += tau
        yield a, (h0[p - 1 - i] if i < p else mp.mpf(0)) + (tau * _f(y[i - p]) if seen else mp.mpf(0))


def _sweep_banded(y, p, tau, g, mg, m0, w0):
    T = len(y)
    n = T + p
    zero = mp.mpf(0)
    L = [[zero] * (p + 1) for _ in range(n + p)]                 # L[i][k] = L(i, i − k)
    inv, v = [zero] * (n + p), [zero] * (n + p)
    for i, (a, hi) in enumerate(_rows(y, p, tau, g, mg, m0, w0)):
        s = [zero] * (p + 1)
        Li = L[i]
        for k in range(min(p, i), 0, -1):
            Lk = L[i - k]
            acc = a[k]
            for mk in range(p, k, -1):
                acc -= s[mk] * Lk[mk - k]
            s[k] = acc
            Li[k] = acc * inv[i - k]
        d, vi = a[0], hi
        for k in range(min(p, i), 0, -1):
            d -= s[k] * Li[k]
            vi -= Li[k] * v[i - k]
        inv[i] = 1 / d
        v[i] = vi
    m = [zero] * (n + p)
    sg = [[zero] * (p + 1) for _ in range(n + p)]                # sg[i][b] = Σ(i, i + b)
    for i in range(n - 1, -1, -1):
        c = [L[i + a][a] for a in range(p + 1)]                  # column i of L (rows beyond n − 1 are zero)
        mi = v[i] * inv[i]
        for a in range(1, p + 1):
            mi -= c[a] * m[i + a]
        m[i] = mi
        row = sg[i]
        for b in range(1, p + 1):
            acc = zero
            for a in range(1, p + 1):
                acc -= c[a] * sg[i + min(a, b)][abs(a - b)]
            row[b] = acc
        acc = inv[i]
        for a in range(1, p + 1):
            acc -= c[a] * row[a]
        row[0] = acc
    cov = lambda i, j: sg[min(i, j)][abs(i - j)]
    return _statistics(y, p, m0, w0, m[:n], cov, -mp.fsum(mp.log(x) for x in inv[:n])), m[:n], [r[:] for r in sg[:n]]


def _sweep_dense(y, p, tau, g, mg, m0, w0):
    T = len(y)
    n = T + p
    lam = mp.zeros(n, n)
    h = mp.zeros(n, 1)
    for a in range(p):                                          # x0 = (z_0 … z_{-p+1}) -> indices p − 1 … 0
        for b in range(p):
            lam[p - 1 - a, p - 1 - b] += w0[a][b]
            h[p - 1 - a] += w0[a][b] * m0[b]
    for t in range(1, T + 1):                                   # w_t = (z_t … z_{t-p}) -> indices t + p − 1 … t − 1
        for a in range(p + 1):
            for b in range(p + 1):
                lam[t + p - 1 - a, t + p - 1 - b] += mg * g[a][b]
        if y[t - 1] == y[t - 1]:
            lam[t + p - 1, t + p - 1] += tau
            h[t + p - 1] += tau * _f(y[t - 1])
    sig, logdet = _spd_inverse([[lam[i, j] for j in range(n)] for i in range(n)])
    cov = lambda i, j: sig[max(i, j)][min(i, j)]
    m = [mp.fsum(cov(i, j) * h[j] for j in range(n)) for i in range(n)]
    band = [[cov(i, i + b) if i + b < n else mp.mpf(0) for b in range(p + 1)] for i in range(n)]
    return _statistics(y, p, m0, w0, m, cov, logdet), m, band


def _spd_inverse(a):
    """(the whole inverse of a dense SPD matrix, ln det), by its Cholesky factor C: a⁻¹ = C⁻ᵀC⁻¹.  Nothing here knows of a band."""
    n = len(a)
    c = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            v = a[i][j] - mp.fsum(c[i][k] * c[j][k] for k in range(j))
            c[i][j] = mp.sqrt(v) if i == j else v / c[j][j]
    w = [[mp.mpf(0)] * n for _ in range(n)]                      # C⁻¹, lower triangular
    for j in range(n):
        w[j][j] = 1 / c[j][j]
        for i in range(j + 1, n):
            w[i][j] = -mp.fsum(c[i][k] * w[k][j] for k in range(j, i)) / c[i][i]
    inv = [[mp.fsum(w[k][i] * w[k][j] for k in range(i, n)) if j <= i else None for j in range(n)] for i in range(n)]
    return inv, 2 * mp.fsum(mp.log(c[i][i]) for i in range(n))


def _statistics(y, p, m0, w0, m, cov, logdet):
    T = len(y)
    S = [[mp.fsum(cov(t + p - 1 - a, t + p - 1 - b) + m[t + p - 1 - a] * m[t + p - 1 - b] for t in range(1, T + 1)) for b in range(p + 1)] for a in range(p + 1)]
    obs = [t for t in range(1, T + 1) if y[t - 1] == y[t - 1]]
    ey = mp.fsum((_f(y[t - 1]) - m[t + p - 1]) ** 2 + cov(t + p - 1, t + p - 1) for t in obs)
    dm = [m[p - 1 - a] - m0[a] for a in range(p)]
    e0 = mp.fsum(w0[a][b] * (dm[a] * dm[b] + cov(p - 1 - a, p - 1 - b)) for a in range(p) for b in range(p))
    return dict(S=S, Ey=ey, nobs=len(obs), E0=e0, logdet=logdet)


def _inverse(w):
    p = len(w)
    v = mp.matrix(w) ** -1
    return [[(v[a, b] + v[b, a]) / 2 for b in range(p)] for a in range(p)]


def _logdet(w):
    return mp.log(mp.det(mp.matrix(w)))


def _residual(S, mth, vth):
    p = len(mth)
    return S[0][0] - 2 * mp.fsum(mth[a] * S[0][a + 1] for a in range(p)) + mp.fsum((mth[a] * mth[b] + vth[a][b]) * S[a + 1][b + 1] for a in range(p) for b in range(p))


def _update(S, mg_old, n_factors, mth0, wth0, a0, b0):
    p = len(mth0)
    vth = _inverse([[wth0[a][b] + mg_old * S[a + 1][b + 1] for b in range(p)] for a in range(p)])
    rhs = [mp.fsum(wth0[a][b] * mth0[b] for b in range(p)) + mg_old * S[0][a + 1] for a in range(p)]
    mth = [mp.fsum(vth[a][b] * rhs[b] for b in range(p)) for a in range(p)]
    return mth, vth, a0 + mp.mpf(n_factors) / 2, b0 + _residual(S, mth, vth) / 2


def _kl(mth, vth, a, b, mth0, wth0, a0, b0):
    p = len(mth)
    d = [mth[i] - mth0[i] for i in range(p)]
    kt = (mp.fsum(wth0[i][j] * (vth[i][j] + d[i] * d[j]) for i in range(p) for j in range(p)) - p - _logdet(vth) - _logdet(wth0)) / 2
    kg = (a - a0) * mp.digamma(a) - mp.loggamma(a) + mp.loggamma(a0) + a0 * (mp.log(b) - mp.log(b0)) + a * (b0 - b) / b
    return kt + kg


def _energy(st, T, p, tau, w0, mth, vth, a, b):
    n = T + p
    two_pi = 2 * mp.pi
    f = -(n * mp.log(two_pi * mp.e) - st["logdet"]) / 2
    f += (p * mp.log(two_pi) - _logdet(w0) + st["E0"]) / 2
    f += (T * mp.log(two_pi) - T * (mp.digamma(a) - mp.log(b)) + (a / b) * _residual(st["S"], mth, vth)) / 2
    f += (st["nobs"] * mp.log(two_pi) - st["nobs"] * mp.log(tau) + tau * st["Ey"]) / 2
    return f


def _cond(y, p, tau, g, mg, w0):
    """cond Λ in fp64, from the extreme eigenvalues of the band"""
    n = len(y) + p
    gf, wf = np.array([[float(v) for v in row] for row in g]), np.array([[float(v) for v in row] for row in w0])
    ab = np.zeros((p + 1, n))
    for i in range(n):
        seen = i >= p and y[i - p] == y[i - p]
        for k in range(min(p, i) + 1):
            ab[k, i - k] = R.lam_entry(i, i - k, n, p, gf, float(mg), wf, float(tau) if seen else 0.0)
    lo = eigvals_banded(ab, lower=True, select="i", select_range=(0, 0))[0]
    hi = eigvals_banded(ab, lower=True, select="i", select_range=(n - 1, n - 1))[0]
    return float(hi / lo)


def run(y, model, iterations, share=False, form="banded"):
    """y [T][series], model as lar_ref.model gives it.  Returns a dict of float64 arrays with lar_ref.run_batch's keys — x_mean, x_cov, z_mean, band
    (last iteration), theta_mean, theta_cov, gamma_shape, gamma_rate (every iteration), fe [iterations], fe_series [iterations][series] (shared:
    without the KL terms) — and "gauges" (ratio, r_over_szz, cond), "fe_mp" (the free energies as mpf) and "raw": (values, denominators), two
    lists of mpf over every z mean, band entry, θ entry, b and F in the contract's measures, for comparing the two forms beyond double precision."""
    y = np.asarray(y, dtype=np.float64)
    T, C = y.shape
    p = model["order"]
    G = 1 if share else C
    sweep = _sweep_banded if form == "banded" else _sweep_dense
    with mp.workdps(DPS):
        tau = _f(model["tau"])
        mth0, wth0 = _vec(model["prior_theta"][0]), _mat(model["prior_theta"][1])
        m0, w0 = _vec(model["prior_x0"][0]), _mat(model["prior_x0"][1])
        a0, b0 = _f(model["prior_gamma"][0]), _f(model["prior_gamma"][1])
        q = [(_vec(model["init_theta"][0]), _mat(model["init_theta"][1]), _f(model["init_gamma"][0]), _f(model["init_gamma"][1])) for _ in range(G)]
        hist, fe, fes = [], [], []
        ratio, rsz, cond = mp.mpf(0), mp.inf, 0.0
        vals, dens = [], []
        for _ in range(iterations):
            sts = []
            for s in range(C):
                mth, vth, a, b = q[0 if share else s]
                g = _g_matrix(mth, vth)
                sts.append(sweep(y[:, s], p, tau, g, a / b, m0, w0))
                cond = max(cond, _cond(y[:, s], p, tau, g, a / b, w0))
                ratio = max(ratio, max(abs(mi) / mp.sqrt(r[0]) for mi, r in zip(sts[-1][1], sts[-1][2])))
            if share:
                tot = [[mp.fsum(st[0]["S"][i][j] for st in sts) for j in range(p + 1)] for i in range(p + 1)]
                stats, q = [tot], [_update(tot, q[0][2] / q[0][3], C * T, mth0, wth0, a0, b0)]
            else:
                stats = [st[0]["S"] for st in sts]
                q = [_update(stats[s], q[s][2] / q[s][3], T, mth0, wth0, a0, b0) for s in range(C)]
            rsz = min(rsz, min(_residual(S, v[0], v[1]) / S[0][0] for S, v in zip(stats, q)))
            kls = [_kl(*v, mth0, wth0, a0, b0) for v in q]
            parts = [_energy(sts[s][0], T, p, tau, w0, *q[0 if share else s]) + (0 if share else kls[s]) for s in range(C)]
            fes.append(parts)
            fe.append(mp.fsum(parts) + (kls[0] if share else 0))
            hist.append(q)
            for mth, vth, a, b in q:
                tsd = [mp.sqrt(vth[i][i]) for i in range(p)]
                vals += mth + [vth[i][j] for i in range(p) for j in range(p)] + [b]
                dens += [max(abs(mth[i]), tsd[i]) for i in range(p)] + [tsd[i] * tsd[j] for i in range(p) for j in range(p)] + [b]
            vals += [fe[-1]] + parts
            dens += [max(1, abs(v)) for v in [fe[-1]] + parts]
        n = T + p
        for _, m, band in sts:
            sd = [mp.sqrt(r[0]) for r in band]
            vals += m + [band[i][k] for i in range(n) for k in range(p + 1) if i + k < n]
            dens += sd + [sd[i] * sd[i + k] for i in range(n) for k in range(p + 1) if i + k < n]
        f64 = lambda a: np.array(a, dtype=object).astype(np.float64)
        zm = np.stack([f64(st[1]) for st in sts], axis=1)
        band = np.stack([f64(st[2]) for st in sts], axis=1)
        out = dict(z_mean=zm, band=band, fe=f64(fe), fe_series=f64(fes), fe_mp=fe, raw=(vals, dens),
                   theta_mean=f64([[v[0] for v in h] for h in hist]), theta_cov=f64([[v[1] for v in h] for h in hist]),
                   gamma_shape=f64([[v[2] for v in h] for h in hist]), gamma_rate=f64([[v[3] for v in h] for h in hist]),
                   gauges=np.array([float(ratio), float(rsz), cond]))
    xm, xc = np.empty((T, C, p)), np.empty((T, C, p, p))
    for t in range(1, T + 1):
        for a_ in range(p):
            ia = t + p - 1 - a_
            xm[t - 1, :, a_] = zm[ia]
            for b_ in range(p):
                ib = t + p - 1 - b_
                xc[t - 1, :, a_, b_] = band[min(ia, ib), :, abs(ia - ib)]
    out.update(x_mean=xm, x_cov=xc)
    return out


def raw_error(a, b):
    """the largest difference of two runs' "raw" lists in units of the second one's denominators (an mpf)"""
    with mp.workdps(DPS):
        assert len(a[0]) == len(b[0])
        return max(abs(u - v) / d for u, v, d in zip(a[0], b[0], b[1]))


# ---- what the fixture keeps of a case ---------------------------------------------------------------------------------------------------------------
def block_steps(spec):
    """the steps t (1 … T) whose whole q(x[t]) the fixture keeps: the first rows of the band (t = 1 holds z_1 and all of x0 but its last
    component, t = p + 1 the first interior row) and the last"""
    return sorted({1, spec.T} if spec.name.startswith("scan") else {1, min(spec.p + 1, spec.T), spec.T})


def z_steps(spec):
    """the steps whose q(z_t) (mean and variance) the fixture keeps"""
    stride = 16 if spec.T <= 64 else 32 if spec.T <= 257 else 256
    return sorted(set(range(1, spec.T + 1, stride)) | {spec.T}) if spec.T > 2 else []


def kept_series(spec):
    """the series whose states the fixture keeps: the first (of the long engines the one with the 200 missing steps); of a shared batch the
    first, both sides of the wavefront's edge and the last"""
    return [1 if spec.missing == "run" else 0] if spec.C <= 3 else [0, 63, 64, spec.C - 1]


def _triu(a):
    iu = np.triu_indices(a.shape[-1])
    return a[..., iu[0], iu[1]]


def pick(spec, r):
    """What the fixture keeps of a case, from a dict with lar_ref.run_batch's keys (`fe_series`: [iterations][series], [series] of the last
    iteration, or None where a program does not report it): a list of (kind, array).  The fixture has a size limit, hence subsets.
    Parameters: θ's mean, the diagonal of its covariance and b of EVERY iteration, the covariance in full of the last one (the off-diagonal
    entries of iteration k enter G, and with it θ, b and F of iteration k + 1, which are kept); a of the last iteration (it does not change).  F of every iteration, per series of the last.  States, of `kept_series`: q(x[t]) in full at `block_steps`, q(z_t) at `z_steps` —
    both recursions carry a wrong row into every row after it, and S, E_y, E_0 and ln det Λ, on which the kept θ, b and F depend, sum over all rows."""
    it, p = spec.iterations, spec.p
    tm, tc = np.asarray(r["theta_mean"]), np.asarray(r["theta_cov"])
    out = []
    for k in range(it):
        full = k == it - 1
        out.append(("theta full" if full else "theta diag", np.concatenate([tm[k], _triu(tc[k]) if full else np.einsum("gii->gi", tc[k])], axis=-1)))
    out.append(("rel", np.asarray(r["gamma_rate"])))
    out.append(("a", np.asarray(r["gamma_shape"])[-1]))
    out.append(("fe", np.asarray(r["fe"])))
    fs = r.get("fe_series")
    out.append(("skip", np.zeros(spec.C)) if fs is None else ("fe", np.asarray(fs)[-1] if np.ndim(fs) == 2 else np.asarray(fs)))
    cs = kept_series(spec)
    xm, xc = np.asarray(r["x_mean"])[:, cs], np.asarray(r["x_cov"])[:, cs]
    ts = [t - 1 for t in block_steps(spec)]
    out.append(("state full", np.concatenate([xm[ts], _triu(xc[ts])], axis=-1).reshape(-1, p + p * (p + 1) // 2)))
    zs = [t - 1 for t in z_steps(spec)]
    if zs:
        out.append(("z", np.stack([xm[zs][..., 0], xc[zs][..., 0, 0]], axis=-1).reshape(-1, 2)))
    return out


def free_energies(spec, flat):
    """F of every iteration, out of a case's slice of the fixture (the layout is `pick`'s)"""
    p, G, it = spec.p, 1 if spec.share else spec.C, spec.iterations
    o = (it - 1) * G * 2 * p + G * (p + p * (p + 1) // 2) + it * G + G
    return flat[o:o + it]


def flatten(picked):
    return np.concatenate([np.asarray(a, dtype=np.float64).ravel() for _, a in picked])


def _gauss(a, ref, d, full, theta):
    """(mean error, covariance error) of rows (mean [d], covariance: upper triangle or diagonal) in the contract's measures"""
    if full:
        iu = np.triu_indices(d)
        var = ref[:, d:][:, iu[0] == iu[1]]
        den = np.sqrt(var[:, iu[0]] * var[:, iu[1]])
    else:
        var = den = ref[:, d:]
    sd = np.sqrt(var)
    em = np.abs(a[:, :d] - ref[:, :d]) / (np.maximum(np.abs(ref[:, :d]), sd) if theta else sd)
    return float(np.max(em)), float(np.max(np.abs(a[:, d:] - ref[:, d:]) / den))


def errors(spec, picked, flat):
    """{"mean", "par", "a", "fe": worst error} of `pick`'s output against the fixture's vector of the same case, in the measures of
    lar_ref.contract_errors: state means in posterior standard deviations; (co)variances relative to √(v_i v_j), θ's mean relative to
    max(|mθ_i|, its standard deviation), b relative — together "par"; a absolute (it is exact); F relative to max(1, |F|), per iteration and per series"""
    out, o, p = dict(mean=0.0, par=0.0, a=0.0, fe=0.0), 0, spec.p
    for kind, a in picked:
        a = np.asarray(a, dtype=np.float64)
        ref = flat[o:o + a.size].reshape(a.shape)
        o += a.size
        if kind == "skip":
            continue
        if not np.all(np.isfinite(a)):
            return dict(mean=np.inf, par=np.inf, a=np.inf, fe=np.inf)
        if kind.startswith("theta"):
            em, ec = _gauss(a, ref, p, kind == "theta full", True)
            out["par"] = max(out["par"], em, ec)
        elif kind in ("state full", "z"):
            em, ec = _gauss(a, ref, p if kind == "state full" else 1, True, False)
            out["mean"], out["par"] = max(out["mean"], em), max(out["par"], ec)
        elif kind == "rel":
            out["par"] = max(out["par"], float(np.max(np.abs(a - ref) / ref)))
        elif kind == "a":
            out["a"] = max(out["a"], float(np.max(np.abs(a - ref))))
        else:
            out["fe"] = max(out["fe"], float(np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref)))))
    assert o == flat.size, (o, flat.size)
    return out


def load(path):
    """{name: (values, crc, gauges [ratio, r_over_szz, cond])} of the fixture, in the order of GRID + SCAN"""
    g = np.load(path)
    specs = GRID + SCAN
    ends = np.cumsum(g["sizes"].astype(np.int64))
    assert len(ends) == len(specs) == len(g["crc"]) == len(g["gauges"]) and ends[-1] == g["values"].size
    return {s.name: (g["values"][e - n:e], int(c), ga) for s, e, n, c, ga in zip(specs, ends, g["sizes"], g["crc"], g["gauges"])}


def in_envelope(gauges):
    return bool(gauges[0] <= ENVELOPE["ratio"] and gauges[2] <= ENVELOPE["cond"] and gauges[1] >= ENVELOPE["r_over_szz"])

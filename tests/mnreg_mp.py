"""The multinomial regression engine's semantic (include/rxhip.h rxhip_mnreg_desc) in 50-digit mpmath arithmetic, written from the statement and not from
tests/mnreg_ref.py: statistics from the per-row stick remainders (not from the column-sum identity), the iteration with an mpmath matrix inverse and
determinant, lnΓ through mpmath.loggamma, the online recursion with an explicit inverse of the step's prior."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50


def _vec(a):
    return [mp.mpf(float(v)) for v in a]


def _mat(A):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(A)])


def statistics(Y):
    """Y [N][K] -> (S [K − 1], kappa [K − 1], lc, n) over the rows without a NaN, from N_ik = N_i − Σ_{j<k} y_ij row by row"""
    K = Y.shape[1]
    S, kappa, lc, n = [mp.mpf(0)] * (K - 1), [mp.mpf(0)] * (K - 1), mp.mpf(0), 0
    for row in Y:
        if np.isnan(row).any():
            continue
        n += 1
        y = _vec(row)
        Ni = sum(y)
        lc += mp.loggamma(Ni + 1) - sum(mp.loggamma(v + 1) for v in y)
        rem = Ni
        for k in range(K - 1):
            S[k] += rem
            kappa[k] += y[k] - rem / 2
            rem -= y[k]
    return S, kappa, lc, n


def _logdet(A):
    L = mp.cholesky(A)
    return 2 * sum(mp.log(L[i, i]) for i in range(A.rows))


def _kl(m, V, mp0, W0):
    d = V.rows
    dm = mp.matrix([m[i] - mp0[i] for i in range(d)])
    tr = sum(W0[i, j] * V[j, i] for i in range(d) for j in range(d))
    return (tr + (dm.T * W0 * dm)[0] - d - _logdet(W0) - _logdet(V)) / 2


def iterate(S, kappa, lc, xi0, W0, m, V, iterations):
    """-> lists of (m, V, F) per iteration, and the last ω̄; xi0, m: lists, W0, V: mp.matrix"""
    d = len(S)
    mp0 = mp.lu_solve(W0, mp.matrix(xi0))
    out, w = [], [mp.mpf(0)] * d
    for _ in range(iterations):
        c = [mp.sqrt(m[k] ** 2 + V[k, k]) for k in range(d)]
        w = [S[k] * (mp.tanh(c[k] / 2) / (2 * c[k]) if c[k] != 0 else mp.mpf(1) / 4) for k in range(d)]
        P = sum(-S[k] * mp.log(2 * mp.cosh(c[k] / 2)) + c[k] ** 2 * w[k] / 2 for k in range(d))
        W = W0.copy()
        for k in range(d):
            W[k, k] += w[k]
        V = W ** -1
        mm = V * mp.matrix([xi0[k] + kappa[k] for k in range(d)])
        m = [mm[k] for k in range(d)]
        like = lc + sum(m[k] * kappa[k] for k in range(d)) - sum((V[k, k] + m[k] ** 2) * w[k] for k in range(d)) / 2 + P
        out.append((m, V, -like + _kl(m, V, mp0, W0)))
    return out, w


def run(Y, prior_xi, prior_precision, init, iterations):
    """as mnreg_ref.run: dict(mean [it][d], cov [it][d][d], fe [it]) rounded to float64"""
    S, kappa, lc, _ = statistics(np.asarray(Y, dtype=np.float64))
    its, _ = iterate(S, kappa, lc, _vec(prior_xi), _mat(prior_precision), _vec(init[0]), _mat(init[1]), iterations)
    return _pack(its)


def online(Y, prior_xi, prior_precision, iterations=1):
    """as mnreg_ref.online: dict(mean [T][d], cov [T][d][d], fe [T])"""
    Y = np.asarray(Y, dtype=np.float64)
    xi, W = _vec(prior_xi), _mat(prior_precision)
    d = len(xi)
    steps = []
    for t in range(len(Y)):
        V = W ** -1
        mm = V * mp.matrix(xi)
        m = [mm[k] for k in range(d)]
        if np.isnan(Y[t]).any():
            steps.append((m, V, mp.mpf(0)))
            continue
        S, kappa, lc, _ = statistics(Y[t:t + 1])
        its, w = iterate(S, kappa, lc, xi, W, m, V, iterations)
        steps.append(its[-1])
        xi = [xi[k] + kappa[k] for k in range(d)]
        for k in range(d):
            W[k, k] += w[k]
    return _pack(steps)


def _pack(its):
    d = len(its[0][0])
    return dict(mean=np.array([[float(v) for v in m] for m, _, _ in its]),
                cov=np.array([[[float(V[i, j]) for j in range(d)] for i in range(d)] for _, V, _ in its]),
                fe=np.array([float(F) for _, _, F in its]), fe_mp=[F for _, _, F in its])

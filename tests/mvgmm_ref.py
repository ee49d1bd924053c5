"""NumPy restatement of the C oracle's multivariate mixture VMP (oracle/rxoracle.c rxo_mvgmm_vmp) at ANY dimension.

The C oracle stops at d = 8; the device engine reaches d = 32.  This module follows the oracle statement by statement — same
schedule (q(z) from the previous marginals; q(s), q(m[k]) with the previous E[W]; q(w[k]) with the new q(m[k])), same algebra
(Σπ, Σπy, Σπyy'), same closed forms of the free energy — with the loops over points and matrix entries written as array
operations.  tests/test_mvgmm_ref_cpu.py pins it to the oracle where both run.

state / init / hist layout per component (rxoracle.mvgmm_pack): mean[d] | cov[d][d] | nu | V[d][d] | alpha."""
import numpy as np
from scipy.special import digamma, gammaln

LOG2 = 0.69314718055994530942
LOG2PI = 1.8378770664093454835606594728112
LOGPI = 1.1447298858494001741434273513531


def _mvdigamma(a, d):
    return float(np.sum(digamma(a - 0.5 * np.arange(d))))


def _mvlgamma(a, d):
    return 0.25 * d * (d - 1) * LOGPI + float(np.sum(gammaln(a - 0.5 * np.arange(d))))


def _cholinv(A):
    """(A⁻¹, log|A|) of a symmetric positive definite matrix; LinAlgError when it is not."""
    L = np.linalg.cholesky(A)
    Li = np.linalg.solve(L, np.eye(A.shape[0]))
    return Li.T @ Li, 2.0 * float(np.sum(np.log(np.diag(L))))


def mvgmm_vmp(y, mu0, S0, nu0, V0, alpha0, init, iterations, want_resp=False):
    """Same signature and return values as rxoracle.mvgmm_vmp: hist [it][K][SZ], fe [it], resp [N][K] | None."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    N, d = y.shape
    mu0, S0, nu0, V0, alpha0 = (np.asarray(a, dtype=np.float64) for a in (mu0, S0, nu0, V0, alpha0))
    K = mu0.shape[0]
    dd = d * d
    SZ = 2 + d + 2 * dd
    st = np.array(init, dtype=np.float64).reshape(K, SZ)
    hist, fe, resp = np.empty((iterations, K, SZ)), np.empty(iterations), None
    S0i, V0i, ldS0, ldV0 = np.empty((K, d, d)), np.empty((K, d, d)), np.empty(K), np.empty(K)
    for k in range(K):
        S0i[k], ldS0[k] = _cholinv(S0[k])
        V0i[k], ldV0[k] = _cholinv(V0[k])
    for it in range(iterations):
        mean, cov = st[:, :d].copy(), st[:, d:d + dd].reshape(K, d, d).copy()
        nu, V, al = st[:, d + dd].copy(), st[:, d + dd + 1:d + 2 * dd + 1].reshape(K, d, d).copy(), st[:, -1].copy()
        asum = float(np.sum(al))
        EW = nu[:, None, None] * V
        Elw = np.array([_mvdigamma(0.5 * nu[k], d) + d * LOG2 + _cholinv(V[k])[1] for k in range(K)])
        Els = digamma(al) - digamma(asum)
        # q(z_i): logit_k = E log s_k − ½[d log 2π − E log|W_k| + tr(E[W_k]((y − m)(y − m)' + cov_k))]
        lg = np.empty((N, K))
        for k in range(K):
            dv = y - mean[k]
            q = np.einsum("na,ab,nb->n", dv, EW[k], dv) + float(np.sum(EW[k] * cov[k]))
            lg[:, k] = Els[k] - 0.5 * (d * LOG2PI - Elw[k] + q)
        pi = np.exp(lg - lg.max(axis=1, keepdims=True))
        pi /= pi.sum(axis=1, keepdims=True)
        Hz = -float(np.sum(np.where(pi > 0.0, pi * np.log(np.where(pi > 0.0, pi, 1.0)), 0.0)))
        if want_resp and it == iterations - 1:
            resp = pi.copy()
        S0k = pi.sum(axis=0)
        S1 = pi.T @ y
        S2 = np.stack([(pi[:, k, None] * y).T @ y for k in range(K)])
        F, Sc = -Hz, np.empty((K, d, d))
        for k in range(K):
            Lam = S0i[k] + S0k[k] * EW[k]
            xi = S0i[k] @ mu0[k] + EW[k] @ S1[k]
            Cm, _ = _cholinv(Lam)
            mb = Cm @ xi
            Sc[k] = S2[k] - np.outer(mb, S1[k]) - np.outer(S1[k], mb) + S0k[k] * (np.outer(mb, mb) + Cm)
            Vn, _ = _cholinv(V0i[k] + Sc[k])
            st[k, :d] = mb
            st[k, d:d + dd] = Cm.ravel()
            st[k, d + dd] = nu0[k] + S0k[k]
            st[k, d + dd + 1:d + 2 * dd + 1] = Vn.ravel()
            st[k, -1] = alpha0[k] + S0k[k]
        hist[it] = st
        as2, a0s = float(np.sum(st[:, -1])), float(np.sum(alpha0))
        lB, lB0, Hs_t, Us_t = -gammaln(as2), -gammaln(a0s), 0.0, 0.0
        for k in range(K):
            mb, Cm = st[k, :d], st[k, d:d + dd].reshape(d, d)
            nuk, Vk, alk = st[k, d + dd], st[k, d + dd + 1:d + 2 * dd + 1].reshape(d, d), st[k, -1]
            ldV, ldC = _cholinv(Vk)[1], _cholinv(Cm)[1]
            Elwk = _mvdigamma(0.5 * nuk, d) + d * LOG2 + ldV
            Elsk = digamma(alk) - digamma(as2)
            trWS = float(np.sum(nuk * Vk * Sc[k].T))
            trV0W = float(np.sum(V0i[k] * nuk * Vk.T))
            dm = mb - mu0[k]
            trS0 = float(np.sum(S0i[k] * (Cm.T + np.outer(dm, dm))))
            F += 0.5 * (S0k[k] * (d * LOG2PI - Elwk) + trWS) - S0k[k] * Elsk
            F += 0.5 * (d * LOG2PI + ldS0[k] + trS0) - 0.5 * (d * (LOG2PI + 1.0) + ldC)
            n0 = nu0[k]
            F += -(0.5 * (n0 - d - 1.0) * Elwk - 0.5 * trV0W - 0.5 * n0 * d * LOG2 - 0.5 * n0 * ldV0[k] - _mvlgamma(0.5 * n0, d))
            F -= (0.5 * (d + 1.0) * ldV + 0.5 * d * (d + 1.0) * LOG2 + _mvlgamma(0.5 * nuk, d)
                  - 0.5 * (nuk - d - 1.0) * _mvdigamma(0.5 * nuk, d) + 0.5 * nuk * d)
            lB += gammaln(alk)
            lB0 += gammaln(alpha0[k])
            Us_t += (alpha0[k] - 1.0) * Elsk
            Hs_t += (alk - 1.0) * digamma(alk)
        if K > 1:
            F += (lB0 - Us_t) - (lB + (as2 - K) * digamma(as2) - Hs_t)
        fe[it] = F
    return hist, fe, resp

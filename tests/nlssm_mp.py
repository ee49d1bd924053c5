"""The nonlinear state-space engine's definition (include/rxhip.h rxhip_nlssm_desc) restated at 50 digits with mpmath: the reference that
tests/nlssm_ref.py (float64) is held to.  It shares the test functions' formulas with nlssm_ref (`f(x, M)` with M = mpmath) and nothing else: the
Jacobians are taken with mpmath.diff at that precision — no differentiation rule in common with the interpreter's duals or with the hand-written
ones —, the linear algebra is mpmath's, digamma and log-gamma are mpmath's.

ENVELOPE: the largest error of the float64 restatement against this one over every series of every case of nlssm_ref.case_grid() — the whole grid of
tests/test_nlssm_gpu.py —, in the contract's gauges (measured by tests/test_nlssm_ref_cpu.py, which asserts that it stays within one hundredth of each
contract bound)."""
import mpmath as mp
import numpy as np

import nlssm_ref as R

DPS = 50

# measured: python tests/nlssm_mp.py  (the float64 restatement against 50 digits over all 2 072 series of the grid above)
ENVELOPE = dict(mean=7.4e-9, cov=5.2e-9, gamma=7.3e-10, fe=9.6e-11)


def _jac(f, d, x):
    return mp.matrix([[mp.diff(lambda *a: f(list(a), mp)[i], tuple(x), tuple(int(k == j) for k in range(d))) for j in range(d)] for i in range(d)])


def delta(name, method, m, V, unscented=(1e-3, 2.0, 0.0)):
    d, f, _ = R.FUNCS[name]
    if method == "linearization":
        J = _jac(f, d, m)
        mt = mp.matrix(f(list(m), mp))
        Ct = V * J.T
        Vt = J * Ct
    else:
        alpha, beta, kappa = (mp.mpf(repr(v)) for v in unscented)
        sc = alpha * alpha * (d + kappa)
        wm0 = (sc - d) / sc
        wc0, wi = wm0 + 1 - alpha * alpha + beta, 1 / (2 * sc)
        L = mp.cholesky(sc * V)
        X = [m] + [m + L[:, k] for k in range(d)] + [m - L[:, k] for k in range(d)]
        Y = [mp.matrix(f(list(x), mp)) for x in X]
        wm, wc = [wm0] + [wi] * (2 * d), [wc0] + [wi] * (2 * d)
        mt = mp.zeros(d, 1)
        for w, y in zip(wm, Y):
            mt += w * y
        Vt, Ct = mp.zeros(d, d), mp.zeros(d, d)
        for w, x, y in zip(wc, X, Y):
            Vt += w * (y - mt) * (y - mt).T
            Ct += w * (x - m) * (y - mt).T
    return mt, (Vt + Vt.T) / 2, Ct


def _logdet(A):
    return mp.log(mp.det(A))


def _gauss_kl(m1, V1, m0, V0):
    P0 = mp.inverse(V0)
    dm = m1 - m0
    return (sum((P0 * V1)[i, i] for i in range(V1.rows)) + (dm.T * P0 * dm)[0, 0] - V1.rows + _logdet(V0) - _logdet(V1)) / 2


def _gamma_kl(a1, b1, a0, b0):
    return (a1 - a0) * mp.digamma(a1) - mp.loggamma(a1) + mp.loggamma(a0) + a0 * (mp.log(b1) - mp.log(b0)) + a1 * (b0 - b1) / b1


def run_series(name, y, m0, V0, Q, H, R_=None, noise=None, method="linearization", mode="filter", iterations=1):
    """as nlssm_ref.run_series, at DPS digits; returns float64 arrays"""
    with mp.workdps(DPS):
        d = R.FUNCS[name][0]
        T = y.shape[0]
        M = lambda a: mp.matrix(np.atleast_2d(np.asarray(a, dtype=np.float64)).tolist())
        H, Q = M(H), M(Q)
        m, V = M(np.asarray(m0).reshape(d, 1)), M(V0)
        Rm = M(R_) if R_ is not None else None
        a, b = (mp.mpf(noise[0]), mp.mpf(noise[1])) if noise is not None else (mp.mpf(1), mp.mpf(1))
        log2pi = mp.log(2 * mp.pi)
        fm, fV, pm, pP, pC, shape, rate = [], [], [], [], [], [], []
        fe = mp.mpf(0)
        for t in range(T):
            mt, Vt, Ct = delta(name, method, m, V)
            P = Vt + Q
            pm.append(mt); pP.append(P); pC.append(Ct)
            if np.any(np.isnan(y[t])):
                m, V = mt, P
            elif noise is not None:
                c, yt = H.T, mp.mpf(float(y[t, 0]))
                E = a / b
                for _ in range(iterations):
                    k = P * c
                    s = (c.T * k)[0, 0]
                    g = E / (1 + E * s)
                    mn = mt + k * g * (yt - (c.T * mt)[0, 0])
                    Vn = P - g * k * k.T
                    an = a + mp.mpf(1) / 2
                    e2 = (yt - (c.T * mn)[0, 0]) ** 2 + (c.T * Vn * c)[0, 0]
                    bn = b + e2 / 2
                    E = an / bn
                fe += _gauss_kl(mn, Vn, mt, P) + _gamma_kl(an, bn, a, b) + (log2pi - (mp.digamma(an) - mp.log(bn)) + (an / bn) * e2) / 2
                m, V, a, b = mn, (Vn + Vn.T) / 2, an, bn
            else:
                yt = M(np.asarray(y[t]).reshape(-1, 1))
                S = H * P * H.T + Rm
                r = yt - H * mt
                Si = mp.inverse(S)
                K = P * H.T * Si
                m = mt + K * r
                V = P - K * S * K.T
                V = (V + V.T) / 2
                fe += (yt.rows * log2pi + _logdet(S) + (r.T * Si * r)[0, 0]) / 2
            fm.append(m); fV.append(V); shape.append(a); rate.append(b)
        sm, sV = list(fm), list(fV)
        if mode == "smooth":
            for t in range(T - 2, -1, -1):
                Gn = pC[t + 1] * mp.inverse(pP[t + 1])
                sm[t] = fm[t] + Gn * (sm[t + 1] - pm[t + 1])
                Vs = fV[t] + Gn * (sV[t + 1] - pP[t + 1]) * Gn.T
                sV[t] = (Vs + Vs.T) / 2
        f64 = lambda A: np.array(A.tolist(), dtype=np.float64)
        return dict(mean=np.array([f64(v)[:, 0] for v in sm]), cov=np.array([f64(v) for v in sV]), shape=np.array([float(v) for v in shape]),
                    rate=np.array([float(v) for v in rate]), fe=float(fe))


def run_case(case, method, mode, iterations):
    y = case["y"]
    outs = []
    for s in range(y.shape[1]):
        m0, V0 = (case["m0"][s], case["V0"][s]) if case["per_series"] else (case["m0"], case["V0"])
        outs.append(run_series(case["name"], y[:, s], m0, V0, case["Q"], case["H"], R_=None if case["noise"] else case["R"], noise=case["noise"], method=method,
                               mode=mode, iterations=iterations))
    return dict(mean=np.stack([o["mean"] for o in outs], 1), cov=np.stack([o["cov"] for o in outs], 1), shape=np.stack([o["shape"] for o in outs], 1),
                rate=np.stack([o["rate"] for o in outs], 1), fe=np.array([o["fe"] for o in outs]))


def _series_errors(task):
    """errors of the float64 restatement against 50 digits on ONE series of case k of nlssm_ref.case_grid() (the grid is rebuilt in the worker: it is
    a deterministic function of its seeds)"""
    k, s = task
    cid, c, method, mode, it = _grid()[k]
    one = dict(c, y=c["y"][:, s:s + 1], m0=c["m0"][s:s + 1] if c["per_series"] else c["m0"], V0=c["V0"][s:s + 1] if c["per_series"] else c["V0"])
    return R.errors(R.run_case(one, method, mode, it), run_case(one, method, mode, it), c["noise"] is not None)


_GRID = None


def _grid():
    global _GRID
    if _GRID is None:
        _GRID = R.case_grid()
    return _GRID


def measure(workers=None):
    """the worst error per gauge over EVERY series of EVERY case of nlssm_ref.case_grid() — the grid of tests/test_nlssm_gpu.py, all 70 series of the
    large cases included (they hold different random data).  About ten CPU minutes of mpmath, spread over `workers` processes (default: the CPUs, 16 at most)."""
    import multiprocessing as mproc
    import os
    tasks = [(k, s) for k, (_, c, *_rest) in enumerate(_grid()) for s in range(c["y"].shape[1])]
    workers = workers or max(1, min(16, os.cpu_count() or 1))
    worst = dict(mean=0.0, cov=0.0, gamma=0.0, fe=0.0)
    with mproc.get_context("fork").Pool(workers) as pool:
        for err in pool.imap_unordered(_series_errors, tasks, chunksize=8):
            for key, v in err.items():
                worst[key] = max(worst[key], v)
    return worst


if __name__ == "__main__":
    print(measure())

"""The Gamma mixture engine's iteration (include/rxhip.h rxhip_gammamix_desc) in 50-digit mpmath arithmetic: the statement tests/gammamix_ref.py is pinned to
(tests/test_gammamix_ref_cpu.py).  Written from the definition — logits, softmax, the three weighted sums and the entropy, the Dirichlet and Gamma updates,
the shape as the root of g' by a bracketing method (Illinois regula falsi between expanded brackets), F from its terms — with no code shared with the
restatement."""
import mpmath as mp
import numpy as np

DIGITS = 50   # set around every run (mp.workdps): the precision of the process is left as it was found


def _kl_gamma(a, b, a0, b0):
    return (a - a0) * mp.digamma(a) - mp.loggamma(a) + mp.loggamma(a0) + a0 * (mp.log(b) - mp.log(b0)) + a * (b0 - b) / b


def _root(c0, d0, S0, B, a_prev):
    g = lambda a: (c0 - 1) / a - d0 + B - S0 * mp.digamma(a)
    lo = hi = a_prev
    while g(lo) <= 0:
        lo = lo / 4
    while g(hi) >= 0:
        hi = hi * 4
    return mp.findroot(g, (lo, hi), solver="illinois", tol=mp.mpf(10) ** (-2 * DIGITS + 10), maxsteps=400)


def run(y, prior, init=None, iterations=10):
    """as gammamix_ref.run; returns float arrays rounded from the 50-digit values: a, e, f, alpha [iterations][K], fe [iterations]"""
    with mp.workdps(DIGITS):
        return _run(y, prior, init, iterations)


def _run(y, prior, init, iterations):
    c0, d0, e0, f0, al0 = [[mp.mpf(float(v)) for v in p] for p in prior]
    K = len(c0)
    if init is None:
        a, e, f, al = [mp.mpf(1)] * K, [mp.mpf(1)] * K, [mp.mpf(1)] * K, list(al0)
    else:
        a, e, f, al = [[mp.mpf(float(v)) for v in q] for q in init]
    ys = [mp.mpf(float(v)) for v in y if v == v]
    ls = [mp.log(v) for v in ys]
    out = dict(a=[], e=[], f=[], alpha=[], fe=[])
    for _ in range(iterations):
        asum = mp.fsum(al)
        cst = [(mp.digamma(al[k]) - mp.digamma(asum) + a[k] * (mp.digamma(e[k]) - mp.log(f[k])) - mp.loggamma(a[k]), a[k] - 1, e[k] / f[k]) for k in range(K)]
        S0, S1, SL, H = [mp.mpf(0)] * K, [mp.mpf(0)] * K, [mp.mpf(0)] * K, mp.mpf(0)
        for yv, lv in zip(ys, ls):
            lg = [c[0] + c[1] * lv - c[2] * yv for c in cst]
            mx = max(lg)
            ex = [mp.exp(v - mx) for v in lg]
            Z = mp.fsum(ex)
            for k in range(K):
                r = ex[k] / Z
                S0[k] += r
                S1[k] += r * yv
                SL[k] += r * lv
                if r > 0:
                    H -= r * mp.log(r)
        al = [al0[k] + S0[k] for k in range(K)]
        Elnb_old = [mp.digamma(e[k]) - mp.log(f[k]) for k in range(K)]
        a = [_root(c0[k], d0[k], S0[k], S0[k] * Elnb_old[k] + SL[k], a[k]) if S0[k] > 0 else a[k] for k in range(K)]
        e = [e0[k] + S0[k] * a[k] for k in range(K)]
        f = [f0[k] + S1[k] for k in range(K)]
        asum, a0sum = mp.fsum(al), mp.fsum(al0)
        F = -H
        for k in range(K):
            Elns, Elnb = mp.digamma(al[k]) - mp.digamma(asum), mp.digamma(e[k]) - mp.log(f[k])
            F -= S0[k] * (Elns + a[k] * Elnb - mp.loggamma(a[k])) + (a[k] - 1) * SL[k] - e[k] / f[k] * S1[k]
            F += _kl_gamma(e[k], f[k], e0[k], f0[k])
            F -= c0[k] * mp.log(d0[k]) - mp.loggamma(c0[k]) + (c0[k] - 1) * mp.log(a[k]) - d0[k] * a[k]
            F += -mp.loggamma(al[k]) + mp.loggamma(al0[k]) + (al[k] - al0[k]) * Elns
        F += mp.loggamma(asum) - mp.loggamma(a0sum)
        out["fe"].append(float(F))
        for key, v in (("a", a), ("e", e), ("f", f), ("alpha", al)):
            out[key].append([float(x) for x in v])
    return {k: np.array(v) for k, v in out.items()}

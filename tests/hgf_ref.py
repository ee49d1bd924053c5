"""High-precision restatement of the online hierarchical Gaussian filter (one series), in mpmath at 60 digits.  It is written from the
model as oracle/rxoracle.h and the header of csrc/hgf_kernels.hpp state it and shares no code with either: it pins the arithmetic of the
C oracle (tests/test_hgf_ref_cpu.py), which in turn is what the engine is held to (tests/test_hgf_contract_gpu.py).

    zt_min ~ N(zm, zv);  xt_min ~ N(xm, xv);  zt ~ N(zt_min, z_variance);  xt ~ GCV(xt_min, zt, κ, ω);  y ~ N(xt, y_variance)
    q(xt, zt, xt_min) = q(xt, xt_min) q(zt),  `iters` VMP iterations per observation, then (zm, zv, xm, xv) ← mean_var(q(zt)), mean_var(q(xt)).

Also here: the parameter grid of the contract test and the cases excluded from it (both test files read them from this one place)."""
import functools
import itertools

import mpmath
import numpy as np
from mpmath import mp, mpf

DIGITS = 60


@functools.lru_cache(maxsize=None)
def gauss_hermite(n):
    """Nodes and weights of the n-point Gauss–Hermite rule (∫ e^{−x²} f ≈ Σ w f), as roots of Hₙ: the eigenvalues of the Jacobi matrix of
    the recurrence start a Newton iteration on the orthonormal ĥₙ; the weights are the Christoffel numbers 1 / Σ_{k<n} ĥ_k(x)²."""
    with mp.workdps(DIGITS + 10):
        def values(x):   # ĥ_0 … ĥ_n at x:  ĥ_{k+1} = x·sqrt(2/(k+1))·ĥ_k − sqrt(k/(k+1))·ĥ_{k−1}
            h = [mp.pi ** mpf(-0.25)]
            if n >= 1:
                h.append(mp.sqrt(2) * x * h[0])
            for k in range(1, n):
                h.append(x * mp.sqrt(mpf(2) / (k + 1)) * h[k] - mp.sqrt(mpf(k) / (k + 1)) * h[k - 1])
            return h

        if n == 1:
            start = [mpf(0)]
        else:
            J = mp.zeros(n, n)
            for k in range(1, n):
                J[k - 1, k] = J[k, k - 1] = mp.sqrt(mpf(k) / 2)
            start = sorted(mp.eigsy(J, eigvals_only=True))
        xs, ws = [], []
        for x in start:
            for _ in range(8):   # ĥₙ' = sqrt(2n)·ĥ_{n−1}
                h = values(x)
                x = x - h[n] / (mp.sqrt(2 * n) * h[n - 1])
            h = values(x)
            assert abs(h[n]) < mpf(10) ** (-DIGITS + 5) * max(1, abs(h[n - 1]))
            xs.append(x)
            ws.append(1 / sum(v * v for v in h[:n]))
        assert abs(sum(ws) - mp.sqrt(mp.pi)) < mpf(10) ** (-DIGITS)
        return tuple(xs), tuple(ws)


class IllPosed(ArithmeticError):
    """a cubature variance that is not positive: the message's mode has left the range of the rule"""


def _moments(points, weights, density):
    """approximate_meancov, its two rounds: (norm, mean), then the second moment about that mean"""
    c = [w * density(p) for p, w in zip(points, weights)]
    norm = mp.fsum(c)
    mean = mp.fsum(ci * p for ci, p in zip(c, points)) / norm
    var = mp.fsum(ci * (p - mean) ** 2 for ci, p in zip(c, points)) / norm
    if not var > 0:
        raise IllPosed("cubature variance is not positive")
    return mean, var


def _pair(l00, l11, off, h0, h1):
    """Gaussian over a pair with precision [[l00, −off], [−off, l11]] and weighted mean (h0, h1): means, covariance entries, det of the precision"""
    det = l00 * l11 - off * off
    c00, c11, c01 = l11 / det, l00 / det, off / det
    return c00 * h0 + c01 * h1, c01 * h0 + c11 * h1, c00, c11, c01, det


def hgf_filter(y, kappa, omega, z_variance, y_variance, z0=(0.0, 5.0), x0=(0.0, 5.0), iters=10, n_gh=31, want_fe=True):
    """zm, zv, xm, xv [T] (posteriors after the last iteration of every observation) and fe [iters] (mean over the observations of the Bethe
    free energy after every iteration), as float64."""
    with mp.workdps(DIGITS):
        gx, gw = gauss_hermite(int(n_gh))
        rpi = mp.sqrt(mp.pi)
        gw = [w / rpi for w in gw]
        k, om, qz, qy = (mpf(float(v)) for v in (kappa, omega, z_variance, y_variance))
        l2pi = mp.log(2 * mp.pi)
        zm, zv, xm, xv = mpf(float(z0[0])), mpf(float(z0[1])), mpf(float(x0[0])), mpf(float(x0[1]))
        std_points = [mp.sqrt(2) * x for x in gx]
        out = [[], [], [], []]
        fe = [mpf(0)] * iters
        for yt in (mpf(float(v)) for v in np.asarray(y, dtype=np.float64).ravel()):
            pzm, pzv, pxm, pxv = zm, zv, xm, xv      # the priors of this observation (@autoupdates)
            fwd_var = pzv + qz                       # the transition's message toward zt
            points = [pzm + mp.sqrt(2 * fwd_var) * x for x in gx]
            for n in range(iters):
                gain = mp.exp(-om) * mp.exp(-k * zm + k * k * zv / 2)            # E exp(−(κ zt + ω)) under the current q(zt)
                m_x, m_xmin, v_x, v_xmin, v_c, det_x = _pair(1 / qy + gain, 1 / pxv + gain, gain, yt / qy, pxm / pxv)
                psi = (m_x - m_xmin) ** 2 + v_x + v_xmin - 2 * v_c               # E (xt − xt_min)²
                msg = lambda z: mp.exp(-(k * z + psi * mp.exp(-om) * mp.exp(-k * z)) / 2)   # the GCV node's message toward zt
                zm, zv = _moments(points, gw, msg)
                xm, xv = m_x, v_x
                if want_fe:
                    # the transition node sees the z-message through its Gaussian moments: those of msg(z)·exp(z²/2) against N(0, 1)
                    em, ev = _moments(std_points, gw, lambda z: msg(z) * mp.exp(z * z / 2))
                    j_z, j_zmin, s_z, s_zmin, s_c, det_z = _pair(1 / ev + 1 / qz, 1 / pzv + 1 / qz, 1 / qz, em / ev, pzm / pzv)
                    F = (l2pi + mp.log(pzv) + ((j_zmin - pzm) ** 2 + s_zmin) / pzv) / 2            # prior of zt_min
                    F += (l2pi + mp.log(pxv) + ((m_xmin - pxm) ** 2 + v_xmin) / pxv) / 2          # prior of xt_min
                    F += (l2pi + mp.log(qz) + ((j_z - j_zmin) ** 2 + s_z + s_zmin - 2 * s_c) / qz) / 2   # transition
                    F += (l2pi + k * zm + om + psi * mp.exp(-om) * mp.exp(-k * zm + k * k * zv / 2)) / 2  # GCV, under the new q(zt)
                    F += (l2pi + mp.log(qy) + ((yt - m_x) ** 2 + v_x) / qy) / 2                  # observation
                    F -= l2pi + 1 - mp.log(det_z) / 2                                             # entropy of q(zt, zt_min)
                    F -= l2pi + 1 - mp.log(det_x) / 2                                             # entropy of q(xt, xt_min)
                    fe[n] += F
            for o, v in zip(out, (zm, zv, xm, xv)):
                o.append(float(v))
        T = len(out[0])
        return tuple(np.array(o) for o in out) + (np.array([float(f / T) for f in fe]),)


# ---- the parameter range the engine is held on (tests/test_hgf_contract_gpu.py); its corners are pinned on the CPU (tests/test_hgf_ref_cpu.py)
KAPPAS, OMEGAS, Z_VARIANCES, Y_VARIANCES = (-1.5, -0.3, 0.3, 1.0), (-6.0, 0.0, 4.0), (1e-4, 0.04, 1.0), (1e-6, 1e-2, 1e2)
CENTRE = (0.3, 0.0, 0.04, 1e-2)
KAPPA_2 = tuple((2.0, w, zv, 1e2) for w in (-6.0, 4.0) for zv in (1e-4, 0.04))
GRID = tuple(itertools.product(KAPPAS, OMEGAS, Z_VARIANCES, Y_VARIANCES)) + KAPPA_2
CORNERS = tuple(itertools.product((KAPPAS[0], KAPPAS[-1]), (OMEGAS[0], OMEGAS[-1]), (Z_VARIANCES[0], Z_VARIANCES[-1]), (Y_VARIANCES[0], Y_VARIANCES[-1]))) + \
    (CENTRE,) + KAPPA_2

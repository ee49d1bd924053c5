"""The nonlinear state-space engine's class (include/rxhip.h rxhip_nlssm_desc): a `_StateEngine` like the other families with posteriors of a latent
state, kept next to the expression tracer (expr.py) that turns its `f` into a program.  rxhip.engine re-exports it."""
import ctypes

import numpy as np

from . import _lib
from .engine import _StateEngine, _c, _p
from .expr import Program, trace


class NonlinearSSMEngine(_StateEngine):
    """Nonlinear state-space model `x[0] ~ N(m0, V0); x[t] ~ N(f(x[t-1]), Q); y[t] ~ N(H x[t], R)` or, with `noise_prior=(shape, rate)`,
    `τ ~ Gamma(shape, rate); y[t] ~ N(cᵀx[t], 1/τ)`, for n_series independent series: batched extended (`method="linearization"`) or unscented
    (`method="unscented"`, `unscented=(alpha, beta, kappa)`) Kalman filtering (`mode="filter"`) and smoothing (`mode="smooth"`), include/rxhip.h
    rxhip_nlssm_desc.  `f` is a callable traced by rxhip.trace, or a Program.  `run(iterations)`: the VMP iterations per observation with unknown
    noise; `marginals()`: x[1 … T], filtered or smoothed; `noise()`: q(τ) after every observation."""

    def __init__(self, f, d, T, m0, V0, H, R=None, Q=None, noise_prior=None, method="linearization", unscented=None, mode="filter", n_series=1,
                 per_series=False, device=-1, stream=None):
        L = _lib.lib()
        prog = f if isinstance(f, Program) else trace(f, d)
        d, n_series = int(d), int(n_series)
        H = _c(H)
        H = H.reshape(1, -1) if H.ndim == 1 else H
        dy = H.shape[0]
        desc = _lib.NlssmDesc()
        desc.T, desc.n_series, desc.d, desc.dy = int(T), n_series, d, dy
        ps, keep = prog.c_struct()
        desc.f = ctypes.pointer(ps)
        m0 = _c(m0, (n_series, d) if per_series else (d,))
        V0 = _c(V0, (n_series, d, d) if per_series else (d, d))
        desc.m0, desc.V0, desc.H = _p(m0), _p(V0), _p(H)
        Qa = _c(Q, (d, d)) if Q is not None else None
        Ra = _c(R, (dy, dy)) if R is not None else None
        desc.Q = _p(Qa) if Qa is not None else None
        desc.R = _p(Ra) if Ra is not None else None
        if noise_prior is not None:
            desc.noise_shape, desc.noise_rate = float(noise_prior[0]), float(noise_prior[1])
        if method not in ("linearization", "unscented"):
            raise ValueError("NonlinearSSMEngine: method is 'linearization' or 'unscented'")
        if mode not in ("filter", "smooth"):
            raise ValueError("NonlinearSSMEngine: mode is 'filter' or 'smooth'")
        desc.method = _lib.NLSSM_UNSCENTED if method == "unscented" else _lib.NLSSM_LINEARIZATION
        desc.alpha, desc.beta, desc.kappa = (float(v) for v in (unscented if unscented is not None else (1e-3, 2.0, 0.0)))   # RXHIP_NLSSM_DEFAULT_*
        desc.mode = _lib.NLSSM_SMOOTH if mode == "smooth" else _lib.NLSSM_FILTER
        desc.per_series, desc.device = int(bool(per_series)), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.T, self.n_series, self.n_chains, self.d, self.dy, self.program = int(T), n_series, n_series, d, dy, prog
        self.unknown_noise = noise_prior is not None
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_nlssm_create(ctypes.byref(desc), ctypes.byref(self._h)))
        del keep

    def noise(self):
        """(shape, rate) of q(τ) after every observation, [T][series] each"""
        shape, rate = np.empty((self.T, self.n_series)), np.empty((self.T, self.n_series))
        self._chk(_lib.lib().rxhip_nlssm_get_noise(self._h, _p(shape), _p(rate)))
        return shape, rate

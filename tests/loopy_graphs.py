"""Loopy Gaussian graphs for the node-array executor's loopy schedule (include/rxhip.h "Loopy graphs"): the linear regression of RxInfer's
initialisation manual (docs/src/manuals/inference/initialization.md; test/models/regression/linreg_tests.jl),

    a ~ Normal(mean = 0, var = 1);  b ~ Normal(mean = 0, var = 1);  y[i] ~ Normal(mean = x[i] * b + a, var = 1)

with `μ(b) = NormalMeanVariance(0, 100)`, here with the inputs x as constants of the graph (the observations y are the data of every replica)."""
import numpy as np

from rxhip import _lib
from rxhip.graph import GraphBuilder


def reference_data(N=100):
    """x = 1:N .+ randn(StableRNG(1234), N) drawn by sequential randn() calls (not checked bit for bit against Julia's randn(rng, N)), y = 10 − 10x"""
    from stable_rng import StableRNG

    rng = StableRNG(1234)
    x = np.arange(1, N + 1, dtype=float) + np.array([rng.randn() for _ in range(N)])
    return x, 10.0 - 10.0 * x


def linreg(x, prior_a=(0.0, 1.0), prior_b=(0.0, 1.0), noise_var=1.0, init=None):
    """The regression graph.  x: [N] (scalar a, b, y) or [N][dy][d] (y[i] ~ MvNormal(X[i] * b + a, Σ) with b of dimension d, a and y of dimension dy; the
    priors and noise then as (mean [·], cov [·][·]) / Σ [dy][dy]).  init: {"a" | "b": (mean, var | cov)} message initialisations, or {"t": (i, (mean,
    var))} on the anonymous output of x[i] * b.  Returns (builder, y data variables, dict(a=, b=, t=[…], s=[…]))."""
    x = np.asarray(x, float)
    vec = x.ndim == 3
    gb = GraphBuilder()
    dy, d = (x.shape[1], x.shape[2]) if vec else (1, 1)
    a, b = gb.randomvar(dy, name="a"), gb.randomvar(d, name="b")
    if vec:
        gb.mvnormal_mean_cov(a, gb.constvar(np.asarray(prior_a[0], float)), gb.constvar(np.asarray(prior_a[1], float)))
        gb.mvnormal_mean_cov(b, gb.constvar(np.asarray(prior_b[0], float)), gb.constvar(np.asarray(prior_b[1], float)))
    else:
        gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, a, gb.constvar(prior_a[0]), gb.constvar(prior_a[1]))
        gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, b, gb.constvar(prior_b[0]), gb.constvar(prior_b[1]))
    ts, ss, ys = [], [], []
    for xi in x:
        t, s, y = gb.randomvar(dy), gb.randomvar(dy), gb.datavar(dy, name="y")
        gb.node(_lib.NODE_MULTIPLY, t, gb.constvar(xi if vec else float(xi)), b)
        gb.node(_lib.NODE_ADD, s, t, a)
        if vec:
            gb.mvnormal_mean_cov(y, s, gb.constvar(np.asarray(noise_var, float)))
        else:
            gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, y, s, gb.constvar(noise_var))
        ts.append(t); ss.append(s); ys.append(y)
    for k, v in (init or {}).items():
        var, mv = (a, v) if k == "a" else (b, v) if k == "b" else (ts[v[0]], v[1])
        if vec:
            gb.initialize_message(var, _lib.INIT_MVNORMAL, np.concatenate([np.ravel(mv[0]), np.ravel(mv[1])]))
        else:
            gb.initialize_message(var, _lib.INIT_NORMAL, mv)
    return gb, ys, dict(a=a, b=b, t=ts, s=ss)


def vector_problem(N, d, seed=0):
    """a vector regression of dimension d (dy = d): well-conditioned maps X[i], priors, noise, the `μ(b)` / `μ(a)` initialisation (non-zero mean,
    correlated covariance) and observations [replica][N][d] for 3 replicas"""
    rng = np.random.default_rng(seed)
    X = np.eye(d) + 0.3 * rng.normal(size=(N, d, d)) / np.sqrt(d)
    def spd(s):
        M = rng.normal(size=(d, d)) / np.sqrt(d)
        return s * (np.eye(d) + 0.3 * (M @ M.T))
    prior_a, prior_b = (rng.normal(size=d), spd(2.0)), (rng.normal(size=d), spd(1.5))
    noise = spd(0.5)
    D = (rng.normal(size=d), spd(10.0))
    b_true = rng.normal(size=d)
    Y = np.stack([np.einsum("nij,j->ni", X, b_true + 0.1 * r) + rng.normal(size=(N, d)) for r in range(3)])
    return X, prior_a, prior_b, noise, D, Y

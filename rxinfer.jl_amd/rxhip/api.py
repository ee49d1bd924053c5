"""`infer(model=..., data=..., ...)` — Python mirror of RxInfer's front door for the hot path.

Mirrors src/inference/inference.jl:577-609 (keyword names, `free_energy`, `iterations`,
`options`, `catch_exception`) and `InferenceResult` (src/inference/batch.jl:18-24) for the model
family the device schedule covers.  The Julia host shim (rxinfer.jl_amd/julia/RxHip.jl) binds the
same C ABI; this mirror exists because no Julia toolchain is present in the build image, so the
parity tests are written against it in the reference tests' own shape
(test/models/statespace/mlgssm_test.jl)."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Optional

import numpy as np

from . import _lib
from ._lib import RxHipError
from .engine import DriftChainEngine, GMMEngine, HGFEngine, LGSSMEngine, MvGMMEngine, ProbitEngine, HMMEngine, LAREngine, BinomialRegressionEngine, ARRegressionEngine, MultinomialRegressionEngine, GammaMixtureEngine, NonlinearSSMEngine


@dataclass
class MvNormalMeanCovariance:
    """ExponentialFamily.MvNormalMeanCovariance(μ, Σ) — the parametrisation posteriors are returned in."""
    mean: np.ndarray
    cov: np.ndarray


@dataclass
class LinearGaussianSSM:
    """Model specification produced by `linear_gaussian_ssm(...)` — the lowered form of
        x[1] ~ MvNormal(μ = m0, Σ = V0); y[t] ~ MvNormal(μ = B*x[t], Σ = Q);
        x[t] ~ MvNormal(μ = A*x[t-1], Σ = P)            (benchmarks notebook, cell 4)."""
    A: np.ndarray
    B: np.ndarray
    P: np.ndarray
    Q: np.ndarray
    prior_mean: np.ndarray
    prior_cov: np.ndarray
    prior_through_transition: bool = False
    step_model: Optional[np.ndarray] = None   # time-varying constants: A, B, P, Q are [n_models, …], step_model[t] picks
    state_offset: Optional[np.ndarray] = None  # known inputs: x[t] ~ MvNormal(μ = A*x[t-1] + c[t], Σ = P); [d] or [T, d]
    obs_offset: Optional[np.ndarray] = None    # y[t] ~ MvNormal(μ = B*x[t] + d[t], Σ = Q); [dy] or [T, dy]
    input_matrix: Optional[np.ndarray] = None  # B_u of x[t] ~ MvNormal(μ = A*x[t-1] + B_u*u[t], Σ = P), u a data variable
    noise_precision_prior: Any = None          # Wishart(ν, S): y[t] ~ MvNormal(μ = B*x[t], Λ = W), W ~ Wishart(ν, S), q(x, W) = q(x)q(W); Q is unused


def linear_gaussian_ssm(A, B, P, Q, prior_mean, prior_cov, prior_through_transition=False, state_offset=None, obs_offset=None,
                        input_matrix=None, noise_precision_prior=None):
    """`state_offset` / `obs_offset`: known inputs added to the means (`A * x[t-1] + c`, `B * x[t] + d`), one vector or one
    per time index.  `input_matrix` = B_u: the inputs are DATA, `infer(..., data = {"y": …, "u": …})` with u [T][du] per chain.
    `noise_precision_prior = Wishart(ν, S)` (Q = None): the observation noise is UNKNOWN, `y[t] ~ MvNormal(μ = B * x[t], Λ = W)` with
    `W ~ Wishart(ν, S)` and `@constraints q(x, W) = q(x)q(W)` — `infer(..., iterations = n, initialization = {"W": Wishart(ν, V)})` runs mean-field
    VMP on the device (d, dy ≤ 4) and returns posteriors["W"] next to posteriors["x"]."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    g = lambda a: None if a is None else f(a)
    if noise_precision_prior is not None:
        if Q is not None or state_offset is not None or obs_offset is not None or input_matrix is not None:
            raise ValueError("an unknown observation precision takes Q = None and no offsets / inputs")
        Q = np.eye(np.asarray(B).shape[0])
    return LinearGaussianSSM(f(A), f(B), f(P), f(Q), f(prior_mean), f(prior_cov), bool(prior_through_transition),
                             state_offset=g(state_offset), obs_offset=g(obs_offset), input_matrix=g(input_matrix),
                             noise_precision_prior=noise_precision_prior)


def time_varying_gaussian_ssm(A, B, P, Q, prior_mean, prior_cov, prior_through_transition=False):
    """The state-space model with per-step constants, as written in a @model loop over arrays of matrices:
        x[t] ~ MvNormal(μ = A[t] * x[t-1], Σ = P[t]);  y[t] ~ MvNormal(μ = B[t] * x[t], Σ = Q[t]).
    Any of A, B, P, Q may carry a leading time axis [T, …] (the others are held constant); equal steps share one model."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    A, B, P, Q = f(A), f(B), f(P), f(Q)
    lens = {a.shape[0] for a in (A, B, P, Q) if a.ndim == 3}
    if len(lens) != 1:
        raise ValueError("time-varying constants: give at least one of A, B, P, Q as [T, …], all with the same T")
    T = lens.pop()
    full = [a if a.ndim == 3 else np.broadcast_to(a, (T,) + a.shape) for a in (A, B, P, Q)]
    keys = np.concatenate([a.reshape(T, -1) for a in full], axis=1)
    _, first, step_model = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    A, B, P, Q = (np.ascontiguousarray(a[first]) for a in full)
    return LinearGaussianSSM(A, B, P, Q, f(prior_mean), f(prior_cov), bool(prior_through_transition),
                             np.ascontiguousarray(step_model.ravel(), dtype=np.int32))


@dataclass
class NormalMeanVariance:
    mean: np.ndarray
    var: np.ndarray


@dataclass
class GammaShapeRate:
    shape: np.ndarray
    rate: np.ndarray


@dataclass
class GammaShapeScale:
    """ExponentialFamily.GammaShapeScale (= Distributions.Gamma(α, θ)); `.rate` is 1/θ"""
    shape: np.ndarray
    scale: np.ndarray

    @property
    def rate(self):
        return 1.0 / np.asarray(self.scale, dtype=np.float64)


@dataclass
class Dirichlet:
    alpha: np.ndarray


@dataclass
class UnivariateGaussianMixture:
    """`s ~ Dirichlet(alpha0); m[k] ~ Normal(mean, variance); p[k] ~ Gamma(shape, rate); z[i] ~ Categorical(s);
    y[i] ~ NormalMixture(switch = z[i], m = m, p = p)` with MeanField() constraints
    (test/models/mixtures/gmm_univariate_tests.jl:7-26).  K = 1: the iid Gaussian with unknown mean and precision
    (test/models/models_tests.jl:114-128)."""
    prior_mean: np.ndarray
    prior_var: np.ndarray
    prior_shape: np.ndarray
    prior_rate: np.ndarray
    prior_alpha: np.ndarray


def gaussian_mixture(prior_mean, prior_var, prior_shape, prior_rate, prior_alpha=None):
    f = lambda a: np.atleast_1d(np.asarray(a, dtype=np.float64))
    pm = f(prior_mean)
    return UnivariateGaussianMixture(pm, f(prior_var), f(prior_shape), f(prior_rate),
                                     np.ones_like(pm) if prior_alpha is None else f(prior_alpha))


def iid_normal_gamma(mean, variance, shape, rate=None, *, scale=None):
    """`μ ~ Normal(mean, variance); τ ~ Gamma(shape, rate); y[i] ~ Normal(mean = μ, precision = τ)`; `scale = θ` is the
    `Gamma(shape = …, scale = …)` spelling of test/models/models_tests.jl:121-127 (rate = 1/θ)."""
    if (rate is None) == (scale is None):
        raise ValueError("give exactly one of rate and scale")
    return gaussian_mixture([mean], [variance], [shape], [rate if scale is None else 1.0 / scale], [1.0])


@dataclass
class Wishart:
    """ExponentialFamily.Wishart(ν, S): degrees of freedom and scale matrix (arrays over components allowed)"""
    nu: Any
    S: Any


@dataclass
class MultivariateGaussianMixture:
    """test/models/mixtures/gmm_multivariate_tests.jl:6-32: m[k] ~ MvNormal(mean, cov), w[k] ~ Wishart(ν, V), s ~ Dirichlet"""
    prior_mean: np.ndarray   # [K][d]
    prior_cov: np.ndarray    # [K][d][d]
    prior_nu: np.ndarray     # [K]
    prior_scale: np.ndarray  # [K][d][d]
    prior_alpha: np.ndarray  # [K]


def multivariate_gaussian_mixture(prior_mean, prior_cov, prior_nu, prior_scale, prior_alpha=None):
    """Model spec of the multivariate Gaussian mixture for `infer`: d = 1…4 (K ≤ 16 at d ≤ 2, K ≤ 8 at d = 3, 4) or d = 5…32 with K ≤ 16."""
    m = np.asarray(prior_mean, dtype=np.float64)
    K = m.shape[0]
    return MultivariateGaussianMixture(m, np.asarray(prior_cov, dtype=np.float64), np.asarray(prior_nu, dtype=np.float64),
                                       np.asarray(prior_scale, dtype=np.float64),
                                       np.ones(K) if prior_alpha is None else np.asarray(prior_alpha, dtype=np.float64))


@dataclass
class HierarchicalGaussianFilter:
    """One-step HGF graph streamed over the observations with posterior→prior autoupdates
    (test/models/statespace/hgf_tests.jl:9-70)."""
    kappa: float
    omega: float
    z_variance: float
    y_variance: float
    n_gh: int = 31


def hierarchical_gaussian_filter(kappa, omega, z_variance, y_variance, n_gh=31):
    return HierarchicalGaussianFilter(float(kappa), float(omega), float(z_variance), float(y_variance), int(n_gh))


@dataclass
class UnivariateDriftChain:
    """`x_prior ~ Normal(μ = mean(x0), v = var(x0)); x[i] ~ x_prev + c; y[i] ~ Normal(μ = x[i], v = P)`
    (test/models/statespace/ulgssm_tests.jl:8-15): noise-free transitions through `typeof(+)` nodes."""
    prior_mean: float
    prior_var: float
    c: float
    obs_var: float
    prior_through_transition: bool = True


def univariate_drift_chain(prior_mean, prior_var, c, obs_var, prior_through_transition=True):
    return UnivariateDriftChain(float(prior_mean), float(prior_var), float(c), float(obs_var), bool(prior_through_transition))


def _guarded(model, kw, body):
    """The second half of every per-family function.  `body(own)` constructs its engines as `own(Engine(...))`, which closes them on every way
    out; what the body raises propagates, or with `catch_exception` comes back as the result's `error` (src/inference/batch.jl:440-446).  What a
    family raises BEFORE it calls this (unknown options, shapes, a missing `initialization`) propagates always."""
    owned = []

    def own(eng):
        owned.append(eng)
        return eng

    try:
        return body(own)
    except Exception as err:
        if not kw.catch_exception:
            raise
        return InferenceResult({}, None, None, model, err)
    finally:
        for eng in owned:
            eng.close()


def _iterations(kw):
    return 1 if kw.iterations is None else int(kw.iterations)


def _infer_drift_chain(model, data, kw):
    """posteriors["x"] = NormalMeanVariance with mean / var [T] (or [chain][T]); free_energy one value per iteration."""
    options = _check_options(kw.options)
    y = np.asarray(data["y"], dtype=np.float64)
    single = y.ndim == 1
    if single:
        y = y[None]
    C, T = y.shape
    iters, free_energy = _iterations(kw), kw.free_energy

    def body(own):
        eng = own(DriftChainEngine(T, model.prior_mean, model.prior_var, model.c, model.obs_var, n_chains=C,
                                   prior_through_transition=model.prior_through_transition, device=int(options.get("device", -1))))
        eng.set_data(y[..., None], layout="chain_time")
        eng.run(iterations=iters, free_energy=free_energy)
        mean, var = eng.marginals(layout="chain_time")
        mean, var = mean[..., 0], var[..., 0, 0]
        fe = np.repeat(eng.free_energy_per_chain()[:, None], iters, axis=1) if free_energy else None
        if single:
            mean, var = mean[0], var[0]
            fe = fe[0] if fe is not None else None
        return InferenceResult({"x": NormalMeanVariance(mean, var)}, None, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class ProbitSSM:
    """`x[1] ~ Normal(prior_mean, prior_var); x[k] ~ Normal(a x[k-1] + c, q); y[k-1] ~ Probit(x[k])`
    (test/models/statespace/probit_tests.jl:11-18): a scalar Gaussian chain with binary observations, inferred by EP."""
    a: float
    c: float
    q: float
    prior_mean: float
    prior_var: float
    n_gh: int = 32


def probit_ssm(a, c, q, prior_mean, prior_var, n_gh=32):
    return ProbitSSM(float(a), float(c), float(q), float(prior_mean), float(prior_var), int(n_gh))


def _infer_probit(model, data, kw):
    """y: [T] or [T][series], entries 0, 1 or NaN (missing).  posteriors["x"] = NormalMeanVariance with mean / var [T+1] (or [T+1][series]);
    free_energy: one value per parallel-EP iteration (summed over the series of a batch)."""
    options = _check_options(kw.options)
    y = np.asarray(data["y"], dtype=np.float64)
    single = y.ndim == 1
    if single:
        y = y[:, None]
    T, C = y.shape
    iters, free_energy = _iterations(kw), kw.free_energy

    def body(own):
        eng = own(ProbitEngine(T, model.a, model.c, model.q, model.prior_mean, model.prior_var, n_series=C, n_gh=model.n_gh,
                               device=int(options.get("device", -1))))
        eng.set_data(y, layout="time_chain")
        eng.run(iterations=iters, free_energy=free_energy)
        mean, var = eng.marginals(layout="time_chain")
        fe = eng.free_energy() if free_energy else None
        if single:
            mean, var = mean[:, 0], var[:, 0]
        return InferenceResult({"x": NormalMeanVariance(mean, var)}, None, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class HiddenMarkovModel:
    """`A ~ DirichletCollection(prior_A); B ~ DirichletCollection(prior_B); s_0 ~ Categorical(prior_s0); s[t] ~ DiscreteTransition(s[t-1], A);
    x[t] ~ DiscreteTransition(s[t], B)` with `q(s, s_0, A, B) = q(s, s_0)q(A)q(B)` (test/models/statespace/hmm_tests.jl:8-24)."""
    prior_A: np.ndarray
    prior_B: np.ndarray
    prior_s0: np.ndarray
    init_A: Optional[np.ndarray] = None
    init_B: Optional[np.ndarray] = None
    share_parameters: bool = False


def hidden_markov_model(prior_A, prior_B, prior_s0, init_A=None, init_B=None, share_parameters=False):
    f = lambda v: None if v is None else np.asarray(v, dtype=np.float64)
    return HiddenMarkovModel(f(prior_A), f(prior_B), f(prior_s0), f(init_A), f(init_B), bool(share_parameters))


def one_hot_to_codes(vectors):
    """The reference's HMM data are one-hot vectors (hmm_tests.jl:47-52): [..., M] -> symbol codes [...]; a vector that is not one-hot becomes
    NaN (missing)."""
    v = np.asarray(vectors, dtype=np.float64)
    ok = (np.sum(v == 1.0, axis=-1) == 1) & (np.sum(v != 0.0, axis=-1) == 1)
    return np.where(ok, np.argmax(v, axis=-1).astype(np.float64), np.nan)


def _infer_hmm(model, data, kw):
    """x: integer symbol codes [T] or [T][series] (floats with NaN = missing are taken as they are).  posteriors["s"]: probabilities
    [T+1][K] (or [T+1][series][K]); posteriors["A"], ["B"]: Dirichlet counts [K][K], [M][K] (a leading series axis for an unshared batch);
    free_energy: one value per iteration (summed over the series of a batch)."""
    options = _check_options(kw.options)
    x = np.asarray(data["x"], dtype=np.float64)
    single = x.ndim == 1
    if single:
        x = x[:, None]
    T, C = x.shape
    iters, free_energy = _iterations(kw), kw.free_energy

    def body(own):
        eng = own(HMMEngine(T, model.prior_A, model.prior_B, model.prior_s0, model.init_A, model.init_B, n_series=C,
                            share_parameters=model.share_parameters, device=int(options.get("device", -1))))
        eng.set_data(x, layout="time_chain")
        eng.run(iterations=iters, free_energy=free_energy)
        s = eng.states(layout="time_chain")
        a, b = eng.parameters()
        fe = eng.free_energy() if free_energy else None
        if single:
            s = s[:, 0]
        if single or model.share_parameters:
            a, b = a[0], b[0]
        return InferenceResult({"s": s, "A": a, "B": b}, None, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class LatentAutoregressive:
    """`γ ~ Gamma(a0, b0); θ ~ MvNormal(mθ0, Wθ0⁻¹); x0 ~ MvNormal(m0, W0⁻¹); x[t] ~ AR(x[t-1], θ, γ); y[t] ~ Normal(dot(c, x[t]), τ⁻¹)` with
    c = e₁ and `q(x, x0, θ, γ) = q(x, x0)q(θ)q(γ)` (test/models/autoregressive/lar_tests.jl:51-76); order 1 is the Univariate spelling."""
    order: int
    tau: float
    prior_theta: Optional[tuple] = None
    prior_gamma: tuple = (1.0, 1.0)
    prior_x0: Optional[tuple] = None
    init_theta: Optional[tuple] = None
    init_gamma: Optional[tuple] = None
    share_parameters: bool = False


def latent_autoregressive(order, tau, prior_theta=None, prior_gamma=(1, 1), prior_x0=None, init_theta=None, init_gamma=None, share_parameters=False):
    """prior_theta, prior_x0: (mean [p], precision [p][p]) or None = zero mean and identity precision; prior_gamma: (shape, rate);
    init_theta: (mean [p], covariance [p][p]), init_gamma: (shape, rate), None = the prior's own values (the reference's initialisation)."""
    f = lambda v: None if v is None else (np.asarray(v[0], dtype=np.float64), np.asarray(v[1], dtype=np.float64))
    g = lambda v: None if v is None else (float(v[0]), float(v[1]))
    return LatentAutoregressive(int(order), float(tau), f(prior_theta), g(prior_gamma), f(prior_x0), f(init_theta), g(init_gamma), bool(share_parameters))


def _infer_lar(model, data, kw):
    """y: [T] or [T][series], NaN = missing.  posteriors["x"]: (mean [T][p], cov [T][p][p]) of the last iteration (a series axis after T for a
    batch); posteriors["theta"]: (mean [iterations][p], cov [iterations][p][p]) and posteriors["gamma"]: (shape [iterations], rate [iterations])
    per iteration (a series axis after the iterations for an unshared batch); free_energy: one value per iteration (summed over the series)."""
    options = _check_options(kw.options)
    y = np.asarray(data["y"], dtype=np.float64)
    single = y.ndim == 1
    if single:
        y = y[:, None]
    T, C = y.shape
    iters, free_energy = _iterations(kw), kw.free_energy

    def body(own):
        eng = own(LAREngine(T, model.order, model.tau, model.prior_theta, model.prior_gamma, model.prior_x0, model.init_theta, model.init_gamma,
                            n_series=C, share_parameters=model.share_parameters, device=int(options.get("device", -1))))
        eng.set_data(y, layout="time_chain")
        eng.run(iterations=iters, free_energy=free_energy)
        xm, xc = eng.states(layout="time_chain")
        tm, tc, ga, gb = eng.parameters()
        fe = eng.free_energy() if free_energy else None
        if single:
            xm, xc = xm[:, 0], xc[:, 0]
        if single or model.share_parameters:
            tm, tc, ga, gb = tm[:, 0], tc[:, 0], ga[:, 0], gb[:, 0]
        return InferenceResult({"x": (xm, xc), "theta": (tm, tc), "gamma": (ga, gb)}, None, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class BinomialRegression:
    """`β ~ MvNormalWeightedMeanPrecision(ξ0, W0); y[i] ~ BinomialPolya(X[i], n_trials[i], β)` with `q(β, ω) = q(β)Πq(ω_i)`
    (test/models/regression/binomialreg_tests.jl)."""
    prior_xi: np.ndarray
    prior_precision: np.ndarray
    init: Optional[tuple] = None


def binomial_regression(prior_xi, prior_precision, init=None):
    """prior_xi [d], prior_precision [d][d]: the weighted mean ξ0 and precision W0 of β's prior; init: (mean [d], covariance [d][d]) of the
    initial q(β), None = the prior's own W0⁻¹ξ0, W0⁻¹ (the reference's `RequireMessageFunctionalDependencies(β = prior)`)."""
    f = lambda v: None if v is None else (np.asarray(v[0], dtype=np.float64), np.asarray(v[1], dtype=np.float64))
    return BinomialRegression(np.asarray(prior_xi, dtype=np.float64), np.asarray(prior_precision, dtype=np.float64), f(init))


def _infer_binreg(model, data, kw):
    """X: [N][d] or [problems][N][d]; y, n_trials: [N] or [problems][N], a NaN y = missing.  posteriors["β"]: (mean [iterations][d], cov
    [iterations][d][d]) after every iteration (a problem axis after the iterations for a batch); free_energy: one value per iteration, per
    problem ([iterations][problems]) for a batch."""
    options = _check_options(kw.options)
    X = np.asarray(data["X"], dtype=np.float64)
    single = X.ndim == 2
    if single:
        X = X[None]
    y = np.asarray(data["y"], dtype=np.float64).reshape(X.shape[:2])
    n = np.asarray(data["n_trials"], dtype=np.float64).reshape(X.shape[:2])
    C, N, d = X.shape
    iters = _iterations(kw)

    def body(own):
        eng = own(BinomialRegressionEngine(N, d, model.prior_xi, model.prior_precision, model.init, n_problems=C, device=int(options.get("device", -1))))
        eng.set_data(X, y, n)
        eng.run(iterations=iters, free_energy=kw.free_energy)
        mean, cov, fe = eng.parameters()
        if single:
            mean, cov, fe = mean[:, 0], cov[:, 0], (fe[:, 0] if fe is not None else None)
        return InferenceResult({"β": (mean, cov)}, None, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class MultinomialRegression:
    """`ψ ~ MvNormalWeightedMeanPrecision(ξ0, W0); y[i] ~ MultinomialPolya(N, ψ)` with `q(ψ, ω) = q(ψ)Πq(ω_ik)`
    (test/models/regression/multinomialreg_tests.jl)."""
    prior_xi: np.ndarray
    prior_precision: np.ndarray
    n_trials: Optional[int] = None
    init: Optional[tuple] = None


def multinomial_regression(prior_xi, prior_precision, n_trials=None, init=None):
    """prior_xi [K − 1], prior_precision [K − 1][K − 1]: the weighted mean ξ0 and precision W0 of ψ's prior; n_trials: the N every observed count
    vector must sum to (None: not checked); init: (mean, covariance) of the initial q(ψ) of an offline run, None = the prior's own W0⁻¹ξ0, W0⁻¹.
    Online (`autoupdates`), the prior is the initial q(ψ) in weighted-mean / precision form."""
    f = lambda v: None if v is None else (np.asarray(v[0], dtype=np.float64), np.asarray(v[1], dtype=np.float64))
    return MultinomialRegression(np.asarray(prior_xi, dtype=np.float64), np.asarray(prior_precision, dtype=np.float64),
                                 None if n_trials is None else int(n_trials), f(init))


def logistic_stick_breaking(m):
    """The K probabilities of the stick-breaking map of ψ = m [K − 1]: p_k = σ(m_k)·(1 − Σ_{j<k} p_j), p_K = the remainder
    (logistic_stic_breaking of the reference's test/utiltests.jl)."""
    m = np.asarray(m, dtype=np.float64)
    s = 1.0 / (1.0 + np.exp(-m))
    rest = np.concatenate(([1.0], np.cumprod(1.0 - s)))
    return np.concatenate((s * rest[:-1], rest[-1:]))


def _infer_mnreg(model, data, kw):
    """Y: [N][K] or [problems][N][K] counts, a row with any NaN = missing.  Offline: posteriors["ψ"]: (mean [iterations][d], cov
    [iterations][d][d]) after every iteration (a problem axis after the iterations for a batch), free_energy [iterations] (per problem for a batch).
    With `autoupdates` the rows are streamed (`ξ_ψ, W_ψ = weightedmean_precision(q(ψ))`), `iterations` per row: history["ψ"] = (mean [T][d], var
    [T][d]), posteriors["ψ"] = the last step's (mean, cov), free_energy [T] = F_t; "ψ_cov" in historyvars adds history["ψ_cov"] [T][d][d]."""
    options = _check_options(kw.options)
    Y = np.asarray(data["y"], dtype=np.float64)
    single = Y.ndim == 2
    if single:
        Y = Y[None]
    C, N, K = Y.shape
    iters = _iterations(kw)
    online = bool(kw.autoupdates)
    if online and kw.keephistory not in (None, N):
        raise ValueError(f"multinomial regression: the streamed run keeps every step, keephistory must be {N}")
    keep_cov = online and kw.historyvars is not None and "ψ_cov" in kw.historyvars

    def body(own):
        eng = own(MultinomialRegressionEngine(N, K, model.prior_xi, model.prior_precision, n_trials=model.n_trials, init=None if online else model.init,
                                              n_problems=C, online=online, keep_cov_history=keep_cov, device=int(options.get("device", -1))))
        eng.set_data(Y)
        eng.run(iterations=iters, free_energy=kw.free_energy)
        mean, cov, fe = eng.parameters()
        if not online:
            if single:
                mean, cov, fe = mean[:, 0], cov[:, 0], (fe[:, 0] if fe is not None else None)
            return InferenceResult({"ψ": (mean, cov)}, None, fe, model, None)
        hm, hv, hc, hf = eng.history()
        if single:
            mean, cov, hm, hv, hc, hf = mean[0], cov[0], hm[:, 0], hv[:, 0], (hc[:, 0] if hc is not None else None), (hf[:, 0] if hf is not None else None)
        hist = {"ψ": (hm, hv)}
        if hc is not None:
            hist["ψ_cov"] = hc
        return InferenceResult({"ψ": (mean, cov)}, None, hf, model, None, history=hist, free_energy_history=hf)

    return _guarded(model, kw, body)


@dataclass
class GaussianRegression:
    """`γ ~ Gamma(a0, b0); θ ~ MvNormal(m0, Λ0⁻¹); y[i] ~ Normal(dot(x[i], θ), γ⁻¹)` with `q(γ, θ) = q(γ)q(θ)` (test/models/autoregressive/
    ar_tests.jl:17-46).  order is not None: the regressors are the `order` previous values of the series itself, most recent first (ar_ssm_data)."""
    order: Optional[int]
    prior_theta: Optional[tuple] = None
    prior_gamma: tuple = (1.0, 1.0)
    init_gamma: Optional[tuple] = None
    share_parameters: bool = False


def autoregression(order, prior_theta=None, prior_gamma=(1, 1), init_gamma=None, share_parameters=False):
    """AR(order) with observed regressors: `data={"y": series}`, [T] or [T][series]; row t has y = z_t and x = (z_{t−1} … z_{t−order}).
    prior_theta: (mean [p], precision [p][p]) or None = zero mean and identity precision; prior_gamma, init_gamma: (shape, rate), init None = the
    prior's (the reference initialises q(γ) = GammaShapeRate(1, 1), its prior)."""
    f = lambda v: None if v is None else (np.asarray(v[0], dtype=np.float64), np.asarray(v[1], dtype=np.float64))
    g = lambda v: None if v is None else (float(v[0]), float(v[1]))
    return GaussianRegression(int(order), f(prior_theta), g(prior_gamma), g(init_gamma), bool(share_parameters))


def gaussian_regression(prior_mean, prior_precision, prior_gamma=(1, 1), init_gamma=None, share_parameters=False):
    """Linear regression with unknown coefficients and noise precision: `data={"x": X, "y": y}`, X [N][d] or [series][N][d], y [N] or [series][N]
    (a NaN y drops the row)."""
    g = lambda v: None if v is None else (float(v[0]), float(v[1]))
    return GaussianRegression(None, (np.asarray(prior_mean, dtype=np.float64), np.asarray(prior_precision, dtype=np.float64)), g(prior_gamma), g(init_gamma),
                              bool(share_parameters))


def _infer_arreg(model, data, kw):
    """posteriors["θ"]: (mean [iterations][d], cov [iterations][d][d]) and posteriors["γ"]: (shape [iterations], rate [iterations]) after every
    iteration (KeepEach; a series axis after the iterations for an unshared batch); free_energy: one value per iteration (summed over the series)."""
    options = _check_options(kw.options)
    dev = int(options.get("device", -1))
    iters = _iterations(kw)

    def body(own):
        if model.order is not None:
            y = np.asarray(data["y"], dtype=np.float64)
            single = y.ndim == 1
            if single:
                y = y[:, None]
            T, C = y.shape
            eng = own(ARRegressionEngine(T, model.order, model.prior_theta, model.prior_gamma, model.init_gamma, n_series=C, lagged=True,
                                         share_parameters=model.share_parameters, device=dev))
            eng.set_data(y, layout="time_chain")
        else:
            X = np.asarray(data["x"], dtype=np.float64)
            single = X.ndim == 2
            if single:
                X = X[None]
            C, N, d = X.shape
            y = np.asarray(data["y"], dtype=np.float64).reshape(C, N)
            eng = own(ARRegressionEngine(N, d, model.prior_theta, model.prior_gamma, model.init_gamma, n_series=C, share_parameters=model.share_parameters,
                                         device=dev))
            eng.set_regressors(X)
            eng.set_observations(y)
        eng.run(iterations=iters, free_energy=kw.free_energy)
        tm, tc, ga, gb, _ = eng.parameters()
        fe = eng.free_energy() if kw.free_energy else None
        if single or model.share_parameters:
            tm, tc, ga, gb = tm[:, 0], tc[:, 0], ga[:, 0], gb[:, 0]
        return InferenceResult({"θ": (tm, tc), "γ": (ga, gb)}, None, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class GammaMixture:
    """`s ~ Dirichlet(α⁰); a[k] ~ Gamma(c⁰_k, d⁰_k); b[k] ~ Gamma(e⁰_k, f⁰_k); z[i] ~ Categorical(s); y[i] ~ GammaMixture(switch = z[i], a = a, b = b)`
    with `q = q(s) Π q(z_i) Π q(b_k) Π δ(a_k − â_k)` (test/models/mixtures/gamma_mixture_tests.jl:7-40).  Arrays are [K] or [problems][K]."""
    prior_a: tuple
    prior_b: tuple
    prior_alpha: np.ndarray
    init_a: Optional[np.ndarray] = None
    init_b: Optional[tuple] = None
    init_s: Optional[np.ndarray] = None


def _gamma_pairs(v, name):
    """a GammaShapeRate / GammaShapeScale, a sequence of them, or a sequence of (shape, rate) pairs -> (shape [K], rate [K])"""
    if isinstance(v, (GammaShapeRate, GammaShapeScale)):
        return np.atleast_1d(np.asarray(v.shape, dtype=np.float64)), np.atleast_1d(np.asarray(v.rate, dtype=np.float64))
    items = list(v)
    if items and all(isinstance(q, (GammaShapeRate, GammaShapeScale)) or np.ndim(q) == 1 for q in items):   # one entry per component
        pair = lambda q: (float(q.shape), float(np.asarray(q.rate))) if isinstance(q, (GammaShapeRate, GammaShapeScale)) else (float(q[0]), float(q[1]))
        if any(not isinstance(q, (GammaShapeRate, GammaShapeScale)) and len(q) != 2 for q in items):
            raise ValueError(f"{name} must be a sequence of GammaShapeRate / GammaShapeScale or of (shape, rate) pairs")
        a = np.array([pair(q) for q in items], dtype=np.float64)
    else:
        a = np.asarray(items, dtype=np.float64)
    if a.ndim < 2 or a.shape[-1] != 2:
        raise ValueError(f"{name} must be a sequence of GammaShapeRate / GammaShapeScale or of (shape, rate) pairs")
    return np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(a[..., 1])


def gamma_mixture(prior_a, prior_b, prior_alpha, init_a=None, init_b=None, init_s=None):
    """Gamma mixture with a point-mass shape: `data={"y": y}`, y [N] or [problems][N] (NaN = a missing point).  prior_a, prior_b (and init_b): sequences of
    GammaShapeRate / GammaShapeScale or of (shape, rate) pairs, one per component; prior_alpha (and init_s): a Dirichlet or an array; init_a: the
    starting shapes (default 1.0, the reference test's starting_point); init_b default GammaShapeRate(1, 1); init_s default the prior."""
    al = lambda v: None if v is None else np.asarray(v.alpha if isinstance(v, Dirichlet) else v, dtype=np.float64)
    return GammaMixture(_gamma_pairs(prior_a, "prior_a"), _gamma_pairs(prior_b, "prior_b"), al(prior_alpha),
                        None if init_a is None else np.asarray(init_a, dtype=np.float64), None if init_b is None else _gamma_pairs(init_b, "init_b"), al(init_s))


def _infer_gammamix(model, data, kw):
    """posteriors["as"]: the point masses â [iterations][K]; ["bs"]: (shape, rate), each [iterations][K] (KeepEach; a problem axis after the iterations for
    a batch); ["s"]: the last α [K]; ["z"]: the last q(z) [N][K]; free_energy: one value per iteration (summed over the problems)."""
    options = _check_options(kw.options)
    dev = int(options.get("device", -1))
    iters = _iterations(kw)

    def body(own):
        y = np.asarray(data["y"], dtype=np.float64)
        single = y.ndim == 1
        if single:
            y = y[None]
        C, N = y.shape
        K = int(np.asarray(model.prior_alpha).shape[-1])
        eng = own(GammaMixtureEngine(N, K, model.prior_a, model.prior_b, model.prior_alpha, model.init_a, model.init_b, model.init_s, n_problems=C,
                                     materialize=True, device=dev))
        eng.set_data(y, layout="chain_time")
        eng.run(iterations=iters, free_energy=kw.free_energy)
        h = eng.history()
        fe = eng.free_energy() if kw.free_energy else None
        a, bs, br, alpha, z = h["a"], h["b_shape"], h["b_rate"], h["alpha"][-1], eng.responsibilities()
        if single:
            a, bs, br, alpha, z = a[:, 0], bs[:, 0], br[:, 0], alpha[0], z[0]
        return InferenceResult({"as": a, "bs": (bs, br), "s": alpha, "z": z}, None, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class InferenceResult:
    """src/inference/batch.jl:18-24"""
    posteriors: dict
    predictions: Optional[dict]
    free_energy: Optional[np.ndarray]
    model: Any
    error: Optional[BaseException] = None
    # streaming runs (src/inference/streaming.jl:18-30): history of the `historyvars`, free_energy_history
    history: Optional[dict] = None
    free_energy_history: Optional[np.ndarray] = None


_OPTION_KEYS = {"limit_stack_depth", "warn", "device", "segments", "backend", "materialize_z"}


def _check_options(options):
    options = dict(options or {})
    unknown = set(options) - _OPTION_KEYS
    if unknown:
        raise ValueError(f"Unknown option keys {sorted(unknown)}; available: {sorted(_OPTION_KEYS)}")
    return options


def _infer_mixture(model, data, kw):
    """posteriors (KeepEach, one entry per iteration as `returnvars = KeepEach()`): m -> NormalMeanVariance [it][K],
    p -> GammaShapeRate [it][K], s -> Dirichlet [it][K]; z (last iteration) if options['materialize_z'].
    Only the fixed point is pinned to the reference: the update order inside an iteration is an assumption, so per-iteration
    entries are drop-in for RxInfer's `KeepEach` results up to that order (include/rxhip.h)."""
    options, initialization = _check_options(kw.options), kw.initialization
    if initialization is None:
        raise ValueError("mean-field VMP needs `initialization` (q(m), q(p), q(s)); cf. test/inference/inference_tests.jl:361-363")
    y = np.asarray(data["y"], dtype=np.float64).ravel()
    iters = _iterations(kw)
    K = model.prior_mean.size
    qm, qp = initialization["m"], initialization["p"]
    qs = initialization.get("s", Dirichlet(np.ones(K)))

    def body(own):
        eng = own(GMMEngine(y.size, model.prior_mean, model.prior_var, model.prior_shape, model.prior_rate, model.prior_alpha,
                            qm.mean, qm.var, qp.shape, qp.rate, qs.alpha,
                            materialize_responsibilities=bool(options.get("materialize_z", False)), device=int(options.get("device", -1))))
        eng.set_data(y)
        eng.run(iters, kw.free_energy)
        h = eng.history()
        post = {"m": NormalMeanVariance(h[:, 0], h[:, 1]), "p": GammaShapeRate(h[:, 2], h[:, 3]), "s": Dirichlet(h[:, 4])}
        if options.get("materialize_z", False):
            post["z"] = eng.responsibilities()
        return InferenceResult(post, None, eng.free_energy() if kw.free_energy else None, model, None)

    return _guarded(model, kw, body)


def _infer_mv_mixture(model, data, kw):
    """posteriors (KeepEach): m -> MvNormalMeanCovariance [it][K], w -> Wishart [it][K], s -> Dirichlet [it][K];
    z (last iteration) if options['materialize_z'].  initialization = {"m": MvNormalMeanCovariance, "w": Wishart, "s": Dirichlet}."""
    options, initialization = _check_options(kw.options), kw.initialization
    if initialization is None or "m" not in initialization or "w" not in initialization:
        raise ValueError("mean-field VMP needs `initialization` (q(m), q(w)[, q(s)]); cf. test/models/mixtures/gmm_multivariate_tests.jl:66-70")
    y = np.asarray(data["y"], dtype=np.float64)
    iters = _iterations(kw)
    K = model.prior_mean.shape[0]
    qm, qw = initialization["m"], initialization["w"]
    qs = initialization.get("s", Dirichlet(np.ones(K)))

    def body(own):
        eng = own(MvGMMEngine(y.shape[0], model.prior_mean, model.prior_cov, model.prior_nu, model.prior_scale, model.prior_alpha,
                              qm.mean, qm.cov, np.broadcast_to(np.asarray(qw.nu, dtype=np.float64), (K,)).copy(), qw.S, qs.alpha,
                              materialize_responsibilities=bool(options.get("materialize_z", False)), device=int(options.get("device", -1))))
        eng.set_data(y)
        eng.run(iters, kw.free_energy)
        h = eng.history()
        post = {"m": MvNormalMeanCovariance(h["mean"], h["cov"]), "w": Wishart(h["nu"], h["V"]), "s": Dirichlet(h["alpha"])}
        if options.get("materialize_z", False):
            post["z"] = eng.responsibilities()
        return InferenceResult(post, None, eng.free_energy() if kw.free_energy else None, model, None)

    return _guarded(model, kw, body)


def _infer_hgf(model, data, kw):
    """history[:zt], history[:xt] (KeepLast per observation) as NormalMeanVariance [T] (or [series][T]);
    free_energy = free_energy_history: mean over observations per VMP iteration (per series)."""
    options = _check_options(kw.options)
    y = np.asarray(data["y"], dtype=np.float64)
    single = y.ndim == 1
    if single:
        y = y[None]
    S, T = y.shape
    iters = _iterations(kw)
    init = kw.initialization or {}
    z0 = init.get("zt", NormalMeanVariance(0.0, 5.0))
    x0 = init.get("xt", NormalMeanVariance(0.0, 5.0))

    def body(own):
        eng = own(HGFEngine(T, S, model.kappa, model.omega, model.z_variance, model.y_variance, (float(z0.mean), float(z0.var)),
                            (float(x0.mean), float(x0.var)), n_gh=model.n_gh, device=int(options.get("device", -1))))
        eng.set_data(y, layout="chain_time")
        eng.run(iters, kw.free_energy)
        zm, zv, xm, xv = eng.history("chain_time")
        fe = None
        if kw.free_energy:
            fe = eng.free_energy() / S if single else None
            if not single:
                fe = eng.free_energy_per_chain()
        if single:
            zm, zv, xm, xv = zm[0], zv[0], xm[0], xv[0]
        return InferenceResult({"zt": NormalMeanVariance(zm, zv), "xt": NormalMeanVariance(xm, xv)}, None, fe, model, None)

    return _guarded(model, kw, body)


def _infer_lgssm_filtering(model, data, kw):
    """Streaming inference with posterior -> prior feedback (`autoupdates`), the notebook's
    `rxinfer_inference_filtering` (benchmarks notebook cell 7): history["x"] = q(x_t) after every observation
    (`historyvars = (x_t = KeepLast(),)`, `keephistory = T`); free_energy_history = mean over observations of the
    per-observation free energy, one value (iterations = 1) per chain.  `initialization = {"x": MvNormalMeanCovariance}`
    overrides the model's prior as the initial q(x_t)."""
    options, free_energy = _check_options(kw.options), kw.free_energy
    y = np.asarray(data["y"], dtype=np.float64)
    single = y.ndim == 2
    if single:
        y = y[None]
    C, T, dy = y.shape
    m0, V0 = model.prior_mean, model.prior_cov
    if kw.initialization and "x" in kw.initialization:
        m0, V0 = kw.initialization["x"].mean, kw.initialization["x"].cov

    def body(own):
        eng = own(LGSSMEngine(model.A, model.B, model.P, model.Q, m0, V0, T=T, n_chains=C,
                              prior_through_transition=model.prior_through_transition,
                              state_offset=model.state_offset, obs_offset=model.obs_offset,
                              segments=int(options.get("segments", 0)), device=int(options.get("device", -1))))
        if single:   # one series: the whole call in one round trip
            m1, c1, f1 = eng.infer(y[0][:, None, :], free_energy=free_energy, filtering=True)
            mean, cov = np.transpose(m1, (1, 0, 2)), np.transpose(c1, (1, 0, 2, 3))
            fe = f1[:, None] if free_energy else None
        else:
            eng.set_data(y, layout="chain_time")
            eng.run_filter(free_energy=free_energy)
            mean, cov = eng.marginals(layout="chain_time")
            fe = eng.free_energy_per_chain()[:, None] if free_energy else None
        if single:
            mean, cov = mean[0], cov[0]
            fe = fe[0] if fe is not None else None
        return InferenceResult({}, None, None, model, None, history={"x": MvNormalMeanCovariance(mean, cov)},
                               free_energy_history=fe)

    return _guarded(model, kw, body)


def _infer_lgssm_noise(model, data, kw):
    """mean-field VMP of the chain with an unknown observation-noise precision (LGSSMNoiseEngine)"""
    from .engine import LGSSMNoiseEngine
    options, initialization, free_energy = _check_options(kw.options), kw.initialization, kw.free_energy

    def body(own):
        y = np.asarray(data["y"], dtype=np.float64)
        single = y.ndim == 2
        if single:
            y = y[None]
        if np.isnan(y).any():
            raise ValueError("unknown observation precision: missing observations have no device schedule")
        C, T, dy = y.shape
        pri = model.noise_precision_prior
        init = (initialization or {}).get("W")
        if init is None:   # the reference refuses mean-field VMP without an @initialization marginal
            raise ValueError("mean-field VMP needs initialization = {\"W\": Wishart(ν, V)}")
        eng = own(LGSSMNoiseEngine(model.A, model.B, model.P, model.prior_mean, model.prior_cov, T, float(pri.nu), np.asarray(pri.S, float).reshape(dy, dy),
                                   float(init.nu), np.asarray(init.S, float).reshape(dy, dy), n_chains=C,
                                   prior_through_transition=model.prior_through_transition, segments=int(options.get("segments", 0)),
                                   device=int(options.get("device", -1))))
        eng.set_data(y, layout="chain_time")
        eng.run(iterations=_iterations(kw), free_energy=free_energy)
        mean, cov = eng.marginals(layout="chain_time")
        nu, V = eng.noise_posterior()
        fe = None
        if free_energy:
            fe = eng.free_energy()                      # per iteration, summed over the chains (every chain is its own graph)
            if single:
                fe = np.asarray(fe)
        if single:
            mean, cov, nu, V = mean[0], cov[0], nu[0], V[0]
        post = {"x": MvNormalMeanCovariance(mean, cov), "W": Wishart(nu, V)}
        if kw.returnvars is not None:
            post = {k: v for k, v in post.items() if k in kw.returnvars}
        return InferenceResult(post, None, fe, model, None)

    return _guarded(model, kw, body)


def _smooth_on_executor(model, y, iters, free_energy, allow_missing, device):
    """y [chain][T][dy] through the node-array executor on the graph GraphPPL would build for the model (graph.lgssm_graph): mean [chain][T][d], cov, fe [chain][iters] | None"""
    from . import graph
    from .tree import TreeEngine
    C, T, dy = y.shape
    so, oo = model.state_offset, model.obs_offset
    kw = {}
    if so is not None:
        so = np.broadcast_to(np.asarray(so, float), (T, model.A.shape[-1]))
        kw["c_of_t"] = lambda t: so[t]
    if oo is not None:
        oo = np.broadcast_to(np.asarray(oo, float), (T, dy))
        kw["d_of_t"] = lambda t: oo[t]
    gb, xs, ys = graph.lgssm_graph(T, model.A, model.B, model.P, model.Q, model.prior_mean, model.prior_cov,
                                   prior_through_transition=model.prior_through_transition, **kw)[:3]
    with TreeEngine(gb, n_replicas=C, allow_missing=allow_missing, device=device) as te:
        te.set_data(ys, np.ascontiguousarray(y.reshape(C, T * dy)))
        te.run(1, bool(free_energy))
        post = te.marginals(xs)
        fe = np.repeat(te.free_energy_per_replica()[:, None], iters, axis=1) if free_energy else None
    return np.stack([post[v][0] for v in xs], axis=1), np.stack([post[v][1] for v in xs], axis=1), fe


def _infer_lgssm(model, data, kw):
    """The state-space family: unknown observation precision, the filtering twin, else smoothing on the chain engine (see `infer`)."""
    if model.noise_precision_prior is not None:
        if kw.autoupdates or kw.predictvars:
            raise ValueError("unknown observation precision: no streaming twin and no predictions on the device")
        return _infer_lgssm_noise(model, data, kw)
    if kw.autoupdates:
        if kw.iterations not in (None, 1):
            raise ValueError("filtering: the one-step graph is a tree, iterations must be 1")
        return _infer_lgssm_filtering(model, data, kw)
    options = _check_options(kw.options)   # closed key set, as reactivemp_inference.jl:129-143
    if "y" not in data:
        raise ValueError("data must provide `y`")
    y = np.asarray(data["y"], dtype=np.float64)
    single = y.ndim == 2
    if single:
        y = y[None]
    C, T, dy = y.shape
    iters, free_energy, returnvars, predictvars = _iterations(kw), kw.free_energy, kw.returnvars, kw.predictvars
    horizon, allow_missing = 0, False
    nans = np.isnan(y)
    if nans.any():
        if not predictvars:   # data with `missing` values is predicted without being asked (src/inference/batch.jl:221-227)
            predictvars = ("y",)
        # `missing` observations (docs/src/manuals/inference/static.md:98-123).  A tail that no chain observed is a forecast
        # horizon and keeps the time-parallel schedule; anything else runs the per-chain masked schedule.
        missing = np.all(nans, axis=(0, 2))
        while horizon < T - 1 and missing[T - 1 - horizon]:
            horizon += 1
        if nans[:, :T - horizon].any():
            horizon, allow_missing = 0, True
        else:
            y, T = y[:, :T - horizon], T - horizon

    def body(own):
        m0, V0, step_model = model.prior_mean, model.prior_cov, model.step_model
        if step_model is not None:
            if step_model.shape[0] != T + horizon:
                raise ValueError(f"time-varying model has {step_model.shape[0]} steps, the data {T + horizon}")
            M = model.A.shape[0]
            m0, V0 = np.broadcast_to(m0, (M,) + m0.shape[-1:]), np.broadcast_to(V0, (M,) + V0.shape[-2:])
        try:
            eng = own(LGSSMEngine(model.A, model.B, model.P, model.Q, m0, V0, T=T, n_chains=C,
                                  prior_through_transition=model.prior_through_transition, horizon=horizon,
                                  allow_missing=allow_missing, step_model=step_model,
                                  state_offset=(model.state_offset if model.input_matrix is None else np.zeros(model.A.shape[-1])),
                                  obs_offset=model.obs_offset,
                                  segments=int(options.get("segments", 0)), device=int(options.get("device", -1))))
        except RxHipError as err:
            # a model beyond the conditioning envelope of the information-form chain engines (include/rxhip.h rxhip_set_conditioning_guard): the same graph on the
            # node-array executor, as rxhip_create does for a host that hands over the graph — plain smoothing only (the executor has no forecast / prediction entry)
            if err.status != _lib.ERR_UNSUPPORTED or "kappa" not in str(err) or horizon or predictvars or step_model is not None or model.input_matrix is not None:
                raise
            mean, cov, fe = _smooth_on_executor(model, y, iters, free_energy, allow_missing, int(options.get("device", -1)))
            if single:
                mean, cov, fe = mean[0], cov[0], (fe[0] if fe is not None else None)
            post = {"x": MvNormalMeanCovariance(mean, cov)}
            if returnvars is not None:
                post = {k: v for k, v in post.items() if k in returnvars}
            return InferenceResult(post, None, fe, model, None)
        if model.input_matrix is not None:   # control inputs as data: c[t] = B_u u[t] (+ the constant part) for every chain
            if "u" not in data:
                raise ValueError("this model has data inputs: data must provide `u`")
            u = np.asarray(data["u"], dtype=np.float64)
            u = u[None] if single else u
            c = u @ model.input_matrix.T
            if model.state_offset is not None:
                c = c + model.state_offset
            if c.shape[1] != T + horizon:
                raise ValueError(f"`u` has {c.shape[1]} steps, the data {T + horizon}")
            eng.set_chain_offsets(c, None, layout="chain_time")
        fe1 = None
        if single:   # one chain: the whole call in one round trip (rxhip_lgssm_infer)
            m1, c1, fe1 = eng.infer(y[0][:, None, :], iterations=iters, free_energy=free_energy)
            mean, cov = np.transpose(m1, (1, 0, 2)), np.transpose(c1, (1, 0, 2, 3))
        else:
            eng.set_data(y, layout="chain_time")
            eng.run(iterations=iters, free_energy=free_energy)
            mean, cov = eng.marginals(layout="chain_time")
        pred = None
        if predictvars:
            pm, pc = eng.predictions(layout="chain_time")
            pred = {"y": MvNormalMeanCovariance(pm[0], pc[0]) if single else MvNormalMeanCovariance(pm, pc)}
        if free_energy:
            # one value per iteration, per chain-graph: what `infer` returns for each chain
            fe = fe1 if fe1 is not None else eng.free_energy_per_chain()
            fe = np.repeat(fe[:, None], iters, axis=1)
        else:
            fe = None
        if single:
            mean, cov = mean[0], cov[0]
            fe = fe[0] if fe is not None else None
        post = {"x": MvNormalMeanCovariance(mean, cov)}
        if returnvars is not None:
            post = {k: v for k, v in post.items() if k in returnvars}
        return InferenceResult(post, pred, fe, model, None)

    return _guarded(model, kw, body)


@dataclass
class Linearization:
    """The delta node's first-order approximation: m̃ = f(m), Ṽ = J V Jᵀ (ReactiveMP's Linearization())."""


@dataclass
class Unscented:
    """The delta node's unscented transform (ReactiveMP's Unscented()); the defaults are this engine's (include/rxhip.h rxhip_nlssm_desc)."""
    alpha: float = 1e-3
    beta: float = 2.0
    kappa: float = 0.0


@dataclass
class NonlinearSSM:
    """`x[0] ~ MvNormal(prior_mean, prior_cov); x[t] ~ MvNormal(f(x[t-1]), process_cov)` (`x[t] := f(x[t-1])` without process_cov) under
    `Linearization()` or `Unscented()`, observed as `y[t] ~ MvNormal(obs_matrix x[t], obs_cov)` or, with `obs_precision_prior`, as
    `τ ~ Gamma; y[t] ~ Normal(obs_matrix x[t], 1/τ)` with q(x, τ) = q(x)q(τ) (the reference's paper/example.jl)."""
    f: Any
    d: int
    prior_mean: Any
    prior_cov: Any
    process_cov: Any
    obs_matrix: Any
    obs_cov: Any
    obs_precision_prior: Any
    method: Any


def nonlinear_ssm(f, d, prior_mean, prior_cov, process_cov=None, obs_matrix=None, obs_cov=None, obs_precision_prior=None, method=None):
    """`f`: a callable on a list of d values (traced once by rxhip.trace) or a Program.  Exactly one of obs_cov (known noise) and
    obs_precision_prior (GammaShapeRate / GammaShapeScale: unknown noise, scalar observations) is given."""
    from .expr import trace
    d = int(d)
    if obs_matrix is None:
        raise ValueError("nonlinear_ssm: obs_matrix is required")
    if (obs_cov is None) == (obs_precision_prior is None):
        raise ValueError("nonlinear_ssm: give obs_cov (known noise) or obs_precision_prior (unknown noise), not both")
    if obs_precision_prior is not None and not isinstance(obs_precision_prior, (GammaShapeRate, GammaShapeScale)):
        raise TypeError("nonlinear_ssm: obs_precision_prior is a GammaShapeRate or GammaShapeScale")
    method = Linearization() if method is None else method
    if not isinstance(method, (Linearization, Unscented)):
        raise TypeError("nonlinear_ssm: method is rxhip.Linearization() or rxhip.Unscented(alpha, beta, kappa)")
    if isinstance(method, Unscented) and not (method.alpha > 0 and np.isfinite([method.alpha, method.beta, method.kappa]).all()):
        raise ValueError(f"nonlinear_ssm: Unscented needs alpha > 0 and finite alpha, beta, kappa (got alpha = {method.alpha})")
    H = np.atleast_2d(np.asarray(obs_matrix, dtype=np.float64))
    return NonlinearSSM(trace(f, d), d, np.asarray(prior_mean, dtype=np.float64), np.asarray(prior_cov, dtype=np.float64),
                        None if process_cov is None else np.asarray(process_cov, dtype=np.float64).reshape(d, d), H,
                        None if obs_cov is None else np.asarray(obs_cov, dtype=np.float64).reshape(H.shape[0], H.shape[0]), obs_precision_prior, method)


def _infer_nlssm(model, data, kw):
    """y: [T] / [T][dy] for one series, [series][T][dy] for a batch (NaN = missing).  Smoothing (known noise): posteriors["x"] =
    MvNormalMeanCovariance of x[1 … T], free_energy per iteration entry.  With `autoupdates` (filtering): history["x"] the filtered marginals and,
    with unknown noise, history["τ"] = GammaShapeRate after every observation, `iterations` VMP iterations per observation; `keephistory` must be T."""
    options = _check_options(kw.options)
    dy = model.obs_matrix.shape[0]
    y = np.asarray(data["y"], dtype=np.float64)
    if y.ndim == 1:
        y = y[:, None]
    single = y.ndim == 2
    if single:
        y = y[None]
    if y.ndim != 3 or y.shape[2] != dy:
        raise ValueError(f"nonlinear_ssm: y is [T][{dy}] or [series][T][{dy}]")
    C, T = y.shape[:2]
    filtering = bool(kw.autoupdates)
    if filtering and kw.keephistory not in (None, T):
        raise ValueError(f"nonlinear_ssm: the streamed run keeps every step, keephistory must be {T}")
    iters, free_energy = _iterations(kw), kw.free_energy
    m = model.method
    prior = model.obs_precision_prior
    noise = None if prior is None else (float(prior.shape), float(prior.rate))

    def body(own):
        eng = own(NonlinearSSMEngine(model.f, model.d, T, model.prior_mean, model.prior_cov, model.obs_matrix, R=model.obs_cov, Q=model.process_cov,
                                     noise_prior=noise, method="unscented" if isinstance(m, Unscented) else "linearization",
                                     unscented=(m.alpha, m.beta, m.kappa) if isinstance(m, Unscented) else None,
                                     mode="filter" if filtering else "smooth", n_series=C, device=int(options.get("device", -1))))
        eng.set_data(y, layout="chain_time")
        eng.run(iterations=iters, free_energy=free_energy)
        mean, cov = eng.marginals(layout="chain_time")
        fe = eng.free_energy() if free_energy else None
        x = MvNormalMeanCovariance(mean[0], cov[0]) if single else MvNormalMeanCovariance(mean, cov)
        if not filtering:
            return InferenceResult({"x": x}, None, fe, model, None)
        hist = {"x": x}
        if noise is not None:
            shape, rate = eng.noise()
            hist["τ"] = GammaShapeRate(shape[:, 0], rate[:, 0]) if single else GammaShapeRate(shape.T.copy(), rate.T.copy())
        return InferenceResult({}, None, None, model, None, history=hist, free_energy_history=fe)

    return _guarded(model, kw, body)


# model type -> the function that runs it; every one takes (model, data, kw) with kw the keyword arguments of `infer`
_FAMILIES = {UnivariateGaussianMixture: _infer_mixture, MultivariateGaussianMixture: _infer_mv_mixture, HierarchicalGaussianFilter: _infer_hgf,
             UnivariateDriftChain: _infer_drift_chain, ProbitSSM: _infer_probit, HiddenMarkovModel: _infer_hmm, LatentAutoregressive: _infer_lar,
             BinomialRegression: _infer_binreg, GaussianRegression: _infer_arreg, MultinomialRegression: _infer_mnreg, GammaMixture: _infer_gammamix,
             NonlinearSSM: _infer_nlssm, LinearGaussianSSM: _infer_lgssm}


def infer(*, model, data, iterations=None, free_energy=False, options=None, returnvars=None, predictvars=None,
          catch_exception=False, initialization=None, autoupdates=None, keephistory=None, historyvars=None):
    """Static (batch) inference on the device engine; with `autoupdates` (any truthy value: the state-space spec has
    exactly one feedback, `mean_cov(q(x_t))` -> prior of the next step) the streaming / filtering twin.

    data = {"y": array}: [T][dy] for one chain (as `data = (y = observations,)`), or
    [chain][T][dy] for a batch of independent chains sharing the model.
    Returns posteriors["x"] as MvNormalMeanCovariance with mean [T][d] / [chain][T][d].
    `predictvars = ("y",)` (reference: `predictvars = (y = KeepLast(),)`): result.predictions["y"] holds the message toward
    every y[t] — leave-one-out predictive for observed steps.  NaN rows of `y` are `missing` observations: a tail that no
    chain observed is a forecast horizon (posteriors and predictions there are forward predictions, the sweep stays
    time-parallel); `missing` values anywhere else select the masked schedule (any d, dy ≤ 64), where a missing y[t] sends no
    message and its prediction is the smoothed predictive."""
    family = _FAMILIES.get(type(model)) or next((f for cls, f in _FAMILIES.items() if isinstance(model, cls)), None)
    if family is None:
        raise TypeError("infer: no device schedule for this model type")
    return family(model, data, SimpleNamespace(iterations=iterations, free_energy=free_energy, options=options, returnvars=returnvars,
                                               predictvars=predictvars, catch_exception=catch_exception, initialization=initialization,
                                               autoupdates=autoupdates, keephistory=keephistory, historyvars=historyvars))

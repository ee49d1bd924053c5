"""NumPy restatement of the C oracle's multivariate mixture VMP (oracle/rxoracle.c rxo_mvgmm_vmp) at ANY dimension.

The C oracle stops at d = 8; the device engine reaches d = 32.  This module follows the oracle statement by statement — same
schedule (q(z) from the previous marginals; q(s), q(m[k]) with the previous E[W]; q(w[k]) with the new q(m[k])), same algebra
(Σπ, Σπy, Σπyy'), same closed forms of the free energy — with the loops over points and matrix entries written as array
operations.  tests/test_mvgmm_ref_cpu.py pins it to the oracle where both run.

state / init / hist layout per component (rxoracle.mvgmm_pack): mean[d] | cov[d][d] | nu | V[d][d] | alpha.

Also the shared side of the mixture tests: the contract (contract_errors, hold), the inputs (ring_data, setup) and the table of every case the
host and device tests of the three mixture engines run (CASES, case)."""
import collections
import functools

import numpy as np
from scipy.special import digamma, gammaln

import rxoracle

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


# ------------------------------------------------------------------------------------------------------------------------------------------
# The contract of the mixture engines, per (iteration, component).  A component that receives no points keeps its prior S0 = 1e6·I as cov
# while populated ones sit near 0.1, so a norm over the whole history lets a populated component be wrong by any factor; here every
# (iteration, component) is measured against its own scale, taken from the reference.
KEYS = ("mean", "cov", "nu", "V", "alpha")
CONTRACT = dict(mean=1e-6, mean_global=1e-6, cov=1e-6, V=1e-6, nu=1e-6, alpha=1e-6, fe=1e-8, resp=1e-9)
# what a case has to satisfy between two summation orders of the reference before a device test may use it: two decades under the contract
CONDITION = dict(mean=1e-8, mean_global=1e-8, cov=1e-8, V=1e-8, nu=1e-8, alpha=1e-8, fe=1e-10, resp=1e-11)
# The one exception, kept from before the table existed with its offset as it was: the case with 1e4 added to every coordinate
# (tests/test_mvgmm_dense_gpu.py::test_offset_data).  The statistics Σπyy' are raw moments: entries of size offset² = 1e8 cancel down to
# variances of 5 … 30, which costs offset²/variance ≈ 2e7 roundings of the sums, so the reference's own order sensitivity there is 1.6e-8
# (cov), 3.0e-8 (V), 6.5e-9 sd (mean), 7e-11 (free energy) — one decade inside the contract, not two.  It is held to that one decade.
CONDITION_OFFSET = {k: 10.0 * v for k, v in CONDITION.items()}


def rel(a, b):
    """max |a − b| over max |b| of the WHOLE array: the norm the mixture tests used for every key before.  Parity keeps it for the mean only (a
    starved component's posterior sd is 1e3, so the per-component norm does not imply it there); beside that, the teeth test shows what it
    accepted, and the engine-against-engine bound of 1e-12 in tests/test_mvgmm_dense_gpu.py::test_split_phase stays in it"""
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def result(hist, d, fe=None, resp=None):
    """raw history [it][K][SZ] (+ free energy, responsibilities) as the dict contract_errors takes"""
    r = dict(rxoracle.mvgmm_unpack(hist, d))
    r["fe"], r["resp"] = fe, resp
    return r


def _diag(a):
    return np.einsum("...ii->...i", a)


def contract_errors(got, ref, components=None):
    """Largest error per key over (iteration, component[, entry]); got, ref: dicts in the rxoracle.mvgmm_unpack layout, optionally with fe [it] and
    resp [N][K].  mean: |Δm_a| / √cov_aa (posterior standard deviations of that component's mean), mean_global: rel() over the whole history,
    cov and V: |Δ_ab| / √(ref_aa · ref_bb), nu and alpha: relative, fe: relative per iteration, resp: absolute.  `components` restricts the
    posterior keys to those components (fe and resp are not per component)."""
    g, r = ({k: np.asarray(x[k], dtype=np.float64) for k in KEYS} for x in (got, ref))
    if components is not None:
        g, r = ({k: x[k][:, components] for k in KEYS} for x in (g, r))
    e = dict(mean=float(np.max(np.abs(g["mean"] - r["mean"]) / np.sqrt(_diag(r["cov"])))), mean_global=rel(g["mean"], r["mean"]))
    for k in ("cov", "V"):
        dg = _diag(r[k])
        e[k] = float(np.max(np.abs(g[k] - r[k]) / np.sqrt(dg[..., :, None] * dg[..., None, :])))
    for k in ("nu", "alpha"):
        e[k] = float(np.max(np.abs(g[k] - r[k]) / np.abs(r[k])))
    if got.get("fe") is not None and ref.get("fe") is not None:
        e["fe"] = float(np.max(np.abs(np.asarray(got["fe"]) - ref["fe"]) / np.abs(ref["fe"])))
    if got.get("resp") is not None and ref.get("resp") is not None:
        e["resp"] = float(np.max(np.abs(np.asarray(got["resp"]) - ref["resp"])))
    return e


def hold(got, ref, what="", components=None, bounds=CONTRACT):
    """asserts shapes, finiteness and the contract (CONTRACT, or the bounds given) on every key present in both; prints and returns the errors"""
    for k in KEYS + ("fe", "resp"):
        if k in KEYS or (got.get(k) is not None and ref.get(k) is not None):
            assert np.shape(got[k]) == np.shape(ref[k]), (what, k, np.shape(got[k]), np.shape(ref[k]))
            assert np.all(np.isfinite(got[k])), (what, k)
    e = contract_errors(got, ref, components)
    print(what, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < bounds[k], (what, k, v, bounds[k])
    return e


# ------------------------------------------------------------------------------------------------------------------------------------------
# inputs
def ring_data(N, K, d, L, seed, one_draw=False):
    """clusters on a ring (the reference test's layout, gmm_multivariate_tests.jl:86-103), numpy default_rng; one_draw: all points from one
    standard-normal draw through the Cholesky factors (other numbers; a draw per point takes seconds at N ≈ 262 000)"""
    rng = np.random.default_rng(seed)
    means, covs = [], []
    for k in range(K):
        v = rng.standard_normal(d)
        v *= L / np.linalg.norm(v)
        A = rng.standard_normal((d, d))
        means.append(v)
        covs.append(A @ A.T + np.diag(rng.uniform(5.0, 20.0, d)))
    z = rng.integers(0, K, N)
    if one_draw:
        chol = np.stack([np.linalg.cholesky(c) for c in covs])
        y = np.array(means)[z] + np.einsum("nab,nb->na", chol[z], rng.standard_normal((N, d)))
    else:
        y = np.stack([rng.multivariate_normal(means[k], covs[k]) for k in z])
    return y, np.array(means), np.array(covs)


def setup(K, d, means, seed):
    rng = np.random.default_rng(seed)
    mu0 = 0.5 * means + rng.uniform(0, 5, (K, d))
    S0 = np.tile(1e6 * np.eye(d), (K, 1, 1))
    nu0 = np.full(K, d + 1.0)
    V0 = np.tile(1e2 * np.eye(d), (K, 1, 1))
    al0 = np.ones(K)
    return mu0, S0, nu0, V0, al0


def uv_case(K, n, seed):
    """(y, priors, init) of the univariate engine's K-component cases (tests/test_gmm_gpu.py): unit-variance clusters 10 apart"""
    mus = np.linspace(-10 * K / 2, 10 * K / 2, K) if K > 1 else np.array([0.75])
    rng = np.random.default_rng(seed)
    y = mus[rng.choice(K, size=n, p=np.ones(K) / K)] + rng.standard_normal(n)
    priors = (mus + 1.0, np.full(K, 1e3), np.full(K, 0.01), np.full(K, 0.01), np.ones(K))
    init = (mus + 2.0, np.full(K, 10.0), np.ones(K), np.ones(K), np.ones(K))
    return y, priors, init


# kind: "ring" = ring_data of radius L with seed 10 d + K, priors setup(seed = K), `offset` added to data and prior means;
#       "ring1" = the same from one draw (ring_data one_draw);  "starved" = ring, with the last component's prior and initial mean at 1e3 in every coordinate: it never receives a point;
#       "axis" = two clusters on the first axis (d = 5, K = 2: the dense path's grid-stride data);  "iid" = K = 1, d = 6, the iid MvNormal×Wishart model
Case = collections.namedtuple("Case", "d K N iters L offset kind", defaults=(50.0, 0.0, "ring"))

# one pass of the lane kernels' grid covers LANE_CAP workgroups × LANE_WG points (rxhip_mvgmm_create, rxhip_gmm_create); the dense one
# DENSE_CAP × DENSE_TILE (MVD_GRID_CAP, MVD_TP).  At STRIDE_N workgroup 0 takes a full second round and workgroup 1 a ragged one.
LANE_WG, LANE_CAP, DENSE_TILE, DENSE_CAP = 256, 1024, 128, 512
STRIDE_N = LANE_CAP * LANE_WG + LANE_WG + 37

# Every case of the host and device tests of the multivariate engines, by group.  tests/test_mvgmm_ref_cpu.py asserts for each that the
# reference on the data in reversed order agrees with itself within CONDITION (the offset case: CONDITION_OFFSET, above); a case that misses
# that is replaced, not loosened.
# Passed over for that reason: ring (d=4, K=8, N=600, 5 iterations) at radius 6 (the two host references already differ by 6e-7 there).
CASES = dict(
    restatement=[Case(2, 3, 500, 10), Case(5, 3, 300, 6), Case(8, 5, 700, 6), Case(8, 16, 2000, 4)],
    lane=[Case(2, 3, 500, 25), Case(1, 3, 777, 8), Case(2, 16, 4000, 6), Case(3, 5, 1500, 10), Case(3, 8, 2000, 5), Case(4, 2, 900, 8),
          Case(4, 8, 3000, 4), Case(2, 1, 300, 5)],
    # the template instantiations (D, KT) = (1,8) (1,16) (2,8) (3,4) of k_mvg_* that no other case launches
    lane_instances=[Case(1, 8, 300, 4), Case(1, 16, 600, 4), Case(2, 8, 500, 4), Case(3, 4, 300, 4)],
    lane_soft=[Case(2, 5, 400, 6, L=6.0)],
    # around a wavefront (64) and a workgroup (256)
    lane_sizes=[Case(d, K, N, 3) for d, K in ((4, 3), (3, 8)) for N in (1, 63, 65, 255, 256, 257)] + [Case(2, 2, 1, 3)],
    lane_stride=[Case(1, 2, STRIDE_N, 2, L=10.0, kind="ring1"), Case(4, 8, STRIDE_N, 2, L=10.0, kind="ring1")],
    # K < KT for KT = 4, 8, 16: responsibilities are written with the row stride K, the statistics are kept for KT components
    lane_padding=[Case(2, 3, 333, 4), Case(2, 5, 333, 4), Case(2, 9, 333, 4)],
    lane_starved=[Case(3, 3, 300, 4, kind="starved")],
    # d ∈ {5, 8, 15, 16, 17, 31, 32}: tile padding, both tile counts; K ∈ {1, 3, 5, 16}: one component per wavefront, uneven ownership, full;
    # N ∈ {1, 15, 17, 257, 1500}: below one MFMA row block, across it, ragged last tile
    dense=[Case(5, 1, 1, 4), Case(5, 3, 15, 4), Case(8, 5, 257, 5), Case(8, 16, 1500, 4), Case(15, 3, 17, 4), Case(16, 5, 257, 4),
           Case(16, 16, 1500, 4), Case(17, 1, 257, 4), Case(17, 3, 1500, 4), Case(31, 5, 17, 4), Case(32, 3, 15, 4), Case(32, 16, 1500, 4)],
    dense_soft=[Case(8, 4, 800, 5, L=6.0), Case(24, 6, 800, 5, L=6.0)],
    dense_offset=[Case(16, 4, 600, 5), Case(16, 4, 600, 5, offset=1e4)],
    dense_stride=[Case(5, 2, DENSE_CAP * DENSE_TILE + 3 * DENSE_TILE + 37, 2, kind="axis")],
    dense_other=[Case(17, 16, 1500, 4), Case(12, 3, 200, 4), Case(6, 1, 300, 5, kind="iid")],
)


def inputs(c):
    """(y [N][d], priors (mu0, S0, nu0, V0, alpha0), initial marginals (mean, cov, nu, V, alpha)) of a Case"""
    d, K, N = c.d, c.K, c.N
    if c.kind == "iid":
        rng = np.random.default_rng(5)
        Lm = rng.standard_normal((d, d))
        y = rng.multivariate_normal(rng.random(d), Lm @ Lm.T + np.eye(d), size=N)
        one = lambda a: np.asarray(a, dtype=np.float64)[None]
        pri = (one(np.zeros(d)), one(0.01 * np.eye(d)), np.array([d + 1.0]), one(np.eye(d)), np.array([1.0]))
        return y, pri, (one(np.zeros(d)), one(np.eye(d)), np.array([d + 1.0]), one(np.eye(d)), np.array([1.0]))
    if c.kind == "axis":
        rng = np.random.default_rng(77)
        means = np.array([[30.0, 0, 0, 0, 0], [-30.0, 5, 0, 0, 0]])
        y = means[rng.integers(0, K, N)] + rng.standard_normal((N, d)) * np.array([3.0, 2.0, 1.0, 4.0, 2.5])
    else:
        y, means, _ = ring_data(N, K, d, c.L, seed=10 * d + K, one_draw=c.kind == "ring1")
    mu0, S0, nu0, V0, al0 = setup(K, d, means, seed=K)
    y, mu0 = y + c.offset, mu0 + c.offset
    if c.kind == "starved":
        mu0[-1] = 1e3
    return y, (mu0, S0, nu0, V0, al0), (mu0, S0, nu0, V0, np.ones(K))


@functools.lru_cache(maxsize=None)
def case(c):
    """inputs and the NumPy reference of a Case (result()), computed once and shared read-only between the tests of one process"""
    y, pri, init = inputs(c)
    hist, fe, resp = mvgmm_vmp(y, *pri, rxoracle.mvgmm_pack(*init), c.iters, want_resp=True)
    for a in (y, hist, fe, resp) + tuple(pri):
        a.setflags(write=False)
    return y, pri, init, result(hist, c.d, fe, resp)


def oracle(c):
    """the C oracle on a Case (d ≤ 8), as result()"""
    y, pri, init = inputs(c)
    hist, fe, resp = rxoracle.mvgmm_vmp(y, *pri, rxoracle.mvgmm_pack(*init), c.iters, want_resp=True)
    return result(hist, c.d, fe, resp)

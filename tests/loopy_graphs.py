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


# ---- random loopy graphs (tests/test_loopy_oracle.py, tests/test_loopy_random_gpu.py, tests/fuzz_cases.py run_loopy_case) ----
# Every builder takes a seed and returns (builder, data variables, dict(x = the Gaussian variables to compare, cut = the initialised variables)).  The cut is a
# random feedback vertex set, grown greedily and pruned to a minimal one, so every cycle passes an initialised variable; each D has a non-zero mean and a
# correlated covariance.  Couplings are weak next to the priors (every ring / grid site has a prior or a strong neighbour), so that loopy BP converges.

DIMS = (1, 2, 3, 4, 5, 8, 12, 20, 33, 48, 64)


def _spd(rng, d, s=1.0):
    M = rng.normal(size=(d, d)) / np.sqrt(d)
    return s * (np.eye(d) + 0.3 * (M @ M.T))


def _weak(rng, r, c, norm):
    """a random r × c map (r ≤ c) of spectral norm `norm` whose singular values lie in [0.3, 1] · norm: a map of condition 1e13 would leave the executor a
    variance it cannot invert (a scalar for 1 × 1)"""
    A = rng.normal(size=(r, c))
    U, sv, Vt = np.linalg.svd(A, full_matrices=False)
    A = (U * (norm * np.clip(sv / sv[0], 0.3, 1.0))) @ Vt
    return float(A[0, 0]) if (r, c) == (1, 1) else A


def _noise(gb, rng, out, mu, V):
    """out ~ N(mu, V) in the covariance or the precision spelling"""
    d = gb.rows[out]
    if rng.random() < 0.5:
        gb.mvnormal_mean_cov(out, mu, gb.constvar(V)) if d > 1 else gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, out, mu, gb.constvar(float(V[0, 0])))
    else:
        W = np.linalg.inv(V)
        gb.node(_lib.NODE_MVNORMAL_MEAN_PRECISION, out, mu, gb.constvar(W)) if d > 1 else gb.node(_lib.NODE_NORMAL_MEAN_PRECISION, out, mu, gb.constvar(float(W[0, 0])))


def _prior(gb, rng, x, ys, derived=False):
    d = gb.rows[x]
    if derived:   # the mean is `a + b` of two data variables: a derived clamped value next to the loop
        a, b, s = gb.datavar(d), gb.datavar(d), gb.randomvar(d)
        gb.node(_lib.NODE_ADD, s, a, b)
        ys.extend([a, b])
        _noise(gb, rng, x, s, _spd(rng, d, rng.uniform(0.5, 2.0)))
    else:
        _noise(gb, rng, x, gb.constvar(rng.normal(size=d) if d > 1 else float(rng.normal())), _spd(rng, d, rng.uniform(0.5, 2.0)))


def _leaves(gb, rng, x, ys, preds, p_obs=0.6, p_pred=0.2):
    """an observation y ~ N(C x, R) (C with rows ≤ columns, sometimes not square) and / or an unobserved leaf (a prediction)"""
    d = gb.rows[x]
    if rng.random() < p_obs:
        r = int(rng.integers(1, d + 1)) if rng.random() < 0.4 else d
        mean = x
        if r != d or rng.random() < 0.3:
            mean = gb.randomvar(r)
            gb.multiply(mean, gb.constvar(_weak(rng, r, d, rng.uniform(0.5, 1.5))), x)
        y = gb.datavar(r)
        _noise(gb, rng, y, mean, _spd(rng, r, rng.uniform(0.3, 1.5)))
        ys.append(y)
    if rng.random() < p_pred:
        p = gb.randomvar(d)
        _noise(gb, rng, p, x, _spd(rng, d, 0.5))
        preds.append(p)


def _gauss(gb):
    import tree_oracle
    g = tree_oracle.TreeGraph(gb.to_dump())
    return g, [v for v in range(len(gb.kind)) if g.gauss[v]]


def uncut_cycle_variables(gb, cut=None):
    """the Gaussian variables that lie on a cycle of the Gaussian factor graph which passes no variable of `cut` (default: the initialised ones)"""
    import tree_oracle
    g = tree_oracle.TreeGraph(gb.to_dump())
    cut = set(gb.msg_init_family) if cut is None else set(cut)
    edges = [e for e in g.gauss_edges() if e[1] not in cut]
    keys = tree_oracle.cycle_edges(edges)
    return {v for _, v, key in edges if key in keys}


def feedback_vertex_set(gb, rng, candidates=None):
    """a random minimal feedback vertex set of the Gaussian variables: greedily add a random variable of an uncut cycle (from `candidates` where one lies
    on it), then drop, in random order, every variable without which all cycles stay cut"""
    cut = []
    while True:
        on = sorted(uncut_cycle_variables(gb, cut))
        if not on:
            break
        pool = [v for v in on if candidates is None or v in candidates] or on
        cut.append(int(pool[int(rng.integers(0, len(pool)))]))
    for v in [cut[i] for i in rng.permutation(len(cut))]:
        rest = [w for w in cut if w != v]
        if not uncut_cycle_variables(gb, rest):
            cut = rest
    return cut


def initialise(gb, rng, cut):
    """`μ(v) = D` on every variable of `cut`: D with a non-zero mean and a correlated covariance"""
    for v in cut:
        d = gb.rows[v]
        gb.initialize_message(v, _lib.INIT_MVNORMAL, np.concatenate([rng.normal(size=d), _spd(rng, d, rng.uniform(2.0, 10.0)).ravel()]))


def drop_one_cut(gb, cut, rng):
    """a copy of the graph with the message initialisation of one variable of the minimal cut `cut` removed; returns (builder, the dropped variable, the
    variables on the cycles that are now uncut)"""
    import copy
    g2 = copy.deepcopy(gb)
    v = int(cut[int(rng.integers(0, len(cut)))])
    del g2.msg_init_family[v], g2.msg_init_off[v]
    return g2, v, uncut_cycle_variables(g2)


def _finish(gb, ys, rng, preds, extra_inits=False, candidates=None):
    """cut the cycles by a random minimal feedback vertex set (named["fvs"]), sometimes with one more initialisation on a cycle (named["cut"]: all)"""
    fvs = feedback_vertex_set(gb, rng, candidates)
    cut = list(fvs)
    if extra_inits:   # a second initialisation on a cycle that one already cuts
        _, gv = _gauss(gb)
        on = [v for v in gv if v not in cut and v in uncut_cycle_variables(gb, [])]
        if on:
            cut.append(int(on[int(rng.integers(0, len(on)))]))
    initialise(gb, rng, cut)
    _, gv = _gauss(gb)
    return gb, ys, dict(x=gv, cut=cut, fvs=fvs, pred=preds)


def ring(seed, d=None, n=None, chord=None):
    """a closed chain x[i + 1] ~ N(A_i x[i], P_i), x[n] = x[0], the links sometimes through two maps with fewer rows than columns that meet in a Gaussian
    node (z_i = B_i x[i + 1] ~ N(C_i x[i], Q_i)); sites with or without a prior (degree 2: the alias path), observations, predictions; with a chord
    (two cycles that share edges) now and then"""
    rng = np.random.default_rng(100_000 + seed)
    d = int(rng.choice(DIMS)) if d is None else d
    n = int(rng.integers(3, 5) if d >= 33 else rng.integers(3, 9)) if n is None else n
    gb, ys, preds = GraphBuilder(), [], []
    xs = [gb.randomvar(d) for _ in range(n)]
    links = [(i, (i + 1) % n) for i in range(n)]
    if (rng.random() < 0.4 if chord is None else chord) and n >= 4 and d < 33:
        links.append((0, int(rng.integers(2, n - 1))))
    meet = [d > 1 and d < 33 and rng.random() < 0.3 for _ in links]
    for i, x in enumerate(xs):   # (a site next to a meeting of two maps hears a rank-deficient message from it: it keeps a prior)
        if i == 0 or rng.random() < 0.6 or any(m and i in ab for m, ab in zip(meet, links)):
            _prior(gb, rng, x, ys, derived=rng.random() < 0.15)
        if d < 33:
            _leaves(gb, rng, x, ys, preds)
    for (a, b), mt in zip(links, meet):
        if mt:
            r = int(rng.integers(1, d))
            za, zb = gb.randomvar(r), gb.randomvar(r)
            gb.multiply(za, gb.constvar(_weak(rng, r, d, 0.6)), xs[a])
            gb.multiply(zb, gb.constvar(_weak(rng, r, d, 0.6)), xs[b])
            _noise(gb, rng, zb, za, _spd(rng, r, 2.0))
        else:
            m = gb.randomvar(d)
            gb.multiply(m, gb.constvar(_weak(rng, d, d, rng.uniform(0.3, 0.8))), xs[a])
            _noise(gb, rng, xs[b], m, _spd(rng, d, rng.uniform(1.5, 3.0)))
    return _finish(gb, ys, rng, preds, extra_inits=rng.random() < 0.3)


def grid(seed, d=None, rows=None, cols=None, cut=None):
    """an rows × cols grid of d-dimensional sites with pairwise Gaussian factors x[j] ~ N(A x[i], P) between neighbours, every site with a prior.
    cut: the initialised sites as (row, column) pairs (default: a random minimal feedback vertex set)"""
    rng = np.random.default_rng(200_000 + seed)
    d = int(rng.choice((1, 2, 3, 4, 5, 8))) if d is None else d
    rows = int(rng.integers(2, 5)) if rows is None else rows
    cols = int(rng.integers(2, 5)) if cols is None else cols
    gb, ys, preds = GraphBuilder(), [], []
    site = {(i, j): gb.randomvar(d) for i in range(rows) for j in range(cols)}
    for (i, j), x in site.items():
        _prior(gb, rng, x, ys)
        _leaves(gb, rng, x, ys, preds, p_obs=0.5, p_pred=0.1)
    for (i, j), x in site.items():
        for nb in ((i + 1, j), (i, j + 1)):
            if nb in site:
                m = gb.randomvar(d)
                gb.multiply(m, gb.constvar(_weak(rng, d, d, rng.uniform(0.2, 0.5))), x)
                _noise(gb, rng, site[nb], m, _spd(rng, d, rng.uniform(2.0, 4.0)))
    if cut is not None:
        initialise(gb, rng, [site[c] for c in cut])
        _, gv = _gauss(gb)
        return gb, ys, dict(x=gv, cut=[site[c] for c in cut], fvs=[site[c] for c in cut], pred=preds, site=site)
    out = _finish(gb, ys, rng, preds, candidates=set(site.values()))
    out[2]["site"] = site
    return out


def plus_cycles(seed, d=None):
    """cycles through `+` nodes with two random inputs: u_k ~ N(B_k x, Q_k), s = u_j + u_k, y ~ N(s, R) for random pairs (j, k) of children of a root x —
    pairs that share a child share the edges x – u_j"""
    rng = np.random.default_rng(300_000 + seed)
    d = int(rng.choice(DIMS)) if d is None else d
    K = 2 if d >= 33 else int(rng.integers(2, 6))
    gb, ys, preds = GraphBuilder(), [], []
    x = gb.randomvar(d)
    _prior(gb, rng, x, ys, derived=rng.random() < 0.2)
    us = []
    for _ in range(K):
        u = gb.randomvar(d)
        m = gb.randomvar(d)
        gb.multiply(m, gb.constvar(_weak(rng, d, d, rng.uniform(0.5, 1.0))), x)
        _noise(gb, rng, u, m, _spd(rng, d, rng.uniform(0.5, 1.5)))
        us.append(u)
    pairs = [(0, 1)] + [tuple(int(i) for i in rng.choice(K, 2, replace=False)) for _ in range(int(rng.integers(0, K)) if d < 33 else 0)]
    for j, k in pairs:
        s = gb.randomvar(d)
        gb.node(_lib.NODE_ADD, s, us[j], us[k])
        if rng.random() < 0.8:
            y = gb.datavar(d)
            _noise(gb, rng, y, s, _spd(rng, d, rng.uniform(0.5, 2.0)))
            ys.append(y)
        else:
            _leaves(gb, rng, s, ys, preds, p_obs=1.0, p_pred=1.0)
    return _finish(gb, ys, rng, preds, extra_inits=rng.random() < 0.3)


def star(seed, d=None, N=None, cut=None):
    """the vector regression y[i] ~ MvNormal(X[i] b + a, Σ) with N > 16 observations (hubs a and b of degree N + 1), cut at a or b"""
    rng = np.random.default_rng(400_000 + seed)
    d = int(rng.choice((2, 5, 8, 12, 20, 33))) if d is None else d
    N = int(rng.integers(17, 21)) if N is None else N
    X, pa, pb, S, D, _ = vector_problem(N, d, seed=seed)
    X = 0.25 * X   # (weak maps: the two hubs converge in tens of iterations, not hundreds)
    cut = str(rng.choice(["a", "b"])) if cut is None else cut
    gb, ys, nm = linreg(X, pa, pb, S, init={cut: D})
    _, gv = _gauss(gb)
    return gb, ys, dict(x=gv, cut=[nm[cut]], fvs=[nm[cut]], pred=[])


def closed_forest(seed, dmax=None):
    """a random forest (tests/tree_graphs.py::random_forest: every construct of the family, no precision variables) with one or two weak Gaussian factors
    between variables of equal dimension added to close cycles"""
    import tree_graphs as tg
    rng = np.random.default_rng(500_000 + seed)
    dmax = int(rng.choice((1, 2, 4, 8, 12))) if dmax is None else dmax
    for attempt in range(20):
        gb, ys, named = tg.random_forest(seed * 20 + attempt, n_steps=int(rng.integers(6, 12)), dmax=dmax)
        _, gv = _gauss(gb)
        by_dim = {}
        for v in gv:
            by_dim.setdefault(gb.rows[v], []).append(v)
        pairs = [vs for vs in by_dim.values() if len(vs) >= 2]
        if not pairs:
            continue
        for _ in range(int(rng.integers(1, 3))):
            vs = pairs[int(rng.integers(0, len(pairs)))]
            a, b = (int(v) for v in rng.choice(vs, 2, replace=False))
            dd = gb.rows[a]
            m = gb.randomvar(dd)
            gb.multiply(m, gb.constvar(_weak(rng, dd, dd, 0.3)), a)
            _noise(gb, rng, b, m, _spd(rng, dd, 3.0))
        if not uncut_cycle_variables(gb, []):
            continue
        out = _finish(gb, ys, rng, [], extra_inits=rng.random() < 0.3)
        try:
            from rxhip.tree import plan
            plan(gb)
        except Exception as e:   # a loop message that only the initialisation informs (a cycle of unobserved leaves) is refused by design: draw again
            if "no information" in str(e):
                continue
            raise
        return out
    raise RuntimeError("no closable forest drawn")


KINDS = ("ring", "grid", "plus", "star", "forest")


def random_loopy(seed, kind=None):
    """one random loopy graph of any kind: (builder, data variables, named, kind)"""
    rng = np.random.default_rng(600_000 + seed)
    kind = KINDS[int(rng.integers(0, len(KINDS)))] if kind is None else kind
    gen = dict(ring=ring, grid=grid, plus=plus_cycles, star=star, forest=closed_forest)[kind]
    gb, ys, named = gen(seed)
    return gb, ys, named, kind


# the random loopy graphs the GPU tests run (tests/test_loopy_random_gpu.py), (kind, seed): dimensions 1 … 64 (≥ 33 with at most 8 Gaussian variables, but for
# star 15: a hub at d = 33 on the LDS-staged kernels), cut variables of degree 2 and hubs of degree > 16, second initialisations on a cycle, predictions and
# derived clamped values next to a loop; tests/test_loopy_oracle.py holds the restatement on every one of them to exact conditioning
GPU_GRAPHS = [("ring", 0), ("ring", 1), ("ring", 2), ("ring", 3), ("ring", 4), ("ring", 7), ("ring", 8), ("plus", 0), ("plus", 2), ("plus", 6), ("plus", 7),
              ("plus", 9), ("grid", 1), ("grid", 3), ("grid", 8), ("star", 0), ("star", 1), ("star", 2), ("star", 4), ("star", 15), ("forest", 0), ("forest", 6), ("forest", 9)]

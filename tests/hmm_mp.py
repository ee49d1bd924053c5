"""The hidden Markov model engine's iteration (include/rxhip.h rxhip_hmm_desc) restated in mpmath at 50 digits, and the grid of cases on which
tests/test_hmm_contract_cpu.py and tests/test_hmm_contract_gpu.py hold the engine to it.

`run` is the iteration written out plainly: digamma, exp, scaled forward–backward, statistics, count update, free energy
    F = −log Z̃ + Σ N∘(lA_old − lA_new) + Σ Mstat∘(lB_old − lB_new) + KL(q(A)‖p(A)) + KL(q(B)‖p(B))        (KL with mp.loggamma)
— the formulas of tests/hmm_ref.py, but with 50 digits under them: where a double-precision formula loses digits (the log-gamma differences of the
KL term at large counts, exp of −1/c at small ones) this one keeps 30 and more.

`GRID` is a list of case specs, `SCAN` the small-initial-count scans; `case(spec)` builds a spec's inputs deterministically.  The results live in
tests/golden/hmm_long.npz (tests/golden/make_hmm_long_golden.py): per case the vector `pick` selects, as float64, and a CRC of the inputs."""
import collections
import zlib

import mpmath as mp
import numpy as np

import hmm_ref as R

DPS = 50

Spec = collections.namedtuple("Spec", "name seed T K M iterations p init edge mixed series share")


def _spec(name, seed, p, init, T=24, K=3, M=4, iterations=4, edge=None, mixed=None, series=1, share=False):
    return Spec(name, seed, T, K, M, iterations, p, init, edge, mixed, series, share)


def _grid():
    """Seeds count up through the list; an odd seed means sticky data, an even one uniform symbols (see `data`)."""
    out, n = [], [0]

    def add(name, p, init, sticky, **kw):
        seed = 2 * n[0] + (1 if sticky else 0)
        n[0] += 1
        out.append(_spec(f"{name} p={p:g} init={init if init == 'default' else format(init, 'g')} {'sticky' if sticky else 'uniform'}", seed, p, init, **kw))

    for p in (1e-3, 1e-2, 0.1, 1.0, 10.0, 1e3, 1e6, 1e9):                       # count scale
        for init in ("default", p):
            if init != "default" and init < 1e-2:
                continue                                                        # an initial scale below 1e-2 belongs to SCAN
            for sticky in (False, True):
                add("scale", p, init, sticky)
    for p in (1e-2, 1.0, 1e6):                                                  # data edges
        for k, edge in enumerate(("symbol never occurs", "one symbol throughout", "nothing observed")):
            add(edge, p, p, k % 2 == 1, edge=edge)
    add("row 2 of B × 1e-3", 1.0, 1.0, False, mixed="B row")                    # mixed magnitudes inside one table
    add("column 1 of A × 1e-3, init_A[0, 2] × 1e-4", 1.0, 1.0, True, mixed="A column")
    for p in (1e-2, 1.0, 1e6):                                                  # widths
        add("widest", p, p, True, T=8, K=16, M=64)
        add("narrowest", p, p, False, T=24, K=2, M=2)
    add("partial row", 1.0, 1.0, True, T=12, K=9, M=3)
    for p in (1e-2, 1e6):                                                       # shortest
        add("T=1", p, p, False, T=1)
        add("T=2", p, p, True, T=2)
    for p in (1e-2, 1e6):                                                       # shared parameters
        add("shared", p, p, p > 1, series=5, share=True)
    for p in (1.0, 1e-2):                                                       # long chain
        add("long", p, "default", True, T=4096, K=3, M=3, iterations=3)
    return out


SCAN_SCALES = tuple(s * 1e-3 for s in (1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 2.5, 3.0, 4.0, 5.0, 10.0))
SCAN2_SCALES = tuple(s * 1e-3 for s in (1.5, 2.0, 3.0, 5.0))


def _scan():
    """Priors at scale 1, initial counts s·U(0.5, 3): K = 3, M = 4, T = 30, seeds 0 … 9 (110 cases), then K = 8, M = 16, T = 12, seeds 0 … 4 (20)."""
    out = [_spec(f"scan s={s:g} seed={seed}", seed, 1.0, s, T=30, iterations=3) for s in SCAN_SCALES for seed in range(10)]
    out += [_spec(f"scan2 s={s:g} seed={seed}", seed, 1.0, s, T=12, K=8, M=16, iterations=3) for s in SCAN2_SCALES for seed in range(5)]
    return out


GRID = _grid()
SCAN = _scan()
LONG_STEPS = (0, 1, 2, 63, 64, 65, 1023, 1024, 2047, 2048, 3071, 3072, 4093, 4094, 4095, 4096)   # of γ_0 … γ_T at T = 4096


def sticky_data(seed, T, K, M, missing=0.05):
    """State-sticky symbols from their own default_rng(seed): the state is kept with probability 0.9, otherwise redrawn uniformly; it emits
    symbol state % M with probability 0.8, otherwise a uniform symbol; `missing` of the steps are NaN.  All draws are made up front, in the
    order below, so the stream does not depend on the path."""
    rng = np.random.default_rng(seed)
    s = int(rng.integers(0, K))
    keep, redraw = rng.random(T) < 0.9, rng.integers(0, K, T)
    own, other = rng.random(T) < 0.8, rng.integers(0, M, T)
    miss = rng.random(T) < missing
    x = np.empty(T)
    for t in range(T):
        if not keep[t]:
            s = int(redraw[t])
        x[t] = s % M if own[t] else other[t]
    x[miss] = np.nan
    return x


def data(seed, T, K, M):
    """odd seeds: `sticky_data`; even seeds: column 0 of hmm_ref.random_case (uniform symbols, 5 % missing)"""
    return sticky_data(seed, T, K, M) if seed % 2 else R.random_case(seed, T, 1, K, M, per_series=False)[0][:, 0]


def shared_pi(K):
    """The engine takes ONE π per engine, and the grid's cases of equal (T, K, M) run as the series of one engine: they share this π (not yet
    normalised), U(0.5, 3) from default_rng(10000 + K).  A scan case is an engine of its own and keeps the π of its seed."""
    return np.random.default_rng(10000 + K).uniform(0.5, 3.0, K)


def case(spec):
    """(x [T] — [T][series] with shared parameters —, dict of model arguments) of a spec.  Draws, in this order from default_rng(seed): π = U(0.5, 3, K)
    (normalised; used by the scan cases, see `shared_pi`), prior_A = p·U(0.5, 3, (K, K)), prior_B = p·U(0.5, 3, (M, K)), init_A = s·U(0.5, 3, (K, K)),
    init_B = s·U(0.5, 3, (M, K)).  The data come from streams of their own (`data`)."""
    rng = np.random.default_rng(spec.seed)
    K, M = spec.K, spec.M
    pi = rng.uniform(0.5, 3.0, K)
    if not spec.name.startswith("scan"):
        pi = shared_pi(K)
    m = dict(prior_s0=pi / pi.sum(), prior_A=spec.p * rng.uniform(0.5, 3.0, (K, K)), prior_B=spec.p * rng.uniform(0.5, 3.0, (M, K)))
    s = 1.0 if spec.init == "default" else spec.init
    m["init_A"], m["init_B"] = s * rng.uniform(0.5, 3.0, (K, K)), s * rng.uniform(0.5, 3.0, (M, K))    # (drawn either way: one stream for every spec)
    if spec.init == "default":
        m["init_A"], m["init_B"] = np.ones((K, K)), np.ones((M, K))
    if spec.mixed == "B row":
        m["prior_B"][2] *= 1e-3
        m["init_B"][2] *= 1e-3
    elif spec.mixed == "A column":
        m["prior_A"][:, 1] *= 1e-3
        m["init_A"][:, 1] *= 1e-3
        m["init_A"][0, 2] *= 1e-4
    x = np.stack([data(spec.seed + 2 * c, spec.T, K, M) for c in range(spec.series)], axis=1)   # (+ 2c keeps the seed's parity)
    if spec.edge == "symbol never occurs":
        x[x == M - 1] = 0.0
    elif spec.edge == "one symbol throughout":
        x[x == x] = 2.0
    elif spec.edge == "nothing observed":
        x[:] = np.nan
    return (x if spec.share else x[:, 0]), m


def checksum(x, m):
    """CRC-32 of a case's inputs, to notice a generator that drifted"""
    parts = [np.ascontiguousarray(v, dtype=np.float64) for v in (x, m["prior_s0"], m["prior_A"], m["prior_B"], m["init_A"], m["init_B"])]
    return zlib.crc32(b"".join(np.where(np.isnan(p), -1.0, p).tobytes() for p in parts))


# ---- the iteration at 50 digits ---------------------------------------------------------------------------------------------------------------------
def _mat(a):
    return [[mp.mpf(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)]


def _tables(c):
    """l[i][j] = ψ(c[i][j]) − ψ(Σ_i c[i][j]) and exp of it"""
    n, K = len(c), len(c[0])
    tot = [mp.digamma(mp.fsum(c[i][j] for i in range(n))) for j in range(K)]
    l = [[mp.digamma(c[i][j]) - tot[j] for j in range(K)] for i in range(n)]
    return l, [[mp.exp(v) for v in row] for row in l]


def _kl(c, p, l):
    """Σ over columns of KL(Dir(c[:, j]) ‖ Dir(p[:, j]))"""
    n, K = len(c), len(c[0])
    out = mp.mpf(0)
    for j in range(K):
        out += mp.loggamma(mp.fsum(c[i][j] for i in range(n))) - mp.loggamma(mp.fsum(p[i][j] for i in range(n)))
        for i in range(n):
            out += (c[i][j] - p[i][j]) * l[i][j] - (mp.loggamma(c[i][j]) - mp.loggamma(p[i][j]))
    return out


def _forward_backward(pi, At, Bt, x):
    """γ [T+1][K], N [K][K], Mstat [M][K], log Z̃, the smallest normaliser"""
    T, K, M = len(x), len(pi), len(Bt)
    one = mp.mpf(1)
    fac = [[one] * K if xt != xt else Bt[int(xt)] for xt in x]
    alpha, logz, small = [list(pi)], mp.mpf(0), mp.inf
    for t in range(1, T + 1):
        v = [fac[t - 1][i] * mp.fsum(At[i][j] * alpha[t - 1][j] for j in range(K)) for i in range(K)]
        c = mp.fsum(v)
        alpha.append([u / c for u in v])
        logz += mp.log(c)
        small = min(small, c)
    beta = [one] * K
    gamma = [None] * (T + 1)
    n = [[mp.mpf(0)] * K for _ in range(K)]
    mstat = [[mp.mpf(0)] * K for _ in range(M)]
    for t in range(T, 0, -1):
        gamma[t] = [alpha[t][i] * beta[i] for i in range(K)]
        xt = x[t - 1]
        if xt == xt:
            row = mstat[int(xt)]
            for i in range(K):
                row[i] += gamma[t][i]
        w = [fac[t - 1][i] * beta[i] for i in range(K)]
        bt = [mp.fsum(At[j][i] * w[j] for j in range(K)) for i in range(K)]
        d = mp.fsum(alpha[t - 1][i] * bt[i] for i in range(K))
        small = min(small, d)
        for i in range(K):
            wd = w[i] / d
            for j in range(K):
                n[i][j] += wd * At[i][j] * alpha[t - 1][j]
        beta = [b / d for b in bt]
    gamma[0] = [alpha[0][i] * beta[i] for i in range(K)]
    return gamma, n, mstat, logz, small


def _f64(a):
    return np.array([[float(v) for v in row] for row in a], dtype=np.float64)


def run(x, prior_A, prior_B, prior_s0, init_A=None, init_B=None, iterations=1, share=False):
    """x [T] (one series) or, with share, [T][series] under one q(A), q(B).  Returns a dict of float64 results, every entry a list over the
    iterations: "gamma" [T+1][K] ([T+1][series][K] with share), "A" [K][K], "B" [M][K], "fe" (a float), and "log10_normaliser": log10 of the
    smallest c_t or d_t of the iteration's sweep (what the engine's guard looks at)."""
    x = np.asarray(x, dtype=np.float64)
    xs = [x] if not share else [x[:, c] for c in range(x.shape[1])]
    with mp.workdps(DPS):
        pA, pB, pi = _mat(prior_A), _mat(prior_B), [mp.mpf(float(v)) for v in prior_s0]
        K, M = len(pi), len(pB)
        a = _mat(np.ones((K, K)) if init_A is None else init_A)
        b = _mat(np.ones((M, K)) if init_B is None else init_B)
        out = {k: [] for k in ("gamma", "A", "B", "fe", "log10_normaliser")}
        for _ in range(iterations):
            (lA, At), (lB, Bt) = _tables(a), _tables(b)
            res = [_forward_backward(pi, At, Bt, xc) for xc in xs]
            n = [[mp.fsum(r[1][i][j] for r in res) for j in range(K)] for i in range(K)]
            ms = [[mp.fsum(r[2][m][i] for r in res) for i in range(K)] for m in range(M)]
            a = [[pA[i][j] + n[i][j] for j in range(K)] for i in range(K)]
            b = [[pB[m][i] + ms[m][i] for i in range(K)] for m in range(M)]
            lA2, lB2 = _tables(a)[0], _tables(b)[0]
            f = -mp.fsum(r[3] for r in res)
            f += mp.fsum(n[i][j] * (lA[i][j] - lA2[i][j]) for i in range(K) for j in range(K))
            f += mp.fsum(ms[m][i] * (lB[m][i] - lB2[m][i]) for m in range(M) for i in range(K))
            f += _kl(a, pA, lA2) + _kl(b, pB, lB2)
            g = [_f64(r[0]) for r in res]
            out["gamma"].append(np.stack(g, axis=1) if share else g[0])
            out["A"].append(_f64(a))
            out["B"].append(_f64(b))
            out["fe"].append(float(f))
            out["log10_normaliser"].append(float(mp.log10(min(r[4] for r in res))))
    return out


# ---- what the fixture keeps of a case ---------------------------------------------------------------------------------------------------------------
def gamma_steps(spec):
    """the steps of γ_0 … γ_T that the fixture keeps (of the last iteration)"""
    if spec.name.startswith("widest"):
        return tuple(range(spec.T + 1))
    if spec.name.startswith("long"):
        return LONG_STEPS
    if spec.name.startswith("scan"):
        return ()
    if spec.share:
        return (0, spec.T // 2, spec.T)
    return tuple(sorted({0, 1, spec.T // 2, spec.T - 1, spec.T}))


def pick(spec, gamma, A, B, fe):
    """What the fixture keeps of a case, from the posteriors of the LAST iteration (γ [T+1][…][K], A [K][K], B [M][K]) and the free energy of every
    iteration: a list of (quantity, array), quantity one of "gamma", "counts", "fe" — the three bounds of the contract.  The fixture has a size
    limit, hence subsets: γ at `gamma_steps`; the counts in full, except B's rows 0, 1, 31, 63 on the widest cases and A alone on the second scan;
    the free energy of every iteration, of the last one only on the scans."""
    gamma, A, B, fe = np.asarray(gamma), np.asarray(A), np.asarray(B), np.atleast_1d(np.asarray(fe, dtype=np.float64))
    out = []
    if gamma_steps(spec):
        out.append(("gamma", gamma[list(gamma_steps(spec))]))
    out.append(("counts", A))
    if spec.name.startswith("widest"):
        out.append(("counts", B[[0, 1, 31, 63]]))
    elif not spec.name.startswith("scan2"):
        out.append(("counts", B))
    out.append(("fe", fe[-1:] if spec.name.startswith("scan") else fe))
    return out


def flatten(picked):
    return np.concatenate([np.asarray(a, dtype=np.float64).ravel() for _, a in picked])


def errors(picked, flat):
    """{quantity: worst error} of `pick`'s output against the fixture's vector of the same case, in the contract's measures: γ absolute, counts
    relative, free energy relative to max(1, |F|)"""
    out, o = {}, 0
    for q, a in picked:
        a = np.asarray(a, dtype=np.float64)
        ref = flat[o:o + a.size].reshape(a.shape)
        o += a.size
        if not np.all(np.isfinite(a)):
            e = np.inf
        elif q == "gamma":
            e = float(np.max(np.abs(a - ref)))
        elif q == "counts":
            e = float(np.max(np.abs(a - ref) / ref))
        else:
            e = float(np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref))))
        out[q] = max(out.get(q, 0.0), e)
    assert o == flat.size, (o, flat.size)
    return out

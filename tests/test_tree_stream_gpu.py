"""rxhip_tree_stream (include/rxhip.h "Streaming"): T observations of a one-step graph in ONE call — `@autoupdates` feedback, VMP iterations, history and free
energy on the device — against the host loop the executor's users spelled out until now (rxhip_tree_continue, set_data, run, marginals, feedback computed in
numpy: tests/test_tree_gcv_gpu.py), bit for bit, and against references that share no code with the project: the HGF restatement of oracle/rxoracle.c, the
closed-form scalar Kalman recursion, conditioning a Gaussian on y in numpy.  Order per observation: src/inference/streaming.jl:341-407."""
import functools

import numpy as np
import pytest

import rxoracle
from rxhip import _lib, graph
from rxhip.tree import TreeEngine

pytestmark = pytest.mark.gpu


def _init_value(gb, src, kind):
    o, d = gb.init_off[src], gb.rows[src]
    q = np.concatenate(gb.pool)[o:o + d + d * d]
    return q[:d] if kind == "mean" else q[d:d + 1] if kind == "var" else 1.0 / q[d:d + 1]


def host_loop(gb, table, variables, series, iterations, history, R, allow_missing=False, extra=None):
    """The loop rxhip_tree_stream replaces, on an engine of its own: per observation the feedback from the current marginals (the `@initialization` ones before
    the first), set_data, run, marginals.  Returns (history {var: (mean [T][R][d], cov [T][R][d][d])}, fe [T][iterations], extra(engine))."""
    T = series.shape[0]
    targets, sources = [t for t, _, _ in table], sorted({s for _, s, _ in table})
    hist = {v: ([], []) for v in history}
    fes = []
    with TreeEngine(gb, n_replicas=R, allow_missing=allow_missing) as eng:
        eng.continue_runs(True)
        post = None
        for t in range(T):
            cols = []
            for _, s, k in table:
                if post is None:
                    cols.append(np.tile(_init_value(gb, s, k), (R, 1)))
                else:
                    m, c = post[s]
                    cols.append(m if k == "mean" else c[:, :, 0] if k == "var" else 1.0 / c[:, :, 0])
            eng.set_data(targets + list(variables), np.concatenate(cols + [series[t].reshape(R, -1)], axis=1))
            eng.run(iterations, True)
            post = eng.marginals(sorted(set(sources) | set(history)))
            for v in history:
                hist[v][0].append(post[v][0].copy())
                hist[v][1].append(post[v][1].copy())
            fes.append(eng.free_energy())
        ex = extra(eng) if extra else None
    return {v: (np.array(m), np.array(c)) for v, (m, c) in hist.items()}, np.array(fes), ex


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _assert_histories_identical(h1, h2):
    assert set(h1) == set(h2)
    for v in h1:
        assert _same(h1[v][0], h2[v][0]) and _same(h1[v][1], h2[v][1]), (v, np.max(np.abs(h1[v][0] - h2[v][0])), np.max(np.abs(h1[v][1] - h2[v][1])))


# ---- 1. the HGF step graph: stream ≡ host loop ≡ the restatement -------------------------------------------------------------------------------------------
HGF = dict(kappa=1.0, omega=0.0, zvar=0.04, yvar=0.01, iters=5, T=12, z0=(0.0, 5.0), x0=(0.0, 5.0))


def _hgf_series(R):
    rng = np.random.default_rng(7)
    return np.stack([np.cumsum(rng.standard_normal(HGF["T"])) * 0.3 for _ in range(R)], axis=1)[:, :, None]   # [T][R][1]


@functools.lru_cache(maxsize=None)
def _hgf_oracle(R):
    y = _hgf_series(R)
    out = [rxoracle.hgf_filter(np.ascontiguousarray(y[:, r, 0]), HGF["kappa"], HGF["omega"], HGF["zvar"], HGF["yvar"], z0=HGF["z0"], x0=HGF["x0"], vmp_iters=HGF["iters"], n_gh=31)
           for r in range(R)]
    return out


def _hgf_graph():
    return graph.hgf_step_graph(HGF["kappa"], HGF["omega"], HGF["zvar"], HGF["yvar"], q_zt=HGF["z0"], q_xt=HGF["x0"], n_gh=31)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("R", [1, 3])
def test_hgf_stream_equals_the_host_loop_and_the_restatement(R, mode, monkeypatch):
    monkeypatch.setenv("RXHIP_TREE_MODE", str(mode))
    gb, names = _hgf_graph()
    y = _hgf_series(R)
    hv = [names["zt"], names["xt"]]
    with TreeEngine(gb, n_replicas=R) as eng:
        eng.set_autoupdates(names["autoupdates"])
        out = eng.stream([names["y"]], y, iterations=HGF["iters"], free_energy=True, history=hv)
        last_fe = eng.free_energy()
    ref_h, ref_fe, _ = host_loop(gb, names["autoupdates"], [names["y"]], y, HGF["iters"], hv, R)
    _assert_histories_identical(out["history"], ref_h)
    assert out["free_energy"].shape == (HGF["T"], HGF["iters"]) and _same(out["free_energy"], ref_fe)
    assert _same(last_fe, ref_fe[-1])
    for r, (zm, zv, xm, xv, fe, _) in enumerate(_hgf_oracle(R)):
        (hzm, hzv), (hxm, hxv) = out["history"][names["zt"]], out["history"][names["xt"]]
        assert hzm[:, r, 0] == pytest.approx(zm, rel=1e-9, abs=1e-11) and hzv[:, r, 0, 0] == pytest.approx(zv, rel=1e-9)
        assert hxm[:, r, 0] == pytest.approx(xm, rel=1e-9, abs=1e-11) and hxv[:, r, 0, 0] == pytest.approx(xv, rel=1e-9)
    if R == 1:   # (the restatement reports the per-iteration free energy averaged over the observations)
        assert np.allclose(np.mean(out["free_energy"], axis=0), _hgf_oracle(1)[0][4], rtol=1e-9)


# ---- 2. a scalar Kalman step against the closed-form recursion ---------------------------------------------------------------------------------------------
KAL = dict(p=0.3, q=0.5, m0=0.4, v0=2.0)


def _kalman_graph(precision=False, init=True):
    """x_prev ~ Normal(mean = m, var = v) [or precision = w], x ~ Normal(x_prev, p), y ~ Normal(x, q); m, v = mean_var(q(x))"""
    gb = graph.GraphBuilder()
    xp, x = gb.randomvar(1), gb.randomvar(1)
    m, v, y = gb.datavar(1), gb.datavar(1), gb.datavar(1)
    gb.node(_lib.NODE_NORMAL_MEAN_PRECISION if precision else _lib.NODE_NORMAL_MEAN_VARIANCE, xp, m, v)
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, x, xp, gb.constvar(KAL["p"]))
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, y, x, gb.constvar(KAL["q"]))
    if init:
        gb.initialize(x, _lib.INIT_NORMAL, (KAL["m0"], KAL["v0"]))
    return gb, dict(x=x, y=y, m=m, v=v, table=[(m, x, "mean"), (v, x, "precision" if precision else "var")])


def _kalman_reference(y):
    """closed form, [T][R]; NaN = no observation (the posterior is the predicted prior)"""
    T, R = y.shape
    m, v = np.full(R, KAL["m0"]), np.full(R, KAL["v0"])
    ms, vs = np.empty((T, R)), np.empty((T, R))
    for t in range(T):
        vp = v + KAL["p"]
        k = np.where(np.isnan(y[t]), 0.0, vp / (vp + KAL["q"]))
        m = m + k * (np.where(np.isnan(y[t]), m, y[t]) - m)
        v = (1.0 - k) * vp
        ms[t], vs[t] = m, v
    return ms, vs


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("precision", [False, True])
def test_scalar_kalman_step_against_the_closed_form(precision):
    T, R = 10, 37
    y = np.random.default_rng(5).standard_normal((T, R)) * 1.5 + np.linspace(-2.0, 2.0, R)   # a different series per replica
    gb, n = _kalman_graph(precision)
    with TreeEngine(gb, n_replicas=R) as eng:
        eng.set_autoupdates(n["table"])
        out = eng.stream([n["y"]], y[:, :, None], iterations=1, free_energy=True, history=[n["x"]])
        final = eng.marginals([n["x"]])[n["x"]]
    ms, vs = _kalman_reference(y)
    hm, hv = out["history"][n["x"]]
    print("kalman", "precision" if precision else "variance", "feedback: mean rel", _rel(hm[:, :, 0], ms), "var rel", _rel(hv[:, :, 0, 0], vs))
    assert _rel(hm[:, :, 0], ms) < 1e-12 and _rel(hv[:, :, 0, 0], vs) < 1e-12
    assert _same(final[0], hm[-1]) and _same(final[1], hv[-1])   # the marginals afterwards are the last observation's
    assert np.all(np.isfinite(out["free_energy"])) and out["free_energy"].shape == (T, 1)
    if not precision:   # (1 / v on the device and on the host may differ in the last bit: the precision variant is not compared bitwise)
        ref_h, ref_fe, _ = host_loop(gb, n["table"], [n["y"]], y[:, :, None], 1, [n["x"]], R)
        _assert_histories_identical(out["history"], ref_h)
        assert _same(out["free_energy"], ref_fe)


# ---- 3. vector MEAN feedback on every storage layout and kernel family -------------------------------------------------------------------------------------
def _vector_graph(d, seed):
    """x_prev ~ MvNormal(mean = m, cov = S0), x ~ MvNormal(A x_prev, P), y ~ MvNormal(B x, Q); m = mean(q(x))"""
    rng = np.random.default_rng(seed)
    qm, _ = np.linalg.qr(rng.standard_normal((d, d)))
    A, B = 0.9 * qm, rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    spd = lambda s: (lambda M: s * (M @ M.T / d + np.eye(d)))(rng.standard_normal((d, d)))
    S0, P, Q = spd(1.0), spd(0.2), spd(0.5)
    gb = graph.GraphBuilder()
    xp, ax, x, bx = gb.randomvar(d), gb.randomvar(d), gb.randomvar(d), gb.randomvar(d)
    m, y = gb.datavar(d), gb.datavar(d)
    gb.mvnormal_mean_cov(xp, m, gb.constvar(S0))
    gb.multiply(ax, gb.constvar(A), xp)
    gb.mvnormal_mean_cov(x, ax, gb.constvar(P))
    gb.multiply(bx, gb.constvar(B), x)
    gb.mvnormal_mean_cov(y, bx, gb.constvar(Q))
    m0 = rng.standard_normal(d)
    gb.initialize(x, _lib.INIT_MVNORMAL, np.concatenate([m0, np.eye(d).ravel()]))
    return gb, dict(x=x, y=y, m=m, table=[(m, x, "mean")]), (A, B, S0, P, Q, m0)


def _vector_reference(mats, y):
    """condition on y with a fixed prior covariance: [T][R][d] means, the (constant) posterior covariance"""
    A, B, S0, P, Q, m0 = mats
    T, R, d = y.shape
    Vp = A @ S0 @ A.T + P
    K = Vp @ B.T @ np.linalg.inv(B @ Vp @ B.T + Q)
    V = Vp - K @ B @ Vp
    m = np.tile(m0, (R, 1))
    ms = np.empty((T, R, d))
    for t in range(T):
        mp = m @ A.T
        m = mp + (y[t] - mp @ B.T) @ K.T
        ms[t] = m
    return ms, V


@pytest.mark.parametrize("d,R,kernels,tile", [(4, 5, 0, None), (8, 5, 0, "0"), (5, 3, 1, None), (11, 5, 1, None), (33, 2, 2, None)])
def test_vector_mean_feedback_on_every_layout(d, R, kernels, tile, monkeypatch):
    if tile is not None:   # (d = 8 below 1 024 replicas would take the register tiles: the lane kernels' instance for 8 × 8 blocks is asked for)
        monkeypatch.setenv("RXHIP_TREE_TILE", tile)
    T = 4
    gb, n, mats = _vector_graph(d, seed=d)
    y = np.random.default_rng(100 + d).standard_normal((T, R, d))
    with TreeEngine(gb, n_replicas=R) as eng:
        assert eng.info["kernels"] == kernels
        eng.set_autoupdates(n["table"])
        out = eng.stream([n["y"]], y, iterations=1, free_energy=True, history=[n["x"]])
    ref_h, ref_fe, _ = host_loop(gb, n["table"], [n["y"]], y, 1, [n["x"]], R)
    _assert_histories_identical(out["history"], ref_h)
    assert _same(out["free_energy"], ref_fe)
    ms, V = _vector_reference(mats, y)
    hm, hv = out["history"][n["x"]]
    print(f"vector feedback d = {d}: mean err {np.max(np.abs(hm - ms)):.2e}, cov err {np.max(np.abs(hv - V)):.2e}")
    assert np.max(np.abs(hm - ms)) < 1e-9 * max(1.0, np.max(np.abs(ms))) and np.max(np.abs(hv - V)) < 1e-9 * np.max(np.abs(V))


# ---- 4. split calls ------------------------------------------------------------------------------------------------------------------------------------------
def test_two_stream_calls_equal_one():
    R = 3
    gb, names = _hgf_graph()
    y = _hgf_series(R)
    hv = [names["zt"], names["xt"]]
    res = []
    for cuts in ((0, 12), (0, 5, 12)):
        with TreeEngine(gb, n_replicas=R) as eng:
            eng.continue_runs(True)
            eng.set_autoupdates(names["autoupdates"])
            outs = [eng.stream([names["y"]], y[a:b], iterations=HGF["iters"], free_energy=True, history=hv) for a, b in zip(cuts[:-1], cuts[1:])]
            hist = {v: tuple(np.concatenate([o["history"][v][k] for o in outs]) for k in (0, 1)) for v in hv}
            res.append((hist, np.concatenate([o["free_energy"] for o in outs]), eng.marginals(hv), eng.counters(), eng.free_energy()))
    (h1, fe1, m1, c1, l1), (h2, fe2, m2, c2, l2) = res
    _assert_histories_identical(h1, h2)
    assert _same(fe1, fe2) and _same(l1, l2) and c1 == c2 and c1["rule_calls"] > 0
    _assert_histories_identical(m1, m2)


# ---- 5. where a stream starts ----------------------------------------------------------------------------------------------------------------------------------
def test_a_fresh_engine_starts_from_the_initialization_and_needs_one():
    T, R = 6, 4
    y = np.random.default_rng(2).standard_normal((T, R, 1))
    gb, n = _kalman_graph()
    with TreeEngine(gb, n_replicas=R) as eng:   # continue off: every call starts from @initialization again
        eng.set_autoupdates(n["table"])
        a = eng.stream([n["y"]], y, history=[n["x"]])
        b = eng.stream([n["y"]], y, history=[n["x"]])
        _assert_histories_identical(a["history"], b["history"])
        ms, vs = _kalman_reference(y[:, :, 0])
        assert _rel(a["history"][n["x"]][0][:, :, 0], ms) < 1e-12
        assert eng.stream([n["y"]], y[:0], history=[n["x"]])["free_energy"].shape == (0, 1)   # T = 0: a no-op
        assert _same(eng.marginals([n["x"]])[n["x"]][0], b["history"][n["x"]][0][-1])
        with pytest.raises(_lib.RxHipError) as ei:   # a target cannot be streamed as data too
            eng.stream([n["y"], n["m"]], np.zeros((T, R, 2)))
        assert ei.value.status == _lib.ERR_BADARG and f"variable {n['m']} " in str(ei.value)
    gb2, n2 = _kalman_graph(init=False)
    with TreeEngine(gb2, n_replicas=R) as eng:
        eng.set_autoupdates(n2["table"])
        with pytest.raises(_lib.RxHipError) as ei:
            eng.stream([n2["y"]], y)
        assert ei.value.status == _lib.ERR_BADARG and f"variable {n2['x']} " in str(ei.value) and "initial value" in str(ei.value)


# ---- 6. `missing` ------------------------------------------------------------------------------------------------------------------------------------------------
def test_missing_observations():
    T, R = 8, 5
    y = np.random.default_rng(9).standard_normal((T, R))
    y[3, 1] = y[3, 4] = y[4, 4] = y[0, 2] = np.nan
    gb, n = _kalman_graph()
    with TreeEngine(gb, n_replicas=R, allow_missing=True) as eng:
        eng.set_autoupdates(n["table"])
        out = eng.stream([n["y"]], y[:, :, None], history=[n["x"]])
    hm, hv = out["history"][n["x"]]
    ms, vs = _kalman_reference(y)
    assert _rel(hm[:, :, 0], ms) < 1e-12 and _rel(hv[:, :, 0, 0], vs) < 1e-12
    # the step with no observation: the posterior IS the predicted prior — the mean fed back, the variance fed back plus p
    assert hm[3, 1, 0] == pytest.approx(hm[2, 1, 0], rel=1e-12) and hv[3, 1, 0, 0] == pytest.approx(hv[2, 1, 0, 0] + KAL["p"], rel=1e-12)
    assert hm[0, 2, 0] == pytest.approx(KAL["m0"], rel=1e-12) and hv[0, 2, 0, 0] == pytest.approx(KAL["v0"] + KAL["p"], rel=1e-12)
    with TreeEngine(gb, n_replicas=R) as eng:
        eng.set_autoupdates(n["table"])
        with pytest.raises(_lib.RxHipError) as ei:
            eng.stream([n["y"]], y[:, :, None])
        assert ei.value.status == _lib.ERR_BADARG and "missing" in str(ei.value)
        out2 = eng.stream([n["y"]], np.nan_to_num(y[:, :, None]), history=[n["x"]])   # the refusal left the engine usable
        assert np.all(np.isfinite(out2["history"][n["x"]][0]))


# ---- 7. q(W) is carried from observation to observation -------------------------------------------------------------------------------------------------------
def test_a_gamma_noise_precision_is_carried_through_the_stream():
    gb = graph.GraphBuilder()
    x, tau, y = gb.randomvar(1), gb.randomvar(1), gb.datavar(1)
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, x, gb.constvar(0.5), gb.constvar(4.0))
    gb.node(_lib.NODE_GAMMA_SHAPE_RATE, tau, gb.constvar(2.0), gb.constvar(0.5))
    gb.initialize(tau, _lib.INIT_GAMMA, [2.0, 1.0])
    gb.node(_lib.NODE_NORMAL_MEAN_PRECISION, y, x, tau)
    T, R, iters = 6, 3, 3
    ys = np.random.default_rng(4).standard_normal((T, R, 1)) * 2.0
    with TreeEngine(gb, n_replicas=R) as eng:
        out = eng.stream([y], ys, iterations=iters, history=[x])
        nu, V = eng.precision(tau)
    ref_h, ref_fe, (rnu, rV) = host_loop(gb, [], [y], ys, iters, [x], R, extra=lambda e: e.precision(tau))
    assert _same(nu, rnu) and _same(V, rV)
    _assert_histories_identical(out["history"], ref_h)
    assert _same(out["free_energy"], ref_fe)
    with TreeEngine(gb, n_replicas=R) as eng:   # … and it IS carried: one observation from @initialization ends elsewhere
        eng.stream([y], ys[-1:], iterations=iters)
        assert not np.array_equal(eng.precision(tau)[0] * eng.precision(tau)[1][:, 0, 0], nu * V[:, 0, 0])


# ---- 8. clearing the table ---------------------------------------------------------------------------------------------------------------------------------------
def test_an_empty_table_streams_without_feedback():
    R, T = 3, 5
    gb, names = _hgf_graph()
    data = [v for v in range(len(gb.kind)) if gb.kind[v] == _lib.VARKIND_DATA]
    rng = np.random.default_rng(3)
    series = np.stack([[[rng.normal(), 0.5 + 2.0 * rng.random(), rng.normal(), 0.5 + 2.0 * rng.random(), rng.normal()] for _ in range(R)] for _ in range(T)])
    hv = [names["zt"], names["xt"]]
    with TreeEngine(gb, n_replicas=R) as eng:
        eng.set_autoupdates(names["autoupdates"])
        eng.set_autoupdates([])
        out = eng.stream(data, series, iterations=2, history=hv)
    ref_h, ref_fe, _ = host_loop(gb, [], data, series, 2, hv, R)
    _assert_histories_identical(out["history"], ref_h)
    assert _same(out["free_energy"], ref_fe)

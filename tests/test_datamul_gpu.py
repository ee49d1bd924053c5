"""Data matrices in `*` on the device: every replica its own regressors / design matrices (rxhip_tree_set_data), held to what the graph with that replica's
matrices as CONSTANTS computes — tests/loopy_ref.py for the reference's regression (test/models/regression/linreg_tests.jl with x and y as data),
oracle/tree_oracle.py on the constant twin (tests/datamul_graphs.py) for everything else, normal equations for the fixed point.  Tolerances: those of
tests/test_loopy_gpu.py — mean within 1e-8 posterior sd, covariance within 1e-8 of sd ⊗ sd, free energy within 1e-8 · max(1, |F|), every iteration, every
replica."""
import functools

import numpy as np
import pytest

import rxhip
from rxhip import _lib
from rxhip.graph import GraphBuilder, linreg_graph
from rxhip.tree import TreeEngine

import datamul_graphs as dg
import loopy_graphs as lg
import loopy_ref as lr
import tree_oracle

pytestmark = pytest.mark.gpu

ITERS = 25
N = 100


def _fe_close(got, want, tol=1e-8):
    return abs(got - want) <= tol * max(1.0, abs(want))


def _check(post, ref_mean, ref_cov, variables, r, what):
    for v in variables:
        V = np.atleast_2d(ref_cov[v])
        sd = np.sqrt(np.diag(V))
        assert np.max(np.abs(post[v][0][r] - np.ravel(ref_mean[v])) / sd) < 1e-8, (what, r, v, "mean")
        assert np.max(np.abs(post[v][1][r] - V) / np.outer(sd, sd)) < 1e-8, (what, r, v, "cov")


def _replica(r):
    """regressors and observations of replica r: replica 0 the reference's own data, the others x = 1:N + randn, y = 10 − 10 x + randn"""
    if r == 0:
        return lg.reference_data(N)
    rng = np.random.default_rng(100 + r)
    x = np.arange(1, N + 1, dtype=float) + rng.normal(size=N)
    return x, 10.0 - 10.0 * x + rng.normal(size=N)


@functools.lru_cache(maxsize=None)
def _ref(r, iterations=ITERS, cut="b", init=(0.0, 100.0)):
    x, y = _replica(r)
    return lr.linreg_loopy(x, y, iterations, cut=cut, init=init)


def _rows(R):
    """set_data rows of R replicas for (ys, xs): [R][N | N]"""
    xy = [_replica(r) for r in range(R)]
    return np.stack([np.concatenate([y, x]) for x, y in xy])


# ---- 1. the reference model --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [None, "0", "1", "2", "3"])
@pytest.mark.parametrize("R", [1, 3, 64, 70])
def test_the_reference_regression_every_iteration_every_replica(R, mode, monkeypatch):
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    gb, ys, xs, nm = linreg_graph(N, init={"b": (0.0, 100.0)}, x_as_data=True)
    refs = [_ref(r) for r in range(R)]
    eng = TreeEngine(gb, n_replicas=R)
    assert eng.info["n_loop_messages"] == N
    eng.set_data(ys + xs, _rows(R))
    for it in range(1, ITERS + 1):
        eng.run(it, True)
        post = eng.marginals([nm["a"], nm["b"]])
        fe_rep = eng.free_energy_per_replica()
        for r in range(R):
            for k in ("a", "b"):
                m, v = refs[r][it - 1][k]
                assert abs(post[nm[k]][0][r, 0] - m) < 1e-8 * np.sqrt(v), (it, r, k)
                assert abs(post[nm[k]][1][r, 0, 0] - v) < 1e-8 * v, (it, r, k)
            assert _fe_close(fe_rep[r], refs[r][it - 1]["fe"]), (it, r, fe_rep[r], refs[r][it - 1]["fe"])
    fe = eng.free_energy()
    assert np.allclose(fe, [sum(refs[r][i]["fe"] for r in range(R)) for i in range(ITERS)], rtol=1e-8)
    assert np.all(np.isfinite(fe)) and fe[-1] < fe[1]   # the reference's `fe[end] < fe[2]`
    fe_rep = eng.free_energy_per_replica()
    assert all(refs[r][-1]["fe"] < refs[r][1]["fe"] for r in range(R)) and all(_fe_close(fe_rep[r], refs[r][-1]["fe"]) for r in range(R))
    post = eng.marginals([nm["a"], nm["b"]])
    assert abs(post[nm["a"]][0][0, 0] - 10.0) < 5.0 and abs(post[nm["b"]][0][0, 0] + 10.0) < 0.1   # the reference test's own bars, on its own data
    eng.close()


@pytest.mark.parametrize("cut,D", [("a", (3.0, 50.0)), ("b", (-2.0, 7.0))])
def test_both_cuts_with_a_non_zero_mean_initialisation(cut, D):
    R = 8
    gb, ys, xs, nm = linreg_graph(N, init={cut: D}, x_as_data=True)
    refs = [_ref(r, 10, cut, D) for r in range(R)]
    eng = TreeEngine(gb, n_replicas=R)
    assert eng.info["n_loop_messages"] == N
    eng.set_data(ys + xs, _rows(R))
    for it in range(1, 11):
        eng.run(it, True)
        post = eng.marginals([nm["a"], nm["b"]])
        fe_rep = eng.free_energy_per_replica()
        for r in range(R):
            for k in ("a", "b"):
                m, v = refs[r][it - 1][k]
                assert abs(post[nm[k]][0][r, 0] - m) < 1e-8 * np.sqrt(v), (it, r, k)
                assert abs(post[nm[k]][1][r, 0, 0] - v) < 1e-8 * v, (it, r, k)
            assert _fe_close(fe_rep[r], refs[r][it - 1]["fe"]), (it, r)
    eng.close()


# ---- 2. the fixed point ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cut", ["a", "b"])
def test_every_replica_converges_to_its_own_normal_equations(cut):
    R = 8
    gb, ys, xs, nm = linreg_graph(N, init={cut: (0.0, 100.0)}, x_as_data=True)
    eng = TreeEngine(gb, n_replicas=R)
    eng.set_data(ys + xs, _rows(R))
    eng.run(400, False)
    post = eng.marginals([nm["a"], nm["b"]])
    for r in range(R):
        m, S = lr.exact_linreg(*_replica(r))
        assert abs(post[nm["a"]][0][r, 0] - m[0]) < 1e-9 * np.sqrt(S[0, 0]), (r, "a")
        assert abs(post[nm["b"]][0][r, 0] - m[1]) < 1e-9 * np.sqrt(S[1, 1]), (r, "b")
    eng.close()


# ---- 3. every kernel family --------------------------------------------------------------------------------------------------------------------------

VEC_ITERS = 6
FAMILIES = [(2, None, 0), (4, None, 0), (5, "0", 0), (5, "1", 1), (8, "0", 0), (12, None, 1), (20, None, 1), (33, None, 2), (64, None, 2)]


def _vector_case(d, cut):
    Nv = 12
    X, pa, pb, S, D, Y = lg.vector_problem(Nv, d, seed=d)
    R = Y.shape[0]
    rng = np.random.default_rng(1000 + d)
    Xr = [X + 0.05 * rng.normal(size=X.shape) for _ in range(R)]
    gb, ys, xs, nm = linreg_graph(Nv, d=d, dy=d, prior_a=pa, prior_b=pb, noise_var=S, init={cut: D}, x_as_data=True)
    rows = np.concatenate([Y.reshape(R, -1), np.stack([x.reshape(-1) for x in Xr])], axis=1)
    return gb, ys, xs, nm, Xr, Y, rows


def _oracle_iterations(twin, data, iterations):
    """the oracle's posteriors and free energy after every iteration (one iteration per call, the loop messages carried)"""
    out, state = [], None
    for _ in range(iterations):
        ref = tree_oracle.infer(twin, data, 1, loop_state=state)
        state = ref["loop_state"]
        out.append(ref)
    return out


@pytest.mark.parametrize("d,tile,kernels", FAMILIES)
@pytest.mark.parametrize("cut", ["a", "b"])
def test_vector_regression_with_per_replica_maps_on_every_kernel_family(d, tile, kernels, cut, monkeypatch):
    if tile is not None:
        monkeypatch.setenv("RXHIP_TREE_TILE", tile)
    gb, ys, xs, nm, Xr, Y, rows = _vector_case(d, cut)
    R = Y.shape[0]
    dump = gb.to_dump()
    refs = [_oracle_iterations(dg.const_twin(dump, dict(zip(xs, Xr[r]))), {y: Y[r, i] for i, y in enumerate(ys)}, VEC_ITERS) for r in range(R)]
    eng = TreeEngine(gb, n_replicas=R)
    assert eng.info["n_loop_messages"] == len(ys)
    assert eng.info["kernels"] == kernels
    eng.set_data(ys + xs, rows)
    for it in range(1, VEC_ITERS + 1):
        eng.run(it, True)
        post = eng.marginals([nm["a"], nm["b"]])
        fe_rep = eng.free_energy_per_replica()
        for r in range(R):
            ref = refs[r][it - 1]
            _check(post, ref["mean"], ref["cov"], [nm["a"], nm["b"]], r, (d, it))
            assert _fe_close(fe_rep[r], ref["fe"][0]), (it, r, fe_rep[r], ref["fe"][0])
    eng.close()


# ---- 4. forests ----------------------------------------------------------------------------------------------------------------------------------------

FORESTS = [("a", dg.chain_obs_maps, dict(T=5, d=3, dy=2)), ("a", dg.chain_obs_maps, dict(T=4, d=20, dy=7)), ("a", dg.chain_obs_maps, dict(T=3, d=40, dy=40)),
           ("b", dg.two_maps, dict(d=4, du=3, dw=2)), ("b", dg.two_maps, dict(d=12, du=9, dw=5)), ("b", dg.two_maps, dict(d=40, du=33, dw=20)),
           ("c", dg.derived_product, dict(d=3, du=2)), ("c", dg.derived_product, dict(d=12, du=5)), ("c", dg.derived_product, dict(d=40, du=20)),
           ("d", dg.square_and_flat, dict(d=4, r=2)), ("d", dg.square_and_flat, dict(d=12, r=5)), ("d", dg.square_and_flat, dict(d=36, r=10)),
           ("e", dg.dot_rows, dict(N=6, d=4)), ("e", dg.dot_rows, dict(N=6, d=12))]
SMALL = [c for c in FORESTS if max(v for k, v in c[2].items() if k not in ("T", "N")) <= 4]


def _forest(builder, kw, R, allow_missing=False, miss=None, engine_kw=None):
    gb, ys, mats, gauss, nominal = builder(x_as_data=True, **kw)
    Y, Ms = dg.draw(gb, ys, nominal, R, seed=17)
    if miss is not None:
        Y = np.where(np.random.default_rng(3).random(Y.shape) < miss, np.nan, Y)
    eng = TreeEngine(gb, n_replicas=R, allow_missing=allow_missing, **(engine_kw or {}))
    eng.set_data(ys + mats, dg.rows_of(Y, Ms))
    eng.run(1, True)
    post, fe = eng.marginals(gauss), eng.free_energy_per_replica()
    dump = gb.to_dump()
    for r in range(R):
        ref = tree_oracle.infer(dg.const_twin(dump, dict(zip(mats, Ms[r]))), dg.data_dict(gb, ys, Y[r]))
        _check(post, ref["mean"], ref["cov"], gauss, r, (builder.__name__, kw))
        assert _fe_close(fe[r], ref["fe"][0]), (builder.__name__, kw, r, fe[r], ref["fe"][0])
    return eng, (gb, ys, mats, gauss, nominal, Y, Ms)


@pytest.mark.parametrize("item,builder,kw", FORESTS)
def test_forests_against_the_oracle_on_the_constant_twin(item, builder, kw):
    _forest(builder, kw, R=5)[0].close()


@pytest.mark.parametrize("mode", ["0", "1", "2", "3"])
@pytest.mark.parametrize("item,builder,kw", SMALL)
def test_small_forests_under_every_schedule(item, builder, kw, mode, monkeypatch):
    monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    _forest(builder, kw, R=19)[0].close()


@pytest.mark.parametrize("tile", ["0", "1"])
def test_a_five_to_eight_dimensional_forest_on_both_kernel_families(tile, monkeypatch):
    monkeypatch.setenv("RXHIP_TREE_TILE", tile)
    eng, _ = _forest(dg.chain_obs_maps, dict(T=4, d=7, dy=5), R=5)
    assert eng.info["kernels"] == int(tile)
    eng.close()


def test_rxhip_create_falls_through_to_the_executor():
    eng, _ = _forest(dg.chain_obs_maps, dict(T=5, d=3, dy=2), R=3, engine_kw=dict(force_executor=False))
    assert eng.info["n_ops"] > 0
    eng.close()


# ---- 5. the data-matrix engine against the constant-twin engine on the device ------------------------------------------------------------------------

def _engines_agree(gb, vector_vars, matrix_vars, row, mats, variables, iterations):
    """one replica: the engine with data matrices and the engine of its constant twin (the loads differ: tolerances, not bits)"""
    twin = GraphBuilder.from_dump(dg.const_twin(gb.to_dump(), dict(zip(matrix_vars, mats))))
    nvec = int(sum(gb.rows[v] for v in vector_vars))
    with TreeEngine(gb, n_replicas=1) as e1, TreeEngine(twin, n_replicas=1) as e2:
        assert e1.info["kernels"] == e2.info["kernels"] and e1.info["n_ops"] == e2.info["n_ops"]
        e1.set_data(vector_vars + matrix_vars, row.reshape(1, -1))
        e2.set_data(vector_vars, row[:nvec].reshape(1, -1))
        for it in range(1, iterations + 1):
            e1.run(it, True)
            e2.run(it, True)
            p1, p2 = e1.marginals(variables), e2.marginals(variables)
            _check(p1, {v: p2[v][0][0] for v in variables}, {v: p2[v][1][0] for v in variables}, variables, 0, it)
            assert _fe_close(e1.free_energy_per_replica()[0], e2.free_energy_per_replica()[0]), it


def test_engines_agree_on_the_reference_regression():
    gb, ys, xs, nm = linreg_graph(N, init={"b": (0.0, 100.0)}, x_as_data=True)
    x, _ = _replica(0)
    _engines_agree(gb, ys, xs, _rows(1)[0], list(x.reshape(N, 1, 1)), [nm["a"], nm["b"]], 10)


@pytest.mark.parametrize("d,tile,kernels", [(4, None, 0), (5, "1", 1), (20, None, 1), (33, None, 2)])
def test_engines_agree_on_the_vector_regression(d, tile, kernels, monkeypatch):
    if tile is not None:
        monkeypatch.setenv("RXHIP_TREE_TILE", tile)
    gb, ys, xs, nm, Xr, Y, rows = _vector_case(d, "b")
    _engines_agree(gb, ys, xs, rows[1], list(Xr[1]), [nm["a"], nm["b"]], VEC_ITERS)


@pytest.mark.parametrize("kw", [dict(T=5, d=3, dy=2), dict(T=4, d=20, dy=7), dict(T=3, d=40, dy=40)])
def test_engines_agree_on_the_chain_with_data_observation_maps(kw):
    gb, ys, mats, gauss, nominal = dg.chain_obs_maps(x_as_data=True, **kw)
    Y, Ms = dg.draw(gb, ys, nominal, 1, seed=23)
    _engines_agree(gb, ys, mats, dg.rows_of(Y, Ms)[0], Ms[0], gauss, 1)


# ---- 6. data policy ------------------------------------------------------------------------------------------------------------------------------------

def test_new_matrices_give_the_new_answer():
    eng, (gb, ys, mats, gauss, nominal, Y, Ms) = _forest(dg.chain_obs_maps, dict(T=5, d=3, dy=2), R=5)
    before = eng.marginals(gauss)
    Y2, Ms2 = dg.draw(gb, ys, nominal, 5, seed=99, scale=0.3)
    eng.set_data(mats, np.stack([np.concatenate([M.ravel() for M in ms]) for ms in Ms2]))   # the matrices alone: the observations stay
    eng.run(1, True)
    post, fe = eng.marginals(gauss), eng.free_energy_per_replica()
    dump = gb.to_dump()
    for r in range(5):
        ref = tree_oracle.infer(dg.const_twin(dump, dict(zip(mats, Ms2[r]))), dg.data_dict(gb, ys, Y[r]))
        _check(post, ref["mean"], ref["cov"], gauss, r, "second set_data")
        assert _fe_close(fe[r], ref["fe"][0]), r
    assert max(np.max(np.abs(post[v][0] - before[v][0])) for v in gauss) > 1e-3   # (and it is a different answer)
    eng.close()


@pytest.mark.parametrize("allow_missing", [False, True])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_matrix_entry_is_refused(allow_missing, bad):
    gb, ys, mats, gauss, nominal = dg.chain_obs_maps(T=3, d=3, dy=2, x_as_data=True)
    Y, Ms = dg.draw(gb, ys, nominal, 4, seed=5)
    with TreeEngine(gb, n_replicas=4, allow_missing=allow_missing) as eng:
        rows = dg.rows_of(Y, Ms)
        rows[2, -1] = bad
        with pytest.raises(rxhip.RxHipError) as ei:
            eng.set_data(ys + mats, rows)
        assert ei.value.status == _lib.ERR_BADARG and "matrix" in str(ei.value)
        if allow_missing:   # NaN in the vector data of the same call is fine; in the matrix it is not
            rows = dg.rows_of(Y, Ms)
            rows[1, 0] = np.nan
            eng.set_data(ys + mats, rows)
            rows[1, -2] = np.nan
            with pytest.raises(rxhip.RxHipError) as ei:
                eng.set_data(ys + mats, rows)
            assert ei.value.status == _lib.ERR_BADARG


@pytest.mark.parametrize("kw", [dict(T=6, d=3, dy=2), dict(T=4, d=12, dy=5)])
def test_missing_observations_next_to_data_matrices(kw):
    _forest(dg.chain_obs_maps, kw, R=5, allow_missing=True, miss=0.3)[0].close()

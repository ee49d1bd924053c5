"""The loopy schedule on the device: the reference's linear regression (test/models/regression/linreg_tests.jl) with `μ(b)` against the numpy
restatement of the schedule (loopy_ref.py) after every iteration, under every sweep schedule; its fixed point against exact conditioning; continued runs
bit for bit one run; an initialisation on a forest changes no bit."""
import numpy as np
import pytest

from rxhip import _lib
from rxhip.tree import TreeEngine

import loopy_graphs as lg
import loopy_ref as lr
import tree_graphs as tg

pytestmark = pytest.mark.gpu

ITERS = 25


def _data(R, N=100):
    x, y = lg.reference_data(N)
    rng = np.random.default_rng(5)
    Y = np.stack([y if r == 0 else y + rng.normal(0.0, 1.0, N) for r in range(R)])
    return x, Y


def _run(gb, ys, Y, iterations, free_energy=True):
    eng = TreeEngine(gb, n_replicas=Y.shape[0])
    eng.set_data(ys, Y)
    eng.run(iterations, free_energy)
    return eng


def _fe_close(got, want, tol=1e-8):
    return abs(got - want) <= tol * max(1.0, abs(want))


@pytest.mark.parametrize("mode", [None, "0", "1", "2", "3"])
@pytest.mark.parametrize("R", [1, 64])
def test_linreg_every_iteration_against_the_restatement(R, mode, monkeypatch):
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    x, Y = _data(R)
    gb, ys, nm = lg.linreg(x, init={"b": (0.0, 100.0)})
    refs = [lr.linreg_loopy(x, Y[r], ITERS) for r in range(R)]
    eng = TreeEngine(gb, n_replicas=R)
    assert eng.info["n_loop_messages"] == len(x)
    eng.set_data(ys, Y)
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
    post = eng.marginals([nm["a"], nm["b"]])
    assert abs(post[nm["a"]][0][0, 0] - 10.0) < 5.0 and abs(post[nm["b"]][0][0, 0] + 10.0) < 0.1
    eng.close()


@pytest.mark.parametrize("cut,D", [("a", (3.0, 50.0)), ("b", (-2.0, 7.0))])
def test_a_non_trivial_initialisation_every_iteration(cut, D):
    """the loop messages of `μ(a)` come out of `+` (its own message form), those of `μ(b)` out of `*`: D with a non-zero mean must arrive in either form"""
    x, Y = _data(8)
    gb, ys, nm = lg.linreg(x, init={cut: D})
    refs = [lr.linreg_loopy(x, Y[r], 10, cut=cut, init=D) for r in range(8)]
    eng = TreeEngine(gb, n_replicas=8)
    eng.set_data(ys, Y)
    for it in range(1, 11):
        eng.run(it, True)
        post = eng.marginals([nm["a"], nm["b"]])
        fe_rep = eng.free_energy_per_replica()
        for r in range(8):
            for k in ("a", "b"):
                m, v = refs[r][it - 1][k]
                assert abs(post[nm[k]][0][r, 0] - m) < 1e-8 * np.sqrt(v), (it, r, k)
                assert abs(post[nm[k]][1][r, 0, 0] - v) < 1e-8 * v, (it, r, k)
            assert _fe_close(fe_rep[r], refs[r][it - 1]["fe"]), (it, r)
    eng.close()


VEC_ITERS = 6


@pytest.mark.parametrize("d,tile", [(2, None), (4, None), (5, "0"), (5, "1"), (8, "0"), (12, None), (20, None), (33, None), (64, None)])
@pytest.mark.parametrize("cut", ["a", "b"])
def test_vector_regression_every_iteration_on_every_kernel_family(d, tile, cut, monkeypatch):
    """y[i] ~ MvNormal(X[i] * b + a, Σ), d-dimensional: the loop messages (and D, with a non-zero mean and a correlated covariance) as d-vectors on the
    lane-per-item kernels, the register-tile kernels (RXHIP_TREE_TILE, 5 … 32) and the LDS-staged ones (33 … 64)"""
    if tile is not None:
        monkeypatch.setenv("RXHIP_TREE_TILE", tile)
    N = 12
    X, pa, pb, S, D, Y = lg.vector_problem(N, d, seed=d)
    gb, ys, nm = lg.linreg(X, pa, pb, S, init={cut: D})
    R = Y.shape[0]
    refs = [lr.linreg_loopy(X, Y[r], VEC_ITERS, cut=cut, init=D, prior_a=pa, prior_b=pb, noise_var=S) for r in range(R)]
    eng = TreeEngine(gb, n_replicas=R)
    assert eng.info["n_loop_messages"] == N
    if tile == "1" or d > 8:
        assert eng.info["kernels"] != 0
    if tile == "0" or d <= 4:
        assert eng.info["kernels"] == 0
    eng.set_data(ys, Y.reshape(R, -1))
    for it in range(1, VEC_ITERS + 1):
        eng.run(it, True)
        post = eng.marginals([nm["a"], nm["b"]])
        fe_rep = eng.free_energy_per_replica()
        for r in range(R):
            for k in ("a", "b"):
                m, V = refs[r][it - 1][k]
                sd = np.sqrt(np.diag(V))
                assert np.max(np.abs(post[nm[k]][0][r] - m) / sd) < 1e-8, (it, r, k)
                assert np.max(np.abs(post[nm[k]][1][r] - V) / np.outer(sd, sd)) < 1e-8, (it, r, k)
            assert _fe_close(fe_rep[r], refs[r][it - 1]["fe"]), (it, r, fe_rep[r], refs[r][it - 1]["fe"])
    eng.close()


@pytest.mark.parametrize("cut", ["a", "b"])
def test_linreg_converges_to_exact_conditioning(cut):
    x, Y = _data(4)
    gb, ys, nm = lg.linreg(x, init={cut: (0.0, 100.0)})
    eng = _run(gb, ys, Y, 400, free_energy=False)
    post = eng.marginals([nm["a"], nm["b"]])
    for r in range(Y.shape[0]):
        m, _ = lr.exact_linreg(x, Y[r])
        assert abs(post[nm["a"]][0][r, 0] - m[0]) < 1e-9 * abs(m[0])
        assert abs(post[nm["b"]][0][r, 0] - m[1]) < 1e-9 * abs(m[1])
    eng.close()


@pytest.mark.parametrize("mode", [None, "0"])
def test_ten_continued_runs_are_one_run_of_ten(mode, monkeypatch):
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    x, Y = _data(16)
    gb, ys, nm = lg.linreg(x, init={"b": (0.0, 100.0)})
    one = _run(gb, ys, Y, 10)
    ref = one.marginals([nm["a"], nm["b"]])
    fe_ref = one.free_energy_per_replica()
    one.close()
    eng = TreeEngine(gb, n_replicas=16)
    eng.set_data(ys, Y)
    eng.continue_runs(True)
    for _ in range(10):
        eng.run(1, True)
    got = eng.marginals([nm["a"], nm["b"]])
    for v in ref:
        assert np.array_equal(got[v][0], ref[v][0]) and np.array_equal(got[v][1], ref[v][1])
    assert np.array_equal(eng.free_energy_per_replica(), fe_ref)
    eng.close()


@pytest.mark.parametrize("seed,tile", [(0, None), (1, None), (2, "1"), (3, None), (4, "0")])
def test_an_initialisation_on_a_forest_changes_no_bit(seed, tile, monkeypatch):
    if tile is not None:
        monkeypatch.setenv("RXHIP_TREE_TILE", tile)
    gb, ys, named = tg.random_forest(seed, n_steps=10, dmax=(1, 2, 4, 8, 12)[seed])
    data = tg.random_data(gb, ys, 8, seed)
    gauss = [v for v in range(len(gb.kind)) if gb.kind[v] == _lib.VARKIND_RANDOM and v not in named.get("W", [])]
    e0 = _run(gb, ys, data, 3)
    m0, fe0 = e0.marginals(gauss), e0.free_energy()
    e0.close()
    v = gauss[0]
    d = gb.rows[v]
    gb.initialize_message(v, _lib.INIT_MVNORMAL, np.concatenate([np.ones(d), 3.0 * np.eye(d).ravel()]))
    e1 = _run(gb, ys, data, 3)
    assert e1.info["n_loop_messages"] == 0
    m1, fe1 = e1.marginals(gauss), e1.free_energy()
    e1.close()
    for w in gauss:
        assert np.array_equal(m0[w][0], m1[w][0]) and np.array_equal(m0[w][1], m1[w][1])
    assert np.array_equal(fe0, fe1)

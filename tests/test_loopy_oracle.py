"""The generic restatement of the loopy schedule (oracle/tree_oracle.py infer with message initialisations, include/rxhip.h "Loopy graphs") against the
hand-written one of the linear regression (loopy_ref.py) at every iteration, against itself without the initialisation on forests, and at its fixed point
against brute-force conditioning (Weiss & Freeman 2001: the converged means of Gaussian BP are exact) on the random loopy graphs of loopy_graphs.py."""
import numpy as np
import pytest

import loopy_graphs as lg
import loopy_ref as lr
import tree_graphs as tg
import tree_oracle

# the random loopy graphs the GPU tests run (tests/test_loopy_random_gpu.py): every one must converge
GPU_GRAPHS = lg.GPU_GRAPHS


def _infer_runs(gb, data, iterations):
    """one restatement run of `iterations`, as `iterations` one-iteration runs that carry the loop messages"""
    st, out = None, []
    for _ in range(iterations):
        o = tree_oracle.infer(gb.to_dump(), data, 1, loop_state=st)
        st = o["loop_state"]
        out.append(o)
    return out


@pytest.mark.parametrize("cut", ["a", "b"])
@pytest.mark.parametrize("d", [1, 2, 5])
def test_the_generic_restatement_is_the_linreg_restatement(d, cut):
    """every iteration: means, covariances and the node-local free energy to 1e-12, scalar and vector regressions, either cut"""
    if d == 1:
        x, y = lg.reference_data(24)
        D = (2.0, 40.0)
        gb, ys, nm = lg.linreg(x, init={cut: D})
        refs = lr.linreg_loopy(x, y, 12, cut=cut, init=D)
        data = {v: [yi] for v, yi in zip(ys, y)}
    else:
        X, pa, pb, S, D, Y = lg.vector_problem(10, d, seed=d)
        gb, ys, nm = lg.linreg(X, pa, pb, S, init={cut: D})
        refs = lr.linreg_loopy(X, Y[1], 12, cut=cut, init=D, prior_a=pa, prior_b=pb, noise_var=S)
        data = {v: Y[1][i] for i, v in enumerate(ys)}
    whole = tree_oracle.infer(gb.to_dump(), data, 12)
    assert len(whole["loop_state"]) == len(ys)
    for it, o in enumerate(_infer_runs(gb, data, 12)):
        for k in ("a", "b"):
            m, V = (np.atleast_1d(a) for a in refs[it][k])
            V = V.reshape(len(m), len(m))
            sd = np.sqrt(np.diag(V))
            assert np.max(np.abs(o["mean"][nm[k]] - m) / sd) < 1e-12, (it, k)
            assert np.max(np.abs(o["cov"][nm[k]] - V) / np.outer(sd, sd)) < 1e-12, (it, k)
        assert abs(o["fe"][0] - refs[it]["fe"]) < 1e-12 * abs(refs[it]["fe"]), it
        assert abs(whole["fe"][it] - refs[it]["fe"]) < 1e-12 * abs(refs[it]["fe"]), it
    for v in whole["mean"]:   # (a continued run of one iteration at a time is the run)
        assert np.array_equal(whole["mean"][v], o["mean"][v]) and np.array_equal(whole["cov"][v], o["cov"][v])


@pytest.mark.parametrize("seed", range(8))
def test_an_initialisation_on_a_forest_changes_no_bit_of_the_restatement(seed):
    gb, ys, named = tg.random_forest(seed, n_steps=10, dmax=(1, 2, 4, 8, 12, 20, 5, 3)[seed])
    data = tg.data_dict(gb, ys, tg.random_data(gb, ys, 1, seed)[0])
    r0 = tree_oracle.infer(gb.to_dump(), data, 3)
    g = tree_oracle.TreeGraph(gb.to_dump())
    rng = np.random.default_rng(seed)
    lg.initialise(gb, rng, [v for v in range(len(gb.kind)) if g.gauss[v]][:3])
    r1 = tree_oracle.infer(gb.to_dump(), data, 3)
    assert r1["loop_state"] == {}
    for v in r0["mean"]:
        assert np.array_equal(r0["mean"][v], r1["mean"][v]) and np.array_equal(r0["cov"][v], r1["cov"][v])
    assert r0["fe"] == r1["fe"]


def _converge(gb, data, gv, budget=400, tol=1e-13):
    st, prev = None, None
    for it in range(budget):
        o = tree_oracle.infer(gb.to_dump(), data, 1, loop_state=st)
        st = o["loop_state"]
        cur = np.concatenate([o["mean"][v] / np.sqrt(np.diag(o["cov"][v])) for v in gv])
        if prev is not None and np.max(np.abs(cur - prev)) < tol:
            return o, it + 1
        prev = cur
    return o, None


@pytest.mark.parametrize("kind,seed", GPU_GRAPHS)
def test_the_restatement_converges_to_exact_conditioning(kind, seed):
    """every random loopy graph the GPU tests use: the restatement converges within its budget, and its means are brute-force conditioning to 1e-9 sd"""
    gb, ys, named, _ = lg.random_loopy(seed, kind)
    data = tg.data_dict(gb, ys, tg.random_data(gb, ys, 1, seed)[0])
    o, its = _converge(gb, data, named["x"])
    assert its is not None, "the generator drew a graph on which loopy BP does not converge"
    bf, _ = tg.brute_force(gb, data)
    for v in named["x"]:
        sd = np.sqrt(np.diag(bf[v][1]))
        assert np.max(np.abs(o["mean"][v] - bf[v][0]) / sd) < 1e-9, v


def test_the_bridge_finder():
    """a ring of three with a pendant: the ring's edges lie on a cycle, the pendant's do not; a second, parallel edge between one pair closes a cycle"""
    E = [(("f", 0), 0, "a"), (("f", 0), 1, "b"), (("f", 1), 1, "c"), (("f", 1), 2, "d"), (("f", 2), 2, "e"), (("f", 2), 0, "f"), (("f", 3), 2, "g"), (("f", 3), 3, "h")]
    assert tree_oracle.cycle_edges(E) == set("abcdef")
    assert tree_oracle.cycle_edges(E + [(("f", 4), 3, "i"), (("f", 4), 3, "j")]) == set("abcdefij")
    assert tree_oracle.cycle_edges(E[:5]) == set()

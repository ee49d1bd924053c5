"""The numpy restatement of the loopy schedule (loopy_ref.py) on the reference's linear regression: its fixed point is exact conditioning, and after 25
iterations it passes the reference's own assertions (test/models/regression/linreg_tests.jl)."""
import numpy as np
import pytest

import loopy_graphs as lg
import loopy_ref as lr


@pytest.mark.parametrize("cut", ["a", "b"])
def test_the_converged_means_are_exact(cut):
    x, y = lg.reference_data()
    post = lr.linreg_loopy(x, y, 400, cut=cut)[-1]
    m, _ = lr.exact_linreg(x, y)
    assert abs(post["a"][0] - m[0]) < 1e-9 * abs(m[0])
    assert abs(post["b"][0] - m[1]) < 1e-9 * abs(m[1])


def test_centred_inputs_converge_too():
    x, y = lg.reference_data()
    xc = x - x.mean()
    post = lr.linreg_loopy(xc, y, 200)[-1]
    m, _ = lr.exact_linreg(xc, y)
    assert np.allclose([post["a"][0], post["b"][0]], m, rtol=1e-9)


def test_the_references_assertions_after_25_iterations():
    x, y = lg.reference_data()
    post = lr.linreg_loopy(x, y, 25)[-1]
    assert abs(post["a"][0] - 10.0) < 5.0
    assert abs(post["b"][0] + 10.0) < 0.1


def test_the_exact_posterior_is_brute_force_conditioning():
    """exact_linreg against tests/tree_graphs.py::brute_force on the same graph"""
    import tree_graphs as tg
    x, y = lg.reference_data(20)
    y = y + np.sin(np.arange(20))
    gb, ys, nm = lg.linreg(x)
    bf, _ = tg.brute_force(gb, {v: [yi] for v, yi in zip(ys, y)})
    m, S = lr.exact_linreg(x, y)
    assert np.allclose([bf[nm["a"]][0][0], bf[nm["b"]][0][0]], m, rtol=1e-10)
    assert np.allclose([bf[nm["a"]][1][0, 0], bf[nm["b"]][1][0, 0]], np.diag(S), rtol=1e-10)


@pytest.mark.parametrize("d,cut", [(1, "b"), (2, "a"), (2, "b"), (5, "a"), (5, "b")])
def test_the_free_energy_is_minus_the_log_evidence_on_a_tree(d, cut):
    """one observation: the graph is a tree, and the first iteration of the restatement — its b → mul message is the prior alone — is exact BP, whose
    Bethe free energy is −log evidence: the node-local sum of loopy_ref against tests/tree_graphs.py::brute_force"""
    import tree_graphs as tg
    if d == 1:
        X, pa, pb, S, D, Y = np.array([2.5]), (0.0, 1.0), (0.0, 1.0), 1.0, (0.0, 100.0), np.array([[1.3]])
        gb, ys, nm = lg.linreg(X)
        data = {ys[0]: [1.3]}
    else:
        X, pa, pb, S, D, Y = lg.vector_problem(1, d, seed=3)
        Y = Y[0]
        gb, ys, nm = lg.linreg(X, pa, pb, S)
        data = {ys[0]: Y[0]}
    post, nle = tg.brute_force(gb, data)
    r = lr.linreg_loopy(X, Y, 1, cut=cut, init=D, prior_a=pa, prior_b=pb, noise_var=S)[0]
    assert r["fe"] == pytest.approx(nle, rel=1e-12)
    assert np.allclose(np.ravel(r["a"][0]), post[nm["a"]][0], rtol=1e-12, atol=1e-12)

"""Data matrices in `*` in the graph compiler (rxhip_tree_plan, no device): the reference's linear regression with x AND y as data
(test/models/regression/linreg_tests.jl) is accepted and scheduled exactly as its constant-x twin, the matrix reads are counted, what stays refused, and
a graph without a data matrix plans to the figures it had before data matrices existed."""
import numpy as np
import pytest

import rxhip
from rxhip import _lib
from rxhip.graph import GraphBuilder, linreg_graph
from rxhip.tree import plan

import datamul_graphs as dg
import loopy_graphs as lg
import tree_graphs as tg

SAME = ("rule_calls", "products", "marginals", "n_ops", "n_levels", "n_strands", "n_strand_levels", "longest_strand", "n_messages", "n_loop_messages", "dmax")


def _pair(N, d, **kw):
    """(data-x graph, constant-x twin, Σ rows·cols of the data matrices)"""
    if d == 1:
        x, _ = lg.reference_data(N)
        con = linreg_graph(N, x=x, x_as_data=False, **kw)
        dat = linreg_graph(N, x_as_data=True, **kw)
        return dat, con, N
    X, pa, pb, S, D, _ = lg.vector_problem(N, d, seed=d)
    init = {kw["cut"]: D} if kw.get("cut") else None
    con = linreg_graph(N, x=X, prior_a=pa, prior_b=pb, noise_var=S, init=init, x_as_data=False)
    dat = linreg_graph(N, d=d, dy=d, prior_a=pa, prior_b=pb, noise_var=S, init=init, x_as_data=True)
    return dat, con, N * d * d


def test_the_reference_regression_with_x_as_data_plans_as_its_constant_twin():
    dat, con, _ = _pair(100, 1, init={"b": (0.0, 100.0)})
    p, q = plan(dat[0]), plan(con[0])
    assert p["n_loop_messages"] == 100
    for k in SAME:
        assert p[k] == q[k], k
    assert len(dat[2]) == 100 and con[2] == []


@pytest.mark.parametrize("d", [2, 5, 12, 33, 64])
@pytest.mark.parametrize("cut", ["a", "b"])
def test_the_vector_regression_plans_as_its_constant_twin(d, cut):
    dat, con, _ = _pair(12, d, cut=cut)
    p, q = plan(dat[0]), plan(con[0])
    assert p["n_loop_messages"] == 12
    for k in SAME:
        assert p[k] == q[k], k


def test_without_an_initialisation_it_is_still_refused_with_cycle():
    gb = linreg_graph(30, x_as_data=True)[0]
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "cycle" in str(ei.value)


def _mul_graph(matrix_var):
    """x ~ N(0, I₂), y ~ N(M x, I) with M made by matrix_var(builder)"""
    gb = GraphBuilder()
    x = gb.randomvar(2)
    gb.mvnormal_mean_cov(x, gb.constvar(np.zeros(2)), gb.constvar(np.eye(2)))
    o = gb.randomvar(3)
    gb.node(_lib.NODE_MULTIPLY, o, matrix_var(gb), x)
    gb.mvnormal_mean_cov(gb.datavar(3), o, gb.constvar(np.eye(3)))
    return gb


def test_refusals():
    assert plan(_mul_graph(lambda gb: gb.datavar(3, cols=2)))["n_ops"] > 0
    # a random matrix
    def random_matrix(gb):
        a = gb.randomvar(3)
        gb.mvnormal_mean_cov(a, gb.constvar(np.zeros(3)), gb.constvar(np.eye(3)))
        return a
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(_mul_graph(random_matrix))
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    # a data matrix of the wrong shape: too few values, the right count in the wrong shape, a vector
    for rows, cols in ((2, 2), (2, 3), (6, 1), (3, 1)):
        with pytest.raises(rxhip.RxHipError) as ei:
            plan(_mul_graph(lambda gb: gb.datavar(rows, cols=cols)))
        assert ei.value.status == _lib.ERR_BADARG, (rows, cols)
    # the matrix variable read as a value somewhere else
    gb = GraphBuilder()
    x = gb.randomvar(1)
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, x, gb.constvar(0.0), gb.constvar(1.0))
    m = gb.datavar(1)
    o = gb.randomvar(1)
    gb.node(_lib.NODE_MULTIPLY, o, m, x)
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, gb.datavar(1), o, gb.constvar(1.0))
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, m, x, gb.constvar(1.0))
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "data matrix" in str(ei.value)


@pytest.mark.parametrize("N,d", [(100, 1), (12, 2), (12, 5), (12, 33)])
def test_the_matrix_reads_are_counted(N, d):
    dat, con, mat_doubles = _pair(N, d, **(dict(init={"b": (0.0, 100.0)}) if d == 1 else dict(cut="b")))
    p, q = plan(dat[0]), plan(con[0])
    assert p["io_bytes_per_sweep"] == q["io_bytes_per_sweep"] + 8 * mat_doubles
    # the sweep reads every x[i] twice (the rule toward the product's output, the rule toward b); the strand schedule no less
    assert p["bytes_per_sweep"] == q["bytes_per_sweep"] + 2 * 8 * mat_doubles
    assert p["strand_bytes_per_sweep"] == q["strand_bytes_per_sweep"] + 2 * 8 * mat_doubles
    assert p["fe_bytes_per_sweep"] >= q["fe_bytes_per_sweep"]
    assert p["doubles_per_replica"] == q["doubles_per_replica"] + mat_doubles


FOREST_BUILDERS = [(dg.chain_obs_maps, dict(T=4, d=3, dy=2)), (dg.chain_obs_maps, dict(T=3, d=20, dy=7)), (dg.two_maps, dict(d=4, du=3, dw=2)),
                   (dg.derived_product, dict(d=3, du=2)), (dg.square_and_flat, dict(d=4, r=2)), (dg.dot_rows, dict(N=5, d=4))]


@pytest.mark.parametrize("builder,kw", FOREST_BUILDERS)
def test_forests_plan_as_their_constant_twins_and_round_trip_through_a_dump(builder, kw):
    gb, ys, mats, _, nominal = builder(x_as_data=True, **kw)
    gc = builder(x_as_data=False, **kw)[0]
    p, q = plan(gb), plan(gc)
    for k in SAME:
        assert p[k] == q[k], k
    assert p["io_bytes_per_sweep"] == q["io_bytes_per_sweep"] + 8 * sum(M.size for M in nominal)
    dump = gb.to_dump()
    assert [dump["variables"][v]["cols"] for v in mats] == [M.shape[1] for M in nominal]
    back = GraphBuilder.from_dump(dump)
    assert back.cols == gb.cols and back.rows == gb.rows
    assert plan(back) == p
    # the twin of a dump is the constant graph
    tw = GraphBuilder.from_dump(dg.const_twin(dump, dict(zip(mats, nominal))))
    assert plan(tw) == q


def test_data_matrices_next_to_mixture_nodes_are_refused_by_name():
    gb, ys, nm = tg.mixture_on_tree(N=4, K=2, d=2)
    x = nm["m"][0]
    o = gb.randomvar(2)
    gb.node(_lib.NODE_MULTIPLY, o, gb.datavar(2, cols=2), x)
    gb.mvnormal_mean_cov(gb.datavar(2), o, gb.constvar(np.eye(2)))
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "data matrix" in str(ei.value)


# figures of graphs WITHOUT a data matrix, computed by the compiler as it was before data matrices existed (tests/test_tree_plan_cpu.py's graphs, the loopy
# regression with constant x): the op tables of such graphs must not move
PINNED = {
    "forest3": (145, 20, 65, 62888, 44504, 12088, 4096, 3258, 41, 45, 23, 14),
    "linreg_const_x": (1856, 21, 1237, 97184, 84192, 17920, 848, 3797, 827, 502, 19800, 2),
    "prediction": (129, 37, 71, 7712, 3632, 2032, 800, 679, 23, 57, 14, 14),
    "star70": (206, 12, 105, 15200, 11600, 8576, 1760, 2291, 81, 95, 0, 1),
    "state_noise_precision": (100, 29, 58, 10424, 5176, 4208, 768, 960, 17, 45, 13, 8),
    "two_branch_T12": (201, 43, 115, 20088, 11472, 4840, 1248, 1616, 37, 93, 43, 12),
    "two_branch_d16": (63, 18, 35, 104416, 55968, 19720, 5696, 8984, 13, 29, 11, 4),
}


def _figures(p):
    return tuple(p[k] for k in ("n_ops", "n_levels", "n_messages", "bytes_per_sweep", "strand_bytes_per_sweep", "fe_bytes_per_sweep", "io_bytes_per_sweep",
                                "doubles_per_replica", "n_strands", "rule_calls", "products", "marginals"))


def _pinned_graphs():
    x, _ = lg.reference_data(100)
    return {"two_branch_T12": tg.two_branch_chain(T=12)[0], "two_branch_d16": tg.two_branch_chain(T=4, d=16, dy1=9, dy2=16)[0],
            "star70": tg.star(n_leaves=70, d=3)[0], "prediction": tg.chain_with_prediction(T=8, H=3)[0],
            "state_noise_precision": tg.chain_state_noise_precision(T=8, d=3, dy=2, also_obs_noise=True)[0],
            "linreg_const_x": lg.linreg(x, init={"b": (0.0, 100.0)})[0], "forest3": tg.random_forest(3, n_steps=14, dmax=12)[0]}


@pytest.mark.parametrize("name", sorted(_pinned_graphs()))
def test_a_graph_without_a_data_matrix_plans_as_before(name):
    assert _figures(plan(_pinned_graphs()[name])) == PINNED[name]

"""The host side of the executor's streaming entry points (include/rxhip.h "Streaming"), no GPU: rxhip_tree_check_autoupdates takes the `@autoupdates` table
of the HGF step graph (test/models/statespace/hgf_tests.jl:46-49) and refuses every malformed table with the offending variable in rxhip_lowering_error();
the library exports the new symbols; the Julia mirror of rxhip_autoupdate has the header's fields in order (the parsing of tests/test_julia_mirrors.py)."""
import ctypes
import re

import pytest

from rxhip import _lib, graph, tree
from test_julia_mirrors import c_fields, julia_fields


def _hgf():
    return graph.hgf_step_graph(1.0, 0.0, 0.04, 0.01)


def test_the_hgf_table_is_accepted():
    gb, names = _hgf()
    table = names["autoupdates"]
    data = [v for v in range(len(gb.kind)) if gb.kind[v] == _lib.VARKIND_DATA]
    # zt_min_mean, zt_min_var = mean_var(q(zt)); xt_min_mean, xt_min_var = mean_var(q(xt)): the four prior parameters, y is the series
    assert [t for t, _, _ in table] == data[:4] and data[4] == names["y"]
    assert [(s, k) for _, s, k in table] == [(names["zt"], "mean"), (names["zt"], "var"), (names["xt"], "mean"), (names["xt"], "var")]
    tree.check_autoupdates(gb, table)
    tree.check_autoupdates(gb, [])
    tree.check_autoupdates(gb, [(table[1][0], names["zt"], "precision")])   # (a variance slot fed 1 / variance is well-formed: scalar to scalar)


def _vector_graph():
    """x_prev ~ MvNormal(m, S), x ~ MvNormal(x_prev, P), y ~ MvNormal(x, Q) at d = 2, a scalar side chain, a Gamma precision and a data matrix"""
    import numpy as np
    gb = graph.GraphBuilder()
    xp, x = gb.randomvar(2), gb.randomvar(2)
    m, y = gb.datavar(2), gb.datavar(2)
    gb.node(_lib.NODE_MVNORMAL_MEAN_COV, xp, m, gb.constvar(np.eye(2)))
    gb.node(_lib.NODE_MVNORMAL_MEAN_COV, x, xp, gb.constvar(0.1 * np.eye(2)))
    gb.node(_lib.NODE_MVNORMAL_MEAN_COV, y, x, gb.constvar(np.eye(2)))
    s, sm, sv, tau = gb.randomvar(1), gb.datavar(1), gb.datavar(1), gb.randomvar(1)
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, s, sm, sv)
    gb.node(_lib.NODE_GAMMA_SHAPE_RATE, tau, gb.constvar(2.0), gb.constvar(1.0))
    ys = gb.datavar(1)
    gb.node(_lib.NODE_NORMAL_MEAN_PRECISION, ys, s, tau)
    gb.gaussian_joint()
    return gb, dict(xp=xp, x=x, m=m, y=y, s=s, sm=sm, sv=sv, tau=tau)


def _matrix_graph():
    """y ~ Normal(A * x, 1) with A a 1 × 2 data matrix (`dot(x, a)`), the prior mean of x data"""
    import numpy as np
    gb = graph.GraphBuilder()
    x, m, A, z, y = gb.randomvar(2), gb.datavar(2), gb.datavar(1, cols=2), gb.randomvar(1), gb.datavar(1)
    gb.node(_lib.NODE_MVNORMAL_MEAN_COV, x, m, gb.constvar(np.eye(2)))
    gb.multiply(z, A, x)
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, y, z, gb.constvar(1.0))
    return gb, dict(x=x, m=m, A=A, z=z, y=y)


def _refused(gb, table):
    with pytest.raises(_lib.RxHipError) as ei:
        tree.check_autoupdates(gb, table)
    return ei.value.status, str(ei.value)


def test_malformed_tables_are_refused_with_the_variable_named():
    gb, n = _vector_graph()
    tree.check_autoupdates(gb, [(n["m"], n["x"], "mean"), (n["sm"], n["s"], "mean"), (n["sv"], n["s"], "var")])
    bad = {
        "target is a random variable": ([(n["xp"], n["x"], "mean")], n["xp"]),
        "source is a data variable": ([(n["m"], n["y"], "mean")], n["y"]),
        "mean: dimensions differ": ([(n["m"], n["s"], "mean")], n["m"]),
        "var: the target is a vector": ([(n["m"], n["s"], "var")], n["m"]),
        "precision: the target is a vector": ([(n["m"], n["s"], "precision")], n["m"]),
        "target listed twice": ([(n["sm"], n["s"], "mean"), (n["sm"], n["s"], "mean")], n["sm"]),
        "unknown kind": ([(n["sm"], n["s"], 7)], n["sm"]),
        "target out of range": ([(10 ** 6, n["s"], "mean")], 10 ** 6),
        "source out of range": ([(n["sm"], -3, "mean")], -3),
    }
    for what, (table, var) in bad.items():
        st, msg = _refused(gb, table)
        assert st == _lib.ERR_BADARG, (what, st, msg)
        assert (re.search(rf"variable {var}(?!\d)", msg)), (what, msg)
    # a target on the matrix interface of `*`
    gm, k = _matrix_graph()
    tree.check_autoupdates(gm, [(k["m"], k["x"], "mean")])
    st, msg = _refused(gm, [(k["A"], k["x"], "mean")])
    assert st == _lib.ERR_BADARG and re.search(rf"variable {k['A']}(?!\d)", msg) and "matrix" in msg, msg


def test_feedback_out_of_scope_is_unsupported_and_says_so():
    gb, n = _vector_graph()
    # a covariance matrix as feedback
    for kind in ("var", "precision"):
        st, msg = _refused(gb, [(n["sv"], n["x"], kind)])
        assert st == _lib.ERR_UNSUPPORTED and "not supported" in msg and re.search(rf"variable {n['x']}(?!\d)", msg) and "MATRIX" in msg, msg
    # the parameters of a Gamma marginal as feedback (`shape(q(τ))`)
    st, msg = _refused(gb, [(n["sv"], n["tau"], "mean")])
    assert st == _lib.ERR_UNSUPPORTED and "not supported" in msg and "Gamma" in msg and re.search(rf"variable {n['tau']}(?!\d)", msg), msg


def test_a_graph_the_executor_refuses_is_refused_here_as_by_the_planner():
    gb = graph.GraphBuilder()
    a, b = gb.randomvar(1), gb.randomvar(1)   # a cycle no initialisation cuts
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, a, b, gb.constvar(1.0))
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, b, a, gb.constvar(1.0))
    with pytest.raises(_lib.RxHipError) as e1:
        tree.plan(gb)
    with pytest.raises(_lib.RxHipError) as e2:
        tree.check_autoupdates(gb, [])
    assert e1.value.status == e2.value.status


def test_library_exports_the_streaming_symbols():
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ("rxhip_tree_check_autoupdates", "rxhip_tree_set_autoupdates", "rxhip_tree_stream", "rxhip_tree_get_history", "rxhip_tree_get_stream_free_energy"):
        assert hasattr(L, name) and name in bound, name
    assert (_lib.AU_MEAN, _lib.AU_VAR, _lib.AU_PRECISION) == (0, 1, 2)


def test_julia_and_python_mirror_rxhip_autoupdate():
    fields = c_fields("rxhip_autoupdate")
    assert fields == ["target", "source", "kind", "reserved"]
    assert julia_fields("Autoupdate") == fields
    assert [f for f, _ in _lib.Autoupdate._fields_] == fields and ctypes.sizeof(_lib.Autoupdate) == 24


def test_julia_wrappers_call_the_new_exports():
    from test_julia_mirrors import JULIA
    for fn, sym in (("tree_set_autoupdates!", "rxhip_tree_set_autoupdates"), ("tree_stream!", "rxhip_tree_stream"), ("tree_history", "rxhip_tree_get_history")):
        body = JULIA[JULIA.index("function " + fn):]
        assert ":" + sym + "," in body[:body.index("\nend")], fn

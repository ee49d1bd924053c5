"""The loopy schedule in the graph compiler (rxhip_tree_plan, no device): which message initialisations cut which cycles, what stays refused, and that
an initialisation off every cycle changes nothing."""
import re

import numpy as np
import pytest

import rxhip
from rxhip import _lib
from rxhip.graph import GraphBuilder
from rxhip.tree import plan

import loopy_graphs as lg
import tree_graphs as tg

X = np.linspace(-3.0, 4.0, 30) + 0.25


def test_linreg_with_an_initialised_b_plans_one_loop_message_per_observation():
    gb, _, _ = lg.linreg(X, init={"b": (0.0, 100.0)})
    p = plan(gb)
    assert p["n_loop_messages"] == len(X)
    assert p["n_ops"] > 0 and p["bytes_per_sweep"] % 8 == 0


def test_linreg_without_an_initialisation_is_refused_with_cycle():
    gb, _, _ = lg.linreg(X)
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "cycle" in str(ei.value)


def test_an_initialised_a_cuts_too():
    gb, _, nm = lg.linreg(X, init={"a": (0.0, 100.0)})
    assert plan(gb)["n_loop_messages"] == len(X)


def test_one_anonymous_product_output_leaves_the_other_loops_uncut():
    gb, _, nm = lg.linreg(X, init={"t": (0, (0.0, 100.0))})
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "cycle" in str(ei.value)
    # the text names a variable of an uncut loop: a, b or one of the other t[i], s[i]
    named = int(str(ei.value).split("through variable ")[1].split()[0])
    assert named in {nm["a"], nm["b"]} | set(nm["t"][1:]) | set(nm["s"][1:])


@pytest.mark.parametrize("seed", range(6))
def test_an_initialisation_on_a_forest_changes_nothing(seed):
    import tree_oracle
    gb, ys, named = tg.random_forest(seed, n_steps=12, dmax=(1, 2, 4, 8, 12, 20)[seed])
    p0 = plan(gb)
    gauss = tree_oracle.TreeGraph(gb.to_dump()).gauss
    v = next(i for i in range(len(gb.kind)) if gauss[i])   # (a random Gaussian variable: the class that takes a message initialisation)
    d = gb.rows[v]
    gb.initialize_message(v, _lib.INIT_MVNORMAL, np.concatenate([np.zeros(d), np.eye(d).ravel()]))
    p1 = plan(gb)
    assert p1["n_loop_messages"] == 0
    for k in ("n_ops", "n_levels", "n_messages", "bytes_per_sweep", "strand_bytes_per_sweep", "rule_calls", "products", "marginals", "doubles_per_replica"):
        assert p1[k] == p0[k], k


def test_loops_in_a_graph_with_precision_variables_are_refused():
    """the loopy schedule is Gaussian sum-product: with Wishart / Gamma variables (VMP state) it is refused, by name"""
    gb, _, nm = lg.linreg(X, init={"b": (0.0, 100.0)})
    tau = gb.randomvar(1)
    gb.node(_lib.NODE_GAMMA_SHAPE_RATE, tau, gb.constvar(1.0), gb.constvar(1.0))
    gb.node(_lib.NODE_NORMAL_MEAN_PRECISION, gb.datavar(1), nm["a"], tau)
    gb.initialize(tau, _lib.INIT_GAMMA, (1.0, 1.0))
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "precision" in str(ei.value)


def test_initialisations_outside_the_gaussian_family_are_refused():
    gb, ys, nm = tg.chain_state_noise_precision(T=4, d=2, dy=2)
    W = next(i for i in range(len(gb.kind)) if gb.kind[i] == _lib.VARKIND_RANDOM and any(
        t == _lib.NODE_WISHART and f[0] == i for t, f in zip(gb.ftype, gb.fiface)))
    gb.initialize_message(W, _lib.INIT_MVNORMAL, np.concatenate([np.zeros(2), np.eye(2).ravel()]))
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED


def test_an_improper_initialisation_is_refused():
    gb, _, _ = lg.linreg(X, init={"b": (0.0, -1.0)})
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_NOT_POSDEF


def test_message_initialisations_survive_a_dump_round_trip():
    gb, _, nm = lg.linreg(X[:5], init={"b": (0.5, 100.0)})
    gb.initialize(nm["a"], _lib.INIT_NORMAL, (1.0, 2.0))
    d = gb.to_dump()
    assert d["variables"][nm["b"]]["msg_init"] == {"family": "normal", "params": [0.5, 100.0]}
    assert "msg_init" not in d["variables"][nm["a"]] and d["variables"][nm["a"]]["init"]["params"] == [1.0, 2.0]
    g2 = GraphBuilder.from_dump(d)
    assert g2.to_dump() == d
    assert plan(g2)["n_loop_messages"] == 5
    old = {**d, "variables": [{k: v for k, v in var.items() if k != "msg_init"} for var in d["variables"]]}   # a dump without the key loads as before
    assert not GraphBuilder.from_dump(old).msg_init_family


# ---- the cut rule on random loopy graphs (tests/loopy_graphs.py), against the restatement's own bridge finder (oracle/tree_oracle.py) ----

def test_the_loop_message_count_of_sixty_random_loopy_graphs():
    import tree_oracle
    for seed in range(60):
        gb, _, named, kind = lg.random_loopy(seed, lg.KINDS[seed % len(lg.KINDS)]) if seed % 3 else lg.random_loopy(seed)
        want = len(tree_oracle.TreeGraph(gb.to_dump()).loop_keys())
        assert want >= 2 and plan(gb)["n_loop_messages"] == want, (seed, kind)


@pytest.mark.parametrize("cut,n_loop", [([(0, 1), (1, 0), (1, 2), (2, 1)], 12), ([(0, 0), (1, 1), (2, 2)], 8)])
def test_a_three_by_three_grid(cut, n_loop):
    gb, _, _ = lg.grid(0, d=2, rows=3, cols=3, cut=cut)
    assert plan(gb)["n_loop_messages"] == n_loop


def test_a_grid_cut_at_its_centre_alone_names_a_site_on_an_uncut_cycle():
    gb, _, named = lg.grid(0, d=2, rows=3, cols=3, cut=[(1, 1)])
    with pytest.raises(rxhip.RxHipError) as ei:
        plan(gb)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "cycle" in str(ei.value)
    assert int(re.search(r"through variable (\d+)", str(ei.value)).group(1)) in lg.uncut_cycle_variables(gb)


@pytest.mark.parametrize("n_cuts", [1, 2])
def test_a_ring_of_six(n_cuts):
    gb, _, named = lg.ring(0, d=3, n=6, chord=False)
    want = len(named["cut"])
    assert plan(gb)["n_loop_messages"] == 2 * want
    rng = np.random.default_rng(1)
    extra = [v for v in lg.uncut_cycle_variables(gb, []) if v not in named["cut"]]
    lg.initialise(gb, rng, extra[:n_cuts])
    assert plan(gb)["n_loop_messages"] == 2 * (want + n_cuts)


def test_dropping_one_variable_of_a_minimal_cut_names_a_variable_of_an_uncut_cycle():
    checked = 0
    for seed in range(40):
        gb, _, named, kind = lg.random_loopy(seed, lg.KINDS[seed % len(lg.KINDS)])
        if kind == "star":   # (one cut: dropping it leaves no initialisation at all)
            continue
        g2, v, uncut = lg.drop_one_cut(gb, named["fvs"], np.random.default_rng(seed))
        if not uncut:   # a second initialisation on the same cycle still cuts it
            assert plan(g2)["n_loop_messages"] > 0
            continue
        with pytest.raises(rxhip.RxHipError) as ei:
            plan(g2)
        assert ei.value.status == _lib.ERR_UNSUPPORTED and "cycle" in str(ei.value), (seed, kind)
        assert int(re.search(r"through variable (\d+)", str(ei.value)).group(1)) in uncut, (seed, kind, v, sorted(uncut))
        checked += 1
    assert checked >= 20


def test_an_initialisation_off_every_cycle_of_a_loopy_graph_changes_nothing():
    checked = 0
    for seed in range(40):
        gb, _, named, kind = lg.random_loopy(seed, lg.KINDS[seed % len(lg.KINDS)])
        off = [v for v in named["x"] if v not in lg.uncut_cycle_variables(gb, [])]
        if not off:
            continue
        p0 = plan(gb)
        lg.initialise(gb, np.random.default_rng(seed), [off[seed % len(off)]])
        p1 = plan(gb)
        for k in ("n_loop_messages", "n_ops", "n_levels", "n_messages", "bytes_per_sweep", "strand_bytes_per_sweep", "rule_calls", "products", "marginals",
                  "doubles_per_replica"):
            assert p1[k] == p0[k], (seed, kind, k)
        checked += 1
    assert checked >= 20

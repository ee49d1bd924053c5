"""The loopy schedule on the device against its generic restatement (oracle/tree_oracle.py infer, pinned by tests/test_loopy_oracle.py) on random loopy
graphs (tests/loopy_graphs.py: rings, grids, cycles through `+`, regression stars with hubs, closed forests): every iteration under every schedule and
kernel family, on every replica; the fixed point against exact conditioning; continued runs, new data between them, `missing` observations, and an
initialisation off every cycle."""
import numpy as np
import pytest

from rxhip import _lib
from rxhip.tree import TreeEngine

import loopy_graphs as lg
import tree_graphs as tg
import tree_oracle

pytestmark = pytest.mark.gpu

ITERS = 6
_REFS = {}


def _graph(kind, seed):
    gb, ys, named, _ = lg.random_loopy(seed, kind)
    return gb, ys, named


def _refs(key, gb, ys, data, iterations=ITERS, cache=True):
    """[replica][iteration] restatement results (one-iteration runs carrying the loop messages: the same numbers as a run of `iterations`)"""
    if cache and key in _REFS:
        return _REFS[key]
    dump, out = gb.to_dump(), []
    for r in range(data.shape[0]):
        st, rows = None, []
        for _ in range(iterations):
            o = tree_oracle.infer(dump, tg.data_dict(gb, ys, data[r]), 1, loop_state=st)
            st = o["loop_state"]
            rows.append(o)
        out.append(rows)
    if cache:
        _REFS[key] = out
    return out


def _check(post, fe, ref, gv, R, tag):
    for r in range(R):
        for v in gv:
            m, V = ref[r]["mean"][v], ref[r]["cov"][v]
            sd = np.sqrt(np.diag(V))
            assert np.max(np.abs(post[v][0][r] - m) / sd) < 1e-8, (tag, r, v)
            assert np.max(np.abs(post[v][1][r] - V) / np.outer(sd, sd)) < 1e-8, (tag, r, v)
        want = ref[r]["fe"][0]
        assert abs(fe[r] - want) <= 1e-8 * max(1.0, abs(want)), (tag, r, fe[r], want)


def _every_iteration(gb, ys, named, data, refs, tag, allow_missing=False):
    R = data.shape[0]
    with TreeEngine(gb, n_replicas=R, allow_missing=allow_missing) as eng:
        assert eng.info["n_loop_messages"] == len(tree_oracle.TreeGraph(gb.to_dump()).loop_keys())
        if ys:
            eng.set_data(ys, data)
        for it in range(1, ITERS + 1):
            eng.run(it, True)
            _check(eng.marginals(named["x"]), eng.free_energy_per_replica(), [refs[r][it - 1] for r in range(R)], named["x"], R, (tag, it))


@pytest.mark.parametrize("tile", ["0", "1"])
@pytest.mark.parametrize("mode", [None, "0", "1", "2", "3"])
def test_every_iteration_on_random_loopy_graphs(mode, tile, monkeypatch):
    """the graphs of loopy_graphs.GPU_GRAPHS, 1 or 3 replicas: means 1e-8 sd, covariances 1e-8 of sd sdᵀ, free energy 1e-8 relative, after every one of
    6 iterations — a reader that takes the wrong iteration's loop value changes the trajectory even where the fixed point stays"""
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    monkeypatch.setenv("RXHIP_TREE_TILE", tile)
    for i, (kind, seed) in enumerate(lg.GPU_GRAPHS):
        gb, ys, named = _graph(kind, seed)
        R = (1, 3)[i % 2]
        data = tg.random_data(gb, ys, R, seed)
        _every_iteration(gb, ys, named, data, _refs((kind, seed, R), gb, ys, data), (kind, seed, mode, tile))


@pytest.mark.parametrize("mode", [None, "0", "1", "2", "3"])
@pytest.mark.parametrize("R", [64, 70])
def test_every_replica_of_a_wide_batch(R, mode, monkeypatch):
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    for kind, seed in (("ring", 3), ("plus", 0), ("grid", 1), ("ring", 1)):
        gb, ys, named = _graph(kind, seed)
        data = tg.random_data(gb, ys, R, seed)
        _every_iteration(gb, ys, named, data, _refs((kind, seed, R), gb, ys, data), (kind, seed, mode, R))


@pytest.mark.parametrize("kind,seed", [("ring", 2), ("plus", 9), ("grid", 3), ("star", 1), ("forest", 6)])
def test_the_fixed_point_is_exact_conditioning(kind, seed):
    """after 400 iterations the means are brute-force conditioning (the covariances of loopy BP are not exact: tests/test_loopy_oracle.py holds the restatement's),
    and the free energy is the restatement's at its own fixed point"""
    gb, ys, named = _graph(kind, seed)
    data = tg.random_data(gb, ys, 2, seed)
    with TreeEngine(gb, n_replicas=2) as eng:
        eng.set_data(ys, data)
        eng.run(400, True)
        post, fe = eng.marginals(named["x"]), eng.free_energy_per_replica()
    for r in range(2):
        dd = tg.data_dict(gb, ys, data[r])
        bf, _ = tg.brute_force(gb, dd)
        for v in named["x"]:
            sd = np.sqrt(np.diag(bf[v][1]))
            assert np.max(np.abs(post[v][0][r] - bf[v][0]) / sd) < 1e-9, (r, v)
        want = tree_oracle.infer(gb.to_dump(), dd, 400)["fe"][-1]
        assert abs(fe[r] - want) <= 1e-8 * max(1.0, abs(want)), (r, fe[r], want)


@pytest.mark.parametrize("mode", [None, "0", "1", "2", "3"])
def test_continued_runs_are_one_run(mode, monkeypatch):
    """six one-iteration runs are one run of six, bit for bit, at dimensions 12 … 64 and on a hub"""
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    for kind, seed in (("ring", 2), ("ring", 4), ("plus", 6), ("plus", 7), ("ring", 8), ("star", 0)):
        gb, ys, named = _graph(kind, seed)
        data = tg.random_data(gb, ys, 3, seed)
        with TreeEngine(gb, n_replicas=3) as one:
            if ys:
                one.set_data(ys, data)
            one.run(ITERS, True)
            ref, fe_ref = one.marginals(named["x"]), one.free_energy_per_replica()
        with TreeEngine(gb, n_replicas=3) as eng:
            if ys:
                eng.set_data(ys, data)
            eng.continue_runs(True)
            for _ in range(ITERS):
                eng.run(1, True)
            got = eng.marginals(named["x"])
            for v in named["x"]:
                assert np.array_equal(got[v][0], ref[v][0]) and np.array_equal(got[v][1], ref[v][1]), (kind, seed, v)
            assert np.array_equal(eng.free_energy_per_replica(), fe_ref), (kind, seed)


@pytest.mark.parametrize("mode", [None, "0", "2"])
def test_new_data_between_continued_runs(mode, monkeypatch):
    """three iterations on one data set, then three more on another from the carried loop messages: the restatement started from its own carried state"""
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    for kind, seed in (("ring", 1), ("grid", 3), ("plus", 7), ("star", 1)):
        gb, ys, named = _graph(kind, seed)
        d1, d2 = tg.random_data(gb, ys, 2, seed), tg.random_data(gb, ys, 2, seed + 77)
        with TreeEngine(gb, n_replicas=2) as eng:
            eng.set_data(ys, d1)
            eng.continue_runs(True)
            eng.run(3, True)
            eng.set_data(ys, d2)
            eng.run(3, True)
            post, fe = eng.marginals(named["x"]), eng.free_energy_per_replica()
        dump, refs = gb.to_dump(), []
        for r in range(2):
            first = tree_oracle.infer(dump, tg.data_dict(gb, ys, d1[r]), 3)
            o = tree_oracle.infer(dump, tg.data_dict(gb, ys, d2[r]), 3, loop_state=first["loop_state"])
            o["fe"] = o["fe"][-1:]
            refs.append(o)
        _check(post, fe, refs, named["x"], 2, (kind, seed, mode))


@pytest.mark.parametrize("mode", [None, "0", "3"])
def test_missing_observations_on_and_next_to_cycles(mode, monkeypatch):
    """allow_missing: a quarter of the observations NaN (per replica), on ring sites, grid sites and the `+` outputs of cycles"""
    if mode is not None:
        monkeypatch.setenv("RXHIP_TREE_MODE", mode)
    for kind, seed in (("ring", 3), ("ring", 7), ("grid", 8), ("plus", 2), ("forest", 0)):
        gb, ys, named = _graph(kind, seed)
        R = 4
        data = tg.random_data(gb, ys, R, seed)
        obs = {ifs[0] for ifs in gb.fiface if gb.kind[ifs[0]] == _lib.VARKIND_DATA}   # (data on the `out` side of a node: not the inputs of a derived value)
        rng, o = np.random.default_rng(seed), 0
        for v in ys:
            for r in range(R):
                if v in obs and rng.random() < 0.25:
                    data[r, o:o + gb.rows[v]] = np.nan
            o += gb.rows[v]
        assert np.isnan(data).any()
        _every_iteration(gb, ys, named, data, _refs(None, gb, ys, data, cache=False), (kind, seed, mode), allow_missing=True)


@pytest.mark.parametrize("kind,seed", [("ring", 7), ("grid", 1), ("plus", 2), ("forest", 9)])
def test_an_initialisation_off_every_cycle_changes_no_bit(kind, seed):
    gb, ys, named = _graph(kind, seed)
    off = [v for v in named["x"] if v not in lg.uncut_cycle_variables(gb, [])]
    assert off
    data = tg.random_data(gb, ys, 3, seed)
    with TreeEngine(gb, n_replicas=3) as e0:
        e0.set_data(ys, data)
        e0.run(4, True)
        m0, fe0 = e0.marginals(named["x"]), e0.free_energy()
        n0 = e0.info["n_loop_messages"]
    lg.initialise(gb, np.random.default_rng(seed), off[:2])
    with TreeEngine(gb, n_replicas=3) as e1:
        e1.set_data(ys, data)
        e1.run(4, True)
        m1, fe1 = e1.marginals(named["x"]), e1.free_energy()
        assert e1.info["n_loop_messages"] == n0
    for v in named["x"]:
        assert np.array_equal(m0[v][0], m1[v][0]) and np.array_equal(m0[v][1], m1[v][1]), v
    assert np.array_equal(fe0, fe1)

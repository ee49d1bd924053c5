"""Per-iteration device time of the loopy schedule (include/rxhip.h "Loopy graphs"): the linear regression of tests/loopy_graphs.py with `μ(b)` at
N observations × R replicas, against a forest with the same op count — the same regression with `a` a constant (a star on b) over as many more
observations as it takes to reach the loopy graph's ops — and the time per op of each.
Prints one JSON line.  Usage: python scripts/time_loopy.py [--N 100] [--replicas 4096] [--iterations 50]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rxinfer.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from rxhip import _lib  # noqa: E402
from rxhip.graph import GraphBuilder  # noqa: E402
from rxhip.tree import TreeEngine, plan  # noqa: E402

import loopy_graphs as lg  # noqa: E402


def star(x):
    gb = GraphBuilder()
    b = gb.randomvar(1)
    gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, b, gb.constvar(0.0), gb.constvar(1.0))
    ys = []
    for xi in x:
        t, s, y = gb.randomvar(1), gb.randomvar(1), gb.datavar(1)
        gb.node(_lib.NODE_MULTIPLY, t, gb.constvar(float(xi)), b)
        gb.node(_lib.NODE_ADD, s, t, gb.constvar(0.5))
        gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, y, s, gb.constvar(1.0))
        ys.append(y)
    return gb, ys


def time_graph(gb, ys, Y, iterations):
    with TreeEngine(gb, n_replicas=Y.shape[0]) as eng:
        eng.set_data(ys, Y)
        eng.run(3, True)   # warm-up
        eng.run(iterations, True)
        return dict(last_iteration_ms=eng.last_iteration_ms(), n_ops=eng.info["n_ops"], n_levels=eng.info["n_levels"], mode=eng.info["mode"],
                    n_loop_messages=eng.info["n_loop_messages"], bytes_per_sweep=eng.info["bytes_per_sweep"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--replicas", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=50)
    a = ap.parse_args()
    x, y = lg.reference_data(a.N)
    Y = np.tile(y, (a.replicas, 1)) + np.random.default_rng(0).normal(0.0, 1.0, (a.replicas, a.N))
    gb, ys, _ = lg.linreg(x, init={"b": (0.0, 100.0)})
    loopy = time_graph(gb, ys, Y, a.iterations)
    n_ops = plan(gb)["n_ops"]
    xs = np.concatenate([x, x + 0.5, x + 0.25])
    M = a.N
    while plan(star(xs[:M])[0])["n_ops"] < n_ops and M < len(xs):
        M += 1
    gs, yss = star(xs[:M])
    Ys = np.concatenate([Y, Y, Y], axis=1)[:, :M]
    tree = time_graph(gs, yss, Ys, a.iterations)
    tree["N"] = M
    per_op = lambda r: r["last_iteration_ms"] / r["n_ops"]
    print(json.dumps(dict(N=a.N, replicas=a.replicas, loopy=loopy, tree=tree, ratio=loopy["last_iteration_ms"] / tree["last_iteration_ms"],
                          ratio_per_op=per_op(loopy) / per_op(tree))))


if __name__ == "__main__":
    main()

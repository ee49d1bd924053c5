"""Per-iteration device time of `*` with DATA matrices against the same graph with the matrices as constants (include/rxhip.h "typeof(*) with a constant or a
DATA matrix"): the reference's linear regression (N observations × R replicas, `μ(b)`; rxhip.graph.linreg_graph) with x as data against x as constants, scalar
and vector (d = dy).  Method of scripts/time_loopy.py: HIP-event time per iteration (rxhip_tree_info.last_iteration_ms), warm, `--pairs` alternating
(constant, data) pairs per case; medians.  Next to each ratio the byte model: the constant graph's time plus the extra bytes of the schedule
(bytes_per_sweep + fe_bytes_per_sweep differences, per replica) over `--tbps` (the part's measured mixed read / write ceiling, profiles/r01/membench.txt).
`--constant-only` times the constant graph alone: with RXHIP_LIB naming a build from before data matrices existed it gives that build's constant-x time for the
same cases (the yardstick of the data path, and the check that the constant path did not move).
Prints one JSON line per case.  Usage: python scripts/time_datamul.py [--cases 1:100:4096,4:12:4096,8:12:4096,16:12:4096,64:12:512] [--iterations 30] [--pairs 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rxinfer.jl_amd"))

import numpy as np  # noqa: E402

from rxhip.graph import linreg_graph  # noqa: E402
from rxhip.tree import TreeEngine  # noqa: E402


def problem(d, N, R, seed=0):
    """the regressors every replica shares in the constant graph (and gets as its own data in the other), priors, noise, initialisation, observations"""
    rng = np.random.default_rng(seed)
    if d == 1:
        x = np.arange(1, N + 1, dtype=float) + rng.normal(size=N)
        Y = 10.0 - 10.0 * x + rng.normal(size=(R, N))
        return x, dict(init={"b": (0.0, 100.0)}), Y
    spd = lambda s: s * (np.eye(d) + 0.3 * (lambda M: M @ M.T)(rng.normal(size=(d, d)) / np.sqrt(d)))
    X = np.eye(d) + 0.3 * rng.normal(size=(N, d, d)) / np.sqrt(d)
    kw = dict(prior_a=(rng.normal(size=d), spd(2.0)), prior_b=(rng.normal(size=d), spd(1.5)), noise_var=spd(0.5), init={"b": (rng.normal(size=d), spd(10.0))})
    Y = (np.einsum("nij,j->ni", X, rng.normal(size=d))[None] + rng.normal(size=(R, N, d))).reshape(R, -1)
    return X, kw, Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1:100:4096,4:12:4096,8:12:4096,16:12:4096,64:12:512", help="d:N:replicas, comma-separated")
    ap.add_argument("--iterations", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--tbps", type=float, default=5.0)
    ap.add_argument("--constant-only", action="store_true")
    a = ap.parse_args()
    for case in a.cases.split(","):
        d, N, R = (int(v) for v in case.split(":"))
        x, kw, Y = problem(d, N, R)
        gc, yc, _, _ = linreg_graph(N, x=x, x_as_data=False, **kw)
        if a.constant_only:
            with TreeEngine(gc, n_replicas=R) as ec:
                ec.set_data(yc, Y)
                ec.run(3, True)
                tc = []
                for _ in range(a.pairs):
                    ec.run(a.iterations, True)
                    tc.append(ec.last_iteration_ms())
                print(json.dumps(dict(d=d, N=N, replicas=R, kernels=ec.info["kernels"], mode=ec.info["mode"], n_ops=ec.info["n_ops"], constant_ms=tc,
                                      constant_median_ms=statistics.median(tc))), flush=True)
            continue
        gd, yd, xd, _ = linreg_graph(N, d=d, dy=d, x_as_data=True, **kw)
        rows = np.concatenate([Y, np.tile(np.asarray(x, float).reshape(1, -1), (R, 1))], axis=1)   # (every replica the same regressors: the two graphs compute the same)
        with TreeEngine(gc, n_replicas=R) as ec, TreeEngine(gd, n_replicas=R) as ed:
            ec.set_data(yc, Y)
            ed.set_data(yd + xd, rows)
            for e in (ec, ed):
                e.run(3, True)   # warm-up
            tc, td = [], []
            for _ in range(a.pairs):
                ec.run(a.iterations, True)
                tc.append(ec.last_iteration_ms())
                ed.run(a.iterations, True)
                td.append(ed.last_iteration_ms())
            same = float(np.max(np.abs(ec.free_energy_per_replica() - ed.free_energy_per_replica()) / np.maximum(1.0, np.abs(ec.free_energy_per_replica()))))
            extra = (ed.info["bytes_per_sweep"] + ed.info["fe_bytes_per_sweep"]) - (ec.info["bytes_per_sweep"] + ec.info["fe_bytes_per_sweep"])
            mc, md = statistics.median(tc), statistics.median(td)
            model_ms = mc + 1e3 * extra * R / (a.tbps * 1e12)
            print(json.dumps(dict(d=d, N=N, replicas=R, kernels=ed.info["kernels"], mode=ed.info["mode"], n_ops=ed.info["n_ops"], constant_ms=tc, data_ms=td,
                                  constant_median_ms=mc, data_median_ms=md, ratio=md / mc, extra_bytes_per_replica=extra, byte_model_ms=model_ms,
                                  byte_model_ratio=model_ms / mc, free_energy_rel_diff=same)), flush=True)


if __name__ == "__main__":
    main()

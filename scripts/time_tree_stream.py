"""Timing of rxhip_tree_stream against the host loop it replaces (DESIGN.md §3.7 "Streaming", profiles/r09/tree_stream.txt): the HGF step graph of
test/models/statespace/hgf_tests.jl:9-31 as an online filter, T = 200 observations, 5 VMP iterations each, at 4 096 series (as bench.py streams it) and at one.
Per shape, median of five:
  (a) wall time per observation of the host loop — continue_runs, set_data, run, marginals, feedback in numpy (--what loop; with RXHIP_LIB pointing at the build
      of the commit before the streaming entry points this is the figure of the parent commit);
  (b) wall time per observation of TreeEngine.stream, upload and history read-back included (--what stream);
  (c) device time per observation of the sweeps alone: last_iteration_ms × iterations of the host loop's runs.
Every process prints one JSON line per shape.  Under `rocprofv3 --kernel-trace --stats -- python scripts/time_tree_stream.py --what stream --repeats 1` the
share of k_tree_stream_step in the kernel time is the cost of the step kernels."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rxinfer.jl_amd"))

from rxhip import _lib  # noqa: E402

if os.environ.get("RXHIP_LIB"):   # an older build of the library (the parent commit's, for (a)): bind what it exports
    _old = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(_old, s[0])]

from rxhip.graph import hgf_step_graph  # noqa: E402
from rxhip.tree import TreeEngine  # noqa: E402

ITERS, T = 5, 200


def series(R):
    return np.cumsum(np.random.default_rng(780).standard_normal((T, R)), axis=0) * 0.3


def host_loop(gb, names, y, R):
    dvars = [v for v in range(len(gb.kind)) if gb.kind[v] == 1]
    qz, qx = np.tile([0.0, 5.0], (R, 1)), np.tile([0.0, 5.0], (R, 1))
    dev = []
    with TreeEngine(gb, n_replicas=R) as eng:
        eng.continue_runs(True)
        t0 = time.perf_counter()
        for t in range(T):
            eng.set_data(dvars, np.column_stack([qz[:, 0], qz[:, 1], qx[:, 0], qx[:, 1], y[t]]))
            eng.run(ITERS, True)
            dev.append(eng.last_iteration_ms() * ITERS)
            post = eng.marginals([names["zt"], names["xt"]])
            qz = np.column_stack([post[names["zt"]][0][:, 0], post[names["zt"]][1][:, 0, 0]])
            qx = np.column_stack([post[names["xt"]][0][:, 0], post[names["xt"]][1][:, 0, 0]])
        wall = time.perf_counter() - t0
    return wall / T * 1e3, float(np.median(dev)), (qz, qx)


def stream(gb, names, y, R):
    with TreeEngine(gb, n_replicas=R) as eng:
        eng.set_autoupdates(names["autoupdates"])
        t0 = time.perf_counter()
        out = eng.stream([names["y"]], y[:, :, None], iterations=ITERS, free_energy=True, history=[names["zt"], names["xt"]])
        wall = time.perf_counter() - t0
        dev = eng.last_iteration_ms() * ITERS
    (zm, zv), (xm, xv) = out["history"][names["zt"]], out["history"][names["xt"]]
    return wall / T * 1e3, dev, (np.column_stack([zm[-1, :, 0], zv[-1, :, 0, 0]]), np.column_stack([xm[-1, :, 0], xv[-1, :, 0, 0]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("loop", "stream"), required=True)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replicas", type=int, nargs="*", default=[4096, 1])
    a = ap.parse_args()
    gb, names = hgf_step_graph(1.0, 0.0, 0.04, 0.01, q_zt=(0.0, 5.0), q_xt=(0.0, 5.0), n_gh=31)
    for R in a.replicas:
        y = series(R)
        fn = host_loop if a.what == "loop" else stream
        fn(gb, names, y, R)   # warm-up: code objects, allocator
        runs = [fn(gb, names, y, R) for _ in range(a.repeats)]
        line = {"what": a.what, "library": _lib.LIB_PATH, "replicas": R, "T": T, "iterations": ITERS, "repeats": a.repeats,
                "wall_ms_per_observation": float(np.median([r[0] for r in runs])), "wall_ms_all": [round(r[0], 4) for r in runs],
                ("sweeps_device_ms_per_observation" if a.what == "loop" else "device_ms_per_observation_with_step_kernels"): float(np.median([r[1] for r in runs])),
                "final_q_zt_series0": [float(v) for v in runs[-1][2][0][0]], "final_q_xt_series0": [float(v) for v in runs[-1][2][1][0]]}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

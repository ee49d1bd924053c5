#!/usr/bin/env python3
"""Times the dense path of the multivariate mixture engine (csrc/mvgmm_dense_kernels.hpp) with the engine's own event timers
(rxhip_set_profiling / rxhip_get_kernel_times: one event pair per kernel, averaged over the launches).

Per shape (d, K, N): the pass kernel, the reduction, the update, a whole iteration (host wall time of run() over the iterations, the
engine synchronises at its end) and three figures:
  streaming floor   N·d·8 B of observations at the part's measured pure-read rate (profiles/r01/membench.txt: 5.4 TB/s)
  matrix cores      executed fp64 MFMA flops 4·N·K·(16·NT)² (logits 2·N·K·D² + statistics 2·N·K·D², D = 16·NT; the statistics skip the
                    strictly upper tile at NT = 2, so the executed count there is 3.5·N·K·D²: both are printed) against 78.6 TFLOP/s
  executor          d = 8, K = 3, N = 200, one replica: this engine against the node-array executor's mixture layer on the same model

Protocol (guide `measuring-on-mi355x`): one process, one device; 3 warm-up iterations discarded; the event times are averages over
`--iters` launches in one run() and the median of `--repeats` such runs is reported with the min–max spread; the host wall time is
reported next to the event times, never instead of them.

    python scripts/time_mvgmm.py [--iters 20] [--repeats 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rxinfer.jl_amd"), os.path.join(ROOT, "oracle")]
import rxhip  # noqa: E402

HBM_READ_TBS = 5.4
FP64_PEAK_TFLOPS = 78.6


def model(d, K, N, seed=0):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((K, d))
    means *= 50.0 / np.linalg.norm(means, axis=1, keepdims=True)
    y = means[rng.integers(0, K, N)] + 3.0 * rng.standard_normal((N, d))
    mu0 = 0.5 * means + rng.uniform(0, 5, (K, d))
    pri = (mu0, np.tile(1e6 * np.eye(d), (K, 1, 1)), np.full(K, d + 1.0), np.tile(1e2 * np.eye(d), (K, 1, 1)), np.ones(K))
    return y, pri


def time_engine(d, K, N, iters, repeats):
    y, pri = model(d, K, N)
    rows = []
    with rxhip.MvGMMEngine(N, *pri, *pri) as eng:
        eng.set_data(y)
        eng.run(3, True)   # warm-up: code objects, clocks
        eng.set_profiling(True)
        for _ in range(repeats):
            eng.reset_kernel_times()
            t0 = time.perf_counter()
            eng.run(iters, True)
            wall = (time.perf_counter() - t0) * 1e3 / iters
            kt = eng.kernel_times()
            rows.append((kt["k_gmm_pass"]["ms_avg"], kt["k_gmm_reduce"]["ms_avg"], kt["k_gmm_update"]["ms_avg"], wall))
    a = np.array(rows)
    return np.median(a, axis=0), a.min(axis=0), a.max(axis=0)


def time_executor(iters, repeats):
    from rxhip.graph import mv_mixture_graph
    from rxhip.tree import TreeEngine
    d, K, N = 8, 3, 200
    y, pri = model(d, K, N)
    gb, ys = mv_mixture_graph(N, *pri, init=dict(m=(pri[0], pri[1]), w=(pri[2], pri[3]), s=np.ones(K)))
    walls = []
    with TreeEngine(gb, n_replicas=1, device=0) as eng:
        eng.set_data(ys, y.reshape(1, -1))
        eng.run(3, True)
        for _ in range(repeats):
            t0 = time.perf_counter()
            eng.run(iters, True)
            eng.free_energy()
            walls.append((time.perf_counter() - t0) * 1e3 / iters)
    return float(np.median(walls)), min(walls), max(walls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"mvgmm dense path, {a.repeats} runs of {a.iters} iterations, median [min, max]; times in ms"]
    for d, K, N in ((16, 8, 10**6), (32, 16, 10**6), (8, 8, 10**6)):
        med, lo, hi = time_engine(d, K, N, a.iters, a.repeats)
        D = 16 * (2 if d > 16 else 1)
        floor_ms = N * d * 8 / (HBM_READ_TBS * 1e12) * 1e3
        fl, fl_exec = 4.0 * N * K * D * D, (4.0 if D == 16 else 3.5) * N * K * D * D
        lines.append(f"d={d} K={K} N={N}: pass {med[0]:.4f} [{lo[0]:.4f}, {hi[0]:.4f}]  reduce {med[1]:.4f}  update {med[2]:.4f}  "
                     f"iteration (host wall) {med[3]:.4f} [{lo[3]:.4f}, {hi[3]:.4f}]")
        lines.append(f"    streaming floor {floor_ms:.4f} ms -> pass at {floor_ms / med[0]:.3f} of it;  fp64 MFMA {fl / med[0] * 1e-9:.2f} TFLOP/s nominal = "
                     f"{fl / med[0] * 1e-9 / FP64_PEAK_TFLOPS:.3f} of peak ({fl_exec / med[0] * 1e-9 / FP64_PEAK_TFLOPS:.3f} on executed instructions)")
    med, lo, hi = time_engine(8, 3, 200, a.iters, a.repeats)
    ex = time_executor(a.iters, a.repeats)
    lines.append(f"d=8 K=3 N=200: engine iteration (host wall) {med[3]:.4f} [{lo[3]:.4f}, {hi[3]:.4f}] (pass {med[0]:.4f}, update {med[2]:.4f});  "
                 f"executor mixture layer, one replica, iteration (host wall) {ex[0]:.4f} [{ex[1]:.4f}, {ex[2]:.4f}]")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

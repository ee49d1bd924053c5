"""Latent autoregressive engine at the HGF / probit / HMM configurations' shape: 4 096 series × T = 2 000 × 15 iterations, at order p = 1 (the
reference's Univariate model), 5 (its Multivariate model) and 8 (the engine's limit).

Times rxhip_run on the device (HIP events on the engine's stream around the whole run, best of --repeats, with and without the free energy) and
writes the time, the bytes moved per (series, step, iteration) as the kernel header derives them (y read by both loops: 16; the row record
l_i[p], 1/d_i, u_i written and read: 16·(p + 2); m and the Σ band on the last sweep only: 8·(p + 2) / iterations) and the share of the 8 TB/s HBM
peak they imply to profiles/lar/bench.json.  Also times the dense numpy restatement (tests/lar_ref.py, one host core) on one series — FOR
ORIENTATION ONLY: it inverts the whole (T + p)² precision matrix, it is not a tuned CPU code.

    python scripts/bench_lar.py [--series 4096] [--T 2000] [--iterations 15] [--repeats 5] [--out profiles/lar/bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rxinfer.jl_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E peak


def generate(T, C, seed=7):
    """C series of a stable AR(2) process with driving-noise precision 5, observed through noise of precision 5 (vectorised over the series)."""
    rng = np.random.default_rng(seed)
    z = np.zeros((T + 50, C))
    e = rng.standard_normal((T + 50, C)) / np.sqrt(5.0)
    for t in range(2, T + 50):
        z[t] = 0.6 * z[t - 1] - 0.3 * z[t - 2] + e[t]
    return z[50:] + rng.standard_normal((T, C)) / np.sqrt(5.0)


def bytes_per_step(p, iterations):
    return 16 + 16 * (p + 2) + 8 * (p + 2) / iterations


def bench_shape(a, p):
    import torch
    import lar_ref as R
    import rxhip

    T, C, I = a.T, a.series, a.iterations
    y = generate(T, C)
    mdl = R.model(p, 5.0)
    nbytes = bytes_per_step(p, I)
    res = {"shape": {"series": C, "T": T, "iterations": I, "order": p}, "bytes_per_series_step_iteration": nbytes}
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)          # the engine runs on this stream: the events below bracket exactly its work
    with rxhip.LAREngine(T, p, 5.0, n_series=C, device=0, stream=stream.cuda_stream) as eng:
        eng.set_data(y)
        for want_fe, key in ((False, "run_ms_without_free_energy"), (True, "run_ms_with_free_energy")):
            eng.run(I, want_fe)   # warm-up: code objects, first touch of the buffers
            ms = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                eng.run_async(I, want_fe)
                e1.record(stream)
                e1.synchronize()
                eng.sync()
                ms.append(e0.elapsed_time(e1))
            best = min(ms)
            gbs = nbytes * C * T * I / (best * 1e-3) / 1e9
            res[key] = {"best": best, "all": ms, "ns_per_series_step_iteration": best * 1e6 / (C * T * I), "moved_GB_per_s": gbs, "hbm_fraction": gbs / HBM_PEAK_GBS}
        # the engine's last free energy on one series against the restatement, at the size timed
        sample = C - 1
        per = eng.free_energy_per_chain()[sample]
        t0 = time.perf_counter()
        fe_ref = R.run(y[:, sample], I, **mdl)["fe"][-1]
        cpu_s = time.perf_counter() - t0
        res["check"] = {"fe_rel_err_sample": float(abs(per - fe_ref) / abs(fe_ref))}
    res["cpu_restatement_for_orientation_only"] = {
        "series_timed": 1, "seconds": cpu_s, "ns_per_series_step_iteration": cpu_s * 1e9 / (T * I),
        "what": "tests/lar_ref.py run (dense: numpy inverts the whole (T + p)² precision matrix every iteration, one core), free energy included; not a tuned CPU code"}
    res["limit_suggested_by_the_code"] = ("latency of the dependent fp64 chain of a row (the p-term recurrences of the LDLᵀ row, a division; the p² terms of the "
                                          "selected inverse), a lane per series with one to seven wavefronts per SIMD in flight: not HBM bandwidth")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=4096)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--iterations", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 5, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lar", "bench.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (before rxhip: the process then holds ONE HIP runtime, the one torch brings, and librxhip binds to it)
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_lar: no HIP device visible")
    res = {"hbm_peak_GB_per_s": HBM_PEAK_GBS, "configurations": [bench_shape(a, p) for p in a.orders]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Nonlinear state-space engine on the reference's published example (paper/example.jl): the pendulum with Δt = 0.01, T = 1000 observations, 5 VMP
iterations per observation, unknown observation precision from q(τ) = Gamma(shape 1, scale 100), for 4 096 independent series.

Times rxhip_run on the device (HIP events on the engine's stream around the whole run) for the streamed filter under both delta-node
approximations, and the smoothing sweep (forward + backward launch) with known unit noise, and writes ms per pass, series·observations per second
and the per-kernel times to profiles/nlssm/bench.json, the kernels a run launches to profiles/nlssm/kernel_list.txt.  There is no earlier version
of this path to compare with.  Next to the figures stands the one true-reference timing of this model, paper/benchmark.txt: 162 ms median for 1 000
observations = 162 µs per observation — ANOTHER MACHINE (one thread of an Intel i7-8850H), ONE series, graph construction included.

    python scripts/bench_nlssm.py [--series 4096] [--T 1000] [--iterations 5] [--repeats 5] [--out profiles/nlssm/bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rxinfer.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

DT, G = 0.01, 9.81
PAPER_US_PER_OBSERVATION = 162.0


def generate(T, C, seed=42):
    """the example's generative loop for C series: a pendulum released at angle 0.5 ± 0.05, its angle observed through unit-precision noise"""
    rng = np.random.default_rng(seed)
    a, w = 0.5 + 0.05 * rng.standard_normal(C), np.zeros(C)
    y = np.empty((T, C, 1))
    for t in range(T):
        a, w = a + w * DT, w - G * np.sin(a) * DT
        y[t, :, 0] = a + rng.standard_normal(C)
    return y


def timed(eng, iterations, repeats):
    import torch
    stream = torch.cuda.ExternalStream(eng.stream())
    eng.run(iterations, True)   # warm-up: code objects, first touch of the buffers
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.run_async(iterations, True)
        e1.record(stream)
        e1.synchronize()
        eng.sync()
        ms.append(e0.elapsed_time(e1))
    eng.set_profiling(True)
    eng.run(iterations, True)
    kernels = {k: v for k, v in eng.kernel_times().items() if v["launches"]}
    eng.set_profiling(False)
    return ms, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=4096)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlssm", "bench.json"))
    a = ap.parse_args()
    import torch
    import nlssm_ref as R
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_nlssm: no HIP device visible")
    torch.cuda.set_device(0)   # (the events of `timed` live on torch's current device: the engines below are created on it)
    T, C, I = a.T, a.series, a.iterations
    y = generate(T, C)
    f = lambda x: [x[0] + DT * x[1], x[1] - G * DT * np.sin(x[0])]
    m0, V0, H = np.array([0.5, 0.0]), 0.01 * np.eye(2), np.array([[1.0, 0.0]])
    res = {"shape": {"series": C, "T": T, "iterations": I, "d": 2, "program_instructions": len(rxhip.trace(f, 2).code)},
           "paper_reference": {"us_per_observation": PAPER_US_PER_OBSERVATION,
                               "note": "paper/benchmark.txt: a different machine (one thread of an Intel i7-8850H), ONE series, graph construction included"}}
    runs = [("filter_unknown_noise_linearization", dict(noise_prior=(1.0, 0.01), method="linearization", mode="filter"), I),
            ("filter_unknown_noise_unscented", dict(noise_prior=(1.0, 0.01), method="unscented", mode="filter"), I),
            ("smooth_known_noise_linearization", dict(R=[[1.0]], method="linearization", mode="smooth"), 1),
            ("smooth_known_noise_unscented", dict(R=[[1.0]], method="unscented", mode="smooth"), 1)]
    launched = []
    for key, kw, iters in runs:
        with rxhip.NonlinearSSMEngine(f, 2, T, m0, V0, H, n_series=C, device=0, **kw) as eng:
            eng.set_data(y)
            ms, kernels = timed(eng, iters, a.repeats)
            best = min(ms)
            res[key] = {"ms_per_pass": best, "all_ms": ms, "series_observations_per_s": C * T / (best * 1e-3), "ns_per_series_observation": best * 1e6 / (C * T),
                        "vmp_iterations_per_observation": iters, "kernel_times": kernels}
            launched.append(f"{key}: " + ", ".join(f"{k} ×{v['launches']}" for k, v in kernels.items()))
            if key.startswith("filter"):   # one series against the restatement, at the size timed
                mean, cov = eng.marginals()
                ref = R.run_series("pendulum", y[:, 0], m0, V0, np.zeros((2, 2)), H, noise=(1.0, 0.01), method=kw["method"], iterations=iters)
                sd = np.sqrt(np.einsum("tii->ti", ref["cov"]))
                res[key]["check_mean_err_sd_series0"] = float(np.max(np.abs(mean[:, 0] - ref["mean"]) / sd))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(os.path.dirname(a.out), "kernel_list.txt"), "w") as fh:
        fh.write("kernels of one rxhip_run of the nonlinear state-space engine (k_forward = k_nlssm_forward<d>, k_backward = k_nlssm_backward<d>; the free-energy\n"
                 "reduction k_nlssm_fe is not profiled separately)\n" + "\n".join(launched) + "\n")
    print(json.dumps({k: (v["ms_per_pass"], v["series_observations_per_s"]) for k, v in res.items() if isinstance(v, dict) and "ms_per_pass" in v}))


if __name__ == "__main__":
    main()

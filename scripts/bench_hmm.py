"""Hidden Markov model engine at the HGF / probit configurations' shape: 4 096 series × T = 2 000 × 20 iterations, at K = M = 3 (the reference
model's size) and at K = 16, M = 64 (the engine's limits).

Times rxhip_run on the device (HIP events on the engine's stream around the whole run, best of --repeats, with and without the free energy) and
writes the time, the bytes moved per (series, step, iteration) as the kernel header derives them (x read by both loops: 16; α̂ written and read:
16·K; γ on the last sweep only: 8·K / iterations) and the share of the 8 TB/s HBM peak they imply to profiles/hmm/bench.json.  Also times the numpy
restatement (tests/hmm_ref.py, one host core) on a few series — FOR ORIENTATION ONLY: it is a per-step Python loop, not a tuned CPU code.

    python scripts/bench_hmm.py [--series 4096] [--T 2000] [--iterations 20] [--repeats 5] [--out profiles/hmm/bench.json]
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


def generate(T, C, K, M, seed=7):
    """C series from one random HMM with sticky states and peaked emissions (numpy's generator, vectorised over the series)."""
    rng = np.random.default_rng(seed)
    A = rng.dirichlet(np.full(K, 0.3), size=K).T * 0.3 + 0.7 * np.eye(K)      # columns sum to 1
    B = rng.dirichlet(np.full(M, 0.3), size=K).T
    cA, cB = np.cumsum(A, axis=0), np.cumsum(B, axis=0)
    s = rng.integers(0, K, C)
    x = np.empty((T, C))
    for t in range(T):
        s = np.minimum((rng.random(C)[None, :] > cA[:, s]).sum(0), K - 1)
        x[t] = np.minimum((rng.random(C)[None, :] > cB[:, s]).sum(0), M - 1)
    return x


def bytes_per_step(K, iterations):
    return 16 + 16 * K + 8 * K / iterations


def bench_shape(a, K, M):
    import torch
    import hmm_ref as R
    import rxhip

    T, C, I = a.T, a.series, a.iterations
    x = generate(T, C, K, M)
    rng = np.random.default_rng(3)
    mdl = dict(prior_A=np.ones((K, K)), prior_B=np.ones((M, K)) + 9.0 * np.eye(M, K), prior_s0=np.full(K, 1.0 / K),
               init_A=rng.uniform(0.5, 3.0, (K, K)), init_B=rng.uniform(0.5, 3.0, (M, K)))
    nbytes = bytes_per_step(K, I)
    res = {"shape": {"series": C, "T": T, "iterations": I, "K": K, "M": M}, "bytes_per_series_step_iteration": nbytes}
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)          # the engine runs on this stream: the events below bracket exactly its work
    with rxhip.HMMEngine(T, mdl["prior_A"], mdl["prior_B"], mdl["prior_s0"], mdl["init_A"], mdl["init_B"], n_series=C, device=0,
                         stream=stream.cuda_stream) as eng:
        eng.set_data(x)
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
        # the engine's last free energy on a sample against the restatement, at the size timed
        sample = [0, C - 1]
        per = eng.free_energy_per_chain()[sample]
        t0 = time.perf_counter()
        fe_ref = [R.run(x[:, s], **mdl, iterations=I)[3][-1] for s in sample]
        cpu_s = time.perf_counter() - t0
        res["check"] = {"fe_rel_err_sample": float(np.max(np.abs(per - fe_ref) / np.abs(fe_ref)))}
    res["cpu_restatement_for_orientation_only"] = {
        "series_timed": len(sample), "seconds": cpu_s, "ns_per_series_step_iteration": cpu_s * 1e9 / (len(sample) * T * I),
        "what": "tests/hmm_ref.py run (a Python loop over the steps with numpy K-vectors, one core), free energy included; not a tuned CPU code"}
    res["limit_suggested_by_the_code"] = ("latency of the dependent fp64 chain of a step (K-term dot product, row reduction, division; shuffles in between), "
                                          "one wavefront per SIMD or fewer in flight: not HBM bandwidth")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=4096)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm", "bench.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (before rxhip: the process then holds ONE HIP runtime, the one torch brings, and librxhip binds to it)
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_hmm: no HIP device visible")
    res = {"hbm_peak_GB_per_s": HBM_PEAK_GBS, "configurations": [bench_shape(a, 3, 3), bench_shape(a, 16, 64)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Probit state-space engine at the HGF configuration's shape: 4 096 series × T = 2 000 × 10 parallel-EP iterations.

Times rxhip_run on the device (HIP events on the engine's stream around the whole run, with and without the free energy), times the inner loop
of the CPU restatement (tests/probit_ref.py, one host core of the same machine) on a stated fraction of the shape and scales it, and writes both,
the bytes moved per (series, step, iteration) and the share of HBM bandwidth they imply to profiles/probit/bench.json.  Also records how many
parallel-EP iterations the reference case and a sample of the headline data need before successive free energies differ by < 1e-10.

    python scripts/bench_probit.py [--series 4096] [--T 2000] [--iterations 10] [--repeats 5] [--out profiles/probit/bench.json]
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
BYTES_NO_FE, BYTES_FE = 88, 128  # per (series, step, iteration): csrc/probit_kernels.hpp header


def generate(T, C, seed=7):
    """The reference's generative loop (probit_tests.jl:33-58) for C series with numpy's generator."""
    from scipy.special import ndtr
    rng = np.random.default_rng(seed)
    x = np.full(C, -2.0)
    y = np.empty((T, C))
    for k in range(T):
        x = x + 0.1 + 0.1 * rng.standard_normal(C)
        x = np.where(x > 3.0, x - 6.0, x)      # keep the series crossing zero: a saturated series carries no information
        y[k] = ndtr(x) > rng.random(C)
    return y


def iterations_to_converge(run, tol=1e-10, cap=40):
    fe = run(cap)
    d = np.abs(np.diff(fe))
    hit = np.nonzero(d < tol)[0]
    return int(hit[0]) + 2 if len(hit) else None, fe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=4096)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-series", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probit", "bench.json"))
    a = ap.parse_args()
    import torch
    import probit_ref as R
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_probit: no HIP device visible")
    T, C, I = a.T, a.series, a.iterations
    mdl = R.REFERENCE_MODEL
    y = generate(T, C)
    res = {"shape": {"series": C, "T": T, "iterations": I}, "bytes_per_series_step_iteration": {"without_free_energy": BYTES_NO_FE, "with_free_energy": BYTES_FE}}
    with rxhip.ProbitEngine(T, mdl["a"], mdl["c"], mdl["q"], mdl["m0"], mdl["v0"], n_series=C) as eng:
        eng.set_data(y)
        stream = torch.cuda.ExternalStream(eng.stream())
        for want_fe, key, nbytes in ((False, "run_ms_without_free_energy", BYTES_NO_FE), (True, "run_ms_with_free_energy", BYTES_FE)):
            eng.run(I, want_fe)   # warm-up: code objects, first-touch of the buffers
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
        fe_dev = eng.free_energy()
        # the engine's last free energy on a sample against the restatement, at the size timed
        sample = [0, C // 2, C - 1]
        fe_ref = [R.run_messages(y[:, s], **mdl, iterations=I)[2][-1] for s in sample]
        per = eng.free_energy_per_chain()[sample]
        res["check"] = {"fe_rel_err_sample": float(np.max(np.abs(per - fe_ref) / np.abs(fe_ref)))}
        eng.set_profiling(True)
        eng.run(I, True)
        res["kernel_times"] = {k: v for k, v in eng.kernel_times().items() if v["launches"]}
        eng.set_profiling(False)
        # convergence of the headline data: total free energy over all series
        eng.run(40, True)
        fe40 = eng.free_energy()
        d = np.abs(np.diff(fe40)) / C
        hit = np.nonzero(d < 1e-10)[0]
        res["headline_iterations_to_1e-10_per_series"] = int(hit[0]) + 2 if len(hit) else None
        res["headline_fe_per_series_by_iteration"] = [float(v / C) for v in fe40[:12]]
    # one host core: the restatement's iteration on a few series, scaled to the shape
    t0 = time.perf_counter()
    for s in range(a.cpu_series):
        R.run_messages(y[:, s], **mdl, iterations=I)
    cpu_s = time.perf_counter() - t0
    res["cpu_restatement"] = {"series_timed": a.cpu_series, "fraction_of_shape": a.cpu_series / C, "seconds": cpu_s, "scaled_seconds_full_shape": cpu_s * C / a.cpu_series,
                              "ns_per_series_step_iteration": cpu_s * 1e9 / (a.cpu_series * T * I), "what": "tests/probit_ref.py run_messages (numpy scalars, one core), free energy included"}
    _, yr = R.reference_data()
    n_ref, _ = iterations_to_converge(lambda n: R.run_messages(yr, **mdl, iterations=n)[2])
    res["reference_case_iterations_to_1e-10"] = n_ref
    res["speedup_vs_scaled_cpu_restatement"] = res["cpu_restatement"]["scaled_seconds_full_shape"] * 1e3 / res["run_ms_with_free_energy"]["best"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Regression / autoregression engine: the reference's own benchmark shape and the shapes that show the statistics pass against its roofs.

  reference     1 series × T = 1000 × order 5 × 15 iterations  (ar_tests.jl:69-72, `@test_benchmark "models" "ar"`; the regenerated StableRNG(32) series)
  batch         4096 series of the same shape
  lag_p4        one series, T = 10⁷, order 4, lagged mode   (lane path)
  lag_p16       … order 16  (matrix cores, one column tile)
  lag_p32       … order 32  (matrix cores, two column tiles)
  reg_p4 / reg_p16 / reg_p32   the same three series from a materialised X in regressor mode

Times rxhip_run on the device (HIP events on the engine's stream around the whole run, best of --repeats): the FIRST run on a data set, which is
the pass plus the iterations, and a REPEATED run, which is the iterations only (the statistics are kept) — so pass = first − repeated.  Each pass is
set against its own byte stream (8·T in lagged mode, 8·N·(d + 1) in regressor mode) at the HBM peak and, above d = 4, against 2·N·D² flops
(D = 16·⌈d/16⌉, nominal: lower tiles only are executed) at the fp64 MFMA rate.  Writes profiles/arreg/bench.json.

Every shape runs in a child process of its own under its own time limit, one after the other; the first that fails ends the script.

    python scripts/bench_arreg.py [--repeats 5] [--shapes reference batch lag_p4 …] [--out profiles/arreg/bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rxinfer.jl_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E peak
FP64_PEAK_TFLOPS = 78.6          # MI355X fp64 matrix (= vector) peak
# name: (series, T, order, iterations, lagged, time limit of the child in seconds)
SHAPES = {"reference": (1, 1000, 5, 15, True, 120), "batch": (4096, 1000, 5, 15, True, 180),
          "lag_p4": (1, 10_000_000, 4, 15, True, 240), "lag_p16": (1, 10_000_000, 16, 15, True, 240), "lag_p32": (1, 10_000_000, 32, 15, True, 240),
          "reg_p4": (1, 10_000_000, 4, 15, False, 300), "reg_p16": (1, 10_000_000, 16, 15, False, 400), "reg_p32": (1, 10_000_000, 32, 15, False, 600)}


def bench_shape(name, repeats):
    import torch  # noqa: F401  (before rxhip: the process then holds ONE HIP runtime, the one torch brings, and librxhip binds to it)
    import arreg_ref as R
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_arreg: no HIP device visible")
    C, T, p, I, lagged, _ = SHAPES[name]
    if name == "reference":
        z = R.golden()[1][:, None]
    else:
        z = np.random.default_rng(11).standard_normal((T, C), dtype=np.float32).astype(np.float64)
    rows = T - p
    D = p if p <= 4 else 16 * ((p + 15) // 16)
    tile, chunks = rxhip.ARRegressionEngine.schedule(rows, p)
    stream_bytes = float(C) * (T if lagged else rows * (p + 1)) * 8
    flops = 2.0 * C * rows * D * D if p >= 5 else None
    res = {"shape": {"series": C, "T": T, "order": p, "iterations": I, "lagged": lagged},
           "schedule": {"tile_rows": tile, "chunks_per_series": chunks, "launches_first_run": 2, "launches_repeated_run": 1, "extra_launch_free_energy_of_a_batch": 1},
           "pass_stream_bytes": stream_bytes, "pass_mfma_flops_nominal": flops}
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)          # the engine runs on this stream: the events below bracket exactly its work
    if lagged:
        eng = rxhip.ARRegressionEngine(T, p, n_series=C, lagged=True, device=0, stream=stream.cuda_stream)
        feed = lambda: eng.set_data(z)
    else:
        X, y = R.lag_rows(z[:, 0], p)
        X, y = X[None], y[None]
        eng = rxhip.ARRegressionEngine(rows, p, n_series=C, device=0, stream=stream.cuda_stream)
        feed = lambda: eng.set_observations(y)    # marks the statistics stale; X stays in place

        eng.set_regressors(X)

    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.run_async(I, True)
        e1.record(stream)
        e1.synchronize()
        eng.sync()
        return e0.elapsed_time(e1)

    with eng:
        feed()
        eng.run(I, True)      # warm-up: code objects, first touch of the buffers
        first, again = [], []
        for _ in range(repeats):
            feed()
            first.append(timed())
            again.append(timed())
        bf, ba = min(first), min(again)
        pass_ms = max(bf - ba, 1e-6)
        gbs = stream_bytes / (pass_ms * 1e-3) / 1e9
        res["first_run_ms"] = {"best": bf, "all": first}
        res["repeated_run_ms"] = {"best": ba, "all": again, "ms_per_iteration": ba / I}
        res["pass_ms"] = {"first_minus_repeated": pass_ms, "stream_GB_per_s": gbs, "hbm_fraction": gbs / HBM_PEAK_GBS}
        if flops is not None:
            tf = flops / (pass_ms * 1e-3) / 1e12
            res["pass_ms"].update({"mfma_TFLOP_per_s_nominal": tf, "fp64_mfma_fraction": tf / FP64_PEAK_TFLOPS})
        # the engine's result on the last series against the restatement, at the size timed
        tm, tc, ga, gb, fe = eng.parameters()
        ref = R.run_lagged(z[:, -1:], p, **R.model(p), iterations=I)
        res["check"] = R.contract_errors(dict(mean=tm[:, -1:], cov=tc[:, -1:], a=ga[:, -1:], b=gb[:, -1:], fe=fe[:, -1:]), ref)
        res["free_energy_first_last"] = [float(fe[0, -1]), float(fe[-1, -1])]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arreg", "bench.json"))
    ap.add_argument("--child", default=None, help="(internal) run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(bench_shape(a.child, a.repeats)))
        return
    res = {"hbm_peak_GB_per_s": HBM_PEAK_GBS, "fp64_mfma_peak_TFLOP_per_s": FP64_PEAK_TFLOPS, "configurations": {}}
    for name in a.shapes:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)], capture_output=True, text=True,
                             timeout=SHAPES[name][5])
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not lines:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"bench_arreg: shape {name} ended with status {out.returncode}; nothing further is started")
        res["configurations"][name] = json.loads(lines[-1][len("RESULT "):])
        print(name, json.dumps(res["configurations"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    lag = {k[4:]: v["pass_ms"]["first_minus_repeated"] for k, v in res["configurations"].items() if k.startswith("lag_")}
    reg = {k[4:]: v["pass_ms"]["first_minus_repeated"] for k, v in res["configurations"].items() if k.startswith("reg_")}
    for k in lag:
        if k in reg:
            print(f"{k}: lagged pass {lag[k]:.3f} ms, regressor pass {reg[k]:.3f} ms, ratio {reg[k] / lag[k]:.2f}")


if __name__ == "__main__":
    main()

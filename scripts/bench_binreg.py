"""Binomial regression engine: the reference's own benchmark shape and the shapes that show the pass against its two roofs.

  reference     20 problems × N = 1000 × d = 2 × 100 iterations  (binomialreg_tests.jl:26-30, `@test_benchmark "models" "binomialreg"`)
  batch         4096 problems × N = 1000 × d = 2 × 100 iterations
  stream_d4     one problem, N = 10⁷, d = 4   (lane path)
  stream_d16    one problem, N = 10⁷, d = 16  (matrix cores, one column tile)
  stream_d32    one problem, N = 10⁷, d = 32  (matrix cores, two column tiles)

Times rxhip_run on the device (HIP events on the engine's stream around the whole run, best of --repeats, with and without the free energy) and
reports each shape against two roofs: the stream of N·(d + 1)·8 bytes per problem and iteration (X and n_eff) against the HBM peak, and, at d ≥ 5,
4·N·D² flops per iteration (D = 16·⌈d/16⌉; S·Xᵀ and the Gram update, 2·N·D² each, nominal: the Gram update executes lower tiles only) against the
fp64 MFMA rate.  Writes profiles/binreg/bench.json.

Every shape runs in a child process of its own under its own time limit, one after the other; the first that fails ends the script.

    python scripts/bench_binreg.py [--repeats 5] [--shapes reference batch stream_d4 stream_d16 stream_d32] [--out profiles/binreg/bench.json]
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
# name: (problems, N, d, iterations, time limit of the child in seconds)
SHAPES = {"reference": (20, 1000, 2, 100, 120), "batch": (4096, 1000, 2, 100, 180), "stream_d4": (1, 10_000_000, 4, 10, 240),
          "stream_d16": (1, 10_000_000, 16, 10, 300), "stream_d32": (1, 10_000_000, 32, 10, 420)}


def generate(C, N, d, seed=11):
    """the reference's recipe at d features: X ~ N(0, 1/d) (so that x_iᵀβ stays O(1) at every d), n_trials uniform on 5 … 20, float32 draws widened"""
    r = np.random.default_rng(seed)
    X = r.standard_normal((C, N, d), dtype=np.float32).astype(np.float64) / np.sqrt(d)
    beta = np.resize(np.array([-1.0, 0.6]), d) * np.sqrt(d / 2.0)
    n = r.integers(5, 21, (C, N)).astype(np.float64)
    p = 0.5 * (1.0 + np.tanh(0.5 * (X @ beta)))
    y = r.binomial(n.astype(np.int64), p).astype(np.float64)
    return X, y, n


def bench_shape(name, repeats):
    import torch  # noqa: F401  (before rxhip: the process then holds ONE HIP runtime, the one torch brings, and librxhip binds to it)
    import binreg_ref as R
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_binreg: no HIP device visible")
    C, N, d, I, _ = SHAPES[name]
    X, y, n = generate(C, N, d)
    D = d if d <= 4 else 16 * ((d + 15) // 16)
    tile, chunks = rxhip.BinomialRegressionEngine.schedule(N, d)
    stream_bytes = float(C) * N * (d + 1) * 8
    flops = 4.0 * C * N * D * D if d >= 5 else None
    res = {"shape": {"problems": C, "N": N, "d": d, "iterations": I}, "schedule": {"tile_points": tile, "chunks_per_problem": chunks, "launches_per_iteration": 2},
           "stream_bytes_per_iteration": stream_bytes, "mfma_flops_per_iteration_nominal": flops}
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)          # the engine runs on this stream: the events below bracket exactly its work
    with rxhip.BinomialRegressionEngine(N, d, np.zeros(d), np.eye(d), n_problems=C, device=0, stream=stream.cuda_stream) as eng:
        eng.set_data(X, y, n)
        for want_fe, key in ((False, "run_ms_without_free_energy"), (True, "run_ms_with_free_energy")):
            eng.run(I, want_fe)   # warm-up: code objects, first touch of the buffers, ξ
            ms = []
            for _ in range(repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                eng.run_async(I, want_fe)
                e1.record(stream)
                e1.synchronize()
                eng.sync()
                ms.append(e0.elapsed_time(e1))
            best = min(ms)
            per_it = best / I
            gbs = stream_bytes / (per_it * 1e-3) / 1e9
            r = {"best": best, "all": ms, "ms_per_iteration": per_it, "us_per_launch": per_it * 1e3 / (3 if want_fe else 2), "stream_GB_per_s": gbs,
                 "hbm_fraction": gbs / HBM_PEAK_GBS}
            if flops is not None:
                tf = flops / (per_it * 1e-3) / 1e12
                r.update({"mfma_TFLOP_per_s_nominal": tf, "fp64_mfma_fraction": tf / FP64_PEAK_TFLOPS})
            res[key] = r
        # the engine's result on the last problem against the restatement, at the size timed
        mean, cov, fe = eng.parameters()
        ref = R.run(X[-1], y[-1], n[-1], np.zeros(d), np.eye(d), R.model(d)["init"], I)
        res["check"] = R.contract_errors(dict(mean=mean[:, -1], cov=cov[:, -1], fe=fe[:, -1]), ref)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binreg", "bench.json"))
    ap.add_argument("--child", default=None, help="(internal) run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(bench_shape(a.child, a.repeats)))
        return
    res = {"hbm_peak_GB_per_s": HBM_PEAK_GBS, "fp64_mfma_peak_TFLOP_per_s": FP64_PEAK_TFLOPS, "configurations": {}}
    for name in a.shapes:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)], capture_output=True, text=True,
                             timeout=SHAPES[name][4])
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not lines:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"bench_binreg: shape {name} ended with status {out.returncode}; nothing further is started")
        res["configurations"][name] = json.loads(lines[-1][len("RESULT "):])
        print(name, json.dumps(res["configurations"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

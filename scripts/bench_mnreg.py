"""Multinomial regression engine: the reference's two workloads and the shapes that show the statistics pass and the online kernel.

  reference       1 problem × 1000 count vectors × K = 10 × 100 iterations  (multinomialreg_tests.jl:11-55; tests/golden/mnreg_seed1.npz)
  batch           4096 problems of that shape
  binreg_expanded the binomial engine on the reference problem expanded to 9000 rows of d = 9 (the comparison both sides exist for)
  stream_k10      one problem, N = 10⁷, K = 10, 3 iterations: the statistics pass against its byte stream 8·N·K at the HBM peak
  stream_k65      … K = 65
  online          1 series × T = 5000 × K = 40, one iteration per step  (multinomialreg_tests.jl:57-116; tests/golden/mnreg_online_seed1.npz), with
                  the reference's assertions on the result
  online_batch    4096 series × T = 500 × K = 10

Times rxhip_run on the device (HIP events on the engine's stream around the whole run, best of --repeats): offline the FIRST run on a data set, which
is the pass plus the iterations, and a REPEATED run, which is the iterations only (the partials are kept) — so pass = first − repeated.  Writes
profiles/mnreg/bench.json.  Reads nothing outside the repository tree.

Every shape runs in a child process of its own under its own time limit, one after the other; the first that fails ends the script.

    python scripts/bench_mnreg.py [--repeats 5] [--shapes reference batch …] [--out profiles/mnreg/bench.json]
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
# name: (problems, N, K, iterations, online, time limit of the child in seconds)
SHAPES = {"reference": (1, 1000, 10, 100, False, 120), "batch": (4096, 1000, 10, 100, False, 180), "binreg_expanded": (1, 9000, 10, 100, False, 120),
          "stream_k10": (1, 10_000_000, 10, 3, False, 300), "stream_k65": (1, 10_000_000, 65, 3, False, 600),
          "online": (1, 5000, 40, 1, True, 180), "online_batch": (4096, 500, 10, 1, True, 240)}


def bench_shape(name, repeats):
    import torch  # noqa: F401  (before rxhip: the process then holds ONE HIP runtime, the one torch brings, and librxhip binds to it)
    import mnreg_ref as R
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_mnreg: no HIP device visible")
    C, N, K, I, online, _ = SHAPES[name]
    d = K - 1
    p_true = None
    if name in ("reference", "binreg_expanded"):
        Y, p_true, W0, _ = R.golden()
        Y = Y[None]
    elif name == "online":
        Y, p_true, W0, _ = R.golden("mnreg_online_seed1")
        Y = Y[None]
    else:
        Y = np.random.default_rng(11).integers(0, 5, (C, N, K), dtype=np.int8).astype(np.float64)
        W0 = np.eye(d)
    res = {"shape": {"problems": C, "N": N, "K": K, "iterations": I, "online": online}}
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)          # the engine runs on this stream: the events below bracket exactly its work
    if name == "binreg_expanded":
        X, y, n = R.expanded(Y[0])
        eng = rxhip.BinomialRegressionEngine(len(y), d, np.zeros(d), W0, device=0, stream=stream.cuda_stream)
        eng.set_regressors(X), eng.set_trials(n)
        feed = lambda: eng.set_observations(y)
    else:
        eng = rxhip.MultinomialRegressionEngine(N, K, np.zeros(d), W0, n_problems=C, online=online, device=0, stream=stream.cuda_stream)
        feed = lambda: eng.set_data(Y)
        tile, chunks = rxhip.MultinomialRegressionEngine.schedule(N, K)
        res["schedule"] = {"tile_rows": tile, "chunks_per_problem": chunks, "launches_first_run": 1 if online else 2, "launches_repeated_run": 1,
                           "extra_launch_free_energy_of_a_batch": 1}

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
        res["first_run_ms"] = {"best": bf, "all": first}
        res["repeated_run_ms"] = {"best": ba, "all": again, "ms_per_iteration": ba / I}
        if name == "binreg_expanded":
            return res
        if online:
            res["per_step_and_series_us"] = 1e3 * ba / (N * C)
            hm, hv, _, hf = eng.history()
            ref = R.online(Y[-1][:50], np.zeros(d), W0, I)
            res["check_first_50_steps"] = R.contract_errors(dict(mean=hm[:50, -1], var=hv[:50, -1], fe=hf[:50, -1]), ref)
            res["free_energy_first_last"] = [float(hf[0, -1]), float(hf[-1, -1])]
            if p_true is not None:   # the reference's assertions (multinomialreg_tests.jl:107-114) and the restatement's recorded figures
                mse = float(np.mean((rxhip.logistic_stick_breaking(hm[-1, 0]) - p_true) ** 2))
                res["reference_assertions"] = {"mse": mse, "F_1": float(hf[0, 0]), "F_T": float(hf[-1, 0])}
                assert mse < 1e-3 and hf[-1, 0] < hf[0, 0], res["reference_assertions"]
                assert all(abs(float(hf[i, 0]) - r) < 1e-8 * r for i, r in zip((0, -1), R.RECORDED_FE_ONLINE)), (res["reference_assertions"], R.RECORDED_FE_ONLINE)
            return res
        stream_bytes = 8.0 * C * N * K
        pass_ms = max(bf - ba, 1e-6)
        gbs = stream_bytes / (pass_ms * 1e-3) / 1e9
        res["pass_stream_bytes"] = stream_bytes
        res["pass_ms"] = {"first_minus_repeated": pass_ms, "stream_GB_per_s": gbs, "hbm_fraction": gbs / HBM_PEAK_GBS}
        mean, cov, fe = eng.parameters()
        if N > 100_000:   # the restatement's lnΓ over 10⁸ entries takes minutes: the exact statistics instead
            Yc, Sc, _, nc = eng.statistics()
            col = Y[-1].sum(axis=0)
            res["statistics_bit_equal"] = bool(np.array_equal(Yc[-1], col) and np.array_equal(Sc[-1], np.cumsum(col[::-1])[::-1]) and nc[-1] == N)
            res["free_energy_first_last"] = [float(fe[0, -1]), float(fe[-1, -1])]
            return res
        ref = R.run(Y[-1], np.zeros(d), W0, R.model(K, None, W0)["init"], I)
        res["check"] = R.contract_errors(dict(mean=mean[:, -1], cov=cov[:, -1], fe=fe[:, -1]), ref)
        res["free_energy_first_last"] = [float(fe[0, -1]), float(fe[-1, -1])]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mnreg", "bench.json"))
    ap.add_argument("--child", default=None, help="(internal) run one shape in this process and print its JSON")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(bench_shape(a.child, a.repeats)))
        return
    res = {"hbm_peak_GB_per_s": HBM_PEAK_GBS, "configurations": {}}
    for name in a.shapes:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)], capture_output=True, text=True,
                             timeout=SHAPES[name][5])
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not lines:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"bench_mnreg: shape {name} ended with status {out.returncode}; nothing further is started")
        res["configurations"][name] = json.loads(lines[-1][len("RESULT "):])
        print(name, json.dumps(res["configurations"][name]), flush=True)
    cf = res["configurations"]
    if "reference" in cf and "binreg_expanded" in cf:
        a_ms, b_ms = cf["reference"]["repeated_run_ms"]["best"], cf["binreg_expanded"]["repeated_run_ms"]["best"]
        res["repeated_run_against_the_binomial_engine"] = {"mnreg_ms": a_ms, "binreg_expanded_ms": b_ms, "ratio": b_ms / a_ms}
        print(f"repeated run at the reference's shape: mnreg {a_ms:.3f} ms, binomial engine on the expanded problem {b_ms:.3f} ms, ratio {b_ms / a_ms:.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

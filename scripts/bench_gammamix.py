"""Gamma mixture engine: the reference's own shape, a batch of it, and the pass against its roofs.

  ref_streamed                       1 problem × N = 250 × K = 2 × 50 iterations with F  (gamma_mixture_tests.jl; the recorded numpy draw)
  batch_streamed                     4096 problems of that shape
  big_k2_recompute / big_k2_stored   one problem, N = 10⁷, K = 2: the pass recomputes ln y (8 B/point) or reads it from memory (16 B/point)
  big_k16_recompute / big_k16_stored the same at K = 16
  gmm_k2 / gmm_k16                   k_gmm_pass of the Gaussian mixture engine at the same N and K (8 B/point, a comparable softmax): the yardstick

Times rxhip_run on the device (HIP events on the engine's stream around the whole run, best of --repeats).  For the N = 10⁷ shapes the pass and update
kernels are also timed one by one (rxhip_set_profiling, in a run of its own) and the pass is set against its byte stream at the HBM peak.
Writes profiles/gammamix/bench.json.  Every shape runs in a child process of its own under its own time limit, one after the other; the first that
fails ends the script.

    python scripts/bench_gammamix.py [--repeats 5] [--shapes ref_streamed …] [--out profiles/gammamix/bench.json]
    python scripts/bench_gammamix.py --child ref_streamed --once      (one run of one shape: the program behind `rocprofv3 --kernel-trace --`)
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
BIG = 10_000_000
# name: (problems, N, K, iterations, schedule, stored ln y, time limit of the child in seconds)
SHAPES = {"ref_streamed": (1, 250, 2, 50, "streamed", True, 120), "batch_streamed": (4096, 250, 2, 50, "streamed", True, 180),
          "big_k2_recompute": (1, BIG, 2, 50, "streamed", False, 240), "big_k2_stored": (1, BIG, 2, 50, "streamed", True, 240),
          "big_k16_recompute": (1, BIG, 16, 50, "streamed", False, 300), "big_k16_stored": (1, BIG, 16, 50, "streamed", True, 300),
          "gmm_k2": (1, BIG, 2, 50, "gmm", False, 240), "gmm_k16": (1, BIG, 16, 50, "gmm", False, 300)}


def _data(C, N, K):
    import gammamix_ref as R
    if N == 250 and K == 2:
        y, prior = R.golden()
        Y = np.stack([np.random.default_rng(c).permutation(y) * (1.0 + 1e-3 * c / max(C, 1)) for c in range(C)])
        return Y, [np.broadcast_to(p, (C, K)).copy() for p in prior], None
    y, prior, init = R.make_problem(77, N, K)
    return y[None], [p[None] for p in prior], [q[None] for q in init]


def bench_shape(name, repeats, once):
    import torch  # noqa: F401  (before rxhip: the process then holds ONE HIP runtime, the one torch brings, and librxhip binds to it)
    import rxhip

    if rxhip.lib().rxhip_device_count() < 1:
        raise RuntimeError("bench_gammamix: no HIP device visible")
    C, N, K, I, sched, stored, _ = SHAPES[name]
    Y, priors, inits = _data(C, N, K)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=0)          # the engine runs on this stream: the events below bracket exactly its work
    res = {"shape": {"problems": C, "N": N, "K": K, "iterations": I, "schedule": sched, "stored_log": stored}}
    if sched == "gmm":
        rng = np.random.default_rng(5)
        mu = np.linspace(-3.0 * K, 3.0 * K, K)
        y = (mu[rng.integers(K, size=N)] + rng.standard_normal(N)).astype(np.float64)
        one = np.ones(K)
        eng = rxhip.GMMEngine(N, mu0=np.zeros(K), v0=100.0 * one, a0=one, b0=one, alpha0=one, init_m_mean=mu + 0.3, init_m_var=one, init_p_shape=one, init_p_rate=one,
                              init_s_alpha=one, device=0, stream=stream.cuda_stream)
        feed = lambda: eng.set_data(y)
        bytes_per_pass = 8.0 * N
    else:
        kw = {} if inits is None else dict(init_a=inits[0], init_b=(inits[1], inits[2]), init_s=inits[3])
        eng = rxhip.GammaMixtureEngine(N, K, (priors[0], priors[1]), (priors[2], priors[3]), priors[4], n_problems=C, schedule=sched, device=0,
                                       stream=stream.cuda_stream, **kw)
        eng.set_stored_log(stored)
        feed = lambda: eng.set_data(Y, layout="chain_time")
        bytes_per_pass = (16.0 if stored else 8.0) * N * C

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
        if once:                                   # the kernel list: everything after ingest is the run
            eng.run(I, True)
            return {"once": True, "free_energy_last": float(eng.free_energy()[-1])}
        eng.run(I, True)                           # warm-up: code objects, first touch of the buffers
        runs = [timed() for _ in range(repeats)]
        res["run_ms"] = {"best": min(runs), "all": runs, "ms_per_iteration": min(runs) / I}
        fe = eng.free_energy()
        res["free_energy_first_last"] = [float(fe[0]), float(fe[-1])]
        if N == BIG:                               # per kernel, in a run of its own (an event pair around every launch)
            eng.set_profiling(True)
            eng.run(I, True)
            kt = {k: v for k, v in eng.kernel_times().items() if v["launches"]}
            eng.set_profiling(False)
            res["kernels_ms_avg"] = kt
            if "k_gmm_pass" in kt:                 # (the Gamma mixture's pass is counted under the Gaussian mixture's id: rxhip.h)
                pass_ms = kt["k_gmm_pass"]["ms_avg"]
                gbs = bytes_per_pass / (pass_ms * 1e-3) / 1e9
                res["pass"] = {"ms": pass_ms, "stream_bytes": bytes_per_pass, "stream_GB_per_s": gbs, "hbm_fraction": gbs / HBM_PEAK_GBS}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gammamix", "bench.json"))
    ap.add_argument("--child", default=None, help="(internal) run one shape in this process and print its JSON")
    ap.add_argument("--once", action="store_true", help="with --child: ingest and ONE run, no timing")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(bench_shape(a.child, a.repeats, a.once)))
        return
    res = {"hbm_peak_GB_per_s": HBM_PEAK_GBS, "configurations": {}}
    for name in a.shapes:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(a.repeats)], capture_output=True, text=True,
                             timeout=SHAPES[name][6])
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not lines:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"bench_gammamix: shape {name} ended with status {out.returncode}; nothing further is started")
        res["configurations"][name] = json.loads(lines[-1][len("RESULT "):])
        print(name, json.dumps(res["configurations"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    cf = res["configurations"]
    for a_, b_ in (("big_k2_recompute", "big_k2_stored"), ("big_k16_recompute", "big_k16_stored")):
        if a_ in cf and b_ in cf:
            print(f"{a_}: {cf[a_]['run_ms']['best']:.3f} ms, {b_}: {cf[b_]['run_ms']['best']:.3f} ms, ratio {cf[b_]['run_ms']['best'] / cf[a_]['run_ms']['best']:.2f}")
    for K in (2, 16):
        g, m = cf.get(f"big_k{K}_recompute"), cf.get(f"gmm_k{K}")
        if g and m and "pass" in g and "pass" in m:
            print(f"K = {K}: k_gammamix_pass {g['pass']['ms']:.3f} ms, k_gmm_pass {m['pass']['ms']:.3f} ms, ratio {g['pass']['ms'] / m['pass']['ms']:.2f}")


if __name__ == "__main__":
    main()

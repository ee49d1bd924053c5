#!/usr/bin/env python3
"""bench.py — BASELINE.json's metric on BASELINE config 2.

A "step" is one full belief-propagation sweep (forward + backward messages, marginals and the
Bethe free energy) of the d=4 linear Gaussian state-space model over one batch of synthetic
observations: T = 100000 steps × 1024 independent chains PER GPU (weak scaling: chains shard
across ranks with no data-path collective; the only exchange is the RCCL all-reduce of the
scalar free energy).  Chain c of the job draws its data from numpy default_rng(42 + c)
(SURVEY §8d C2); the observations are resident in HBM when the timed region starts.

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

N > 1 without a torch.distributed environment re-executes itself under torch.distributed.run
(one rank per GPU, 127.0.0.1 rendezvous); under a launcher it reads RANK/LOCAL_RANK/WORLD_SIZE.

Prints ONE JSON line (rank 0).  `value` = reference-equivalent message-rule evaluations per
second over all ranks (6 per (chain, time step) per sweep, SURVEY Appendix C — what the
reference counts as after_message_rule_call events); `ms_per_step` = milliseconds of one timed step.
A plain run sets up, warms up, times the K steps and prints that line, nothing else.

--dump-outputs DIR: after the timed steps rank 0 writes what the last step computed (dump_outputs) as DIR/<name>.npy.
--full: everything beyond the headline figure as well — the CPU baseline (before the GPU legs), a check of two chains
(first / last) against the CPU oracle after the timed region (`parity_spot`: the checker, never the thing measured),
the other BASELINE configurations and variants (`extra`, `roofline_per_chain_models`) and the detail file.
"""
import argparse
import hashlib
import json
import os
import socket
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "rxinfer.jl_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rxhip  # noqa: E402
from rxhip import workloads  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md:35); 6290 measured copy
FP64_PEAK_TFLOPS = 78.6  # fp64 vector = matrix peak of the part (confirmed by scripts/dense_micro.hip)


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rxoracle

    rxoracle.build()
    return rxoracle


def host_cores():
    """(cores this process may use, note): the scheduler affinity, capped by the cgroup CPU quota where there is one — the GPU boxes show 256
    hardware threads and grant 16 CPUs' worth of time (cpu.max = 1600000 100000): 256 OpenMP threads on that quota run 2× SLOWER than 32."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    note = f"{n} hardware threads visible"
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            q = max(1, int(round(int(quota) / int(period))))
            if q < n:
                note += f", cgroup quota cpu.max = {quota} {period} = {q} CPUs"
                n = q
    except (OSError, ValueError):
        pass
    return n, note


def cpu_baseline(mdl, y_host, sample_chains):
    """CPU restatement oracle (reference message schedule, fp64) timed on a bounded sample of THE SAME observations the
    GPU leg ran on: one thread (the reference is single-threaded) and all host cores (OpenMP over chains).
    Checker/baseline only.  Returns (baseline dict, per-chain free energies of the sampled chains)."""
    rxo = _oracle()
    T = y_host.shape[0]
    ncores, cores_note = host_cores()
    nthreads = min(2 * ncores, os.cpu_count() or 1)   # two threads per granted CPU (measured best on the quota: 65 vs 29 M rule calls/s at 32 vs 8)
    y1 = np.ascontiguousarray(y_host[:, :sample_chains])
    t0 = time.perf_counter()
    *_, fe1, cnt = rxo.lgssm_bp_batch(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], y1, free_energy=True, nthreads=1)
    dt1 = time.perf_counter() - t0
    n_all = min(y_host.shape[1], max(sample_chains, 8 * nthreads))
    ya = np.ascontiguousarray(y_host[:, :n_all])
    # result arrays with their pages already mapped (written once, outside the timed region): what is timed is the oracle's arithmetic and
    # its streaming of the results, not the first touch of ≈ 16 GB of fresh pages by every thread of the process at once
    d = mdl["A"].shape[0]
    out = (np.zeros((T, n_all, d)), np.zeros((T, n_all, d, d)))
    out[0].fill(1.0)
    out[1].fill(1.0)
    t0 = time.perf_counter()
    *_, cnta = rxo.lgssm_bp_batch(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], ya, free_energy=True, nthreads=nthreads, out=out)
    dta = time.perf_counter() - t0
    del out
    base = {"value": cnt.rule_calls / dt1, "unit": "rule-calls/s", "cores": 1, "kind": "port",
            "sample": f"chains 0..{sample_chains - 1} x T={T} of the benchmarked batch, 1 BP sweep with free energy, {dt1:.1f} s on 1 of "
                      f"{ncores} usable host cores (CPU restatement of the reference schedule, not RxInfer); the same restatement on all {ncores} cores "
                      f"({nthreads} OpenMP threads over chains 0..{n_all - 1}): {cnta.rule_calls / dta:.3e} rule-calls/s",
            "all_cores": {"value": cnta.rule_calls / dta, "unit": "rule-calls/s", "cores": ncores, "threads": nthreads, "cores_note": cores_note,
                          "sample": f"chains 0..{n_all - 1} x T={T}, OpenMP over chains ({nthreads} threads), {dta:.1f} s"}}
    return base, fe1


def parity_spot(eng, mdl, y_host, chains, missing=False):
    """HIP result vs the oracle on the same observations, at the benchmarked size: relative errors PER TIME STEP — every posterior
    mean / covariance on the scale of its own step (max |Δ| / max |reference| of that step), maximum over steps and chains.
    `missing`: the observations carry NaN rows; the checker is then the smoother with skipped updates (the schedule the
    reference runs for `missing` data, docs/src/manuals/inference/static.md:98-123), itself pinned to brute-force conditioning."""
    return _parity_check(*_parity_fetch(eng, chains), mdl, y_host, chains, missing)


def _parity_fetch(eng, chains):
    mean, cov = eng.marginals_of_chains(chains)
    return mean, cov, eng.free_energy_per_chain()


def parity_spot_deferred(eng, mdl, y_host, chains, missing=False):
    """parity_spot with the oracle on a host thread: the device results are fetched now (the engine may be closed afterwards), the
    checker runs while the bench goes on."""
    got = _parity_fetch(eng, chains)
    return Background(lambda: _parity_check(*got, mdl, y_host, chains, missing))


def _parity_check(mean, cov, fe, mdl, y_host, chains, missing):
    rxo = _oracle()
    out = {"chains": [int(c) for c in chains], "mean_rel": 0.0, "cov_rel": 0.0, "fe_rel": 0.0}
    for i, c in enumerate(chains):
        yc = np.ascontiguousarray(y_host[c] if isinstance(y_host, dict) else y_host[:, c])   # {chain: [T][dy]} or [T][chain][dy]
        if missing:
            om, oc, ofe = rxo.lgssm_kalman_rts(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], yc)
        else:
            om, oc, ofe, _ = rxo.lgssm_bp(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], yc)
        sd = np.sqrt(np.einsum("tii->ti", oc))   # posterior standard deviations: the scale of a mean error at that step
        out["mean_rel"] = max(out["mean_rel"], float(np.max(np.abs(mean[i] - om) / sd)))
        out["cov_rel"] = max(out["cov_rel"], float(np.max(np.abs(cov[i] - oc) / np.max(np.abs(oc), axis=(1, 2), keepdims=True))))
        out["fe_rel"] = max(out["fe_rel"], float(abs(fe[c] - ofe) / abs(ofe)))
    out["ok"] = bool(out["mean_rel"] < 1e-6 and out["cov_rel"] < 1e-6 and out["fe_rel"] < 1e-8)
    return out


def dump_outputs(eng, out_dir, fe_global, n_chains=32, n_steps=4096, seed=20240):
    """What a caller of the timed path receives after its last step, as float64 DIR/<name>.npy (≈ 21 MB at the headline size):
      posterior_mean [n_chains][n_steps][d], posterior_cov [n_chains][n_steps][d][d] — the posteriors of a fixed, seeded sample of this rank's
        chains at a fixed, seeded sample of time steps (both ascending; the whole posterior of the headline batch is 16 GB);
      free_energy_per_chain [chains of this rank]; free_energy [1]: the job's Bethe free energy (the sum over ranks).
    The sample depends on T and the chain count only, so two builds run with the same arguments write comparable files."""
    T, C = eng.T, eng.n_chains
    rng = np.random.default_rng(seed)
    chains = np.sort(rng.choice(C, size=min(n_chains, C), replace=False))
    steps = np.sort(rng.choice(T, size=min(n_steps, T), replace=False))
    mean, cov = eng.marginals_of_chains(chains)
    arrays = {"posterior_mean": mean[:, steps], "posterior_cov": cov[:, steps], "free_energy_per_chain": eng.free_energy_per_chain(),
              "free_energy": np.array([fe_global])}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def timed_sweeps(eng, steps, warmup, filter_run=False, repeats=2):
    """`steps` sweeps between two synchronisations, WITHOUT per-kernel instrumentation: the HIP events that give the kernel breakdown sit
    between the kernels of a sweep and cost 6 – 10 µs of queue gap each (five per sweep: ≈ 4 % of the 0.8 ms sweep of C3), so the breakdown
    comes from a second, instrumented pass that is not timed.  (The headline region keeps its events inside the timed region, as the contract
    asks: four per 5 ms sweep.)  The EXTRA lines take the better of `repeats` such measurements: a process that has just released tens of
    gigabytes of device memory (the engines of the previous lines) occasionally stalls a queue for 50–80 ms once — seen as 3–9 ms "per sweep"
    in one of several identical runs while the kernel times stayed at their 0.9 ms sum."""
    run = (lambda: eng.run_filter_async(True)) if filter_run else (lambda: eng.run_async(1, True))
    for _ in range(warmup):
        run()
    eng.sync()
    best = None
    for _ in range(max(1, repeats)):
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        eng.sync()
        dt = (time.perf_counter() - t0) / steps
        if best is None or dt < best:
            best = dt
    eng.set_profiling(True)
    kt = {}
    for _ in range(max(1, repeats)):   # the same rule for the instrumented pass: a stalled queue sits inside one kernel's event pair
        eng.reset_kernel_times()
        for _ in range(steps):
            run()
        eng.sync()
        for k, v in eng.kernel_times().items():
            if v["launches"]:
                kt[k] = min(kt.get(k, float("inf")), round(v["ms_avg"], 4))
    eng.set_profiling(False)
    return best * 1e3, kt


def timing_mode(repeats):
    """How an extra line was timed: the headline region is timed once, as the contract says; the extra lines take the better of two
    such measurements (timed_sweeps).  Every line says which."""
    return "single" if repeats <= 1 else f"min_of_{repeats}"


class Background:
    """A checker that runs on a host thread while the bench goes on (the C oracle releases the GIL): `parity_spot` of the d = 64 chain
    is ≈30 s of one CPU core — outside every timed region, and joined before the JSON line is printed."""

    live = []   # every checker started so far

    @classmethod
    def quiesce(cls):
        """Wait for the checkers started so far: the legs that measure HOST-side latency (a first touch, an `infer(...)` call) run on an
        idle host — under the box's CPU quota (16 CPUs, cgroup) a checker's threads get the timed thread throttled for tens of ms."""
        for b in cls.live:
            b.t.join()

    def __init__(self, fn):
        self.out = None
        Background.live.append(self)

        def run():
            try:
                self.out = fn()
            except Exception as e:  # noqa: BLE001
                self.out = {"error": repr(e), "ok": False}

        self.t = threading.Thread(target=run, daemon=True)
        self.t.start()

    def result(self):
        self.t.join()
        return self.out


def extra_per_chain_models(mdl, T, C, y_dev, device, y_host=None, steps=3):
    """The same batch with one constant set PER CHAIN (n_models = n_chains): nothing is shared between chains, every chain
    stores and re-reads its full forward message, SURVEY's 416 B/U applies unmodified."""
    tile = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (C,) + np.shape(a)).copy()
    eng = rxhip.LGSSMEngine(tile(mdl["A"]), tile(mdl["B"]), tile(mdl["P"]), tile(mdl["Q"]), tile(mdl["m0"]), tile(mdl["V0"]), T=T,
                            n_chains=C, chain_model=np.arange(C, dtype=np.int32), device=device)
    eng.set_data_device(y_dev.data_ptr(), y_dev.numel(), keepalive=y_dev)
    ms, kt = timed_sweeps(eng, steps, 1)
    spot = parity_spot(eng, mdl, y_host, [0, C - 1] if C > 1 else [0]) if y_host is not None else None
    eng.close()
    units = T * C
    b_bwd, b_sweep = 272, 416
    k = kt.get("k_backward", 0.0)
    return {"ms_per_step": ms, "kernels_ms_avg": kt, "bound": "hbm", "kernel": "k_backward", "bytes_per_U": b_bwd,
            "achieved": b_bwd * units / (k * 1e-3) / 1e9 if k else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": b_bwd * units / (k * 1e-3) / 1e9 / HBM_PEAK_GBS if k else None,
            "sweep_bytes_per_U": b_sweep, "sweep_achieved": b_sweep * units / (ms * 1e-3) / 1e9,
            "sweep_frac": b_sweep * units / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "rule_calls_per_s": (6 * T - 3) * C / (ms * 1e-3), "parity_spot": spot, "timing": timing_mode(2),
            # SURVEY's algorithmic bytes are charged unmodified (272 B/U for the backward sweep, 416 for the sweep).  Since round 4 a time-invariant chain stops
            # computing, writing and reading what has reached its fixed point: behind the fixed point of V_f the forward records carry the mean only,
            # so the backward kernel MOVES ≈ 160 (posterior) + 32 (mean record) B/U and the sweep ≈ 32 + 32 + 32 + 160 + the element pass's 32 — `frac` and
            # `sweep_frac` are throughput in reference-equivalent bytes (they may exceed what the HBM can do), `moved_frac` is the kernel's own traffic estimate
            "moved_bytes_per_U_estimate": 192, "moved_frac": 192 * units / (k * 1e-3) / 1e9 / HBM_PEAK_GBS if k else None}


def extra_c1(device, with_cpu=True):
    """BASELINE config 1 (the reference's own CPU-runnable case): d = 4, T = 1000, one chain — `infer(...)` END TO END per call
    (engine construction, host → device, sweep + free energy, device → host), next to the CPU restatement on the same data
    (the cpu_baseline leg of this config: checker and baseline, never the product path)."""
    mdl = workloads.c1_model()
    _, y = workloads.generate_chain(mdl, 1000, 42)
    Background.quiesce()
    spec = rxhip.linear_gaussian_ssm(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"])
    rxhip.infer(model=spec, data={"y": y}, free_energy=True, options={"device": device})
    best = 1e9
    for _ in range(10):
        t0 = time.perf_counter()
        res = rxhip.infer(model=spec, data={"y": y}, free_energy=True, options={"device": device})
        best = min(best, time.perf_counter() - t0)
    # the same with the engine pool switched off (csrc/rxhip.hip: rxhip_destroy parks a small engine, the next rxhip_lgssm_create of a byte-identical
    # descriptor takes it back): every call then builds its tables, takes an arena and a stream, uploads, and gives them back
    os.environ["RXHIP_TEST_HOOKS"], os.environ["RXHIP_ENGINE_POOL"] = "1", "0"
    cold = 1e9
    try:
        for _ in range(10):
            t0 = time.perf_counter()
            rxhip.infer(model=spec, data={"y": y}, free_energy=True, options={"device": device})
            cold = min(cold, time.perf_counter() - t0)
    finally:
        os.environ.pop("RXHIP_ENGINE_POOL", None)
        os.environ.pop("RXHIP_TEST_HOOKS", None)
    out = {"workload": "LGSSM d=4 T=1000, 1 chain: infer(...) end to end (engine for the model + H2D + sweep + free energy + D2H), minimum of 10",
           "infer_ms": best * 1e3, "rule_calls_per_s": (6 * 1000 - 3) / best, "timing": "min_of_10",
           "engine": "the second and later calls of a process with the same model take the parked engine of the previous call (engine pool)",
           "infer_ms_engine_built_per_call": cold * 1e3}
    if with_cpu:
        rxo = _oracle()
        t0 = time.perf_counter()
        om, oc, ofe, cnt = rxo.lgssm_bp(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], y)
        cpu = time.perf_counter() - t0
        out["cpu_baseline"] = {"ms": cpu * 1e3, "kind": "port", "cores": 1,
                               "mean_rel_vs_gpu": float(np.max(np.abs(res.posteriors["x"].mean - om)) / np.max(np.abs(om))),
                               "free_energy_rel_vs_gpu": float(abs(res.free_energy[-1] - ofe) / abs(ofe))}
    return out


def extra_missing(mdl, T, C, y, device, y_host=None):
    """The C2 batch with 10 % of the observations `missing` (masked, table-free schedule)."""
    yy = y.clone()
    mask = torch.rand((T, C), device=yy.device, generator=torch.Generator(device=yy.device).manual_seed(0)) < 0.1
    yy[mask] = float("nan")
    eng = rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C, device=device, allow_missing=True)
    eng.set_data_device(yy.data_ptr(), yy.numel(), keepalive=yy)
    ms, kt = timed_sweeps(eng, 5, 2)
    spot = None
    if y_host is not None:   # the two checked chains with the SAME mask, on the host
        chains = [0, C - 1] if C > 1 else [0]
        cols = {}
        for c in chains:
            yc = np.array(y_host[:, c], copy=True)
            yc[mask[:, c].cpu().numpy()] = np.nan
            cols[c] = yc
        spot = parity_spot(eng, mdl, cols, chains, missing=True)
    eng.close()
    return {"workload": f"the headline batch with 10 % of the observations missing (T={T}, {C} chains), 1 BP sweep + free energy",
            "ms_per_step": ms, "kernels_ms_avg": kt, "steps_per_s": T * C / (ms * 1e-3), "parity_spot": spot, "timing": timing_mode(2)}


def extra_c3(device, parity=True):
    """BASELINE config 3: d = dy = 64, T = 10^4, one chain — the MFMA path."""
    mdl = workloads.c3_model()
    T, d = 10000, 64
    y = workloads.generate_batch(mdl, T, 1, seed0=6400)
    Background.quiesce()
    # a throwaway engine of ANOTHER d = 64 model first: the first launch of a kernel loads its code object (a property of the
    # process); the model timed below has never been seen by any engine, so its tables are built, not fetched from the cache
    with rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"] * 1.5, mdl["Q"], mdl["m0"], mdl["V0"], T=400, n_chains=1, device=device) as warm:
        warm.set_data(y[:400])
        warm.run(1, True)
    t0 = time.perf_counter()
    eng = rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=1, device=device)
    t1 = time.perf_counter()
    eng.set_data(y)
    t2 = time.perf_counter()
    eng.run(1, True)
    t3 = time.perf_counter()
    create_ms = (t3 - t0) * 1e3
    first_split = {"create_ms": (t1 - t0) * 1e3, "set_data_ms": (t2 - t1) * 1e3, "first_run_ms": (t3 - t2) * 1e3}
    cstages = eng.create_stages()
    ms, kt = timed_sweeps(eng, 20, 3)
    spot = parity_spot_deferred(eng, mdl, y, [0]) if parity else None   # the timed engine against the oracle's reference schedule over the whole chain (≈30 s of one host core, on a thread)
    fms, _ = timed_sweeps(eng, 10, 2, filter_run=True)
    eng.close()
    # The same sweep with everything data-independent hoisted (the model / data split that batches of one model take by default, DESIGN
    # §6b): the matrices of the smoother are computed once per engine, a sweep is vectors only — what a user with iterations > 1 pays per
    # iteration, next to the figure above, in which every sweep recomputes every message as the reference does.
    hoisted = None
    os.environ["RXHIP_DENSE_SPLIT"], os.environ["RXHIP_TEST_HOOKS"] = "1", "1"   # (a schedule switch: read only together with RXHIP_TEST_HOOKS)
    try:
        with rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=1, device=device) as eh:
            eh.set_data(y)
            eh.run(1, True)
            hms, hkt = timed_sweeps(eh, 20, 3)
            hoisted = {"ms_per_step": hms, "kernels_ms_avg": hkt, "timing": timing_mode(2),
                       "note": "data-independent matrices once per engine (model pass), vectors per sweep"}
    except Exception as e:  # noqa: BLE001
        hoisted = {"error": repr(e)}
    finally:
        os.environ.pop("RXHIP_DENSE_SPLIT", None)
        os.environ.pop("RXHIP_TEST_HOOKS", None)
    # Flop counts.  ref: SURVEY §8d's reference-schedule count (18 d³ per step).  mfma: what the matrix pipe executes, from the
    # instruction counts of the shipped kernels — v_mfma_f64_16x16x4_f64 = 2048 flop; per time step and workgroup (4 waves):
    # forward 4·76 (panel inverse: 4·4 tile-inverse rounds, 12 row block, 3·(4 + 16) panel updates) + 4·64 (G' = K C) + 160
    # (M = PLW − K G, 10 of 16 tiles: symmetric) = 720, + 16 where the tile inverses are seeded (4·8 products of a Newton – Schulz step instead of 4·4
    # rank-4 rounds: every step but a segment's first once the Riccati recursion has converged — 19 of 20 here) = 736; backward 256 (J' = C K') + 160 (V_s = C + J V_s J', 10 of 16 tiles) = 416; residual forms of the free energy 256 per 16 steps;
    # aggregation GEMM [2d × L·dy]·[L·dy × S] ≈ 8 per step — confirmed by SQ_INSTS_VALU_MFMA_F64 (profiles/r04/pmc_c3.txt).  The round-2 kernels
    # executed 768 + 512 (bench counted 12 d³ = 1536 per step, the counters said 1280).
    mfma_step = {"kd_forward_info": 736, "kd_backward_info": 416, "kd_fe_resid_mfma": 16, "kd_agg_gemm": 8}
    mfma_flop = sum(mfma_step.values()) * 2048 * T
    ref_flop = 18 * d ** 3 * T
    tf = lambda flop, t_ms: flop / (t_ms * 1e-3) / 1e12
    fwd_ms, bwd_ms = kt.get("k_forward", 0.0), kt.get("k_backward", 0.0)
    # Since round 4 the sweep kernels leave the matrix work of a segment once its matrices repeat, so the MFMA work a sweep EXECUTES is no longer
    # T x the per-step counts above.  The roofline figure of this line is therefore built from what the matrix pipe was measured to execute:
    # SQ_INSTS_VALU_MFMA_F64 per launch of every sweep kernel (profiles/mfma_insts.json, collected by scripts/profile_r05.sh on this very
    # workload, guarded by the hash of dense_kernels.hpp: a stale file gives null, never an old number) x 2048 flop / the kernel times of THIS
    # run.  `frac` = executed MFMA flops of the sweep / sweep time / fp64 peak — a utilisation; the reference-equivalent rate (SURVEY's 18 d^3
    # per step over the sweep time: work done for the user, which passes 1 when products are skipped) is reported under its own key.
    executed, stale_mfma = None, None
    mpath = os.path.join(ROOT, "profiles", "mfma_insts.json")
    try:
        mj = json.load(open(mpath))
        with open(os.path.join(ROOT, "rxinfer.jl_amd", "csrc", "dense_kernels.hpp"), "rb") as f:
            stale_mfma = mj.get("dense_kernels_sha256") != hashlib.sha256(f.read()).hexdigest()
        if not stale_mfma:
            executed = {k: float(v) for k, v in mj["mfma_f64_per_launch"].items()}
    except (OSError, ValueError, KeyError):
        pass
    roof = {"bound": "mfma", "kernel": "kd_forward_info", "ms": ms, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s (executed v_mfma_f64_16x16x4_f64 x 2048 flop)",
            "achieved": None, "frac": None, "per_kernel": None, "full_step_mfma": mfma_step,
            "reference_equivalent": {"flop": ref_flop, "tflops": tf(ref_flop, ms), "frac_of_peak": tf(ref_flop, ms) / FP64_PEAK_TFLOPS,
                                     "note": "SURVEY 8d's 18 d^3 per step over the sweep time: a rate of work done for the user, not a utilisation"},
            "source": "profiles/mfma_insts.json (rocprofv3 --pmc SQ_INSTS_VALU_MFMA_F64, scripts/profile_r05.sh)" + (" — STALE: dense_kernels.hpp changed since the counters were collected" if stale_mfma else "")}
    if executed:
        ex_flop = 2048.0 * sum(executed.values())
        # kernel names of the profile -> the engine's timing slots (k_forward = kd_forward_info, k_backward = kd_backward_info)
        per = {}
        for kn, slot in (("kd_forward_info", "k_forward"), ("kd_backward_info", "k_backward")):
            if kn in executed and kt.get(slot):
                per[kn] = {"mfma_insts": executed[kn], "ms": kt[slot], "tflops": tf(2048.0 * executed[kn], kt[slot]), "frac": tf(2048.0 * executed[kn], kt[slot]) / FP64_PEAK_TFLOPS}
        roof.update({"flop": ex_flop, "achieved": tf(ex_flop, ms), "frac": tf(ex_flop, ms) / FP64_PEAK_TFLOPS, "per_kernel": per,
                     "note": "executed MFMA flops of ALL sweep kernels over the sweep time; inside full (non-repeating) steps the matrix pipe is busy 0.47 of the time (profiles/r04/pmc_c3.txt)"})
    return {"workload": "LGSSM d=64 dy=64 T=10000, 1 chain, 1 BP sweep + Bethe free energy per step", "ms_per_step": ms,
            "kernels_ms_avg": kt, "tflops_ref_count": tf(ref_flop, ms), "ref_flop_per_sweep": ref_flop,
            "mfma_flop_per_sweep_if_every_step_were_full": mfma_flop,
            "peak_tflops_fp64": FP64_PEAK_TFLOPS, "frac": roof["frac"],
            "frac_ref_count": tf(ref_flop, ms) / FP64_PEAK_TFLOPS,
            "roofline": roof, "filter_ms_per_step": fms, "timing": timing_mode(2), "parity_spot": spot,
            "hoisted_matrices": hoisted,
            "create_set_data_first_run_ms": create_ms, "create_set_data_first_run_split_ms": first_split, "create_stages_ms": cstages,
            "create_note": "a model no engine of the process has seen: tables built on the device (csrc/dense_tab_kernels.hpp)"}


def extra_node_array(device, parity=True):
    """Not a BASELINE config — the level-scheduled node-array executor (SURVEY §7's design stance) on a graph OUTSIDE the
    pattern-matched families: the benchmark chain with TWO observation branches per state (`rxhip_create` used to answer RXHIP_ERR_UNSUPPORTED),
    d = 4, dy = 2 + 2, T = 128 time steps × 65 536 replicas (workgroup-resident levels, 128 replicas per workgroup: the executor's schedule at this batch; the same
    graph at T = 256 × 4096 replicas — workgroup-resident levels, latency-bound — is in profiles/r05/tree_modes.txt), one sum-product sweep + Bethe free
    energy per step; and the plain state-space chain
    of the same size through the executor next to the specialised engine.  Rates: reference-equivalent rule calls (the messages the named
    marginals pull in) per second; HBM fraction on the algorithmic bytes of the executor's own schedule, 8·(d + d(d+1)/2) per message a rule reads
    or writes (rxhip_tree_info.bytes_per_sweep)."""
    from rxhip.graph import lgssm_graph, two_branch_chain_graph
    from rxhip.tree import TreeEngine
    mdl = workloads.c1_model()
    T, R, d = 128, 65536, 4
    B1, B2 = mdl["B"][:2], mdl["B"][2:]
    Q1, Q2 = mdl["Q"][:2, :2], mdl["Q"][2:, 2:]
    y = np.random.default_rng(777).standard_normal((T, R, 4)) * 3.0      # [T][R][4]: the two branches observe halves of the same y (timing does not depend on the values)
    rows = np.ascontiguousarray(np.transpose(y, (1, 0, 2))).reshape(R, T * 4)
    out = {"workload": f"two observation branches per state (d=4, dy=2+2), T={T}, {R} replicas: 1 sum-product sweep + Bethe free energy on the node-array executor"}
    for name, build in (("two_branch", lambda: two_branch_chain_graph(T, mdl["A"], B1, B2, mdl["P"], Q1, Q2, mdl["m0"], mdl["V0"])),
                        ("plain_chain", lambda: lgssm_graph(T, mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"]))):
        t0 = time.perf_counter()
        gb, xs, ys = build()
        t1 = time.perf_counter()
        eng = TreeEngine(gb, n_replicas=R, device=device)
        t2 = time.perf_counter()
        eng.set_data(ys, rows)
        eng.run(1, True)
        best, dev = 1e9, 1e9
        for _ in range(5):
            t = time.perf_counter()
            eng.run(1, True)
            best = min(best, time.perf_counter() - t)
            dev = min(dev, eng.last_iteration_ms())
        cnt, info = eng.counters(), eng.info
        moved = (info["bytes_per_sweep"] + info["fe_bytes_per_sweep"]) * R       # what this schedule moves through HBM per iteration: the sweep's messages + the second phase
        line = {"ms_per_step": best * 1e3, "device_ms_per_step": dev, "rule_calls_per_s": cnt["rule_calls"] / (dev * 1e-3),
                "graph_build_ms": (t1 - t0) * 1e3, "compile_and_allocate_ms": (t2 - t1) * 1e3, "info": info,
                "roofline": {"bound": "hbm", "achieved": moved / (dev * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": moved / (dev * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                             # the floor of ANY schedule on this graph: the data in, the posteriors of the named variables out (rxhip_tree_info.io_bytes_per_sweep)
                             "io_frac": info["io_bytes_per_sweep"] * R / (dev * 1e-3) / 1e9 / HBM_PEAK_GBS, "moved_over_io": moved / (info["io_bytes_per_sweep"] * R),
                             "bytes": "messages a rule, product or marginal of the schedule reads from / writes to HBM (register hand-overs along a strand left out) + what the Bethe "
                                      "phase reads and writes (rxhip_tree_info.bytes_per_sweep + fe_bytes_per_sweep) × replicas"}}
        if name == "two_branch":   # HBM bytes of an iteration's launches by the PMC counters (profiles/tree_traffic.json, guarded by the hash of tree_kernels.hpp)
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", "tree_traffic.json")))
                with open(os.path.join(ROOT, "rxinfer.jl_amd", "csrc", "tree_kernels.hpp"), "rb") as f:
                    fresh = tj.get("tree_kernels_sha256") == hashlib.sha256(f.read()).hexdigest()
                if fresh and tj.get("moved_bytes_per_sweep") == moved and tj.get("hbm_bytes_per_iteration"):
                    line["roofline"]["traffic"] = tj["hbm_bytes_per_iteration"]
                    line["roofline"]["traffic_note"] = f"FETCH_SIZE x {tj.get('fetch_factor_8B_per_lane'):.3g} (calibrated for 8 B/lane unit-stride loads, scripts/fetch_calib.hip) + WRITE_SIZE over all launches of an iteration"
            except (OSError, ValueError, KeyError, TypeError):
                pass
        if parity and name == "two_branch":
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import tree_oracle
            post = eng.marginals(xs)
            fe = eng.free_energy_per_replica()
            spot = {"replicas": [0, R - 1], "mean_rel": 0.0, "cov_rel": 0.0, "fe_rel": 0.0}
            for r in (0, R - 1):
                data, o = {}, 0
                for v in ys:
                    data[v] = rows[r, o:o + gb.rows[v]]
                    o += gb.rows[v]
                ref = tree_oracle.infer(gb.to_dump(), data)
                for v in xs:
                    sd = np.sqrt(np.diag(ref["cov"][v]))
                    spot["mean_rel"] = max(spot["mean_rel"], float(np.max(np.abs(post[v][0][r] - ref["mean"][v]) / sd)))
                    spot["cov_rel"] = max(spot["cov_rel"], float(np.max(np.abs(post[v][1][r] - ref["cov"][v]) / np.outer(sd, sd))))
                spot["fe_rel"] = max(spot["fe_rel"], float(abs(fe[r] - ref["fe"][0]) / abs(ref["fe"][0])))
            spot["ok"] = bool(spot["mean_rel"] < 1e-6 and spot["cov_rel"] < 1e-6 and spot["fe_rel"] < 1e-8)
            line["parity_spot"] = spot
        eng.close()
        out[name] = line
    # the same plain chain on the specialised engine (the fast path the pattern matcher picks)
    with rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=R, device=device) as ref:
        ref.set_data(y)
        ref.run(1, True)
        ms, _ = timed_sweeps(ref, 10, 2)
    out["plain_chain"]["specialised_engine_ms_per_step"] = ms
    out["ms_per_step"] = out["two_branch"]["device_ms_per_step"]
    # above d = 8 the rules run on the LDS-staged kernels (work items of 1 / 2 / 4 wavefronts per op and replica, products and the inverse on the fp64 matrix
    # cores, csrc/tree_wave_kernels.hpp): time, rule calls per second, a parity spot against the generic CPU restatement — and, for the d = 64 workload the
    # PMC pass was taken on, the executed v_mfma_f64_16x16x4_f64 instructions over the time against the fp64 MFMA peak (profiles/tree_mfma.json, hash-guarded)
    for dd, T_, R_ in ((16, 64, 4096), (32, 32, 2048), (64, 16, 256)):   # (the sizes VERDICT r5 "Next 3" set its bars on: ≤ 10 / 15 / 12 ms)
        mm = workloads.random_model(dd, dd, seed=100 * dd + dd)
        h = dd // 2
        gb, xs, ys = two_branch_chain_graph(T_, mm["A"], mm["B"], mm["B"][:h], mm["P"], mm["Q"], mm["Q"][:h, :h], mm["m0"], mm["V0"])
        rows_ = np.random.default_rng(778).standard_normal((R_, T_ * (dd + h))) * 2.0
        with TreeEngine(gb, n_replicas=R_, device=device) as eng:
            eng.set_data(ys, rows_)
            eng.run(1, True)
            dev = 1e9
            for _ in range(3):
                eng.run(1, True)
                dev = min(dev, eng.last_iteration_ms())
            fam = {0: "a lane per item", 1: "a wavefront per item on register tiles (tree_tile_kernels.hpp)", 2: "a workgroup per item on LDS tiles (tree_wave_kernels.hpp)"}[eng.info["kernels"]]
            line = {"workload": f"two observation branches per state (d={dd}, dy={dd}+{h}), T={T_}, {R_} replicas: 1 sweep + Bethe free energy; {fam}",
                    "device_ms_per_step": dev, "rule_calls_per_s": eng.counters()["rule_calls"] / (dev * 1e-3), "info": eng.info}
            if dd == 64:
                try:
                    tj = json.load(open(os.path.join(ROOT, "profiles", "tree_mfma.json")))
                    with open(os.path.join(ROOT, "rxinfer.jl_amd", "csrc", "tree_wave_kernels.hpp"), "rb") as f:
                        fresh = tj.get("tree_wave_kernels_sha256") == hashlib.sha256(f.read()).hexdigest()
                    if fresh and tj.get("workload") == {"d": dd, "T": T_, "replicas": R_} and tj.get("mfma_f64_per_iteration"):
                        tf = tj["mfma_f64_per_iteration"] * tj["flop_per_instruction"] / (dev * 1e-3) / 1e12
                        line["roofline"] = {"bound": "mfma", "achieved": tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s (executed v_mfma_f64_16x16x4_f64 x 2048 flop)",
                                            "frac": tf / FP64_PEAK_TFLOPS, "mfma_frac": tf / FP64_PEAK_TFLOPS, "mfma_insts_per_iteration": tj["mfma_f64_per_iteration"],
                                            "source": tj.get("source")}
                except (OSError, ValueError, KeyError):
                    pass
            if parity:
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import tree_oracle
                post, fe = eng.marginals(xs), eng.free_energy_per_replica()
                r = R_ - 1
                data, o = {}, 0
                for v in ys:
                    data[v] = rows_[r, o:o + gb.rows[v]]
                    o += gb.rows[v]
                ref = tree_oracle.infer(gb.to_dump(), data)
                em = max(float(np.max(np.abs(post[v][0][r] - ref["mean"][v]) / np.sqrt(np.diag(ref["cov"][v])))) for v in xs)
                ef = float(abs(fe[r] - ref["fe"][0]) / abs(ref["fe"][0]))
                line["parity_spot"] = {"replica": r, "mean_rel": em, "fe_rel": ef, "ok": bool(em < 1e-6 and ef < 1e-8)}
        out[f"two_branch_d{dd}"] = line
    # a mixture layer as ops of the executor: the reference's multivariate mixture model (test/models/mixtures/gmm_multivariate_tests.jl:6-32, K = 3, d = 2) as a graph of
    # one NormalMixture + one Categorical node per data point, N = 200 points x 4096 replicas (independent data sets), per VMP iteration; the specialised mixture engine
    # (sufficient statistics over ONE data set) on replica 0's data next to it
    try:
        from rxhip.graph import mv_mixture_graph
        K, dm, N, Rm, its = 3, 2, 200, 4096, 5
        rng = np.random.default_rng(779)
        cent = np.array([[6.0, 0.0], [-4.0, 5.0], [0.0, -6.0]])
        ym = cent[rng.integers(0, K, size=(Rm, N))] + rng.standard_normal((Rm, N, dm))
        mu0, S0 = cent + rng.standard_normal((K, dm)), np.array([1e2 * np.eye(dm)] * K)
        nu0, V0, al0 = np.array([3.0] * K), np.array([0.1 * np.eye(dm)] * K), np.ones(K)
        gb, ys = mv_mixture_graph(N, mu0, S0, nu0, V0, al0, init=dict(m=(mu0, S0), w=(nu0, V0), s=np.ones(K)))
        with TreeEngine(gb, n_replicas=Rm, device=device) as eng:
            eng.set_data(ys, ym.reshape(Rm, N * dm))
            eng.run(its, True)
            dev = 1e9
            for _ in range(3):
                eng.run(its, True)
                dev = min(dev, eng.last_iteration_ms())
            fe_exec = eng.free_energy_per_replica()
            line = {"workload": f"NormalMixture layer as executor ops: K={K}, d={dm}, N={N} points (a mixture + a Categorical node each), {Rm} replicas, {its} VMP iterations",
                    "device_ms_per_step": dev, "rule_calls_per_s": eng.counters()["rule_calls"] / its / (dev * 1e-3), "info": eng.info,
                    "points_per_s": N * Rm / (dev * 1e-3)}
            with rxhip.MvGMMEngine(N, mu0, S0, nu0, V0, al0, mu0, S0, nu0, V0, np.ones(K), device=device) as ref:
                ref.set_data(ym[0])
                ref.run(its, True)
                fe_ref = ref.free_energy()
            line["specialised_engine_fe_rel"] = float(abs(fe_exec[0] - fe_ref[-1]) / abs(fe_ref[-1]))
            if parity:
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import tree_oracle
                r = Rm - 1
                ref = tree_oracle.infer(gb.to_dump(), {ys[i]: ym[r, i] for i in range(N)}, iterations=its)
                g_ = tree_oracle.TreeGraph(gb.to_dump())
                ms_ = g_.mixtures[0]["m"]
                post = eng.marginals(ms_)
                em = max(float(np.max(np.abs(post[v][0][r] - ref["mean"][v]) / np.sqrt(np.diag(ref["cov"][v])))) for v in ms_)
                ef = float(abs(fe_exec[r] - ref["fe"][-1]) / abs(ref["fe"][-1]))
                line["parity_spot"] = {"replica": r, "mean_rel": em, "fe_rel": ef, "ok": bool(em < 1e-6 and ef < 1e-8 and line["specialised_engine_fe_rel"] < 1e-8)}
        out["mixture_layer"] = line
    except Exception as e:   # (an extra: never the headline's problem)
        out["mixture_layer"] = {"error": repr(e)[:300]}
    # GCV as an executor op: the reference's HGF step graph (test/models/statespace/hgf_tests.jl:9-31: data-valued prior means and variances, GCV under q(y, x) q(z), 31-point
    # cubature) as an ONLINE filter — 4096 independent series, one observation per call, rxhip_tree_continue keeps the node's precision state, the posteriors are fed back
    # as the next priors ON THE HOST (that round trip is in the wall time, not in the device time); 5 VMP iterations per observation; series 0 against the restatement
    try:
        from rxhip.graph import hgf_step_graph
        kap, om, zv_, yv_, its, Th, Rh = 1.0, 0.0, 0.04, 0.01, 5, 20, 4096
        yh = np.cumsum(np.random.default_rng(780).standard_normal((Th, Rh)), axis=0) * 0.3
        gb, names = hgf_step_graph(kap, om, zv_, yv_, q_zt=(0.0, 5.0), q_xt=(0.0, 5.0), n_gh=31)
        dvars = [v for v in range(len(gb.kind)) if gb.kind[v] == 1]
        qz = np.tile([0.0, 5.0], (Rh, 1))
        qx = np.tile([0.0, 5.0], (Rh, 1))
        dev_ms, t0 = [], time.perf_counter()
        with TreeEngine(gb, n_replicas=Rh, device=device) as eng:
            eng.continue_runs(True)
            for t in range(Th):
                eng.set_data(dvars, np.column_stack([qz[:, 0], qz[:, 1], qx[:, 0], qx[:, 1], yh[t]]))
                eng.run(its, True)
                dev_ms.append(eng.last_iteration_ms() * its)
                post = eng.marginals([names["zt"], names["xt"]])
                qz = np.column_stack([post[names["zt"]][0][:, 0], post[names["zt"]][1][:, 0, 0]])
                qx = np.column_stack([post[names["xt"]][0][:, 0], post[names["xt"]][1][:, 0, 0]])
            info = eng.info
        wall = (time.perf_counter() - t0) / Th
        line = {"workload": f"GCV as an executor op: the HGF step graph as an online filter, {Rh} series, {its} VMP iterations per observation, {Th} observations",
                "device_ms_per_step": float(np.median(dev_ms)), "wall_ms_per_observation": wall * 1e3, "observations_per_s": Rh / (float(np.median(dev_ms)) * 1e-3), "info": info}
        if parity:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import rxoracle
            zm, zvv, xm, xvv, _, _ = rxoracle.hgf_filter(np.ascontiguousarray(yh[:, 0]), kap, om, zv_, yv_, vmp_iters=its, n_gh=31)
            em = max(abs(qz[0, 0] - zm[-1]) / np.sqrt(zvv[-1]), abs(qx[0, 0] - xm[-1]) / np.sqrt(xvv[-1]))
            ev = max(abs(qz[0, 1] - zvv[-1]) / zvv[-1], abs(qx[0, 1] - xvv[-1]) / xvv[-1])
            line["parity_spot"] = {"series": 0, "mean_rel": float(em), "cov_rel": float(ev), "ok": bool(em < 1e-6 and ev < 1e-6)}
        out["hgf_online_filter"] = line
    except Exception as e:
        out["hgf_online_filter"] = {"error": repr(e)[:300]}
    return out


def extra_noise_vmp(device, parity=True):
    """Not a BASELINE config — the first composed graph: the benchmark chain with an unknown observation-noise precision,
    W ~ Wishart, q(x, W) = q(x) q(W): d = dy = 4, 1024 chains × T = 10⁴, 10 VMP iterations (one BP sweep of every chain + every chain's Wishart
    update per iteration, all on the device), with the free energy per iteration.  Here a VMP iteration is NOT an idempotent sweep."""
    mdl = workloads.c1_model()
    T, C, iters, dy = 10000, 1024, 10, 4
    y = workloads.generate_batch(mdl, T, C, seed0=4242, threads=min(32, os.cpu_count() or 1))
    nu0, S0 = dy + 1.0, np.eye(dy)
    eng = rxhip.LGSSMNoiseEngine(mdl["A"], mdl["B"], mdl["P"], mdl["m0"], mdl["V0"], T, nu0, S0, n_chains=C, device=device)
    eng.set_data(y)
    eng.run(iters, True)
    ms = 1e9
    for _ in range(2):
        t0 = time.perf_counter()
        eng.run_async(iters, True)
        eng.sync()
        ms = min(ms, (time.perf_counter() - t0) * 1e3)
    fe = eng.free_energy()
    spot = None
    if parity:
        chains = [0, C - 1]
        mean, cov = eng.marginals_of_chains(chains)
        fec = eng.free_energy_per_chain()
        nu, V = eng.noise_posterior()

        def check():
            rxo = _oracle()
            out = {"chains": chains, "mean_rel": 0.0, "cov_rel": 0.0, "fe_rel": 0.0, "w_rel": 0.0}
            for i, c in enumerate(chains):
                om, oc, wh, ofe = rxo.lgssm_noise_vmp(mdl["A"], mdl["B"], mdl["P"], mdl["m0"], mdl["V0"], np.ascontiguousarray(y[:, c]), nu0, S0, nu0, S0, iters)
                sd = np.sqrt(np.einsum("tii->ti", oc))
                out["mean_rel"] = max(out["mean_rel"], float(np.max(np.abs(mean[i] - om) / sd)))
                out["cov_rel"] = max(out["cov_rel"], float(np.max(np.abs(cov[i] - oc) / np.max(np.abs(oc), axis=(1, 2), keepdims=True))))
                out["fe_rel"] = max(out["fe_rel"], float(abs(fec[c] - ofe[-1]) / abs(ofe[-1])))
                out["w_rel"] = max(out["w_rel"], float(np.max(np.abs(V[c] - wh[-1, 1:].reshape(dy, dy)) / np.max(np.abs(wh[-1, 1:])))))
            out["ok"] = bool(out["mean_rel"] < 1e-6 and out["cov_rel"] < 1e-6 and out["fe_rel"] < 1e-8 and out["w_rel"] < 1e-8)
            return out

        spot = Background(check)
    eng.close()
    return {"workload": f"LGSSM d=4 dy=4 T={T}, {C} chains, unknown observation-noise precision W ~ Wishart({nu0:g}, I), q(x, W) = q(x)q(W): {iters} VMP iterations "
                        "(BP sweep + Wishart update per chain and iteration) with the Bethe free energy per iteration",
            "ms_per_iteration": ms / iters, "vmp_iters_per_sec": iters / (ms * 1e-3), "rule_calls_per_s": (6 * T - 3) * C * iters / (ms * 1e-3),
            "free_energy_first_last": [float(fe[0]), float(fe[-1])], "free_energy_monotone": bool(np.all(np.diff(fe) <= 1e-9 * np.abs(fe[:-1]))),
            "timing": timing_mode(2), "parity_spot": spot}


def extra_masked(device):
    """Not BASELINE configs: `missing` observations and per-step constants at d = 64 on the masked MFMA schedule
    (csrc/dense_mseg_kernels.hpp) next to the fully observed sweep of the same chain — median of five sweeps each
    (rounds 1–2 ran these engines sequentially in time: ≈700 ms)."""
    d, T = 64, 2000
    m = workloads.random_model(d, d, seed=d)
    y = workloads.generate_batch(m, T, 1, seed0=1)
    one = (m["A"], m["B"], m["P"], m["Q"], m["m0"], m["V0"])

    def med(eng):
        eng.run(1, True)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            eng.run(1, True)
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[2]

    out = {"workload": "LGSSM d=64 dy=64 T=2000, 1 chain, 1 BP sweep + free energy", "timing": "median_of_5"}
    with rxhip.LGSSMEngine(*one, T=T, n_chains=1, device=device) as eng:
        eng.set_data(y)
        out["fully_observed_ms"] = med(eng)
    ym = y.copy()
    ym[np.random.default_rng(0).random((T, 1)) < 0.1] = np.nan
    with rxhip.LGSSMEngine(*one, T=T, n_chains=1, allow_missing=True, device=device) as eng:
        eng.set_data(ym)
        out["missing_10pct_ms"] = med(eng)
        out["missing_10pct_schedule"] = eng.schedule()   # segments × segment length of the element pass (log-depth boundary recursion over them)
        out["missing_10pct_parity_spot"] = parity_spot(eng, m, ym, [0], missing=True)   # the timed engine against the oracle, after the timing
    ms = [workloads.random_model(d, d, seed=d + 7 * k) for k in range(4)]
    mdl = tuple(np.stack([q[k] for q in ms]) for k in ("A", "B", "P", "Q", "m0", "V0"))
    sm = np.random.default_rng(0).integers(0, 4, T).astype(np.int32)
    with rxhip.LGSSMEngine(*mdl, T=T, n_chains=1, step_model=sm, device=device) as eng:
        eng.set_data(y)
        out["per_step_constants_4_models_ms"] = med(eng)
        mean, cov = eng.marginals_of_chains([0])
        fe = eng.free_energy_per_chain()
    om, oc, ofe = _oracle().lgssm_kalman_rts_affine(*mdl, np.ascontiguousarray(y[:, 0]), step_model=sm)
    sd = np.sqrt(np.einsum("tii->ti", oc))
    spot = {"mean_rel": float(np.max(np.abs(mean[0] - om) / sd)), "fe_rel": float(abs(fe[0] - ofe) / abs(ofe)),
            "cov_rel": float(np.max(np.abs(cov[0] - oc) / np.max(np.abs(oc), axis=(1, 2), keepdims=True)))}
    spot["ok"] = bool(spot["mean_rel"] < 1e-6 and spot["cov_rel"] < 1e-6 and spot["fe_rel"] < 1e-8)
    out["per_step_constants_parity_spot"] = spot
    out["missing_over_observed"] = out["missing_10pct_ms"] / out["fully_observed_ms"]
    return out


def extra_mid(device):
    """Not BASELINE configs: batches of one model at mid-size state dimensions on the MFMA path (model pass once per engine,
    data pass per sweep — DESIGN §6b), 1 BP sweep + free energy per step."""
    out = {}
    Background.quiesce()
    for d, dy, C, T in ((8, 4, 1024, 1000), (64, 64, 64, 1000)):
        m = workloads.random_model(d, dy, seed=d)
        y = workloads.generate_batch(m, T, 8, seed0=1)
        y = np.tile(y, (1, C // 8, 1))
        t0 = time.perf_counter()
        eng = rxhip.LGSSMEngine(m["A"], m["B"], m["P"], m["Q"], m["m0"], m["V0"], T=T, n_chains=C, device=device)
        eng.set_data(y)
        eng.run(1, True)
        first = (time.perf_counter() - t0) * 1e3
        ms, kt = timed_sweeps(eng, 10, 2)
        # the timed engine against the oracle (two chains), after the timing; the checker is the oracle's smoother: the reference-schedule
        # restatement sends the observation message in moment form, which does not exist for dy < d (first shape)
        spot = parity_spot(eng, m, y, [0, C - 1], missing=True)
        # the covariances of a shared-model batch are one table per model: with rxhip_set_covariance_mode(1) the per-chain copies are
        # written when somebody asks for them instead of every sweep (an OPTION; every BASELINE timing of this file writes them every sweep)
        eng.set_covariance_mode(1)
        eng.run(1, True)
        ms1, kt1 = timed_sweeps(eng, 10, 2)
        t1 = time.perf_counter()
        eng.marginals_device()
        eng.sync()
        on_request = (time.perf_counter() - t1) * 1e3
        spot1 = parity_spot(eng, m, y, [0, C - 1], missing=True)
        eng.close()
        out[f"d{d}_chains{C}_T{T}"] = {"ms_per_step": ms, "steps_per_s": T * C / (ms * 1e-3), "kernels_ms_avg": kt, "timing": timing_mode(2),
                                       "create_set_data_first_run_ms": first, "parity_spot": spot,
                                       "covariances_on_request": {"ms_per_step": ms1, "kernels_ms_avg": kt1, "materialise_ms": on_request,
                                                                  "parity_spot": spot1}}
    return out


VALU_PEAK_WAVE_INSTS = 1024 * 2.4e9 / 4   # wave-instructions / s: 256 CUs × 4 SIMDs, one VALU instruction per wave every 4 cycles at 2.4 GHz


def valu_roofline(kernel, key, ms):
    """Issue-bound kernels (C4, C5): VALU instructions per launch — SQ_INSTS_VALU of the committed PMC pass (profiles/valu_insts.json,
    scripts/profile_c4c5_pmc.sh) — over the launch time measured here, against the part's VALU issue rate."""
    try:
        vj = json.load(open(os.path.join(ROOT, "profiles", "valu_insts.json")))
        insts, src = float(vj[key]["SQ_INSTS_VALU"]), vj.get("source")
        # the counters were collected from the kernels of ONE source state: its hash is recorded with them and compared here (absent in files older than round 6)
        hdr = {"c4": "hgf_kernels.hpp", "c5": "gmm_kernels.hpp"}[key]
        want = vj.get(hdr.replace(".hpp", "_sha256"))
        with open(os.path.join(ROOT, "rxinfer.jl_amd", "csrc", hdr), "rb") as f:
            stale = None if want is None else want != hashlib.sha256(f.read()).hexdigest()
    except Exception:
        return {"bound": "valu-issue", "kernel": kernel, "achieved": None, "peak": VALU_PEAK_WAVE_INSTS, "unit": "wave-instructions/s", "frac": None}
    ach = insts / (ms * 1e-3)
    return {"bound": "valu-issue", "kernel": kernel, "valu_insts_per_launch": insts, "ms": ms, "achieved": ach, "peak": VALU_PEAK_WAVE_INSTS,
            "unit": "wave-instructions/s", "frac": ach / VALU_PEAK_WAVE_INSTS, "counter_source": src, "counter_stale": stale}


def extra_c4(device, parity=True):
    """BASELINE config 4 on one GPU: 4096 HGF series × T = 2000, 10 VMP iterations per observation, GH-31."""
    S, T, iters = 4096, 2000, 10
    _, _, y = workloads.generate_hgf_batch(T, S, seed=42)
    eng = rxhip.HGFEngine(T, S, 1.0, 0.0, 0.04, 0.01, device=device)
    eng.set_data(y)
    eng.run(iters, True)
    n, ms = 3, 1e9
    for _ in range(2):   # the better of two timings (see timed_sweeps)
        t0 = time.perf_counter()
        for _ in range(n):
            eng.run_async(iters, True)
        eng.sync()
        ms = min(ms, (time.perf_counter() - t0) / n * 1e3)
    fe = eng.free_energy()
    # the timed engine against the oracle on three series (first lane row, middle, last): filtered means / variances of both layers at every
    # observation and the per-series free energy after the last iteration
    spot = None
    if parity:
        rxo = _oracle()
        zm, zv, xm, xv = eng.history()
        fes = eng.free_energy_per_chain()
        spot = {"series": [0, S // 2 - 1, S - 1], "post_rel": 0.0, "fe_rel": 0.0}
        for sidx in spot["series"]:
            o = rxo.hgf_filter(y[:, sidx], 1.0, 0.0, 0.04, 0.01, vmp_iters=iters)
            for got, want in ((zm[:, sidx], o[0]), (zv[:, sidx], o[1]), (xm[:, sidx], o[2]), (xv[:, sidx], o[3])):
                spot["post_rel"] = max(spot["post_rel"], float(np.max(np.abs(got - want)) / np.max(np.abs(want))))
            spot["fe_rel"] = max(spot["fe_rel"], float(abs(fes[sidx] - o[4][-1]) / abs(o[4][-1])))
        spot["ok"] = bool(spot["post_rel"] < 1e-6 and spot["fe_rel"] < 1e-8)
    eng.close()
    # the 8-GPU shape of BASELINE config 4 (512 series per GPU): a series is a latency chain of 2·10⁴ dependent VMP iterations, so
    # it strong-scales by capacity, not by latency — the expectation for the scaling run is on record here
    eng = rxhip.HGFEngine(T, 512, 1.0, 0.0, 0.04, 0.01, device=device)
    eng.set_data(np.ascontiguousarray(y[:, :512]))
    eng.run(iters, True)
    ms512 = 1e9
    for _ in range(2):
        t0 = time.perf_counter()
        for _ in range(n):
            eng.run_async(iters, True)
        eng.sync()
        ms512 = min(ms512, (time.perf_counter() - t0) / n * 1e3)
    eng.close()
    return {"workload": f"HGF {S} series x T={T}, {iters} VMP iterations per observation, GH-31, with free energy", "ms_per_step": ms,
            "gh_evaluations_per_s": 31 * iters * T * S / (ms * 1e-3), "series_observations_per_s": T * S / (ms * 1e-3),
            "free_energy_mean_per_series_it10": float(fe[-1] / S), "roofline": valu_roofline("k_hgf_filter", "c4", ms),
            "ms_per_step_512_series": ms512, "timing": timing_mode(2), "parity_spot": spot}


def extra_c5(device, parity=True):
    """BASELINE config 5 on one GPU: univariate GMM, K = 16, N = 10^7, 20 VMP iterations."""
    K, N, iters = 16, 10_000_000, 20
    mus = np.arange(1, K + 1) * 10.0 - 80.0
    rng = np.random.default_rng(12345)
    y = mus[rng.integers(0, K, size=N)] + rng.standard_normal(N)
    eng = rxhip.GMMEngine(N, mus + 1.5, np.full(K, 1e3), np.full(K, 0.01), np.full(K, 0.01), np.ones(K), mus + 1.5,
                          np.full(K, 10.0), np.ones(K), np.ones(K), np.ones(K), device=device)
    eng.set_data(y)
    eng.run(2, True)
    # the first two VMP iterations of the timed engine against the oracle in its split-phase form (rxo_gmm_accumulate over 64 shards on host
    # threads, statistics summed in shard order, rxo_gmm_update): every q(m_k), q(w_k), q(s) parameter and the free energy of both iterations
    spot = None
    if parity:
        hist2, fe2 = eng.history(), eng.free_energy()

        def check():
            from concurrent.futures import ThreadPoolExecutor
            rxo = _oracle()
            priors = (mus + 1.5, np.full(K, 1e3), np.full(K, 0.01), np.full(K, 0.01), np.ones(K))
            state = np.ascontiguousarray(np.stack([mus + 1.5, np.full(K, 10.0), np.ones(K), np.ones(K), np.ones(K)]))
            shards = np.array_split(y, 64)
            out = {"iterations_checked": 2, "post_rel": 0.0, "fe_rel": 0.0}
            with ThreadPoolExecutor(16) as ex:
                for it in range(2):
                    parts = list(ex.map(lambda sh: rxo.gmm_accumulate(sh, state.copy()), shards))
                    ofe = rxo.gmm_update(*priors, np.sum(np.stack(parts), axis=0), state)
                    out["post_rel"] = max(out["post_rel"], float(np.max(np.abs(hist2[it] - state) / np.maximum(np.abs(state), 1e-300))))
                    out["fe_rel"] = max(out["fe_rel"], float(abs(fe2[it] - ofe) / abs(ofe)))
            out["ok"] = bool(out["post_rel"] < 1e-6 and out["fe_rel"] < 1e-8)
            return out

        spot = Background(check)
    ms = 1e9
    for _ in range(2):
        t0 = time.perf_counter()
        eng.run(iters, True)
        ms = min(ms, (time.perf_counter() - t0) / iters * 1e3)
    fe = eng.free_energy()
    eng.close()
    n8 = N // 8   # the 8-GPU shape: 1.25·10⁶ points per GPU
    eng = rxhip.GMMEngine(n8, mus + 1.5, np.full(K, 1e3), np.full(K, 0.01), np.full(K, 0.01), np.ones(K), mus + 1.5,
                          np.full(K, 10.0), np.ones(K), np.ones(K), np.ones(K), device=device)
    eng.set_data(y[:n8])
    eng.run(2, True)
    t0 = time.perf_counter()
    eng.run(iters, True)
    ms8 = (time.perf_counter() - t0) / iters * 1e3
    eng.close()
    return {"workload": f"GMM K={K}, N={N}, {iters} VMP iterations (q(z) not materialised: 8 B per point-iteration)", "ms_per_iteration": ms,
            "vmp_iters_per_sec": 1e3 / ms, "point_iterations_per_s": N / (ms * 1e-3), "free_energy_last": float(fe[-1]),
            "free_energy_monotone": bool(np.all(np.diff(fe) <= 1e-6 * abs(fe[-1]))), "roofline": valu_roofline("k_gmm_pass", "c5", ms),
            "ms_per_iteration_1p25M_points": ms8, "timing": timing_mode(2), "parity_spot": spot}


def _sig(x, n=6):
    """floats to n significant digits (the line is for reading; the detail file keeps everything)"""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")) or x == 0.0:
        return x
    return float(f"{x:.{n}g}")


def _slim(o, n=6):
    if isinstance(o, dict):   # (free energies and the headline value keep every digit: they are results, the rest are measurements)
        return {k: (v if ("free_energy" in k or k == "value") else _slim(v, n)) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_slim(v, n) for v in o]
    return _sig(o, n)


def _spot(sp):
    """a parity spot as [ok, largest relative error of the posteriors, of the free energy]"""
    if not isinstance(sp, dict):
        return None
    errs = [sp.get(k) for k in ("mean_rel", "cov_rel", "post_rel") if sp.get(k) is not None]
    return [bool(sp.get("ok")), max(errs) if errs else None, sp.get("fe_rel")]


def compact_line(out):
    """The ONE line rank 0 prints, below 8 KB (the driver keeps the parsed fixed keys and an 8 KB tail: a 15 KB line lost most extras): the
    contract's fields, the dominant kernel's roofline with a scalar summary [ms, roofline fraction, parity ok] of EVERY configuration under
    roofline.per_config, the CPU baseline, and per configuration the few rates that name it.  Workload texts, kernel breakdowns, notes, counter sources:
    the detail file (--detail; with --full by default bench_detail.json) and DESIGN.md §6."""
    pick = lambda d, keys: {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}
    line = pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"))
    line["vs_baseline"] = out.get("vs_baseline")
    line["config"] = pick(out["config"], ("workload", "chains_per_gpu", "T", "segments", "segment_len", "parallelism"))
    line.update(pick(out, ("vmp_iters_per_sec", "timing", "engine_create_ms", "model_tables_ms", "free_energy_rank0", "free_energy_global", "gpu_over_cpu")))
    r = out["roofline"]
    line["roofline"] = pick(r, ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_frac", "traffic_stale", "algorithmic_bytes_per_U",
                                "algorithmic_bytes_per_launch", "kernel_ms_avg", "sweep_frac"))
    line["roofline"]["traffic"] = r.get("traffic")
    line["kernels_ms_avg"] = out.get("kernels_ms_avg")
    if "parity_spot" in out:
        line["parity_spot"] = out["parity_spot"]
    cb = out.get("cpu_baseline")
    if isinstance(cb, dict):
        c = pick(cb, ("value", "unit", "cores", "kind", "free_energy_rel_vs_gpu"))
        c["sample"] = cb.get("sample", "").split(" (")[0][:160]
        if isinstance(cb.get("all_cores"), dict):
            c["all_cores"] = pick(cb["all_cores"], ("value", "cores", "threads"))
        line["cpu_baseline"] = c
    else:
        line["cpu_baseline"] = cb
    per, ex = {}, {}

    def add(name, ms, frac, spot, bound=None, **more):
        per[name] = [ms, frac, None if spot is None else bool(spot[0])]
        e = {"ms": ms}
        if bound:
            e["bound"] = bound
        if frac is not None:
            e["frac"] = frac
        if spot is not None:
            e["parity"] = spot
        e.update({k: v for k, v in more.items() if v is not None})
        ex[name] = e

    pc = out.get("roofline_per_chain_models")
    if isinstance(pc, dict) and "error" not in pc:
        add("per_chain_models", pc.get("ms_per_step"), pc.get("frac"), _spot(pc.get("parity_spot")), "hbm", sweep_frac=pc.get("sweep_frac"), moved_frac=pc.get("moved_frac"),
            rule_calls_per_s=pc.get("rule_calls_per_s"))
    extra = out.get("extra") or {}
    g = lambda d, *ks: (g(d.get(ks[0]), *ks[1:]) if len(ks) > 1 else d.get(ks[0])) if isinstance(d, dict) else None
    for name, v in extra.items():
        if not isinstance(v, dict):
            continue
        if "error" in v:
            ex[name] = {"error": str(v["error"])[:200]}
            per[name] = [None, None, False]
            continue
        if name == "c1":
            add(name, v.get("infer_ms"), None, None, rule_calls_per_s=v.get("rule_calls_per_s"), engine_built_per_call_ms=v.get("infer_ms_engine_built_per_call"),
                cpu_ms=g(v, "cpu_baseline", "ms"), cpu_mean_rel=g(v, "cpu_baseline", "mean_rel_vs_gpu"), cpu_fe_rel=g(v, "cpu_baseline", "free_energy_rel_vs_gpu"))
        elif name == "c2_missing":
            add(name, v.get("ms_per_step"), None, _spot(v.get("parity_spot")), steps_per_s=v.get("steps_per_s"), k_forward_ms=g(v, "kernels_ms_avg", "k_forward"),
                k_backward_ms=g(v, "kernels_ms_avg", "k_backward"))
        elif name == "c3":
            rf = v.get("roofline") or {}
            add(name, v.get("ms_per_step"), rf.get("frac"), _spot(v.get("parity_spot")), "mfma", achieved_tflops=rf.get("achieved"), peak_tflops=rf.get("peak"),
                fwd_frac=g(rf, "per_kernel", "kd_forward_info", "frac"), bwd_frac=g(rf, "per_kernel", "kd_backward_info", "frac"), ref_count_tflops=v.get("tflops_ref_count"),
                filter_ms=v.get("filter_ms_per_step"), hoisted_ms=g(v, "hoisted_matrices", "ms_per_step"), kernels_ms=v.get("kernels_ms_avg"))
        elif name in ("c4", "c5"):
            rf = v.get("roofline") or {}
            add(name, v.get("ms_per_step", v.get("ms_per_iteration")), rf.get("frac"), _spot(v.get("parity_spot")), rf.get("bound"),
                gh_evaluations_per_s=v.get("gh_evaluations_per_s"), point_iterations_per_s=v.get("point_iterations_per_s"), vmp_iters_per_sec=v.get("vmp_iters_per_sec"),
                per_gpu_shape_ms=v.get("ms_per_step_512_series", v.get("ms_per_iteration_1p25M_points")), fe_monotone=v.get("free_energy_monotone"),
                n_gpus=v.get("n_gpus"), free_energy_last=v.get("free_energy_last"), series_observations_per_s=v.get("series_observations_per_s"),
                free_energy_mean_per_series_global=v.get("free_energy_mean_per_series_global"))
        elif name == "mid_sizes":
            for k2, w in v.items():
                add(k2, w.get("ms_per_step"), None, _spot(w.get("parity_spot")), on_request_ms=g(w, "covariances_on_request", "ms_per_step"))
        elif name == "masked_mfma":
            add("d64_T2000_observed", v.get("fully_observed_ms"), None, None)
            add("d64_T2000_missing10", v.get("missing_10pct_ms"), None, _spot(v.get("missing_10pct_parity_spot")))
            add("d64_T2000_4_step_models", v.get("per_step_constants_4_models_ms"), None, _spot(v.get("per_step_constants_parity_spot")))
        elif name == "lgssm_noise_vmp":
            add(name, v.get("ms_per_iteration"), None, _spot(v.get("parity_spot")), rule_calls_per_s=v.get("rule_calls_per_s"), fe_monotone=v.get("free_energy_monotone"))
        elif name == "node_array":
            for k2, w in v.items():
                if not isinstance(w, dict):
                    continue
                rf = w.get("roofline") or {}
                i = w.get("info") or {}
                add("executor_" + k2, w.get("device_ms_per_step"), rf.get("frac"), _spot(w.get("parity_spot")), rf.get("bound"), rule_calls_per_s=w.get("rule_calls_per_s"),
                    io_frac=rf.get("io_frac"), traffic=rf.get("traffic"), mode=i.get("mode"), dmax=i.get("dmax"), bytes_per_sweep=i.get("bytes_per_sweep"),
                    io_bytes_per_sweep=i.get("io_bytes_per_sweep"), specialised_engine_ms=w.get("specialised_engine_ms_per_step"), mfma_frac=rf.get("mfma_frac"),
                    kernels=i.get("kernels"), points_per_s=w.get("points_per_s"), observations_per_s=w.get("observations_per_s"))
        else:
            ms = v.get("ms_per_step", v.get("ms_per_iteration"))
            add(name, ms, g(v, "roofline", "frac"), _spot(v.get("parity_spot")), **{k: w for k, w in v.items() if isinstance(w, (int, float, bool)) and k not in ("ms_per_step",)})
    line["roofline"]["per_config"] = per   # [ms, roofline fraction (null: a time, not a roofline), parity ok] per configuration
    if ex:
        line["extra"] = ex
    slim = _slim(line)
    for k in ("achieved", "peak", "frac"):   # (the dominant kernel's roofline keeps its digits: frac = achieved / peak exactly)
        if k in line["roofline"]:
            slim["roofline"][k] = line["roofline"][k]
    return slim


def _join_background(o):
    if isinstance(o, Background):
        return o.result()
    if isinstance(o, dict):
        return {k: _join_background(v) for k, v in o.items()}
    return o


def respawn_under_launcher(n):
    """`python bench.py --gpus N` (no launcher): re-execute under torch.distributed.run, one rank per GPU."""
    have = torch.cuda.device_count()
    if have < n:
        sys.exit(f"bench.py --gpus {n}: only {have} HIP device(s) visible on this node (one rank per GPU is required)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execv(sys.executable, cmd)


def sharded_extras(dist, gpu, world, rank, local_rank, hgf_cls=None, gmm_cls=None, shard_cls=None, c4_series=512, c4_T=2000, c5_points=1_250_000, steps4=3, steps5=20):
    """BASELINE configs 4 and 5 as BASELINE.json DEFINES them — on N GPUs: every rank of an N > 1 run executes its shard and the line carries the
    whole-job figures (the bodies of scripts/bench_configs.py).  Timing contract of the headline: barrier + synchronise on both
    sides of exactly K steps, maximum over the ranks.
      c4: `c4_series` HGF series per GPU × T observations, 10 VMP iterations per observation, GH-31; step = one filtering pass; the exchange is the
          free energy (10 values): all-gather + sum in rank order, once per step.
      c5: univariate mixture, K = 16, `c5_points` per GPU; step = ONE VMP iteration = accumulate → all-reduce of the 3K + 1 statistics → update, all
          three enqueued on one stream (no host wait).  The all-reduce sits on the critical path of every iteration by construction (the update needs
          the global statistics, the next accumulate the updated marginals): splitting the data in halves only moves which half's reduce is exposed.
    `*_cls`: test seams (tests/test_bench_main_cpu.py drives this over gloo with stub engines)."""
    hgf_cls = hgf_cls or rxhip.HGFEngine
    gmm_cls = gmm_cls or rxhip.GMMEngine
    if shard_cls is None:
        from rxhip import distributed as rd
        shard_cls = rd.DeviceMixtureShard
    dev = gpu.device

    def timed(step, steps, finish, warmup=2):
        for _ in range(warmup):
            step()
        finish()
        dist.barrier()
        gpu.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        finish()
        gpu.synchronize()
        dist.barrier()
        gpu.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    out = {}
    # ---- c4 ----
    S, T, iters = c4_series, c4_T, 10
    _, _, y = workloads.generate_hgf_batch(T, S, seed=42 + rank)
    eng = hgf_cls(T, S, 1.0, 0.0, 0.04, 0.01, device=local_rank)
    eng.set_data(y)
    fe_loc = torch.zeros(iters, dtype=torch.float64, device=dev)
    fe_all = torch.zeros(world * iters, dtype=torch.float64, device=dev)
    fe_glob = torch.zeros(iters, dtype=torch.float64, device=dev)

    def step4():
        eng.run_async(iters, True)
        eng.sync()
        fe_loc.copy_(torch.as_tensor(np.asarray(eng.free_energy(), dtype=np.float64)).to(dev))
        dist.all_gather_into_tensor(fe_all, fe_loc)
        torch.sum(fe_all.view(world, iters), dim=0, out=fe_glob)   # rank order: bit-identical on every rank

    dt = timed(step4, steps4, eng.sync)
    out["c4"] = {"workload": f"HGF {S} series per GPU x T={T}, 10 VMP iterations per observation, GH-31 (BASELINE config 4), series sharded over {world} GPUs",
                 "ms_per_step": dt / steps4 * 1e3, "gh_evaluations_per_s": 31 * iters * T * S * world * steps4 / dt, "series_observations_per_s": T * S * world * steps4 / dt,
                 "exchange": "free energy per iteration: all-gather + sum in rank order, once per filtering pass", "n_gpus": world, "steps": steps4,
                 "free_energy_mean_per_series_global": (fe_glob.cpu().numpy() / (S * world)).tolist()}
    eng.close()
    # ---- c5 ----
    K, N = 16, c5_points
    mus = np.arange(1, K + 1) * 10.0 - 80.0
    rng = np.random.default_rng(12345 + rank)
    yv = mus[rng.integers(0, K, size=N)] + rng.standard_normal(N)
    sh = gpu.make_stream()
    eng = gmm_cls(N, mus + 1.5, np.full(K, 1e3), np.full(K, 0.01), np.full(K, 0.01), np.ones(K), mus + 1.5, np.full(K, 10.0), np.ones(K), np.ones(K), np.ones(K),
                  device=local_rank, stream=sh)
    eng.set_data(yv)
    shard = shard_cls(eng)
    warm5 = 2
    with gpu.on_stream():
        shard.begin(warm5 + steps5)

    from rxhip import distributed as rdist
    gathered = [None]

    def step5():
        with gpu.on_stream():
            stats = shard.accumulate()
            # all-gather + ONE local reduction over the rank axis, in place: the same data through the same kernel on every rank — bit-identical on every
            # rank and from run to run whatever ring or tree RCCL picks (an all-reduce's summation order is the backend's)
            gathered[0] = rdist.allgather_ordered_sum_(stats, dist, gathered[0])
            shard.update(True)

    dt = timed(step5, steps5, eng.sync, warmup=warm5)
    fe = np.asarray(eng.free_energy())
    out["c5"] = {"workload": f"GMM K=16, {N} points per GPU (BASELINE config 5), points sharded over {world} GPUs", "ms_per_step": dt / steps5 * 1e3,
                 "vmp_iters_per_sec": steps5 / dt, "point_iterations_per_s": N * world * steps5 / dt, "n_gpus": world, "steps": steps5,
                 "exchange": "3K + 1 statistics per VMP iteration: all-gather + one reduction over the rank axis (bit-identical on every rank), enqueued between accumulate and update on one stream",
                 "free_energy_last": float(fe[-1]), "free_energy_monotone": bool(np.all(np.diff(fe[warm5:]) <= 1e-6 * abs(fe[-1])))}
    eng.close()
    return out


class _Gpu:
    """torch's handle on the rank's GPU: device selection, the stream the engine and the collectives share, synchronisation."""
    backend = "nccl"   # RCCL on ROCm

    def __init__(self, local_rank):
        if not torch.cuda.is_available():
            sys.exit("bench.py needs an MI355X: no HIP device visible (the product has no CPU path)")
        torch.cuda.set_device(local_rank)  # before the process group: every collective (and barrier) runs on THIS rank's GPU
        self.device = torch.device("cuda", local_rank)
        self.index = local_rank

    def init_kwargs(self):
        return {"device_id": self.device}

    def make_stream(self):
        self.stream = torch.cuda.Stream(device=self.device)
        return self.stream.cuda_stream

    def on_stream(self):
        return torch.cuda.stream(self.stream)

    def synchronize(self):
        torch.cuda.synchronize()


class _HostOnly:
    """The same seam without a GPU: tests/test_bench_main_cpu.py drives main() at world size 2 over `gloo` with a stub engine, so that the
    rank / shard / free-energy-exchange logic of this file is covered where no MI355X exists.  Never used by a bench run."""
    backend = "gloo"

    def __init__(self, local_rank):
        self.device = torch.device("cpu")
        self.index = local_rank

    def init_kwargs(self):
        return {}

    def make_stream(self):
        return 0

    def on_stream(self):
        import contextlib
        return contextlib.nullcontext()

    def synchronize(self):
        pass


def main(argv=None, engine_cls=None, gpu_cls=_Gpu, extra_cls=None):
    """`engine_cls` / `gpu_cls` / `extra_cls` ({'hgf': …, 'gmm': …, 'shard': …, sizes}): test seams (see _HostOnly); a bench run uses rxhip's engines on the rank's MI355X."""
    engine_cls = engine_cls or rxhip.LGSSMEngine
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=int, default=100000)
    ap.add_argument("--chains", type=int, default=1024, help="chains per GPU (weak scaling) / of the whole job (strong scaling)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --chains per GPU (the driver's scaling run); strong: --chains in total, split over the ranks")
    ap.add_argument("--segments", type=int, default=0)
    ap.add_argument("--full", action="store_true",
                    help="also run the CPU baseline, the parity spot, the extra configurations and write the detail file (a plain run: the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (a seeded sample of the posteriors, the free energies) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-sample-chains", type=int, default=96,
                    help="chains of the benchmarked batch the single-core CPU restatement is timed on (96: about 12 s of one host core)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the per-chain-model variant and the C3/C4/C5 lines")
    ap.add_argument("--no-parity", action="store_true", help="with --full: skip the parity spots")
    ap.add_argument("--detail", default=None,
                    help="file that receives the full record (the printed line is its compact form, below 8 KB); '' = none; "
                         "default: bench_detail.json with --full, none without")
    ap.add_argument("--force-dist", action="store_true",
                    help="create the RCCL process group and run the free-energy exchange even with one rank (exercises the N > 1 code path on a 1-GPU box)")
    args = ap.parse_args(argv)
    if not args.full:   # a plain run: the headline figure only
        args.no_cpu_baseline = args.no_parity = args.no_extras = True
    if args.detail is None:
        args.detail = os.path.join(ROOT, "bench_detail.json") if args.full else ""

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_launcher(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    gpu = gpu_cls(local_rank)
    device = gpu.device
    mdl = workloads.c1_model()
    T, C = args.T, args.chains
    if args.scaling == "strong":
        if C % world:
            sys.exit(f"bench.py --scaling strong: {C} chains do not split over {world} ranks")
        C //= world
    # chain c of the JOB: default_rng(42 + c); every rank draws its own shard with its share of the host cores
    y_host = workloads.generate_batch(mdl, T, C, seed0=42 + rank * C, threads=max(1, min(32, (os.cpu_count() or 1) // world)))
    # The CPU baseline (rank 0, on a sample of ITS shard) runs BEFORE the process group exists: in an N-GPU run the other ranks wait for
    # rank 0 at the rendezvous with nothing enqueued, instead of idling ≈ 20 s at the teardown with their engines alive.
    cpu_base, cpu_fe = None, None
    if rank == 0 and not args.no_cpu_baseline:
        cpu_base, cpu_fe = cpu_baseline(mdl, y_host, min(args.cpu_sample_chains, C))
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        own_port = "MASTER_PORT" not in os.environ   # (a launcher sets it; a single self-launched rank picks a free one)
        for attempt in range(5):
            if own_port:
                s = socket.socket()
                s.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(s.getsockname()[1])
                s.close()
            try:
                dist.init_process_group(gpu.backend, rank=rank, world_size=world, **gpu.init_kwargs())  # "nccl" = RCCL on ROCm
                break
            except RuntimeError:   # the port was taken between the probe and the store's bind (EADDRINUSE): another one
                if not own_port or attempt == 4:
                    raise

    y = torch.from_numpy(y_host).to(device)
    stream_handle = gpu.make_stream()
    fe_all = torch.zeros(world, dtype=torch.float64, device=device)
    fe_buf = torch.zeros(1, dtype=torch.float64, device=device)
    fe_sum = torch.zeros(1, dtype=torch.float64, device=device)
    if dist is not None:  # RCCL builds its communicator on the first collective: do that here, never inside the timed region
        with gpu.on_stream():
            dist.all_gather_into_tensor(fe_all, fe_buf)
    gpu.synchronize()

    # a throwaway engine of the same kind first: the first launch of a kernel loads its code object (≈17 ms for the table
    # kernels), which is a property of the process, not of an engine
    engine_cls(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=min(T, 4096), n_chains=C, device=local_rank,
               stream=stream_handle).close()
    gpu.synchronize()
    t_create = time.perf_counter()
    eng = engine_cls(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C,
                     segments=args.segments, device=local_rank, stream=stream_handle)
    gpu.synchronize()
    create_ms = (time.perf_counter() - t_create) * 1e3  # device allocation + every data-independent table of the model
    tables_ms = eng.model_tables_ms()
    eng.set_data_device(y.data_ptr(), y.numel(), keepalive=y)

    def step():
        with gpu.on_stream():
            eng.run_async(iterations=1, free_energy=True)
            if dist is not None:
                # the path's only exchange: the global Bethe free energy, 1 double per rank — all-gather + a sum in rank
                # order (bit-identical on every rank and from run to run, whatever ring/tree RCCL picks)
                eng.copy_free_energy_to_device(fe_buf.data_ptr())
                dist.all_gather_into_tensor(fe_all, fe_buf)
                torch.sum(fe_all, dim=0, keepdim=True, out=fe_sum)

    for _ in range(args.warmup):
        step()
    eng.sync()
    gpu.synchronize()
    eng.set_profiling(True)
    eng.reset_kernel_times()
    if dist is not None:
        dist.barrier()
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    eng.sync()
    gpu.synchronize()
    if dist is not None:
        dist.barrier()
    gpu.synchronize()
    dt = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    eng.set_profiling(False)

    kt = eng.kernel_times()
    cnt = eng.counters()  # per run_async(1): rule calls of one sweep over this rank's chains
    fe_local = float(eng.free_energy()[0])
    sched = eng.schedule()
    rule_calls_per_step = cnt["rule_calls"] * world
    value = rule_calls_per_step * args.steps / dt
    units = T * C  # (chain, time-step) units per launch on this rank
    d, dy = 4, 4
    # Algorithmic bytes per (chain, step).  SURVEY §8d's model (416 B/U) lets every chain write and re-read its own packed
    # forward message (d + d(d+1)/2 doubles).  In a batch that shares one model the covariance half of that message does not
    # depend on the data — it is ONE table per model, not a per-chain stream — so the floor for THIS workload is
    # y (32) + forward mean record out/in (32 + 32) + dense posterior (160) = 256 B/U, of which k_backward owns 32 + 160 = 192.
    # Since round 2 the sweep moves exactly these bytes: the observations are read once (k_forward0).
    floor_bwd, floor_sweep = 8 * (d + (d + d * d)), 8 * (dy + 2 * d + (d + d * d))                   # 192, 256
    dom_ms = kt["k_backward"]["ms_avg"]
    sweep_ms = dt / args.steps * 1e3
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    traffic, tsrc, traffic_stale = None, None, None
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if os.path.exists(tpath) and (T, C) == (100000, 1024):
        try:
            tj = json.load(open(tpath))
            traffic, tsrc = tj.get("k_backward_hbm_bytes_per_launch"), tj.get("source")
            # the counters were collected from the kernels of ONE source state: recorded with them, compared here
            with open(os.path.join(ROOT, "rxinfer.jl_amd", "csrc", "lgssm_kernels.hpp"), "rb") as f:
                traffic_stale = tj.get("lgssm_kernels_sha256") != hashlib.sha256(f.read()).hexdigest()
        except Exception:
            traffic = None
    achieved = gbs(floor_bwd * units, dom_ms)
    out = {
        "metric": "node-message-updates/sec (d=4 LGSSM, T=100k, BP sweep with Bethe free energy)",
        "value": value,
        "unit": "rule-calls/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": sweep_ms,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"LGSSM d=4 dy=4 T={T}, {C} independent chains per GPU (BASELINE config 2"
                               f"{'' if args.scaling == 'weak' else f': {C * world} chains split over the ranks'}), "
                               "1 BP sweep + Bethe free energy per step; chain c drawn from numpy default_rng(42+c)",
                   "chains_per_gpu": C, "T": T, "segments": sched["segments"], "segment_len": sched["segment_len"],
                   "parallelism": f"chains sharded over {world} GPU(s), RCCL all-gather + ordered sum of the free-energy scalar"},
        "vmp_iters_per_sec": args.steps / dt,
        "timing": "single",   # the headline region is timed once, between two barriers (the extra lines say how they were timed)
        # `achieved` = algorithmic bytes of THIS workload (shared-model batch: 192 B/U for this kernel, see above) ÷ the kernel's
        # HIP-event time measured in the timed region; it coincides with what the HBM physically moves (`traffic`, PMC passes of
        # the same command under profiles/, which also counts the per-time-index tables the kernel streams: +3 %).
        "roofline": {"bound": "hbm", "kernel": "k_backward", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": tsrc, "traffic_stale": traffic_stale,
                     "traffic_achieved": gbs(traffic, dom_ms) if traffic else None,
                     "traffic_frac": gbs(traffic, dom_ms) / HBM_PEAK_GBS if traffic else None,
                     "algorithmic_bytes_per_launch": floor_bwd * units, "algorithmic_bytes_per_U": floor_bwd,
                     "algorithmic_floor_bytes_per_U_sweep": floor_sweep, "kernel_ms_avg": dom_ms,
                     "sweep_achieved": gbs(floor_sweep * units, sweep_ms), "sweep_frac": gbs(floor_sweep * units, sweep_ms) / HBM_PEAK_GBS},
        "kernels_ms_avg": {k: round(v["ms_avg"], 4) for k, v in kt.items() if v["launches"]},
        # Not in the timed sweep: what depends on the model only (gains, covariances, smoother gains of a batch that shares one
        # model) is built once per engine — `engine_create_ms` is that cost plus the device allocation.  Every sweep reads all
        # observations, recomputes every mean and the free energy, and writes the full posterior (mean + covariance per chain).
        "engine_create_ms": create_ms,
        # where that went: host arithmetic on tables | device table kernels (enqueue) | uploads | device memory (one hipMalloc of
        # ≈23 GB here: its cost is the driver's page-table work and varies from box to box — 1 … 500 ms have been seen)
        "engine_create_stages_ms": eng.create_stages(),
        # `value` counts the reference's events: 6 rule calls per (chain, step) and sweep.  In a batch that shares ONE model the
        # covariance half of each of them does not depend on the data and is evaluated once per model (tables above), the mean
        # half per chain; with nothing shared the same batch runs at roofline_per_chain_models.rule_calls_per_s.
        "value_note": "reference-equivalent rule calls; shared-model batch: covariance halves evaluated once per model (see roofline_per_chain_models for the nothing-shared figure)",
        # device time of those once-per-engine kernels, and the sweep if they were rebuilt with every sweep
        "model_tables_ms": tables_ms, "ms_per_step_incl_model_tables": sweep_ms + tables_ms,
        "free_energy_rank0": fe_local,
        "free_energy_global": float(fe_sum.item()) if dist is not None else fe_local,
    }
    if rank == 0 and args.dump_outputs:
        dump_outputs(eng, args.dump_outputs, out["free_energy_global"])
    if rank == 0 and not args.no_parity:
        out["parity_spot"] = parity_spot(eng, mdl, y_host, [0, C - 1] if C > 1 else [0])
    if rank == 0 and cpu_base is not None:   # timed before the process group was created (above)
        out["cpu_baseline"] = cpu_base
        out["cpu_baseline"]["when"] = "before the GPU legs and before the process group (ranks > 0 wait at the rendezvous)"
        out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
        gfe = eng.free_energy_per_chain()[:cpu_fe.size]
        out["cpu_baseline"]["free_energy_rel_vs_gpu"] = float(np.max(np.abs(gfe - cpu_fe) / np.abs(cpu_fe)))
    elif rank == 0:
        out["cpu_baseline"] = None
    eng.close()
    if world > 1 and not args.no_extras:   # the configurations BASELINE defines on several GPUs: every rank runs its shard (collectives inside)
        try:
            sh = sharded_extras(dist, gpu, world, rank, local_rank, **(extra_cls or {}))
        except Exception as e:  # noqa: BLE001 — an extra line must never cost the headline line (every rank fails or none: same code, same sizes)
            sh = {"error": repr(e)}
        if rank == 0:
            out["extra"] = sh
    if rank == 0 and world == 1 and not args.no_extras:
        extra = {}
        yh = None if args.no_parity else y_host
        par = not args.no_parity
        for name, fn in (("per_chain_models", lambda: extra_per_chain_models(mdl, T, C, y, local_rank, yh)), ("c1", lambda: extra_c1(local_rank, not args.no_cpu_baseline)),
                         ("c2_missing", lambda: extra_missing(mdl, T, C, y, local_rank, yh)), ("c3", lambda: extra_c3(local_rank, par)),
                         ("c4", lambda: extra_c4(local_rank, par)), ("c5", lambda: extra_c5(local_rank, par)), ("mid_sizes", lambda: extra_mid(local_rank)),
                         ("masked_mfma", lambda: extra_masked(local_rank)), ("lgssm_noise_vmp", lambda: extra_noise_vmp(local_rank, par)),
                         ("node_array", lambda: extra_node_array(local_rank, par))):
            try:
                extra[name] = fn()
            except Exception as e:  # noqa: BLE001 — an extra line must never cost the headline line
                extra[name] = {"error": repr(e)}
        out["roofline_per_chain_models"] = extra.pop("per_chain_models")
        out["extra"] = _join_background(extra)   # the checkers still running on host threads
    if rank == 0:
        line = compact_line(out)
        if args.detail:   # everything measured, with the workload texts, kernel breakdowns, notes and counter sources
            try:
                with open(args.detail, "w") as f:
                    json.dump(out, f, indent=1)
                line["detail"] = os.path.relpath(args.detail, ROOT) if os.path.isabs(args.detail) else args.detail
            except OSError:
                pass
        print(json.dumps(line, separators=(",", ":")))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

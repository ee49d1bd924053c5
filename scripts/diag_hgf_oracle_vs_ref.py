"""The C oracle's HGF filter against the mpmath restatement (tests/hgf_ref.py) on the whole grid of tests/test_hgf_contract_gpu.py at that
test's sizes (T = 40, 18 iterations, GH-31, five seeds per case): the worst agreement per quantity and the cases that miss the 100×-inside
bounds of tests/test_hgf_ref_cpu.py.  CPU only, ≈ 40 CPU-minutes (spread over the cores); the DESIGN.md table quotes its output.
    python scripts/diag_hgf_oracle_vs_ref.py [out.json]"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "rxinfer.jl_amd")]
import numpy as np

T, ITERS, N_GH, SEEDS = 40, 18, 31, (11, 12, 13, 14, 15)


def one(job):
    import hgf_ref as R
    import rxoracle
    from test_hgf_gpu import hgf_series
    case, seed = job
    k, w, zv, yv = case
    y = hgf_series(T, k, w, zv, yv, seed)[2]
    try:
        o = rxoracle.hgf_filter(y, k, w, zv, yv, vmp_iters=ITERS, n_gh=N_GH)
    except RuntimeError as e:
        return dict(case=case, seed=seed, error=str(e))
    r = R.hgf_filter(y, k, w, zv, yv, iters=ITERS, n_gh=N_GH)
    return dict(case=case, seed=seed,
                mean=float(max(np.max(np.abs(o[0] - r[0]) / np.sqrt(r[1])), np.max(np.abs(o[2] - r[2]) / np.sqrt(r[3])))),
                var=float(max(np.max(np.abs(o[1] - r[1]) / r[1]), np.max(np.abs(o[3] - r[3]) / r[3]))),
                fe=float(np.max(np.abs(o[4] - r[4]) / np.abs(r[4]))), fe_min=float(np.min(np.abs(r[4]))), fe_max=float(np.max(np.abs(r[4]))),
                zv_min=float(np.min(r[1])))


if __name__ == "__main__":
    import hgf_ref as R
    jobs = [(c, s) for c in R.GRID for s in SEEDS]
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        res = pool.map(one, jobs, chunksize=4)
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], "w"), indent=0)
    for q, bound in (("mean", 1e-8), ("var", 1e-8), ("fe", 1e-10)):
        ok = [r for r in res if "error" not in r]
        worst = max(ok, key=lambda r: r[q])
        print(f"worst {q}: {worst[q]:.3e} at {worst['case']} seed {worst['seed']} (bound {bound:g})")
    for r in res:
        if "error" in r or r["mean"] >= 1e-8 or r["var"] >= 1e-8 or r["fe"] >= 1e-10 or r["fe_min"] < 0.1:
            print("MISS", r)

#!/usr/bin/env python3
"""What the shared-model sweep computes on every schedule it has, as one .npz — the check of a change that must not move a bit.
    python scripts/dump_sweep_outputs.py OUT.npz [--tree DIR]      (DIR: the checkout whose package and library run; default: this one)
    python scripts/dump_sweep_outputs.py --compare A.npz B.npz     (one line per array, np.array_equal; exit status 1 if any differs)
Per case: posterior means and covariances of every chain, free energy per chain and in total (where asked for), after the first and after the
second sweep of a handle (the first stores the per-chain covariances, the second does not).  Cases: five (d, dy), two segment shapes, with and
without the free energy, and seven (chains, hook) arms — 65 chains (waves straddle segments: k_forward0's memory path, k_backward<FUSED>),
128 chains with z records (k_forward0, k_backward_sh), 256 chains on the reverse-filter schedule at the shipped widths, at one and four waves
per workgroup, with the depth-1 y ring and with the boundary-scan launch.  (2, 3) has dy > d: never a reverse-filter candidate."""
import os
import sys

import numpy as np

MODELS = {(4, 4): None, (3, 2): 20, (2, 2): 4, (1, 1): 3, (2, 3): 7}   # seed of workloads.random_model; (4, 4): workloads.c1_model
SHAPES = [(365, 3), (60, 5)]   # T, segments asked for: L = 122 (last 120), and L = 12 (last 11), shorter than the stride 16
CK = {"RXHIP_MEAN_CHECKPOINT": "16"}
ARMS = [("c65", 65, {}), ("c128_records", 128, {"RXHIP_MEAN_RECORDS": "1"}), ("c256", 256, CK),
        ("c256_waves1", 256, {**CK, "RXHIP_SWEEP_WAVES": "1"}), ("c256_waves4", 256, {**CK, "RXHIP_SWEEP_WAVES": "4"}),
        ("c256_yring1", 256, {**CK, "RXHIP_Y_RING": "1"}), ("c256_boundary_kernel", 256, {**CK, "RXHIP_BOUNDARY_KERNEL": "1"})]
HOOKS = ("RXHIP_MEAN_CHECKPOINT", "RXHIP_MEAN_RECORDS", "RXHIP_SWEEP_WAVES", "RXHIP_Y_RING", "RXHIP_BOUNDARY_KERNEL")


def dump(out, tree):
    sys.path.insert(0, os.path.join(tree, "rxinfer.jl_amd"))
    import rxhip
    from rxhip import _lib, workloads
    print("library:", os.path.relpath(_lib.LIB_PATH))
    arrays = {}
    os.environ["RXHIP_TEST_HOOKS"] = "1"
    os.environ["RXHIP_ONE_PASS"] = "1"
    for (d, dy), seed in MODELS.items():
        mdl = workloads.c1_model() if seed is None else workloads.random_model(d, dy, seed)
        for T, S in SHAPES:
            for arm, C, env in ARMS:
                y = workloads.generate_batch(mdl, T, C, seed0=17)
                for fe in (True, False):
                    for k in HOOKS:
                        os.environ.pop(k, None)
                    os.environ.update(env)
                    with rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C, segments=S, device=0) as eng:
                        eng.set_data(y)
                        case = f"d{d}dy{dy}_T{T}_{arm}_{'fe' if fe else 'nofe'}"
                        arrays[case + "_stride_waves"] = np.array([eng.mean_checkpoint_stride(), *eng.sweep_waves()])   # which schedule runs
                        print(case, "checkpoint stride", eng.mean_checkpoint_stride(), "waves (forward, backward)", eng.sweep_waves())
                        for sweep in ("first", "second"):
                            eng.run(iterations=1, free_energy=fe)
                            mean, cov = eng.marginals_of_chains(np.arange(C))
                            key = f"{case}_{sweep}"
                            arrays[key + "_mean"], arrays[key + "_cov"] = np.array(mean), np.array(cov)
                            if fe:
                                arrays[key + "_fe_per_chain"] = np.array(eng.free_energy_per_chain())
                                arrays[key + "_fe"] = np.array(eng.free_energy())
    np.savez(out, **arrays)
    print(f"{len(arrays)} arrays -> {out}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in bad:
        print(f"{k}: in one file only")
    for k in sorted(set(A.files) & set(B.files)):
        same = A[k].shape == B[k].shape and np.array_equal(A[k], B[k]) and bool(np.all(np.isfinite(A[k])))
        diff = float(np.max(np.abs(A[k] - B[k]))) if A[k].shape == B[k].shape else float("nan")
        print(f"{k}: shape {A[k].shape}, finite and np.array_equal: {same}, max |diff| {diff:.3e}")
        bad += [] if same else [k]
    print(f"{len(A.files)} arrays, {len(bad)} not equal")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    dump(sys.argv[1], os.path.abspath(tree))

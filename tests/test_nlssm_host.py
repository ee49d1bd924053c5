"""The nonlinear state-space engine's kernels on the HOST: tests/host_emul/nlssm_main.cpp compiles csrc/expr.hpp and csrc/nlssm_kernels.hpp with g++
(-ffp-contract=off) through the stand-in <hip/hip_runtime.h> of tests/host_emul/ and runs them one "thread" at a time — the same
__host__ __device__ functions, loops and indexing as on the device, the expression interpreter with its slots in the [row][component][lane] block
included.  Held to tests/nlssm_ref.py on the cases of tests/test_nlssm_gpu.py at the same tolerances: the check of this arithmetic that needs no GPU."""
import os
import subprocess

import numpy as np
import pytest

import nlssm_ref as R
import rxhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("nlssm_host") / "nlssm_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC, "-o", out,
                    os.path.join(EMUL, "nlssm_main.cpp")], check=True)
    return out


def program_text(prog):
    return " ".join([f"{len(prog.code)} {len(prog.consts)} {prog.n_slots}"] + [str(int(v)) for v in prog.code.ravel()] + [repr(float(v)) for v in prog.consts])


def case_text(case, method, mode, iterations):
    d, f, _ = R.FUNCS[case["name"]]
    prog = rxhip.trace(lambda x: f(x, np), d)
    y = case["y"]
    T, S, dy = y.shape
    noise = case["noise"]
    a0, b0 = noise if noise else (1.0, 1.0)
    head = [d, dy, T, S, int(method == "unscented"), int(mode == "smooth"), int(noise is not None), int(case["per_series"]), iterations, a0, b0,
            *R.unscented_weights(d)]
    pri = np.concatenate([np.reshape(case["m0"], (-1, d)), np.reshape(case["V0"], (-1, d * d))], axis=1)
    nums = np.concatenate([case["Q"].ravel(), case["H"].ravel(), (np.zeros_like(case["R"]) if noise else case["R"]).ravel(), pri.ravel(), y.ravel()])
    return " ".join([" ".join(repr(v) for v in head), program_text(prog)] + [repr(float(v)) for v in nums])


def run_cases(exe, cases):
    text = f"{len(cases)}\n" + "\n".join(case_text(c, m, mode, it) for _, c, m, mode, it in cases) + "\n"
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    out, i = [], 0
    for _, c, m, mode, it in cases:
        status = lines[i].split()
        assert status[0] == "status"
        i += 1
        if int(status[1]):
            out.append(dict(status=int(status[1]), step=int(status[2]), series=int(status[3])))
            continue
        T, S, _ = c["y"].shape
        d = R.FUNCS[c["name"]][0]
        arr = [np.array(lines[i + j].split(), dtype=np.float64) for j in range(5)]
        i += 5
        out.append(dict(status=0, mean=arr[0].reshape(T, S, d), cov=arr[1].reshape(T, S, d, d), shape=arr[2].reshape(T, S), rate=arr[3].reshape(T, S), fe=arr[4]))
    assert i == len(lines)
    return out


def test_host_build_of_the_kernels_equals_the_restatement(exe):
    cases = R.case_grid()
    got = run_cases(exe, cases)
    for (cid, c, method, mode, it), g in zip(cases, got):
        assert g["status"] == 0, cid
        ref = R.run_case(c, method, mode, it)
        err = R.errors(g, ref, c["noise"] is not None)
        for k, v in err.items():
            assert v < R.BOUNDS[k], (cid, k, v)
        if c["y"].shape[1] > 1:   # series 1 observes nothing: its free energy is exactly 0
            assert g["fe"][1] == 0.0, cid


def test_host_build_reports_the_first_value_that_is_not_finite(exe):
    """f = sqrt(x0) − 1.5 with prior means that take series 1 (of 3) below zero at the third application of f (step 2, counted from 0): flagged there, no
    other series; Q = 0 with f = [x0, x0] loses positive definiteness in the smoother"""
    R.FUNCS["_sqrt"] = (1, lambda x, M=np: [M.sqrt(x[0]) - 1.5], None)
    R.FUNCS["_dup"] = (2, lambda x, M=np: [x[0], x[0]], None)
    try:
        y = np.full((4, 3, 1), np.nan)
        # x ← sqrt(x) − 1.5 from 9: 1.5, −0.275 < 0 → the third evaluation is NaN; from 1e6: 998.5, 30.1, 3.99, 0.50: series 0 and 2 stay in the domain for T = 4
        sq = dict(name="_sqrt", y=y, m0=np.array([[1e6], [9.0], [1e6]]), V0=np.full((3, 1, 1), 1e-4), Q=np.zeros((1, 1)), H=np.ones((1, 1)), R=np.ones((1, 1)),
                  noise=None, per_series=True)
        dup = dict(name="_dup", y=np.zeros((4, 1, 1)), m0=np.zeros(2), V0=np.eye(2), Q=np.zeros((2, 2)), H=np.array([[1.0, 0.0]]), R=np.ones((1, 1)),
                   noise=None, per_series=False)
        got = run_cases(exe, [("sqrt", sq, "linearization", "filter", 1), ("dup", dup, "linearization", "smooth", 1), ("sqrt-smooth", sq, "linearization", "smooth", 1),
                              ("sqrt-smooth-ut", sq, "unscented", "smooth", 1)])
    finally:
        del R.FUNCS["_sqrt"], R.FUNCS["_dup"]
    assert got[0] == dict(status=64, step=2, series=1)
    assert got[1]["status"] == 1
    # SMOOTH: the stopped lane left its later records unwritten; the backward pass (launched whatever the status, as on the device) must not read them
    assert got[2] == dict(status=64, step=2, series=1) and got[3] == dict(status=64, step=2, series=1)


def test_host_interpreter_equals_numpy_and_the_hand_written_jacobians(exe):
    rng = np.random.default_rng(3)
    for name in ("pendulum", "coupled", "four", "scalar"):
        d, f, jac = R.FUNCS[name]
        prog = rxhip.trace(lambda x: f(x, np), d)
        x = rng.uniform(-2, 2, (130, d))
        text = f"expr {d} {program_text(prog)} {len(x)} " + " ".join(repr(float(v)) for v in x.ravel()) + "\n"
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        value = np.array(lines[0].split(), dtype=np.float64).reshape(-1, d)
        J = np.array(lines[1].split(), dtype=np.float64).reshape(-1, d, d)
        want = np.array([f(p, np) for p in x])
        wantJ = np.array([jac(p) for p in x])
        assert np.max(np.abs(value - want) / np.spacing(np.abs(want))) <= 4, name
        assert np.max(np.abs(J - wantJ) / np.maximum(1.0, np.abs(wantJ))) < 1e-12, name

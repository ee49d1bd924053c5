"""The binomial regression engine's `__host__ __device__` helpers on the HOST: tests/host_emul/binreg_main.cpp compiles csrc/binreg_kernels.hpp with
g++ through the stand-in <hip/hip_runtime.h> of tests/host_emul/ and runs ω̄ (with its series near c = 0), ln 2cosh, the per-point term and the
free-energy assembly inside a serial statement of pass and update in the device's order (chunks and tiles from breg::chunks, partials in ascending
order, the Cholesky inverse in mvd_chol_inv's steps).  Held to tests/binreg_ref.py at the project's contract (binreg_ref.hold: means 1e-6 posterior
standard deviations, covariances 1e-6 relative, free energy 1e-8 relative per iteration and problem): the check of this arithmetic that needs no GPU.
The cases hold an all-zero row of X (c = 0), rows scaled by 1e-9 and to c ≈ 1500, a missing y and n_i = 0 (binreg_ref.random_case, degenerate).
The same program is built once more with -fsanitize=address,undefined and run as it is, nothing preloaded."""
import math
import os
import subprocess

import numpy as np
import pytest

import binreg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")
BASE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("binreg_host") / "binreg_main")
    subprocess.run(BASE + ["-O1", "-o", out, os.path.join(EMUL, "binreg_main.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("binreg_host_san") / "binreg_main_san")
    r = subprocess.run(BASE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, os.path.join(EMUL, "binreg_main.cpp")],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("no sanitizer runtime for g++ on this machine")
    assert r.returncode == 0, r.stderr
    return out


def case_text(X, y, n, m, iters):
    C, N, d = X.shape
    nums = np.concatenate([m["prior_xi"], m["prior_precision"].ravel(), [np.linalg.slogdet(m["prior_precision"])[1]], m["init"][0], m["init"][1].ravel(),
                           X.ravel(), y.ravel(), n.ravel()])
    return f"{N} {C} {d} {iters} " + " ".join(repr(float(v)) for v in nums)


def all_cases():
    X, y, n = R.golden_data()
    return [(X[None], y[None], n[None], R.model(2), 100)] + [R.case(spec) for spec in R.CASES["host"]]


def run_and_hold(exe):
    cases = all_cases()
    text = f"{len(cases)}\n" + "\n".join(case_text(*c) for c in cases) + "\n"
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 1 + 3 * len(cases)
    head = lines[0].split()
    assert [int(v) for v in head[:4]] == [R.SMALL_TILE, R.SMALL_CAP, R.MFMA_TILE, R.MFMA_CAP]      # the constants the size tests are built on
    w0, below, above, l2c = (float(v) for v in head[4:])
    assert w0 == 2.0                                                                               # exactly n/4 at c = 0
    for got, c2 in ((below, 0.999e-3), (above, 1.001e-3)):                                         # the series meets the quotient at its threshold
        want = math.tanh(0.5 * math.sqrt(c2)) / (2.0 * math.sqrt(c2))
        assert abs(got - want) < 1e-15 * want                                                      # truncation 8.6e-17 + a handful of roundings on each side
    assert l2c == 750.0                                                                            # ln 2cosh(750): finite, exp(−1500) = 0
    worst = {}
    for k, (X, y, n, m, iters) in enumerate(cases):
        ref = R.run_batch(X, y, n, **m, iterations=iters)
        C, N, d = X.shape
        v = [np.array(ln.split(), dtype=np.float64) for ln in lines[1 + 3 * k:4 + 3 * k]]
        got = dict(mean=v[0].reshape(iters, C, d), cov=v[1].reshape(iters, C, d, d), fe=v[2].reshape(iters, C))
        for key, val in R.hold(got, ref).items():
            worst[key] = max(worst.get(key, 0.0), val)
        assert np.all(np.diff(got["fe"], axis=0) <= 1e-9 * np.abs(got["fe"][1:]))
        if k == 0:                                                                                 # the golden data: the recorded free energies
            for it, want in zip((0, 99), R.RECORDED_FE):
                assert abs(got["fe"][it, 0] - want) < 1e-8 * want
    print("worst:", worst)


def test_host_build_of_the_helpers_equals_the_restatement(exe):
    run_and_hold(exe)


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(exe_sanitized):
    run_and_hold(exe_sanitized)

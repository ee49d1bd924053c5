"""The regression / autoregression engine's `__host__ __device__` helpers on the HOST: tests/host_emul/arreg_main.cpp compiles csrc/arreg_kernels.hpp
with g++ through the stand-in <hip/hip_runtime.h> of tests/host_emul/ and runs the schedule constants, the residual, the two KL terms and the
free-energy assembly inside a serial statement of pass and iterate in the device's order (chunks and tiles from arreg::chunks, partials in ascending
chunk and series order, the Cholesky inverse in mvd_chol_inv's steps, lagged operands read from the series itself).  Held to tests/arreg_ref.py at
the project's contract (arreg_ref.hold): the check of this arithmetic that needs no GPU.  The same program is built once more with
-fsanitize=address,undefined and run as it is, nothing preloaded."""
import os
import subprocess

import numpy as np
import pytest

import arreg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")
BASE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("arreg_host") / "arreg_main")
    subprocess.run(BASE + ["-O1", "-o", out, os.path.join(EMUL, "arreg_main.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("arreg_host_san") / "arreg_main_san")
    r = subprocess.run(BASE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, os.path.join(EMUL, "arreg_main.cpp")],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("no sanitizer runtime for g++ on this machine")
    assert r.returncode == 0, r.stderr
    return out


def case_text(lagged, data, d, m, iters, shared):
    (m0, L0), (a0, b0) = m["prior_theta"], m["prior_gamma"]
    ia, ib = m["prior_gamma"] if m["init_gamma"] is None else m["init_gamma"]
    if lagged:
        N, C = data.shape
        arrays = [data.ravel()]
    else:
        C, N, _ = data[0].shape
        arrays = [data[0].ravel(), data[1].ravel()]
    nums = np.concatenate([L0.ravel(), m0, [a0, b0, ia, ib, np.linalg.slogdet(L0)[1]]] + arrays)
    return f"{int(lagged)} {N} {C} {d} {iters} {int(shared)} " + " ".join(repr(float(v)) for v in nums)


def all_cases():
    """(lagged, data, d, model, iterations, shared, reference)"""
    out = []
    series, _ = R.golden()
    for order in (1, 5):
        z, m = series[order - 1][:, None], R.model(order)
        out.append((True, z, order, m, 15, False, R.run_lagged(z, order, **m, iterations=15)))
    for X, y, m, iters in R.size_cases():
        if X.shape[2] in (1, 4, 5, 17, 32):
            out.append((False, (X, y), X.shape[2], m, iters, False, R.run_batch(X, y, **m, iterations=iters)))
    for z, p, m, iters in R.lag_cases():
        if p in (1, 5, 32):
            out.append((True, z, p, m, iters, False, R.run_lagged(z, p, **m, iterations=iters)))
    for X, y, m, iters, shared in R.batch_cases():
        if X.shape[0] <= 3:
            out.append((False, (X, y), X.shape[2], m, iters, shared, R.run_batch(X, y, **m, iterations=iters, shared=shared)))
    for z, p, m, iters, shared in R.lag_batch_cases():
        if z.shape[1] <= 3:
            out.append((True, z, p, m, iters, shared, R.run_lagged(z, p, **m, iterations=iters, shared=shared)))
    return out


def run_and_hold(exe):
    cases = all_cases()
    text = f"{len(cases)}\n" + "\n".join(case_text(*c[:6]) for c in cases) + "\n"
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 1 + 6 * len(cases)
    assert [int(v) for v in lines[0].split()] == [R.SMALL_TILE, R.SMALL_CAP, R.MFMA_TILE, R.MFMA_CAP, 1, 0, 4]     # the constants the size tests are built on
    worst = {}
    for k, (lagged, data, d, m, iters, shared, ref) in enumerate(cases):
        v = [np.array(ln.split(), dtype=np.float64) for ln in lines[1 + 6 * k:7 + 6 * k]]
        G = ref["mean"].shape[1]
        got = dict(mean=v[0].reshape(iters, G, d), cov=v[1].reshape(iters, G, d, d), a=v[2].reshape(iters, G), b=v[3].reshape(iters, G), fe=v[4].reshape(iters, G))
        for key, val in R.hold(got, ref).items():
            worst[key] = max(worst.get(key, 0.0), val)
        assert R.non_increasing(got["fe"])
        if k < 2:                                                                                 # the golden data: the recorded free energies
            for it, want in zip((0, 14), R.RECORDED_FE[d]):
                assert abs(got["fe"][it, 0] - want) < 1e-8 * want
        if lagged:                                                                                # n counted by the pass: the rows without a NaN
            want_n = [float(np.sum(~np.isnan(R.lag_rows(data[:, c], d)[1]))) for c in range(data.shape[1])]
        else:
            want_n = [float(np.sum(~np.isnan(data[1][c]))) for c in range(data[1].shape[0])]
        assert v[5].tolist() == want_n
    print("worst:", worst)


def test_host_build_of_the_helpers_equals_the_restatement(exe):
    run_and_hold(exe)


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(exe_sanitized):
    run_and_hold(exe_sanitized)

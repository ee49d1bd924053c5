"""The multinomial regression engine's `__host__ __device__` helpers on the HOST: tests/host_emul/mnreg_main.cpp compiles csrc/mnreg_kernels.hpp (and the
point arithmetic of csrc/binreg_kernels.hpp it uses) with g++ through the stand-in <hip/hip_runtime.h> of tests/host_emul/ and runs the schedule, the
partial layout, the suffix sums, the per-point term and the free-energy assembly inside a serial statement of the statistics pass, the iterations and
the online recursion in the device's order, for both dimension classes (d ≤ 32, and d = 33 … 64 with L⁻¹ packed).  Held to tests/mnreg_ref.py at the
project's contract (mnreg_ref.hold): the check of this arithmetic that needs no GPU.  The same program is built once more with
-fsanitize=address,undefined and run as it is, nothing preloaded."""
import os
import subprocess

import numpy as np
import pytest

import mnreg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")
BASE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mnreg_host") / "mnreg_main")
    subprocess.run(BASE + ["-O1", "-o", out, os.path.join(EMUL, "mnreg_main.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mnreg_host_san") / "mnreg_main_san")
    r = subprocess.run(BASE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, os.path.join(EMUL, "mnreg_main.cpp")],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("no sanitizer runtime for g++ on this machine")
    assert r.returncode == 0, r.stderr
    return out


def case_text(online, Y, m, iters):
    C, N, K = Y.shape
    nums = np.concatenate([m["prior_xi"], m["prior_precision"].ravel(), [np.linalg.slogdet(m["prior_precision"])[1]], m["init"][0], m["init"][1].ravel(), Y.ravel()])
    return f"{int(online)} {N} {C} {K} {iters} " + " ".join(repr(float(v)) for v in nums)


def all_cases():
    Y, _, W0, _ = R.golden()
    cases = [(False, Y[None], R.model(10, None, W0), 100)]
    cases += [(False,) + R.case(spec) for spec in R.CASES["dims"] + R.CASES["small"]]
    cases += [(False,) + R.random_case(700, 700, 1, 10, 0.05) + (3,)]                      # three tiles of 256 rows: more than one chunk
    cases += [(True,) + R.case(spec) for spec in R.CASES["online"]]
    return cases


def run_and_hold(exe):
    cases = all_cases()
    text = f"{len(cases)}\n" + "\n".join(case_text(*c) for c in cases) + "\n"
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 1 + 3 * len(cases)
    assert [int(v) for v in lines[0].split()] == [R.tile_rows(K) for K in (2, 9, 17, 33, 65)] + [R.CHUNKS_CAP]   # the constants the size tests are built on
    worst = {}
    for k, (online, Y, m, iters) in enumerate(cases):
        C, N, K = Y.shape
        rows = N if online else iters
        v = [np.array(ln.split(), dtype=np.float64) for ln in lines[1 + 3 * k:4 + 3 * k]]
        got = dict(mean=v[0].reshape(rows, C, K - 1), cov=v[1].reshape(rows, C, K - 1, K - 1), fe=v[2].reshape(rows, C))
        if online:
            ref = R.online_batch(Y, m["prior_xi"], m["prior_precision"], iters)
            ref = {q: ref[q] for q in ("mean", "cov", "fe")}
        else:
            ref = R.run_batch(Y, **m, iterations=iters)
            assert R.does_not_rise(got["fe"], K - 1)
        for key, val in R.hold(got, ref).items():
            worst[key] = max(worst.get(key, 0.0), val)
        if k == 0:                                                                         # the golden data: the recorded free energies
            for it, want in zip((0, 99), R.RECORDED_FE):
                assert abs(got["fe"][it, 0] - want) < 1e-8 * want
    print("worst:", worst)


def test_host_build_of_the_helpers_equals_the_restatement(exe):
    run_and_hold(exe)


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(exe_sanitized):
    run_and_hold(exe_sanitized)

"""The Gamma mixture engine's `__host__ __device__` helpers on the HOST: tests/host_emul/gammamix_main.cpp compiles csrc/gammamix_kernels.hpp with g++ through
the stand-in <hip/hip_runtime.h> of tests/host_emul/ and drives the point function (logits, softmax, statistics) and gammamix::update_component — the
per-component update a lane of k_gammamix_update runs: the safeguarded Newton solve with trigamma_dev, the rates, the constants, the free-energy terms —
serially in the device's order (thread, wavefront tree, wave order, ascending chunks).  Held to tests/gammamix_ref.py at 1e-10 — the check of this arithmetic that needs no GPU; the restatement finds the shape
by Brent's method, the helpers by Newton.  The same program is built once more with -fsanitize=address,undefined and run as it is, nothing preloaded.
trigamma_dev is held against mpmath on a grid over [1e-3, 1e4]."""
import os
import subprocess

import mpmath
import numpy as np
import pytest

import gammamix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")
BASE = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC]
TOL = 1e-10
# trigamma_dev: at most 10 steps of the recurrence, each a division and an addition of positive terms (≤ 1 ulp of the running sum each: 10), the tail's
# Horner form (8 steps on a term ≤ 1/600 of the result: < 1), 1/x, the bracket's two additions and the product (≤ 2.5), the final addition (0.5): 14 ulps
# plus the truncation (6e-17 relative: < 1) -> 16.
TRIGAMMA_ULPS = 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gammamix_host") / "gammamix_main")
    subprocess.run(BASE + ["-O1", "-o", out, os.path.join(EMUL, "gammamix_main.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gammamix_host_san") / "gammamix_main_san")
    r = subprocess.run(BASE + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", out, os.path.join(EMUL, "gammamix_main.cpp")],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("no sanitizer runtime for g++ on this machine")
    assert r.returncode == 0, r.stderr
    return out


def all_cases():
    """(y, prior, init, iterations): single problems of every group, the streamed ones with several chunks included, NaN points, the reference's configuration"""
    out = []
    for seed, N, K, it in R.CPU_CASES[:8] + R.STREAMED_CASES + R.SMALL_CASES[:5]:
        y, prior, init = R.make_problem(seed, N, K)
        out.append((y, prior, init, it))
    for seed, N, K, it, idx in R.NAN_CASES:
        y, prior, init = R.make_problem(seed, N, K)
        y[idx] = np.nan
        out.append((y, prior, init, it))
    y, prior = R.golden()
    out.append((y, prior, (np.ones(2), np.ones(2), np.ones(2), prior[4]), 50))
    return out


def run_and_hold(exe):
    cases = all_cases()
    text = [str(len(cases))]
    for y, prior, init, it in cases:
        text.append(f"{len(y)} {len(prior[0])} {it} " + " ".join(repr(float(v)) for v in np.concatenate(list(prior) + list(init) + [y])))
    lines = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 1 + 6 * len(cases)
    assert [int(v) for v in lines[0].split()] == [R.MAX_K, R.TILE, R.CHUNK_CAP, 40]
    worst = {}
    for c, (y, prior, init, it) in enumerate(cases):
        K = len(prior[0])
        v = [np.array(ln.split(), dtype=np.float64) for ln in lines[1 + 6 * c:7 + 6 * c]]
        ref = R.run(y, prior, init, it)
        got = dict(a=v[0].reshape(it, K), e=v[1].reshape(it, K), f=v[2].reshape(it, K), alpha=v[3].reshape(it, K), fe=v[4], resp=v[5].reshape(len(y), K))
        for key in ("a", "e", "f", "alpha"):
            worst[key] = max(worst.get(key, 0.0), float(np.max(np.abs(got[key] - ref[key]) / np.abs(ref[key]))))
        worst["fe"] = max(worst.get("fe", 0.0), float(np.max(np.abs(got["fe"] - ref["fe"]) / np.maximum(1.0, np.abs(ref["fe"])))))
        worst["resp"] = max(worst.get("resp", 0.0), float(np.max(np.abs(got["resp"] - ref["resp"]))))
        assert float(np.sum(got["alpha"][-1] - prior[4])) == pytest.approx(ref["n"], rel=1e-12)    # the counted points
    print("worst:", worst)
    assert max(worst.values()) < TOL, worst


def test_host_build_of_the_helpers_equals_the_restatement(exe):
    run_and_hold(exe)


def test_host_build_is_clean_under_address_and_undefined_behaviour_sanitizers(exe_sanitized):
    run_and_hold(exe_sanitized)


def test_trigamma_against_mpmath(exe):
    xs = np.concatenate([np.exp(np.linspace(np.log(1e-3), np.log(1e4), 4001)), np.arange(1, 41) * 0.5, [5.999999, 6.0, 9.999999, 10.0, 10.000001]])
    text = f"{len(xs)}\n" + "\n".join(repr(float(x)) for x in xs) + "\n"
    out = np.array([ln.split() for ln in subprocess.run([exe, "trigamma"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()], dtype=np.float64)
    worst = 0.0
    with mpmath.workdps(40):
        for x, got in zip(xs, out[:, 0]):
            want = mpmath.psi(1, mpmath.mpf(float(x)))
            worst = max(worst, float(abs(mpmath.mpf(float(got)) - want) / mpmath.mpf(float(np.spacing(float(want))))))
    print("trigamma_dev: worst error %.2f ulps over %d points" % (worst, len(xs)))
    assert worst <= TRIGAMMA_ULPS

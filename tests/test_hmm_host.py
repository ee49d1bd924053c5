"""The hidden Markov model engine's `__host__ __device__` helpers on the HOST: tests/host_emul/hmm_main.cpp compiles csrc/hmm_kernels.hpp with g++
through the stand-in <hip/hip_runtime.h> of tests/host_emul/ and drives the column table (digamma, KL), the forward and backward step of a state and
the ξ row serially over a row, in the order of the device's run.  Held to tests/hmm_ref.py at the tolerances of tests/test_hmm_gpu.py
(probabilities 1e-9 absolute, counts 1e-9 relative, free energy 1e-8 relative per iteration): the check of this arithmetic that needs no GPU."""
import os
import subprocess

import numpy as np
import pytest
from scipy.special import digamma

import hmm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hmm_host") / "hmm_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC, "-o", out,
                    os.path.join(EMUL, "hmm_main.cpp")], check=True)
    return out


def _case_text(x, m, iters):
    K, M = m["prior_A"].shape[-1], m["prior_B"].shape[-2]
    nums = np.concatenate([m["prior_s0"], m["prior_A"].ravel(), m["prior_B"].ravel(), m["init_A"].ravel(), m["init_B"].ravel(), x])
    return f"{len(x)} {K} {M} {iters} " + " ".join(repr(float(v)) for v in nums)


def _cases():
    x, _ = R.reference_data()
    ref = dict(R.REFERENCE_MODEL, init_A=np.ones((3, 3)), init_B=np.ones((3, 3)))
    out = [(x, ref, 20)]
    for seed, (T, K, M) in enumerate([(37, 5, 7), (16, 16, 64), (9, 2, 2), (1, 3, 4), (2, 4, 3), (11, 8, 5), (11, 9, 2)]):   # every row width, full and partial rows
        xx, m = R.random_case(50 + seed, T, 1, K, M, missing=0.1, per_series=False)
        out.append((xx[:, 0], m, 4))
    xx, m = R.random_case(60, 6, 1, 3, 3, per_series=False)
    out.append((np.full(6, np.nan), m, 3))       # nothing observed
    return out


def test_host_build_of_the_helpers_equals_the_restatement(exe):
    cases = _cases()
    text = f"{len(cases)}\n" + "\n".join(_case_text(*c) for c in cases) + "\n"
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert float(lines[0]) == R.K_MIN_NORMALISER      # the first line: hmm::kMinNormaliser
    lines = lines[1:]
    assert len(lines) == 5 * len(cases)
    for n, (x, m, iters) in enumerate(cases):
        gamma, a, b, fe = R.run(x, **m, iterations=iters)
        gg, ga, gb, gf, flag = (np.array(lines[5 * n + j].split(), dtype=np.float64) for j in range(5))
        small = R.min_normaliser(x, **m, iterations=iters)
        assert flag[0] == 0.0 and small > 1e-30 and abs(flag[1] - small) < 1e-9 * small, (n, flag, small)   # not refused: ordinary counts
        assert np.all(np.isfinite(gg)) and np.all(np.isfinite(gf))
        assert np.max(np.abs(gg - gamma.ravel())) < 1e-9
        assert np.max(np.abs(ga - a.ravel()) / a.ravel()) < 1e-9 and np.max(np.abs(gb - b.ravel()) / b.ravel()) < 1e-9
        assert np.max(np.abs(gf - fe) / np.abs(fe)) < 1e-8, (n, gf, fe)
    last = float(lines[3].split()[-1])
    assert abs(last - R.GOLDEN_FE) < 0.01 and abs(last - R.RECORDED_FE[20]) < 1e-8 * last


def test_digamma_of_the_header(exe):
    """ψ of csrc/digamma.hpp against scipy.  The bound is the method's own: the asymptotic series stops after the B_14 term and is used from x = 6 on,
    so its truncation error is below the next term |B_16| / (16 · 6^16) = (3617 / 510) / (16 · 6^16) = 1.6e-13; the recurrence below 6 adds at most
    six roundings of O(1) terms (1e-15).  3e-13 absolute (relative to |ψ| where that is above 1) covers both."""
    pts = [1e-3, 0.5, 1.0, 2.5, 5.999, 6.0, 6.001, 17.0, 1e3, 1e8]
    lines = subprocess.run([exe], input="0\n" + "\n".join(repr(p) for p in pts) + "\n", capture_output=True, text=True, check=True).stdout.split()
    got = np.array(lines[1:], dtype=np.float64)      # (after the constant of the first line)
    assert np.max(np.abs(got - digamma(pts)) / np.maximum(1.0, np.abs(digamma(pts)))) < 3e-13

#!/usr/bin/env python3
"""Regenerates the data of the reference's hidden Markov model test (test/models/statespace/hmm_tests.jl:54-80: StableRNG(123), 100 samples)
with the StableRNG restatement (oracle/stable_rng.py, imported unchanged) and writes hmm_stablerng123.npz next to this script.  Run from the
repo root:  python tests/golden/make_hmm_golden.py

Every state and symbol there is ONE draw `rand(rng, Categorical(p))`, which Distributions.jl serves by inverse CDF on one `rand(rng)`
(`StableRNG.categorical_inverse_cdf`).  Stored as codes 0 … 2 instead of the test's one-hot vectors: x [100] symbols, s [100] states.
What pins it: the engine's iteration on these data ends at 60.6153 after 20 iterations, the reference asserts 60.614480654 ± 0.01
(hmm_tests.jl:95; tests/test_hmm_ref_cpu.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from stable_rng import StableRNG  # noqa: E402


def hmm(n_samples=100):
    rng = StableRNG(123)
    A = np.array([[0.9, 0.0, 0.1], [0.1, 0.9, 0.0], [0.0, 0.1, 0.9]])
    B = np.array([[0.9, 0.05, 0.05], [0.05, 0.9, 0.05], [0.05, 0.05, 0.9]])
    s_prev = np.array([1.0, 0.0, 0.0])
    s, x = np.empty(n_samples, dtype=np.int64), np.empty(n_samples, dtype=np.int64)
    for t in range(n_samples):
        a = A @ s_prev
        s[t] = rng.categorical_inverse_cdf(list(a / a.sum()))
        b = B @ np.eye(3)[s[t]]
        x[t] = rng.categorical_inverse_cdf(list(b / b.sum()))
        s_prev = np.eye(3)[s[t]]
    return x, s


if __name__ == "__main__":
    x, s = hmm()
    np.savez(os.path.join(HERE, "hmm_stablerng123.npz"), x=x, s=s)
    print("x[:20] =", *x[:20], "  s[:20] =", *s[:20])

#!/usr/bin/env python3
"""Writes binreg_seed1.npz next to this script: one data set by the recipe of the reference's binomial regression test
(test/models/regression/binomialreg_tests.jl:6-25, seed = 1): N = 1000 points, true β = (−1, 0.6), X ~ N(0, 1), n_trials uniform on 5 … 20,
y_i ~ Binomial(n_i, σ(x_iᵀβ)).  Run from the repo root:
    python tests/golden/make_binreg_golden.py

X is `randn(StableRNG(1), 1000, 2)` through the StableRNG restatement (oracle/stable_rng.py, imported unchanged; Julia fills the matrix column by
column).  The draws of n_trials and of the binomial outcomes come from numpy's default_rng(1): Distributions.jl's binomial sampler is not restated,
so THE DATA ARE NOT THE REFERENCE'S BITS, only its recipe.  The reference asserts no values on them, only that the free energy falls and that the
credible intervals cover the true β.
Stored: X [1000][2], y [1000], n_trials [1000].  What pins it: the engine's iteration on these data (zero ξ0, unit W0) gives the free energies
recorded in tests/binreg_ref.py RECORDED_FE after iterations 1 and 100 (tests/test_binreg_ref_cpu.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from stable_rng import StableRNG  # noqa: E402

BETA = np.array([-1.0, 0.6])


def data(n_samples=1000, seed=1):
    rng = StableRNG(seed)
    X = np.array([rng.randn() for _ in range(n_samples * len(BETA))]).reshape(len(BETA), n_samples).T.copy()
    r = np.random.default_rng(seed)
    n = r.integers(5, 21, n_samples)
    y = r.binomial(n, 1.0 / (1.0 + np.exp(-X @ BETA)))
    return X, y.astype(np.float64), n.astype(np.float64)


if __name__ == "__main__":
    X, y, n = data()
    np.savez(os.path.join(HERE, "binreg_seed1.npz"), X=X, y=y, n_trials=n)
    print("X[0] =", *X[0], "  y[:4] =", *y[:4], "  n[:4] =", *n[:4])

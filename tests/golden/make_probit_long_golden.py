#!/usr/bin/env python3
"""Writes probit_long.npz next to this script: the CPU restatement (tests/probit_ref.py run_messages) on ONE probit chain of T = 524 289 steps,
the smallest length at which the engine's Probit-energy kernel takes more than 16 steps per partial sum (⌈T / 32768⌉ = 17).  One iteration,
4-point Gauss–Hermite rule.  The restatement is a Python loop and takes about a minute here, hence a fixture.  Run from the repo root:
    python tests/golden/make_probit_long_golden.py

Stored: T, seed, n_gh, iterations, the model (a, c, q, m0, v0), the free energy [1], `steps` (every 1024th index of x[0 … T] and the last 64)
and the posterior means and variances at those indices.  The observations are not stored: `observations(T, seed)` below regenerates them
(numpy default_rng: 0 / 1 with probability ½, 10 % missing), and tests/test_probit_contract_gpu.py imports it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

T, SEED, N_GH, ITERATIONS = 524289, 2024, 4, 1
MODEL = dict(a=0.98, c=0.01, q=0.05, m0=0.3, v0=2.0)


def observations(T, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random(T) < 0.5).astype(np.float64)
    y[rng.random(T) < 0.1] = np.nan
    return y


def steps(T):
    return np.unique(np.concatenate([np.arange(0, T + 1, 1024), np.arange(T + 1 - 64, T + 1)]))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(HERE, ".."))
    import probit_ref as R

    mean, var, fe = R.run_messages(observations(T, SEED), iterations=ITERATIONS, n_gh=N_GH, **MODEL)
    k = steps(T)
    np.savez(os.path.join(HERE, "probit_long.npz"), T=T, seed=SEED, n_gh=N_GH, iterations=ITERATIONS, fe=fe, steps=k, mean=mean[k], var=var[k],
             **{name: np.float64(v) for name, v in MODEL.items()})
    print("fe =", repr(float(fe[0])), "  mean[-1] =", repr(float(mean[-1])), "  var[-1] =", repr(float(var[-1])))

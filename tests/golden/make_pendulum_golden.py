#!/usr/bin/env python3
"""Regenerates the data set of the reference's published example (paper/example.jl `dataset(T = 1000, precision = 1.0, seed = 42)`: a pendulum with
Δt = 0.01 started at angle 0.5, its angle observed through unit-precision noise) with the StableRNG restatement (oracle/stable_rng.py, imported
unchanged) and writes pendulum_stablerng42.npz next to this script.  Run from the repo root:
    python tests/golden/make_pendulum_golden.py

The states are deterministic: states[0] = (0.5, 0), states[t] = f(states[t-1]).  One draw per step t ≥ 1, in time order:
`rand(rng, NormalMeanPrecision(angle_t, 1.0))`.  stable_rng.normal restates `rand(rng, Normal(μ, σ))` = μ + σ·randn(rng); the sampler of
NormalMeanPrecision lives in the un-vendored ExponentialFamily.jl and is taken to be the same μ + randn(rng)/√precision — one ziggurat draw per
sample, which is the whole stream here.  observations[0] stays 0.0 as in the reference (its loop starts at the second step).
Stored: y [1000] observations, states [1000][2] (angle, angular velocity).  f is written here afresh; nothing of the reference's text is kept."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from stable_rng import StableRNG  # noqa: E402

DT, G = 0.01, 9.81


def pendulum(T=1000, precision=1.0, seed=42):
    rng = StableRNG(seed)
    states, y = np.zeros((T, 2)), np.zeros(T)
    states[0] = (0.5, 0.0)
    for t in range(1, T):
        a, w = states[t - 1]
        states[t] = (a + w * DT, w - G * np.sin(a) * DT)
        y[t] = rng.normal(states[t, 0], np.sqrt(1.0 / precision))
    return y, states


if __name__ == "__main__":
    y, states = pendulum()
    np.savez(os.path.join(HERE, "pendulum_stablerng42.npz"), y=y, states=states)
    print("y[1:5] =", *y[1:5], "  states[999] =", *states[999])

#!/usr/bin/env python3
"""Regenerates the data of the reference's latent autoregressive test (test/models/autoregressive/lar_tests.jl:130-158: StableRNG(123), 500
samples of an AR(5) process with driving-noise precision 5, observed through noise of the same precision) with the StableRNG restatement
(oracle/stable_rng.py, imported unchanged) and writes lar_stablerng123.npz next to this script.  Run from the repo root:
    python tests/golden/make_lar_golden.py

The first state is five `randn` draws; every further step draws the new component `rand(rng, Normal(θ·s, √(1/5)))` and then the observation
`rand(rng, Normal(s₁, √(1/5)))`; rows 16 … 515 (1-based) are kept.  Stored: y [500] observations, z [500] the first state components.
What pins it: y[0:4] = 0.67220215, 1.73669239, 0.63298751, −0.4117014, and the engine's iteration on these data ends at 518.918234 (p = 1)
and 514.653888 (p = 5) after 15 iterations, where the reference asserts 518.9182342 and 514.66086 ± 0.01 (tests/test_lar_ref_cpu.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from stable_rng import StableRNG  # noqa: E402

COEFS = [0.10699399235785655, -0.5237303489793305, 0.3068897071844715, -0.17232255282458891, 0.13323964347539288]


def lar(n=500, gamma=5.0):
    rng = StableRNG(123)
    theta = np.array(COEFS)
    p = len(theta)
    states = [np.array([rng.randn() for _ in range(p)])]
    obs = [np.nan]
    sd = np.sqrt(1.0 / gamma)
    for _ in range(1, n + 3 * p):
        z = rng.normal(theta @ states[-1], sd)
        states.append(np.concatenate([[z], states[-1][:-1]]))
        obs.append(rng.normal(states[-1][0], sd))
    return np.array(obs[3 * p:]), np.array([s[0] for s in states[3 * p:]])


if __name__ == "__main__":
    y, z = lar()
    np.savez(os.path.join(HERE, "lar_stablerng123.npz"), y=y, z=z)
    print("y[:4] =", *y[:4], "  y[499] =", repr(float(y[499])))

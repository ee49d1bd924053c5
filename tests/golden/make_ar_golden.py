#!/usr/bin/env python3
"""Regenerates the data of the reference's autoregression test (test/models/autoregressive/ar_tests.jl) with the StableRNG restatement
(oracle/stable_rng.py, imported unchanged) and writes ar_stablerng1234.npz next to this script.  Run from the repo root:
    python tests/golden/make_ar_golden.py

The test draws `series = randn(rng, 1_000)` five times in sequence from ONE `StableRNG(1234)` (:48-53), one series per order 1 … 5, and the
benchmark draws `randn(StableRNG(32), 1_000)` (:69) for order 5.  Stored: series [5][1000] (row k is the series of order k + 1), bench [1000].
What pins it: the first draws printed below, and the free energies of the engine's iteration on these data (tests/arreg_ref.py RECORDED_FE)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
from stable_rng import StableRNG  # noqa: E402


def draws(seed, n, count=1):
    rng = StableRNG(seed)
    return np.array([[rng.randn() for _ in range(n)] for _ in range(count)])


if __name__ == "__main__":
    series, bench = draws(1234, 1000, 5), draws(32, 1000)[0]
    np.savez(os.path.join(HERE, "ar_stablerng1234.npz"), series=series, bench=bench)
    print("series[0][:3] =", *series[0][:3], "  series[4][999] =", repr(float(series[4][999])), "  bench[:3] =", *bench[:3])

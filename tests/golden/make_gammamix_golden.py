"""Writes tests/golden/gammamix_reference_config.npz: the configuration of test/models/mixtures/gamma_mixture_tests.jl (two Gamma components of equal mean
1/3, 250 points, its priors) by the reference's RECIPE under numpy's default_rng(43) with the mixing weights its test asserts, (0.8, 0.2) — not the
reference's bits: rand(rng, MixtureModel) under StableRNG(43), and the mixing weights it draws first, are not restated here (gammamix_ref.recipe)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gammamix_ref  # noqa: E402

if __name__ == "__main__":
    y, (ca, da, eb, fb, al) = gammamix_ref.recipe(43, 250)
    path = os.path.join(HERE, "gammamix_reference_config.npz")
    np.savez_compressed(path, y=y, prior_a_shape=ca, prior_a_rate=da, prior_b_shape=eb, prior_b_rate=fb, prior_alpha=al)
    print(path, os.path.getsize(path), "bytes")

"""Pins tests/mvgmm_ref.py (the NumPy restatement the device tests use above d = 8) to the C oracle rxo_mvgmm_vmp, every
iteration, where both run.  Largest differences seen on these four cases: 1.5e-13 relative (posteriors), 1.4e-14 relative
(free energy), 4e-15 absolute (responsibilities); the bounds leave three decades for another BLAS summation order."""
import numpy as np
import pytest

import rxoracle

import mvgmm_ref
from test_mvgmm_gpu import rel, ring_data, setup


@pytest.mark.parametrize("d,K,N,iters", [(2, 3, 500, 10), (5, 3, 300, 6), (8, 5, 700, 6), (8, 16, 2000, 4)])
def test_restatement_matches_the_oracle_every_iteration(d, K, N, iters):
    y, means, covs = ring_data(N, K, d, 50.0, seed=10 * d + K)
    mu0, S0, nu0, V0, al0 = setup(K, d, means, seed=K)
    init = rxoracle.mvgmm_pack(mu0, S0, nu0, V0, np.ones(K))
    ohist, ofe, oresp = rxoracle.mvgmm_vmp(y, mu0, S0, nu0, V0, al0, init, iters, want_resp=True)
    rhist, rfe, rresp = mvgmm_ref.mvgmm_vmp(y, mu0, S0, nu0, V0, al0, init, iters, want_resp=True)
    o, r = rxoracle.mvgmm_unpack(ohist, d), rxoracle.mvgmm_unpack(rhist, d)
    for key in ("mean", "cov", "nu", "V", "alpha"):
        e = rel(r[key], o[key])
        print(f"d={d} K={K} {key}: rel {e:.2e}")
        assert e < 1e-10, key
    efe, eresp = float(np.max(np.abs(rfe - ofe) / np.abs(ofe))), float(np.max(np.abs(rresp - oresp)))
    print(f"d={d} K={K} fe rel {efe:.2e}  resp abs {eresp:.2e}")
    assert efe < 1e-12
    assert eresp < 1e-12

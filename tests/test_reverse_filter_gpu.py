"""The reverse-filter schedule of the shared-model sweep (k_forward0 with checkpoints + k_backward_sh_rev) against
the oracle (posteriors 1e-6 relative, free energy 1e-8) and against the per-step records schedule on the same data (covariances
and free energy bit-identical, means within 1e-12 posterior sd); the stride each model gets is the numpy restatement's."""
import math
import os

import numpy as np
import pytest

import rxhip
from rxhip import workloads
import reverse_filter_ref as R
from test_lgssm_gpu import oracle_batch, rel
from test_reverse_filter import MODELS, c1_variant

pytestmark = pytest.mark.gpu

RTOL_POST = 1e-6
RTOL_FE = 1e-8


def run(mdl, y, segments=0, **hooks):
    env = {"RXHIP_TEST_HOOKS": "1", "RXHIP_ONE_PASS": "1", **hooks}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        T, C = y.shape[0], y.shape[1]
        with rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C,
                               segments=segments, device=0) as eng:
            K = eng.mean_checkpoint_stride()
            eng.set_data(y)
            eng.run(iterations=1, free_energy=True)
            mean, cov = eng.marginals()
            return K, np.array(mean), np.array(cov), np.array(eng.free_energy_per_chain())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_against_oracle(mdl, y, mean, cov, fe):
    om, oc, ofe = oracle_batch(mdl, y)[:3]
    assert rel(mean, om) < RTOL_POST, rel(mean, om)
    assert rel(cov, oc) < RTOL_POST, rel(cov, oc)
    assert float(np.max(np.abs(fe - ofe) / np.abs(ofe))) < RTOL_FE


def check_against_records(mdl, y, segments, mean, cov, fe):
    K0, m0, c0, f0 = run(mdl, y, segments, RXHIP_MEAN_RECORDS="1")
    assert K0 == 0
    assert np.array_equal(cov, c0)
    assert np.array_equal(fe, f0)
    sd = np.sqrt(np.einsum("tcii->tci", c0))
    assert float(np.max(np.abs(mean - m0) / sd)) < 1e-12


@pytest.mark.parametrize("name,make,K", MODELS, ids=[m[0] for m in MODELS])
def test_engine_picks_the_restated_stride(name, make, K):
    mdl = make()
    T, C, S = 1201, 64, 8
    y = workloads.generate_batch(mdl, T, C, seed0=7)
    Kg, mean, cov, fe = run(mdl, y, segments=S)
    assert Kg == R.choose_stride(mdl, T, math.ceil((T - 1) / S)) == K
    if name == "singular_a":   # outside the oracle's domain: the stride is what is checked
        return
    check_against_oracle(mdl, y, mean, cov, fe)
    if K:
        check_against_records(mdl, y, S, mean, cov, fe)


@pytest.mark.parametrize("K", [8, 16, 32])
@pytest.mark.parametrize("T,S", [(1001, 4), (777, 3), (250, 40)])   # T − 1 not a multiple of K; (250, 40): segments shorter than K
def test_forced_strides(K, T, S):
    mdl = workloads.c1_model()
    y = workloads.generate_batch(mdl, T, 128, seed0=11)
    Kg, mean, cov, fe = run(mdl, y, segments=S, RXHIP_MEAN_CHECKPOINT=str(K))
    assert Kg == K
    check_against_oracle(mdl, y, mean, cov, fe)
    check_against_records(mdl, y, S, mean, cov, fe)


@pytest.mark.parametrize("dy", [1, 2, 3, 4])
def test_observation_dimensions(dy):
    mdl = c1_variant(q=100.0, dy=dy)
    T, S = 901, 5
    y = workloads.generate_batch(mdl, T, 64, seed0=3)
    Kg, mean, cov, fe = run(mdl, y, segments=S)
    assert Kg == R.choose_stride(mdl, T, math.ceil((T - 1) / S)) == (16 if dy in (1, 3) else 32)
    check_against_oracle(mdl, y, mean, cov, fe)
    check_against_records(mdl, y, S, mean, cov, fe)

"""Host side of the mixture engines' contract (tests/mvgmm_ref.py: contract_errors, hold, CASES).

* the NumPy restatement the device tests use is pinned to the C oracle rxo_mvgmm_vmp under the per-component contract, every iteration,
  on every case of the table where both run (d ≤ 8) below N = 1e4;
* every case of the table is shown to be well conditioned before a device test may use it: the restatement on the data in reversed order
  agrees with itself within mvgmm_ref.CONDITION (1e-8 on the posteriors, 1e-10 on the free energy), two decades inside the contract.  That is
  a condition on the inputs, not a measurement: a case that misses it is replaced;
* the per-component norm rejects what the old norm over the whole history accepted (test_teeth).

Largest differences seen, per (iteration, component).  Restatement against oracle: means 3.7e-9 posterior sd, nu and alpha 2.6e-12,
responsibilities 6.2e-12 (all lane (2, 16, 4000, 6)), cov 5.1e-11 (lane (2, 5, 333, 4)), V 7.1e-11 (lane (3, 8, 257, 3)), free energy
6.8e-13 (dense (5, 3, 15, 4)); on the four cases of the pin 1.5e-11 sd, 4e-13, 5e-14, 5e-14.  Order sensitivity of the restatement: means
1.1e-9 sd (the dense grid-stride case, N = 65 957), cov 5.9e-11 (dense (32, 3, 15, 4)), V 2.1e-10 (dense (31, 5, 17, 4)), free energy
3.9e-12 (dense (15, 3, 17, 4)), responsibilities 1.2e-12; at the lane grid-stride size 1.6e-10 sd, 9e-14, 4e-13, 2e-14; the offset case
1.6e-8 (cov), 3.0e-8 (V), 6.5e-9 sd, 7e-11 (mvgmm_ref.CONDITION_OFFSET)."""
import numpy as np
import pytest

import rxoracle

import mvgmm_ref
from mvgmm_ref import CASES, CONDITION, CONTRACT, KEYS, contract_errors, hold, rel

ALL = sorted({c for group in CASES.values() for c in group})
ident = lambda c: f"d{c.d}-K{c.K}-N{c.N}-it{c.iters}-L{c.L:g}" + (f"-off{c.offset:g}" if c.offset else "") + ("" if c.kind == "ring" else "-" + c.kind)
# the bounds of the pin: CONDITION (reference against reference has to sit two decades inside the contract); the four cases this test
# always had (CASES["restatement"]) keep their earlier bounds — 1e-10 on the posteriors, now per (iteration, component), which implies the
# norm over the whole history it was taken in; 1e-12 on the free energy and the responsibilities
PIN = dict(CONDITION, mean_global=1e-10, cov=1e-10, V=1e-10, nu=1e-10, alpha=1e-10, fe=1e-12, resp=1e-12)


@pytest.mark.parametrize("d,K,N,iters", [c[:4] for c in CASES["restatement"]])
def test_restatement_matches_the_oracle_every_iteration(d, K, N, iters):
    c = mvgmm_ref.Case(d, K, N, iters)
    hold(mvgmm_ref.case(c)[3], mvgmm_ref.oracle(c), ident(c), bounds=PIN)


@pytest.mark.parametrize("c", [c for c in ALL if c.d <= 8 and c.N < 10 ** 4 and c not in CASES["restatement"]], ids=ident)
def test_restatement_matches_the_oracle_on_every_device_case(c):
    """At the grid-stride sizes (N ≈ 262 000) the oracle is left out, here and in the device tests: it sums sequentially and differs from the
    restatement's pairwise sums by up to 1.0e-7 posterior sd in the means there, while the restatement's own order sensitivity at that size is
    1.6e-10 (test_cases_are_well_conditioned); the reference at that size is the restatement."""
    hold(mvgmm_ref.case(c)[3], mvgmm_ref.oracle(c), ident(c), bounds=CONDITION)


@pytest.mark.parametrize("c", ALL, ids=ident)
def test_cases_are_well_conditioned(c):
    """the same reference on the data in reversed order: only the summation order differs, as it does on the device"""
    y, pri, init, ref = mvgmm_ref.case(c)
    hist, fe, resp = mvgmm_ref.mvgmm_vmp(y[::-1], *pri, rxoracle.mvgmm_pack(*init), c.iters, want_resp=True)
    hold(mvgmm_ref.result(hist, c.d, fe, resp[::-1]), ref, "order " + ident(c), bounds=mvgmm_ref.CONDITION_OFFSET if c.offset else CONDITION)


def test_univariate_stride_cases_are_well_conditioned():
    """the univariate engine's grid-stride cases (tests/test_gmm_gpu.py) against the C oracle, which sums sequentially: reversed against original
    order within 1e-8 element-wise, 1e-10 on the free energy"""
    for K in (2, 11):
        y, priors, init = mvgmm_ref.uv_case(K, mvgmm_ref.STRIDE_N, 20 + K)
        h0, f0, _, _ = rxoracle.gmm_vmp(y, *priors, *init, 3)
        h1, f1, _, _ = rxoracle.gmm_vmp(y[::-1].copy(), *priors, *init, 3)
        e, ef = float(np.max(np.abs(h1 - h0) / np.abs(h0))), float(np.max(np.abs(f1 - f0) / np.abs(f0)))
        print(f"univariate K={K} order: hist {e:.2e} fe {ef:.2e}")
        assert e < 1e-8 and ef < 1e-10


def test_teeth():
    """What the per-component norm buys.  Lane case (1, 3, 777, 8) has starved components, whose cov stays at the prior's 1e6 and V at 1e2: the
    norm over the whole history divides every populated component's error by those.  A populated component's cov, and separately its V, off by
    1e-4 relative in every iteration: hold rejects it, the old norm accepts it."""
    c = mvgmm_ref.Case(1, 3, 777, 8)
    assert c in CASES["lane"]
    _, pri, _, ref = mvgmm_ref.case(c)
    gained = ref["nu"][-1] - pri[2]
    assert np.sum(gained < 1e-6) >= 1                     # a starved component …
    k = int(np.argmax(gained))
    assert gained[k] > 100                                # … and a populated one
    for key in ("cov", "V"):
        bad = {q: np.array(v) for q, v in ref.items()}
        bad[key][:, k] *= 1.0 + 1e-4
        old = {q: rel(bad[q], ref[q]) for q in KEYS}
        print(key, "old norm", old)
        assert all(v < 1e-6 for v in old.values())        # every assertion of the old tests passes
        assert contract_errors(bad, ref)[key] > 0.99e-4
        with pytest.raises(AssertionError):
            hold(bad, ref, "perturbed " + key)
    hold({q: np.array(v) for q, v in ref.items()}, ref, "unperturbed")


def test_hold_rejects_shapes_and_non_finite_values():
    _, _, _, ref = mvgmm_ref.case(mvgmm_ref.Case(2, 1, 300, 5))
    copy = lambda: {q: np.array(v) for q, v in ref.items()}
    bad = copy()
    bad["V"][2, 0, 1, 1] = np.nan
    with pytest.raises(AssertionError):
        hold(bad, ref)
    bad = copy()
    bad["fe"] = bad["fe"][:-1]
    with pytest.raises(AssertionError):
        hold(bad, ref)
    bad = copy()
    bad["mean"][0, 0, 0] += 2e-6 * np.sqrt(ref["cov"][0, 0, 0, 0])   # 2e-6 posterior sd: inside the old norm, outside the contract
    assert rel(bad["mean"], ref["mean"]) < 1e-6
    with pytest.raises(AssertionError):
        hold(bad, ref)
    assert set(CONTRACT) == set(CONDITION) == set(KEYS) | {"mean_global", "fe", "resp"}

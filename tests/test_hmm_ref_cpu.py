"""The CPU restatement of the hidden Markov model engine (tests/hmm_ref.py) held to what does not depend on it: the enumeration of every path
on tiny cases, the free energy written out term by term, and the reference's own known answer on its regenerated data."""
import numpy as np
import pytest

import hmm_ref as R


def _tiny(seed, T, K, M, missing):
    x, m = R.random_case(seed, T, 1, K, M, missing=0.0, per_series=False)
    x = x[:, 0]
    if missing:
        x[np.random.default_rng(seed).integers(0, T)] = np.nan
    return x, m


@pytest.mark.parametrize("missing", [False, True])
@pytest.mark.parametrize("T,K,M", [(1, 2, 2), (2, 3, 2), (3, 2, 3), (5, 3, 3), (4, 3, 3)])
def test_forward_backward_equals_the_enumeration_of_all_paths(T, K, M, missing):
    x, m = _tiny(100 * T + 10 * K + M, T, K, M, missing)
    At, Bt = R.tables(m["init_A"])[1], R.tables(m["init_B"])[1]
    gamma, xi, n, mstat, logz = R.forward_backward(m["prior_s0"], At, Bt, x)
    bg, bn, bm, bz = R.brute_force(m["prior_s0"], At, Bt, x)
    assert np.max(np.abs(gamma - bg)) < 1e-13 and np.max(np.abs(n - bn)) < 1e-13 and np.max(np.abs(mstat - bm)) < 1e-13
    assert abs(logz - bz) < 1e-13 * max(1.0, abs(bz))
    assert np.allclose(gamma.sum(1), 1.0, atol=1e-14) and np.allclose(xi.sum((1, 2)), 1.0, atol=1e-14)
    assert np.allclose(xi.sum(2), gamma[1:], atol=1e-14) and np.allclose(xi.sum(1), gamma[:-1], atol=1e-14)


@pytest.mark.parametrize("seed,T,K,M", [(1, 5, 3, 3), (2, 37, 5, 7), (3, 64, 16, 64), (4, 9, 2, 2), (5, 1, 3, 4), (6, 2, 4, 3)])
def test_the_two_free_energy_forms_agree(seed, T, K, M):
    x, m = R.random_case(seed, T, 1, K, M, missing=0.1, per_series=False)
    short = R.run(x[:, 0], **m, iterations=5)[3]
    direct = R.run(x[:, 0], **m, iterations=5, direct=True)[3]
    assert np.all(np.isfinite(short))
    assert np.max(np.abs(short - direct) / np.abs(direct)) < 1e-10


@pytest.fixture(scope="module")
def golden_run():
    x, s = R.reference_data()
    return x, s, R.run(x, **R.REFERENCE_MODEL, iterations=20)


def test_golden_data_are_the_recorded_draws(golden_run):
    x, s, _ = golden_run
    assert x.shape == (100,) and s.shape == (100,)
    assert list(x[:20].astype(int)) == [0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 1]
    assert np.all(s[:20] == 0)


def test_golden_free_energy(golden_run):
    _, _, (gamma, a, b, fe) = golden_run
    print("free energy:", [repr(float(v)) for v in fe[[0, 1, -1]]])
    assert abs(fe[-1] - R.GOLDEN_FE) < 0.01                                   # hmm_tests.jl:95
    for it, want in R.RECORDED_FE.items():
        assert abs(fe[it - 1] - want) < 1e-8 * want, (it, fe[it - 1])
    assert np.all(np.diff(fe) <= 1e-9 * np.abs(fe[1:]))                       # the free energy never rises
    assert np.allclose(gamma.sum(1), 1.0, atol=1e-13)
    assert np.allclose(a.sum(), 9.0 + 100.0) and np.allclose(b.sum(), 36.0 + 100.0)


def test_shared_parameters_with_one_series_is_the_unshared_run():
    x, m = R.random_case(7, 12, 1, 3, 4, per_series=False)
    g1, a1, b1, f1, _ = R.run_batch(x, **m, iterations=4)
    g2, a2, b2, f2, parts = R.run_batch(x, **m, iterations=4, share_parameters=True)
    assert np.array_equal(g1, g2) and np.allclose(a1, a2, rtol=1e-15) and np.allclose(b1, b2, rtol=1e-15)
    assert np.allclose(f1, f2, rtol=1e-13) and parts.shape == (4, 1)


def test_one_hot_helper():
    v = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 0, 0], [0.5, 0.5, 0], [0, 1.0, 0]])
    c = R.one_hot_to_codes(v)
    assert list(c[[0, 1, 4]]) == [0.0, 2.0, 1.0] and np.isnan(c[2]) and np.isnan(c[3])

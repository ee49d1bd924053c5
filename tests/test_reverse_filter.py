"""The reverse-filter schedule restated in numpy (no GPU): the inverted Kalman update reproduces a forward filter run, the
checkpoint windows the chooser admits keep the rebuilt means within 1e-12 posterior sd, and the stride every model of
test_reverse_filter_gpu.py should get (the GPU test checks the engine reports the same)."""
import numpy as np
import pytest

import reverse_filter_ref as R
from rxhip import workloads


def c1_variant(q=10.0, dy=4):
    m = dict(workloads.c1_model())
    m["B"] = m["B"][:dy]
    m["Q"] = q * np.eye(dy)
    return m


def singular_a(scale=0.0):
    m = dict(workloads.c1_model())
    A = m["A"].copy()
    A[3] *= scale
    m["A"] = A
    return m


# (name, model, expected stride) — the models of the GPU test
MODELS = [
    ("c1", lambda: workloads.c1_model(), 16),
    ("c1_q2", lambda: c1_variant(q=2.0), 8),
    ("c1_q100", lambda: c1_variant(q=100.0), 32),
    ("c1_dy2", lambda: c1_variant(dy=2), 16),
    ("c1_dy1", lambda: c1_variant(dy=1), 0),          # the unobserved components make the reverse step grow fast
    ("high_snr", lambda: c1_variant(q=1e-4), 0),
    ("singular_a", singular_a, 0),
    ("nearly_singular_a", lambda: singular_a(1e-8), 0),
    ("notebook_d2", lambda: workloads.notebook_model(), 16),
]


@pytest.mark.parametrize("name,make,K", MODELS, ids=[m[0] for m in MODELS])
def test_chooser(name, make, K):
    m = make()
    for L in (100, 150):   # past the first segment's transient the bound is stationary: the choice does not depend on L
        assert R.choose_stride(m, 600, L) == K


def test_dy_above_d_falls_back():
    m = workloads.random_model(2, 3, seed=4)
    assert R.choose_stride(m, 600, 100) == 0


def test_chains_not_multiple_of_64_fall_back():
    assert R.choose_stride(workloads.c1_model(), 600, 100, n_chains=96) == 0


def test_singular_a_has_no_bound():
    assert np.all(np.isinf(R.step_bounds(singular_a(), 50)))


def test_spec_norm_bound_is_an_upper_bound():
    rng = np.random.default_rng(3)
    for _ in range(200):
        M = rng.standard_normal((4, 4)) * rng.uniform(0.1, 10.0)
        s = np.linalg.norm(M, 2)
        b = R.spec_norm_bound(M)
        assert s * (1 - 1e-12) <= b <= s * 4 ** (1 / 32) * (1 + 1e-12)
    Qm, _ = np.linalg.qr(rng.standard_normal((4, 4)))
    assert abs(R.spec_norm_bound(Qm) - 1.0) < 1e-12   # exact for an orthogonal matrix


@pytest.mark.parametrize("name,make", [("c1", lambda: workloads.c1_model()), ("c1_dy2", lambda: c1_variant(dy=2)),
                                       ("random_d3", lambda: workloads.random_model(3, 2, seed=8))])
def test_one_reverse_step_inverts_the_update(name, make):
    """m_f(t) = A⁻¹[m_f(t+1) + V_p(t+1)(B'Q⁻¹B m_f(t+1) − B'Q⁻¹ y_{t+1})] against a forward filter run, to rounding"""
    m = make()
    T, C = 300, 8
    y = workloads.generate_batch(m, T, C)
    mf, Vf, Vps = R.kalman_means(m, y)
    lobs, g = R.obs_terms(m["B"], m["Q"])
    Ai = np.linalg.inv(m["A"])
    scale = np.abs(mf).max()
    for t in range(T - 1):
        mp = mf[t + 1] + (Vps[t + 1] @ (lobs @ mf[t + 1].T - g @ y[t + 1].T)).T
        assert np.abs(mp @ Ai.T - mf[t]).max() <= 1e-12 * scale


@pytest.mark.parametrize("name,make,K", [m for m in MODELS if m[2]], ids=[m[0] for m in MODELS if m[2]])
def test_admitted_windows_keep_the_means(name, make, K):
    """with the stride the chooser admits, the means rebuilt from checkpoints stay within 1e-12 posterior sd"""
    m = make()
    T, C, L = 2000, 4, 250
    y = workloads.generate_batch(m, T, C)
    mf, Vf, Vps = R.kalman_means(m, y)
    mr = R.reverse_means(m, y, mf, K, L, Vps)
    sd = np.sqrt(np.einsum("tii->ti", Vf))[:, None, :]
    assert np.max(np.abs(mr - mf) / sd) < 1e-12

"""The C oracle's HGF filter (oracle/rxoracle.c rxo_hgf_filter — the reference the engine is held to, tests/test_hgf_contract_gpu.py) against
the 60-digit restatement tests/hgf_ref.py, at the corners of that test's parameter grid and at its centre.  The oracle has to agree 100× inside
the project's contract — means 1e-8 posterior sd, variances 1e-8 relative, free energy 1e-10 relative, per element, iteration and series — so
that the GPU comparison keeps its whole budget."""
import numpy as np
import pytest

import hgf_ref as R
import rxoracle
from test_hgf_gpu import hgf_series

T, SEED = 12, 11
ITERS, ORDERS = (1, 6), (3, 17, 31, 32)
MEAN_BOUND, VAR_BOUND, FE_BOUND = 1e-8, 1e-8, 1e-10

# Ill-posed: the three-point rule's nodes (0, ±1.22·sqrt(2·forward variance)) miss the mode of the z-message, one weight carries the whole sum
# and q(zt)'s variance is what the subtraction of the two reduction rounds leaves — in exact arithmetic 1e-15 … 1e-236 of the forward variance
# (third entry, from hgf_ref), in fp64 rounding residue or zero.  Second entry: what the oracle gives there (its status, or its mean error in
# posterior sd against hgf_ref).  All of them have n_gh = 3, κ = −1.5; the contract test runs GH-31 on the grid and meets none of them.
ILL_POSED = {
    # (κ, ω, z variance, y variance), iterations, n_gh : (oracle, min over t of var q(zt) / forward variance)
    ((-1.5, -6.0, 1e-4, 1e-6), 1, 3): ("mean 1.3e-8 sd", 1.4e-15),
    ((-1.5, 4.0, 1e-4, 1e-6), 1, 3): ("mean 8.6e-5 sd", 3.2e-23),
    ((-1.5, -6.0, 1.0, 1e-6), 1, 3): ("status 4", 1.5e-236),
    ((-1.5, -6.0, 1.0, 1e-6), 6, 3): ("status 4", 2.6e-36),
    ((-1.5, 4.0, 1.0, 1e-6), 1, 3): ("status 4", 0.0),
    ((-1.5, 4.0, 1.0, 1e-6), 6, 3): ("status 4", 7.4e-36),
    ((-1.5, 4.0, 1.0, 1e2), 6, 3): ("status 4", 0.0),
}
RESIDUE = 1e-12   # var q(zt) below this fraction of the forward variance: fewer than four digits of it survive the fp64 subtraction

_worst = {"mean": (0.0, None), "var": (0.0, None), "fe": (0.0, None)}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """after the module: the worst agreement per quantity (-s shows it; DESIGN.md's HGF table quotes it)"""
    yield
    for q, (v, key) in _worst.items():
        if key is not None:
            print(f"\nworst {q}: {v:.2e} at {key}")


def _errors(o, r):
    em = max(float(np.max(np.abs(o[0] - r[0]) / np.sqrt(r[1]))), float(np.max(np.abs(o[2] - r[2]) / np.sqrt(r[3]))))
    ev = max(float(np.max(np.abs(o[1] - r[1]) / r[1])), float(np.max(np.abs(o[3] - r[3]) / r[3])))
    ef = float(np.max(np.abs(o[4] - r[4]) / np.abs(r[4])))
    return em, ev, ef


def test_gauss_hermite_nodes_of_the_oracle():
    """the rule itself, at every order the engine accepts: nodes 1e-14 absolute (they are O(1 … 7)), weights 1e-12 relative — down to the 7e-30
    of the outermost weights at n = 32"""
    for n in range(1, 33):
        x, w = R.gauss_hermite(n)
        x, w = np.array([float(v) for v in x]), np.array([float(v) for v in w])
        ox, ow = rxoracle.gauss_hermite(n)
        order = np.argsort(ox)
        assert np.max(np.abs(ox[order] - x)) < 1e-14, n
        assert np.max(np.abs(ow[order] - w) / w) < 1e-12, n


@pytest.mark.parametrize("case", R.CORNERS, ids=lambda c: "k%g_w%g_zv%g_yv%g" % c)
def test_oracle_against_the_restatement(case):
    k, w, zv, yv = case
    y = hgf_series(T, k, w, zv, yv, SEED)[2]
    for iters in ITERS:
        for n_gh in ORDERS:
            r = R.hgf_filter(y, k, w, zv, yv, iters=iters, n_gh=n_gh)
            key = (case, iters, n_gh)
            if key in ILL_POSED:
                forward = np.concatenate([[5.0], r[1][:-1]]) + zv
                assert np.min(r[1] / forward) < RESIDUE, key   # … and is listed for that reason only
                continue
            o = rxoracle.hgf_filter(y, k, w, zv, yv, vmp_iters=iters, n_gh=n_gh)
            em, ev, ef = _errors(o, r)
            print(f"{key}: mean {em:.2e} sd, var rel {ev:.2e}, fe rel {ef:.2e}")
            for q, v in (("mean", em), ("var", ev), ("fe", ef)):
                if v > _worst[q][0]:
                    _worst[q] = (v, key)
            assert em < MEAN_BOUND and ev < VAR_BOUND and ef < FE_BOUND, (key, em, ev, ef)


def test_the_ill_posed_list_is_short_and_inside_the_corners():
    assert all(c in R.CORNERS for c, _, _ in ILL_POSED) and len(ILL_POSED) <= 10


@pytest.mark.parametrize("s", [1e-6, 1e6])
def test_the_oracle_is_scale_equivariant(s):
    """y → s·y with y variance, x0 variance → s²·, x0 mean → s·, ω → ω + 2 ln s: the model for x/s is the original one, so q(z) is unchanged, q(x)
    scales, and the free energy (−log of a density of y) gains ln s per observation — hence ln s, it being the mean over the observations.
    The engine is held to this at the contract (tests/test_hgf_contract_gpu.py); the oracle here at 100× inside it, at the test's sizes."""
    for k, w, zv, yv in R.CORNERS:
        y = hgf_series(40, k, w, zv, yv, SEED)[2]
        a = rxoracle.hgf_filter(y, k, w, zv, yv, x0=(-0.2, 3.0), vmp_iters=18)
        b = rxoracle.hgf_filter(y * s, k, w + 2.0 * np.log(s), zv, yv * s * s, x0=(-0.2 * s, 3.0 * s * s), vmp_iters=18)
        em, ev, ef = _errors((b[0], b[1], b[2] / s, b[3] / (s * s), b[4] - np.log(s)), a)
        ef = float(np.max(np.abs(b[4] - np.log(s) - a[4]) / np.minimum(np.abs(a[4]), np.abs(b[4]))))
        assert em < MEAN_BOUND and ev < VAR_BOUND and ef < FE_BOUND, ((k, w, zv, yv), em, ev, ef)

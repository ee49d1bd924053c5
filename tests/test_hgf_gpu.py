"""GPU parity tests for the hierarchical Gaussian filter (BASELINE config 4): HIP path vs the CPU
oracle's restatement on the same seeded series (posteriors 1e-6 relative, free energy 1e-8 relative), shaped after
test/models/statespace/hgf_tests.jl.  The VMP order and the free-energy treatment of the non-Gaussian z-message are
assumptions of the oracle (see oracle/rxoracle.h): parity against the real reference is unpinned."""
import numpy as np
import pytest

import rxhip
import rxoracle

pytestmark = pytest.mark.gpu


def hgf_series(n, k, w, zv, yv, seed):
    """generate_data of test/models/statespace/hgf_tests.jl:72-92 with numpy's default_rng"""
    rng = np.random.default_rng(seed)
    z = np.zeros(n); x = np.zeros(n); y = np.zeros(n)
    zp = xp = 0.0
    for i in range(n):
        z[i] = zp + np.sqrt(zv) * rng.standard_normal()
        x[i] = xp + np.sqrt(np.exp(k * z[i] + w)) * rng.standard_normal()
        y[i] = x[i] + np.sqrt(yv) * rng.standard_normal()
        zp, xp = z[i], x[i]
    return z, x, y


def _hold(got, ref):
    """the project's contract per element: means within 1e-6 posterior sd (the reference's variance), variances within 1e-6 relative;
    got, ref = (zm, zv, xm, xv) of one series"""
    em = max(float(np.max(np.abs(got[i] - ref[i]) / np.sqrt(ref[i + 1]))) for i in (0, 2))
    ev = max(float(np.max(np.abs(got[i] - ref[i]) / ref[i])) for i in (1, 3))
    print(f"mean err {em:.3e} sd, var rel {ev:.3e}")
    assert all(np.all(np.isfinite(a)) for a in got) and em < 1e-6 and ev < 1e-6, (em, ev)


def test_hgf_reference_test_shape():
    """κ = 1, ω = 0, z variance 0.04, y variance 0.01, T = 2000, 10 iterations, GH-31, init N(0, 5) (hgf_tests.jl:94-105)."""
    k, w, zv, yv, n = 1.0, 0.0, 0.2 ** 2, 0.1 ** 2, 2000
    S = 5
    data = [hgf_series(n, k, w, zv, yv, 42 + s) for s in range(S)]
    y = np.stack([d[2] for d in data], axis=1)  # [T][series]
    with rxhip.HGFEngine(n, S, k, w, zv, yv) as eng:
        eng.set_data(y)
        eng.run(10, True)
        zm, zvv, xm, xv = eng.history()
        fe_tot, fe_s, cnt = eng.free_energy(), eng.free_energy_per_chain(), eng.counters()
    fe_sum = np.zeros(10)
    for s in range(S):
        ozm, ozv, oxm, oxv, ofe, ocnt = rxoracle.hgf_filter(y[:, s], k, w, zv, yv)
        for a, b in ((zm[:, s], ozm), (zvv[:, s], ozv), (xm[:, s], oxm), (xv[:, s], oxv)):
            assert np.max(np.abs(a - b)) < 1e-6 * np.max(np.abs(b))
        _hold((zm[:, s], zvv[:, s], xm[:, s], xv[:, s]), (ozm, ozv, oxm, oxv))
        assert abs(fe_s[s] - ofe[-1]) < 1e-8 * abs(ofe[-1])
        fe_sum += ofe
        # the reference test's statistical assertions (hgf_tests.jl:119-133)
        z, x = data[s][0], data[s][1]
        if s == 0:  # one series, as in the reference test; mean-field VMP is over-confident on some other seeds
            assert np.mean(np.abs(zm[:, s] - z) < 3 * np.sqrt(zvv[:, s])) > 0.95
        assert np.mean(np.abs(xm[:, s] - x) < 3 * np.sqrt(xv[:, s])) > 0.95
        assert np.all(zvv[:, s] > 0) and np.all(xv[:, s] > 0)
        assert np.all(ofe[:-1] - ofe[1:] > -1e-9)  # free energy decreasing over iterations
    assert np.max(np.abs(fe_tot - fe_sum) / np.abs(fe_sum)) < 1e-8
    assert cnt["rule_calls"] == S * ocnt.rule_calls


@pytest.mark.parametrize("S,T,iters,n_gh,layout", [(1, 50, 3, 31, "time_chain"), (3, 200, 5, 21, "chain_time"), (130, 64, 2, 32, "time_chain"),
                                                   (2, 1, 10, 31, "time_chain"), (5, 30, 20, 17, "time_chain"), (7, 20, 18, 3, "chain_time"),
                                                   (4, 25, 16, 16, "time_chain")])
def test_hgf_shapes(S, T, iters, n_gh, layout):
    k, w, zv, yv = 0.8, -0.5, 0.05, 0.02
    ys = np.stack([hgf_series(T, k, w, zv, yv, 7 + s)[2] for s in range(S)], axis=1)
    with rxhip.HGFEngine(T, S, k, w, zv, yv, z0=(0.1, 2.0), x0=(-0.2, 3.0), n_gh=n_gh) as eng:
        eng.set_data(ys if layout == "time_chain" else ys.T.copy(), layout=layout)
        eng.run(iters, True)
        zm, zvv, xm, xv = eng.history(layout)
        fe = eng.free_energy()
    if layout == "chain_time":
        zm, zvv, xm, xv = zm.T, zvv.T, xm.T, xv.T
    fe_sum = np.zeros(iters)
    for s in range(S):
        o = rxoracle.hgf_filter(ys[:, s], k, w, zv, yv, z0=(0.1, 2.0), x0=(-0.2, 3.0), vmp_iters=iters, n_gh=n_gh)
        assert np.max(np.abs(zm[:, s] - o[0])) <= 1e-6 * max(np.max(np.abs(o[0])), 1e-30)
        assert np.max(np.abs(xv[:, s] - o[3])) <= 1e-6 * np.max(np.abs(o[3]))
        _hold((zm[:, s], zvv[:, s], xm[:, s], xv[:, s]), o[:4])
        fe_sum += o[4]
    assert np.max(np.abs(fe - fe_sum) / np.abs(fe_sum)) < 1e-8


def test_hgf_free_energy_outside_cubature_range_fails_like_the_reference():
    """A log-volatility far outside the ±9.9 range of the 31-point rule: `mean_var` of the z-message collapses to zero
    variance, the reference's free energy is NaN (src/score/diagnostics.jl:19-51 raises) — the engine reports
    RXHIP_ERR_NONFINITE_FE, the oracle RXO_ERR_NONFINITE_FE; the posteriors (free energy off) are unaffected."""
    rng = np.random.default_rng(3)
    T = 60
    y = np.cumsum(np.exp(0.5 * 17.0) * rng.standard_normal(T)) + 0.1 * rng.standard_normal(T)
    with pytest.raises(RuntimeError):
        rxoracle.hgf_filter(y, 1.0, 0.0, 0.04, 0.01)
    with rxhip.HGFEngine(T, 1, 1.0, 0.0, 0.04, 0.01) as eng:
        eng.set_data(y[:, None])
        with pytest.raises(rxhip.RxHipError) as ei:
            eng.run(10, True)
        assert ei.value.status == 4
    with rxhip.HGFEngine(T, 1, 1.0, 0.0, 0.04, 0.01) as eng:
        eng.set_data(y[:, None])
        eng.run(10, False)
        zm, zv, xm, xv = eng.history()
    o = rxoracle.hgf_filter(y, 1.0, 0.0, 0.04, 0.01, want_fe=False)
    assert np.max(np.abs(zm[:, 0] - o[0])) <= 1e-6 * np.max(np.abs(o[0]))

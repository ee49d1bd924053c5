"""The latent autoregressive engine (include/rxhip.h rxhip_lar_desc, csrc/lar_kernels.hpp) held to the project's contract across its range,
against 50 digits: state means within 1e-6 posterior standard deviations; (co)variances, θ and b within 1e-6 relative; a exact; the free energy
within 1e-8·max(1, |F|) per iteration and, of the last iteration, per series — on every case of lar_mp.GRID: every order 1 … 8 over 257 steps and
15 iterations (249 and more interior rows through the shortcut, the record prefetch and the register windows of every k_lar_sweep<P>), T = 4096
at p = 1 and p = 8 with a run of 200 missing steps, T = 1, 2, p − 1, p, p + 1 at p = 8 and 5, τ over twelve decades and γ over nine, data scales
1e-4 and 1e3, θ = 0.999, 1 and 1.02, all the mass on lag 8, prior precisions 1e-6 and 1e6 and of condition 1e4, an initial q(θ) far from the
prior, everything missing, one observed step, offsets up to the envelope's edge, and 65 and 70 series of scales 1 … 100 under one q(θ), q(γ) in
both layouts.  The reference is the fixture tests/golden/lar_long.npz (tests/lar_mp.py at 50 digits; a stated subset of every case, lar_mp.pick),
which tests/test_lar_contract_cpu.py admits case by case: nothing is recomputed at 50 digits here.

Then lar_mp.SCAN, one engine per case: inside the envelope (lar_mp.ENVELOPE: |m_i|/sd_i ≤ 1e8, cond Λ ≤ 1e8, R/Szz ≥ 1e-6) held to the same
contract; outside it Λ is still SPD, so the engine has nothing to refuse: it must answer with every output finite, and its errors are printed."""
import os

import numpy as np
import pytest

import lar_mp as MP
import rxhip

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lar_long.npz")

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """after the module: the worst error per quantity with its case (-s shows it; DESIGN.md §3.5c quotes it)"""
    yield
    for q, (v, what) in sorted(_worst.items()):
        print(f"\nworst {q}: {v:.3e} at {what}")


def _note(errs, what, tag=""):
    for q, v in errs.items():
        if v > _worst.get(q + tag, (-1.0, None))[0]:
            _worst[q + tag] = (v, what)


@pytest.fixture(scope="module")
def golden():
    return MP.load(FIXTURE)


def _case(spec, golden):
    """the inputs of a case, checked against the CRC the fixture was computed on"""
    y, m, iters, share = MP.case(spec)
    assert MP.checksum(y, m) == golden[spec.name][1], spec.name
    return y, m, iters, share


def _run(y, m, iters, share, layout="time_chain"):
    with rxhip.LAREngine(y.shape[0], m["order"], m["tau"], m["prior_theta"], m["prior_gamma"], m["prior_x0"], m["init_theta"], m["init_gamma"],
                         n_series=y.shape[1], share_parameters=share) as eng:
        eng.set_data(y if layout == "time_chain" else np.ascontiguousarray(y.T), layout=layout)
        eng.run(iters, True)                                        # (a status other than OK raises)
        xm, xc = eng.states(layout)
        if layout == "chain_time":
            xm, xc = np.ascontiguousarray(np.swapaxes(xm, 0, 1)), np.ascontiguousarray(np.swapaxes(xc, 0, 1))
        tm, tc, ga, gb = eng.parameters()
        return dict(x_mean=xm, x_cov=xc, theta_mean=tm, theta_cov=tc, gamma_shape=ga, gamma_rate=gb, fe=eng.free_energy(), fe_series=eng.free_energy_per_chain())


def _shapes(got, spec):
    T, C, p, it, G = spec.T, spec.C, spec.p, spec.iterations, 1 if spec.share else spec.C
    want = dict(x_mean=(T, C, p), x_cov=(T, C, p, p), theta_mean=(it, G, p), theta_cov=(it, G, p, p), gamma_shape=(it, G), gamma_rate=(it, G), fe=(it,), fe_series=(C,))
    assert {k: v.shape for k, v in got.items()} == want
    assert all(np.all(np.isfinite(v)) for v in got.values()), spec.name


def _non_increasing(fe):
    return bool(np.all(np.diff(fe) <= 1e-9 * np.abs(fe[1:])))


def test_the_grid_is_the_grid():
    assert len(MP.GRID) == 49 and len(MP.SCAN) == 47 and sum(s.share for s in MP.GRID) == 2
    assert max((s.T + s.p) * s.C * s.p * s.iterations for s in MP.GRID) == (4096 + 8) * 3 * 8 * 2          # the largest engine


@pytest.mark.parametrize("spec", MP.GRID, ids=lambda s: s.name)
def test_grid(spec, golden):
    y, m, iters, share = _case(spec, golden)
    for layout in ("time_chain", "chain_time") if share else ("time_chain",):
        got = _run(y, m, iters, share, layout)
        _shapes(got, spec)
        errs = MP.errors(spec, MP.pick(spec, got), golden[spec.name][0])
        print(spec.name, layout, "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        _note(errs, spec.name)
        assert all(v <= MP.CONTRACT[k] for k, v in errs.items()), (spec.name, layout, errs)
        assert _non_increasing(got["fe"]), (spec.name, got["fe"])


def test_scan(golden):
    """inside the envelope: the contract; outside: answered, finite, printed"""
    misses, inside_n = [], 0
    for spec in MP.SCAN:
        y, m, iters, share = _case(spec, golden)
        got = _run(y, m, iters, share)
        _shapes(got, spec)
        flat, _, gauges = golden[spec.name]
        errs = MP.errors(spec, MP.pick(spec, got), flat)
        inside = MP.in_envelope(gauges)
        inside_n += inside
        print(f"{spec.name}: |m|/sd {gauges[0]:.2e}, R/Szz {gauges[1]:.1e}, cond Λ {gauges[2]:.1f}, {'inside ' if inside else 'OUTSIDE'} | "
              + "  ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        _note(errs, spec.name, " (scan, inside)" if inside else " (scan, outside: not asserted)")
        if inside:
            misses += [(spec.name, k, v) for k, v in errs.items() if not v <= MP.CONTRACT[k]]
            if not _non_increasing(got["fe"]):
                misses.append((spec.name, "F rises", got["fe"]))
    assert not misses, misses
    assert inside_n >= 25

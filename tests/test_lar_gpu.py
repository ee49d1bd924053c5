"""The latent autoregressive engine (include/rxhip.h rxhip_lar_desc, csrc/lar_kernels.hpp) against its dense CPU restatement tests/lar_ref.py:
q(x[t]) of the last iteration, q(θ) and q(γ) of every iteration, and the free energy per iteration and per series — at the project's contract
(lar_ref.hold: state means 1e-6 posterior standard deviations; (co)variances, θ and γ 1e-6 relative; free energy 1e-8 relative).  Every random
case keeps cond Λ ≤ 1e8 (asserted in tests/test_lar_ref_cpu.py), so the contract has two decades over cond·ε; the host build of the same
arithmetic sits near 1e-14 (tests/test_lar_host.py)."""
import ctypes

import numpy as np
import pytest

import lar_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu

KEYS = ("x_mean", "x_cov", "theta_mean", "theta_cov", "gamma_shape", "gamma_rate")


def _engine(y, m, **kw):
    return rxhip.LAREngine(y.shape[0], m["order"], m["tau"], m["prior_theta"], m["prior_gamma"], m["prior_x0"], m["init_theta"], m["init_gamma"],
                           n_series=y.shape[1], **kw)


def _read(eng, fe, layout="time_chain"):
    xm, xc = eng.states(layout)
    if layout == "chain_time":
        xm, xc = np.ascontiguousarray(np.swapaxes(xm, 0, 1)), np.ascontiguousarray(np.swapaxes(xc, 0, 1))
    tm, tc, ga, gb = eng.parameters()
    return dict(x_mean=xm, x_cov=xc, theta_mean=tm, theta_cov=tc, gamma_shape=ga, gamma_rate=gb, fe=eng.free_energy() if fe else None,
                parts=eng.free_energy_per_chain() if fe else None)


def _run(y, m, iters, fe=True, layout="time_chain", **kw):
    with _engine(y, m, **kw) as eng:
        eng.set_data(y if layout == "time_chain" else np.ascontiguousarray(y.T), layout=layout)
        eng.run(iters, fe)
        return _read(eng, fe, layout)


def _non_increasing(fe):
    return bool(np.all(np.diff(fe) <= 1e-9 * np.abs(fe[1:])))


def _check(spec, layout="time_chain"):
    y, m, iters, shared = R.case(spec)
    ref = R.run_batch(y, **m, iterations=iters, share_parameters=shared)
    got = _run(y, m, iters, layout=layout, share_parameters=shared)
    R.hold(got, ref)
    ep = float(np.max(np.abs(got["parts"] - ref["fe_series"][-1]) / np.maximum(1.0, np.abs(ref["fe_series"][-1]))))
    assert ep < 1e-8, ep
    assert _non_increasing(got["fe"]), got["fe"]
    return got, ref


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- 1. the reference case through infer ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_runs():
    y, _ = R.reference_data()
    return y, {p: R.run(y, 15, **R.model(p, 5.0)) for p in (1, 5)}


@pytest.mark.parametrize("p", [1, 5])
def test_reference_case_through_infer(reference_runs, p):
    y, refs = reference_runs
    res = rxhip.infer(model=rxhip.latent_autoregressive(p, 5.0), data={"y": y}, iterations=15, free_energy=True)
    assert res.error is None
    xm, xc = res.posteriors["x"]
    tm, tc = res.posteriors["theta"]
    ga, gb = res.posteriors["gamma"]
    assert xm.shape == (500, p) and xc.shape == (500, p, p) and tm.shape == (15, p) and tc.shape == (15, p, p) and ga.shape == (15,) and gb.shape == (15,)
    fe = res.free_energy
    R.hold(dict(x_mean=xm, x_cov=xc, theta_mean=tm, theta_cov=tc, gamma_shape=ga, gamma_rate=gb, fe=fe), refs[p])
    print("free energy:", repr(float(fe[0])), repr(float(fe[-1])))
    assert fe.shape == (15,) and abs(fe[-1] - R.GOLDEN_FE[p]) < 0.01                # lar_tests.jl:171, :202
    for it, want in zip((0, 14), R.RECORDED_FE[p]):
        assert abs(fe[it] - want) < 1e-8 * want
    assert np.all(np.diff(fe) < 0)


# ---- 2. every order; the boundary rows of the band --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", R.CASES["orders"], ids=lambda s: f"p{s[3]}")
def test_every_order(spec):
    _check(spec)


@pytest.mark.parametrize("spec", R.CASES["short"], ids=lambda s: f"T{s[1]}-p{s[3]}")
def test_short_series_cover_the_boundary_rows(spec):
    _check(spec)


# ---- 3. a ragged wavefront and a second block, both layouts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["time_chain", "chain_time"])
@pytest.mark.parametrize("spec", R.CASES["batches"], ids=lambda s: f"C{s[2]}")
def test_batches(spec, layout):
    _check(spec, layout)


# ---- 4. missing observations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", R.CASES["missing"], ids=lambda s: f"missing-{s[4]}")
def test_missing_observations(spec):
    _check(spec)


# ---- 5. shared parameters ---------------------------------------------------------------------------------------------------------------------------
def test_shared_parameters():
    got, ref = _check(R.CASES["shared"][0])
    assert got["theta_mean"].shape == (3, 1, 3) and got["gamma_shape"].shape == (3, 1)
    kl = R.kl_theta(got["theta_mean"][-1, 0], got["theta_cov"][-1, 0], R.case(R.CASES["shared"][0])[1]["prior_theta"]) + \
        R.kl_gamma(got["gamma_shape"][-1, 0], got["gamma_rate"][-1, 0], R.case(R.CASES["shared"][0])[1]["prior_gamma"])
    assert abs(got["fe"][-1] - (got["parts"].sum() + kl)) < 1e-8 * abs(got["fe"][-1])   # the KL terms enter the total once


def test_shared_and_unshared_agree_bit_for_bit_with_one_series():
    y, m, iters, _ = R.case(R.CASES["shared"][1])
    u, s = _run(y, m, iters), _run(y, m, iters, share_parameters=True)
    assert _same(u, s) and np.array_equal(u["fe"], s["fe"])


# ---- 6. bit for bit ---------------------------------------------------------------------------------------------------------------------------------
def test_series_does_not_depend_on_its_batch():
    y, m, iters, _ = R.case(R.CASES["nine"][0])
    full = _run(y, m, iters)
    for s in range(9):
        one = _run(y[:, s:s + 1], m, iters)
        assert np.array_equal(one["x_mean"][:, 0], full["x_mean"][:, s]) and np.array_equal(one["x_cov"][:, 0], full["x_cov"][:, s])
        for k in KEYS[2:]:
            assert np.array_equal(one[k][:, 0], full[k][:, s])
        assert one["fe"][-1] == full["parts"][s]


def test_runs_repeat_and_do_not_depend_on_the_free_energy():
    y, m, iters, _ = R.case(R.CASES["nine"][0])
    ref = R.run_batch(y, **m, iterations=iters)
    with _engine(y, m) as eng:
        eng.set_data(y)
        eng.run(iters, True)
        first = _read(eng, True)
        eng.run(iters, False)
        without = _read(eng, False)
        with pytest.raises(rxhip.RxHipError):
            eng.free_energy()
        eng.run(1, True)                  # every run starts from the initial q: one iteration after three is the first iterate
        one = _read(eng, True)
        eng.run(iters, True)
        again = _read(eng, True)
    R.hold(first, ref)
    assert _same(first, without)
    assert _same(first, again) and np.array_equal(first["fe"], again["fe"]) and np.array_equal(first["parts"], again["parts"])
    assert one["theta_mean"].shape[0] == 1 and np.array_equal(one["theta_mean"][0], first["theta_mean"][0]) and one["fe"][0] == first["fe"][0]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------
def _refused(**change):
    kw = dict(T=5, order=2, tau=5.0, n_series=2)
    kw.update(change)
    with pytest.raises(rxhip.RxHipError) as ei:
        rxhip.LAREngine(**kw)
    assert ei.value.status == _lib.ERR_BADARG and len(str(ei.value)) > 10, str(ei.value)
    return str(ei.value)


def test_bad_descriptors_are_refused_with_a_text():
    assert "order" in _refused(order=0)
    assert "order" in _refused(order=9)
    assert "T" in _refused(T=0)
    for v in (0.0, -1.0, np.inf, np.nan):
        assert "tau" in _refused(tau=v)
        assert "prior_gamma" in _refused(prior_gamma=(v, 1.0))
        assert "prior_gamma" in _refused(prior_gamma=(1.0, v))
        assert "init_gamma" in _refused(init_gamma=(v, 1.0))
        assert "init_gamma" in _refused(init_gamma=(1.0, v))
    indefinite, skew, nan = np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[1.0, 0.1], [0.2, 1.0]]), np.array([[1.0, np.nan], [np.nan, 1.0]])
    for bad in (indefinite, skew, nan, np.zeros((2, 2))):
        assert "prior_theta_precision" in _refused(prior_theta=(np.zeros(2), bad))
        assert "prior_x0_precision" in _refused(prior_x0=(np.zeros(2), bad))
        assert "init_theta_cov" in _refused(init_theta=(np.zeros(2), bad))
    h = ctypes.c_void_p()
    assert rxhip.lib().rxhip_lar_create(None, ctypes.byref(h)) == _lib.ERR_BADARG and not h.value


def test_bad_observations_are_refused_and_the_engine_stays_usable():
    y, m, iters, _ = R.case(R.CASES["missing"][2])
    ref = R.run_batch(y, **m, iterations=iters)
    for layout in ("time_chain", "chain_time"):
        with _engine(y, m) as eng:
            for v in (np.inf, -np.inf):
                bad = y.copy()
                bad[5, 1] = v
                with pytest.raises(rxhip.RxHipError) as ei:
                    eng.set_data(bad if layout == "time_chain" else np.ascontiguousarray(bad.T), layout=layout)
                assert ei.value.status == _lib.ERR_BADARG and "infinite" in str(ei.value)
                with pytest.raises(rxhip.RxHipError) as ei:      # refused data is not run on
                    eng.run(1, True)
                assert ei.value.status == _lib.ERR_STATE
            eng.set_data(y if layout == "time_chain" else np.ascontiguousarray(y.T), layout=layout)
            eng.run(iters, True)
            R.hold(_read(eng, True, layout), ref)


def test_call_order_is_checked():
    y, m, _, _ = R.case(R.CASES["short"][1])
    with _engine(y, m) as eng:
        for call in (lambda: eng.run(1, True), eng.states, eng.parameters):
            with pytest.raises(rxhip.RxHipError) as ei:
                call()
            assert ei.value.status == _lib.ERR_STATE
        with pytest.raises(rxhip.RxHipError):
            eng.set_data(np.zeros((5, 2)))       # wrong length

"""The hidden Markov model engine (include/rxhip.h rxhip_hmm_desc, csrc/hmm_kernels.hpp) against its CPU restatement tests/hmm_ref.py: q(s_t), the
counts of q(A) and q(B), and the free energy per iteration and per series.  Tolerances: free energy 1e-8 relative (the project's contract),
probabilities 1e-9 absolute, counts 1e-9 relative — the iteration does not amplify rounding on such inputs (a 1e-13 relative perturbation of the
initial counts moves every output by at most 2e-13 on the CPU), device exp / log / digamma differ from numpy's by a few ulp."""
import ctypes

import numpy as np
import pytest

import hmm_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu


def _hold(gamma, a, b, ref_gamma, ref_a, ref_b):
    assert np.all(np.isfinite(gamma)) and np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    eg = float(np.max(np.abs(gamma - ref_gamma)))
    ea, eb = float(np.max(np.abs(a - ref_a) / ref_a)), float(np.max(np.abs(b - ref_b) / ref_b))
    print(f"gamma abs {eg:.3e}, A counts rel {ea:.3e}, B counts rel {eb:.3e}")
    assert eg < 1e-9 and ea < 1e-9 and eb < 1e-9, (eg, ea, eb)


def _hold_fe(fe, ref):
    ef = float(np.max(np.abs(fe - ref) / np.abs(ref)))
    print(f"fe rel {ef:.3e}")
    assert np.all(np.isfinite(fe)) and ef < 1e-8, ef


def _engine(x, m, **kw):
    return rxhip.HMMEngine(x.shape[0], m["prior_A"], m["prior_B"], m["prior_s0"], m.get("init_A"), m.get("init_B"), n_series=x.shape[1], **kw)


def _run(x, m, iters, fe=True, layout="time_chain", **kw):
    """(γ [T+1][series][K], A counts, B counts, fe [iters] | None, per-series fe of the last iteration | None)"""
    with _engine(x, m, **kw) as eng:
        eng.set_data(x if layout == "time_chain" else np.ascontiguousarray(x.T), layout=layout)
        eng.run(iters, fe)
        g = eng.states(layout)
        a, b = eng.parameters()
        return (g if layout == "time_chain" else np.ascontiguousarray(g.transpose(1, 0, 2))), a, b, (eng.free_energy() if fe else None), \
            (eng.free_energy_per_chain() if fe else None)


def _check_every_iteration(x, m, iters, layout="time_chain", refs=None, **kw):
    """The ABI returns posteriors and per-series free energies of the LAST iteration: one run per iteration count gives every (iteration, series) —
    and shows that n iterations in one run give the n-th iterate."""
    share = kw.get("share_parameters", False)
    for n in range(1, iters + 1):
        rg, ra, rb, rfe, rparts = refs[n - 1] if refs else R.run_batch(x, **m, iterations=n, share_parameters=share)
        g, a, b, fe, parts = _run(x, m, n, layout=layout, **kw)
        _hold(g, a, b, rg, ra, rb)
        _hold_fe(fe, rfe)
        _hold_fe(parts, rparts[-1])


# ---- 1. the reference case -------------------------------------------------------------------------------------------------------------------------
def test_reference_case():
    x, _ = R.reference_data()
    m = R.REFERENCE_MODEL
    rg, ra, rb, rfe = R.run(x, **m, iterations=20)
    with rxhip.HMMEngine(100, m["prior_A"], m["prior_B"], m["prior_s0"]) as eng:
        eng.set_data(x[:, None])
        eng.run(20, True)
        g, (a, b), fe, parts, counters = eng.states(), eng.parameters(), eng.free_energy(), eng.free_energy_per_chain(), eng.counters()
    assert g.shape == (101, 1, 3) and a.shape == (1, 3, 3) and b.shape == (1, 3, 3) and fe.shape == (20,)
    _hold(g[:, 0], a[0], b[0], rg, ra, rb)
    _hold_fe(fe, rfe)
    print("free energy:", [repr(float(v)) for v in fe[[0, 1, -1]]])
    assert parts[0] == fe[-1]
    assert abs(fe[-1] - R.GOLDEN_FE) < 0.01                                   # hmm_tests.jl:95
    for it, want in R.RECORDED_FE.items():
        assert abs(fe[it - 1] - want) < 1e-8 * want
    assert np.all(np.diff(fe) <= 1e-9 * np.abs(fe[1:]))
    assert all(counters[k] > 0 for k in ("rule_calls", "products", "marginals"))


# ---- 2. 130 series × T = 37, K = 5, M = 7: partial rows, more than one wavefront and a ragged last one ------------------------------------------------
@pytest.fixture(scope="module")
def batch_case():
    T, C, K, M = 37, 130, 5, 7
    x, m = R.random_case(20, T, C, K, M, missing=0.05)
    x[:, 1] = np.nan                  # nothing observed
    x[:, 2] = 3.0                     # a single symbol throughout
    x[0, 3] = x[-1, 3] = np.nan       # first and last step missing
    return x, m, [R.run_batch(x, **m, iterations=n) for n in range(1, 7)]     # the n-th iterate for every n, computed once


@pytest.mark.parametrize("layout", ["time_chain", "chain_time"])
def test_batch_partial_rows_ragged_wavefront(batch_case, layout):
    x, m, refs = batch_case
    _check_every_iteration(x, m, 6, layout=layout, refs=refs)


# ---- 3., 4. full rows with the largest LDS table; 32 series per wavefront ----------------------------------------------------------------------------
@pytest.mark.parametrize("T,C,K,M,iters", [(64, 9, 16, 64, 3), (9, 70, 2, 2, 4), (11, 19, 8, 5, 3), (11, 10, 9, 3, 3), (11, 21, 3, 64, 3), (11, 17, 4, 4, 3)])
def test_row_widths(T, C, K, M, iters):
    x, m = R.random_case(1000 * K + M, T, C, K, M, missing=0.05)
    _check_every_iteration(x, m, iters)


# ---- 5. the shortest series ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2])
def test_shortest_series(T):
    x, m = R.random_case(30 + T, T, 5, 3, 4, missing=0.0)
    x[0, 1] = np.nan
    _check_every_iteration(x, m, 3)


# ---- 6. shared parameters -----------------------------------------------------------------------------------------------------------------------------
def test_shared_parameters():
    x, m = R.random_case(40, 20, 33, 3, 4, missing=0.05, per_series=False)
    _check_every_iteration(x, m, 4, share_parameters=True)
    with _engine(x, m, share_parameters=True) as eng:
        eng.set_data(x)
        eng.run(4, True)
        total, parts = eng.free_energy()[-1], eng.free_energy_per_chain()
        a, b = eng.parameters()
    assert a.shape == (1, 3, 3) and b.shape == (1, 4, 3)
    kl = R.dirichlet_kl(a[0], m["prior_A"]) + R.dirichlet_kl(b[0], m["prior_B"])
    assert abs(total - (parts.sum() + kl)) < 1e-8 * abs(total)     # the KL terms enter the total once


def test_shared_and_unshared_agree_bit_for_bit_with_one_series():
    x, m = R.random_case(41, 20, 1, 3, 4, missing=0.05, per_series=False)
    u, s = _run(x, m, 5), _run(x, m, 5, share_parameters=True)
    for got, want in zip(s[:3], u[:3]):
        assert np.array_equal(got, want)
    assert np.array_equal(s[3], u[3])


# ---- 7. independence of the batch ---------------------------------------------------------------------------------------------------------------------
def test_series_does_not_depend_on_its_batch(batch_case):
    x, m, _ = batch_case
    g, a, b, _, parts = _run(x, m, 6)
    for s in (0, 129):
        one = {k: (v[s:s + 1] if v.ndim == 3 else v) for k, v in m.items()}
        g1, a1, b1, fe1, _ = _run(x[:, s:s + 1], one, 6)
        assert np.array_equal(g1[:, 0], g[:, s]) and np.array_equal(a1[0], a[s]) and np.array_equal(b1[0], b[s])
        assert fe1[-1] == parts[s]


# ---- 8. repeatable runs -------------------------------------------------------------------------------------------------------------------------------
def test_runs_repeat_and_do_not_depend_on_the_free_energy(batch_case):
    x, m, refs = batch_case
    rg, ra, rb, rfe, _ = refs[5]
    with _engine(x, m) as eng:
        eng.set_data(x)
        eng.run(6, True)
        first = (eng.states(), *eng.parameters(), eng.free_energy())
        eng.run(6, False)
        without = (eng.states(), *eng.parameters())
        with pytest.raises(rxhip.RxHipError):
            eng.free_energy()
        eng.run(3, True)              # every run starts from the initial q: 3 iterations after 6 are the third iterate
        third = (eng.states(), *eng.parameters())
        eng.run(6, True)
        again = (eng.states(), *eng.parameters(), eng.free_energy())
    _hold(*first[:3], rg, ra, rb)
    _hold_fe(first[3], rfe)
    for u, v in zip(first[:3], without):
        assert np.array_equal(u, v)
    for u, v in zip(first, again):
        assert np.array_equal(u, v)
    _hold(*third, *refs[2][:3])


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def _refused(**change):
    kw = dict(T=5, prior_A=np.ones((3, 3)), prior_B=np.ones((4, 3)), prior_s0=np.full(3, 1.0 / 3.0), init_A=None, init_B=None, n_series=2, share_parameters=False)
    kw.update(change)
    with pytest.raises(rxhip.RxHipError) as ei:
        rxhip.HMMEngine(**kw)
    assert ei.value.status == _lib.ERR_BADARG and len(str(ei.value)) > 10, str(ei.value)
    return str(ei.value)


def test_bad_descriptors_are_refused_with_a_text():
    bad = np.ones((3, 3))
    assert "K" in _refused(prior_A=np.ones((17, 17)), prior_B=np.ones((4, 17)), prior_s0=np.full(17, 1.0 / 17))
    assert "K" in _refused(prior_A=np.ones((1, 1)), prior_B=np.ones((4, 1)), prior_s0=np.ones(1))
    assert "M" in _refused(prior_B=np.ones((65, 3)))
    assert "M" in _refused(prior_B=np.ones((1, 3)))
    assert "T" in _refused(T=0)
    for v in (0.0, -1.0, np.inf, np.nan):
        bad = np.ones((3, 3)); bad[1, 2] = v
        assert "prior_A" in _refused(prior_A=bad)
        assert "init_A" in _refused(init_A=bad)
        badb = np.ones((4, 3)); badb[3, 0] = v
        assert "prior_B" in _refused(prior_B=badb)
        assert "init_B" in _refused(init_B=badb)
    assert "prior_s0" in _refused(prior_s0=np.array([0.5, 0.5, 0.0]))
    assert "prior_s0" in _refused(prior_s0=np.array([0.5, 0.3, 0.3]))
    assert "prior_s0" in _refused(prior_s0=np.array([0.5, 0.25, 0.25 + 1e-9]))
    assert "prior_s0" in _refused(prior_s0=np.array([1.5, -0.25, -0.25]))
    assert "per series" in _refused(prior_A=np.ones((2, 3, 3)), prior_B=np.ones((2, 4, 3)), share_parameters=True)
    h = ctypes.c_void_p()
    assert rxhip.lib().rxhip_hmm_create(None, ctypes.byref(h)) == _lib.ERR_BADARG and not h.value


def test_bad_observations_are_refused_and_the_engine_stays_usable():
    x, m = R.random_case(50, 8, 3, 3, 4, missing=0.1)
    ref = R.run_batch(x, **m, iterations=2)
    for layout in ("time_chain", "chain_time"):
        with _engine(x, m) as eng:
            for v in (0.5, -1.0, 4.0, np.inf, -np.inf, 1e300):
                bad = x.copy()
                bad[5, 2] = v
                with pytest.raises(rxhip.RxHipError) as ei:
                    eng.set_data(bad if layout == "time_chain" else np.ascontiguousarray(bad.T), layout=layout)
                assert ei.value.status == _lib.ERR_BADARG and "symbol" in str(ei.value)
                with pytest.raises(rxhip.RxHipError) as ei:      # refused data is not run on
                    eng.run(1, True)
                assert ei.value.status == _lib.ERR_STATE
            eng.set_data(x if layout == "time_chain" else np.ascontiguousarray(x.T), layout=layout)
            eng.run(2, True)
            g = eng.states(layout)
            _hold(g if layout == "time_chain" else g.transpose(1, 0, 2), *eng.parameters(), *ref[:3])
            _hold_fe(eng.free_energy(), ref[3])


def test_call_order_is_checked():
    x, m = R.random_case(51, 4, 1, 2, 2)
    with _engine(x, m) as eng:
        for call in (lambda: eng.run(1, True), eng.states, eng.parameters):
            with pytest.raises(rxhip.RxHipError) as ei:
                call()
            assert ei.value.status == _lib.ERR_STATE
        with pytest.raises(rxhip.RxHipError):
            eng.set_data(np.zeros((5, 1)))       # wrong length


# ---- 10. infer end to end -----------------------------------------------------------------------------------------------------------------------------
def test_infer_on_the_reference_data():
    x, _ = R.reference_data()
    one_hot = np.eye(3)[x.astype(int)]                                   # the reference's own data format
    codes = rxhip.one_hot_to_codes(one_hot)
    assert np.array_equal(codes, x)
    res = rxhip.infer(model=rxhip.hidden_markov_model(**R.REFERENCE_MODEL), data={"x": codes.astype(np.int64)}, iterations=20, free_energy=True)
    rg, ra, rb, rfe = R.run(x, **R.REFERENCE_MODEL, iterations=20)
    assert res.posteriors["s"].shape == (101, 3) and res.posteriors["A"].shape == (3, 3) and res.posteriors["B"].shape == (3, 3)
    _hold(res.posteriors["s"], res.posteriors["A"], res.posteriors["B"], rg, ra, rb)
    _hold_fe(res.free_energy, rfe)
    assert res.free_energy.shape == (20,) and abs(res.free_energy[-1] - R.GOLDEN_FE) < 0.01
    # a batch with shared parameters through the same door
    xb, m = R.random_case(60, 12, 4, 3, 3, per_series=False)
    res = rxhip.infer(model=rxhip.hidden_markov_model(**m, share_parameters=True), data={"x": xb}, iterations=3, free_energy=True)
    rb_ = R.run_batch(xb, **m, iterations=3, share_parameters=True)
    assert res.posteriors["s"].shape == (13, 4, 3) and res.posteriors["A"].shape == (3, 3)
    _hold(res.posteriors["s"], res.posteriors["A"], res.posteriors["B"], rb_[0], rb_[1][0], rb_[2][0])
    _hold_fe(res.free_energy, rb_[3])

"""The Gamma mixture engine (include/rxhip.h rxhip_gammamix_desc, csrc/gammamix_kernels.hpp) against its CPU restatement tests/gammamix_ref.py, per iteration
and per problem, at the contract (gammamix_ref.hold): â, e, f, α within 1e-6 relative, responsibilities within 1e-6 absolute, F within 1e-8 relative to
max(1, |F|).  Every case meets the conditions asserted in tests/test_gammamix_ref_cpu.py (S0_k ≥ 1 at every iteration; a permutation of y moves the
history by less than 1e-10).
Shapes: the streamed pass at N = 1, 63, 64, 65, a tile of 256 points − 1, a tile, a tile + 1, and 20 001 (79 chunks with a ragged tail), K = 1, 2, 3, 4, 5, 8,
16 (every padded width and the unpadded ones between); further small sizes N = 1, 64, 65, 250 (the reference's) and 3584 (14 full tiles).
The engine has ONE schedule, streamed: a resident kernel was taken out whole after it faulted on the device for a cause not found."""
import ctypes

import numpy as np
import pytest

import gammamix_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu
SCHED = {R.STREAMED: "streamed"}


def _collect(eng, iters, fe=True):
    eng.run(iters, fe)
    h = eng.history()
    out = dict(a=h["a"], e=h["b_shape"], f=h["b_rate"], alpha=h["alpha"])
    if fe:
        out["fe"], out["fe_total"], out["last"] = h["fe"], eng.free_energy(), eng.free_energy_per_chain()
    if eng.materialize:
        out["resp"] = eng.responsibilities()
    return out


def _run(Y, priors, inits, iters, schedule, fe=True, materialize=True):
    """Y [problems][N]; priors [5][problems][K]; inits [4][problems][K]"""
    C, N = Y.shape
    K = priors[0].shape[-1]
    with rxhip.GammaMixtureEngine(N, K, (priors[0], priors[1]), (priors[2], priors[3]), priors[4], init_a=inits[0], init_b=(inits[1], inits[2]), init_s=inits[3],
                                  n_problems=C, schedule=schedule, materialize=materialize) as eng:
        eng.set_data(Y, layout="chain_time")
        return _collect(eng, iters, fe)


def _single(y, prior, init, iters, schedule, **kw):
    return _run(y[None], [np.asarray(p)[None] for p in prior], [np.asarray(q)[None] for q in init], iters, schedule, **kw)


def _hold(got, ref):
    """the contract per iteration and problem; then rxhip_get_free_energy (summed over the problems) and rxhip_get_free_energy_per_chain (last iteration)"""
    worst = R.hold(got, ref)
    tot = ref["fe"].sum(axis=1)
    worst["fe_total"] = float(np.max(np.abs(got["fe_total"] - tot) / np.maximum(1.0, np.abs(tot))))
    assert worst["fe_total"] < R.TOL_FE, worst
    assert np.array_equal(got["last"], got["fe"][-1])
    if got["fe"].shape[1] == 1:
        assert np.array_equal(got["fe_total"], got["fe"][:, 0])
    return worst


def _ref_single(y, prior, init, iters):
    return R.run_batch(y[None], [np.asarray(p)[None] for p in prior], [np.asarray(q)[None] for q in init], iters)


def _same(a, b, keys=("a", "e", "f", "alpha")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- 1. the two schedules over their sizes ------------------------------------------------------------------------------------------------------------------
def test_schedule_constants():
    S = rxhip.GammaMixtureEngine.schedule
    assert S(1, 1) == S(250, 2) == S(3584, 16) == S(10 ** 7, 16) == R.STREAMED
    assert {N for _, N, _, _ in R.STREAMED_CASES} >= {1, 63, 64, 65, R.TILE - 1, R.TILE, R.TILE + 1, 20001}
    assert {K for _, _, K, _ in R.STREAMED_CASES} >= {1, 2, 3, 4, 5, 8, 16}
    assert {N for _, N, _, _ in R.SMALL_CASES} >= {1, 64, 65, 250, 3584}


@pytest.mark.parametrize("case", R.STREAMED_CASES, ids=lambda c: "N%d-K%d" % (c[1], c[2]))
def test_streamed_edges(case):
    seed, N, K, iters = case
    y, prior, init = R.make_problem(seed, N, K)
    ref = _ref_single(y, prior, init, iters)
    got = _single(y, prior, init, iters, "streamed")
    print("streamed", case, _hold(got, ref))
    assert R.does_not_rise(got["fe_total"], N, K)


@pytest.mark.parametrize("case", R.SMALL_CASES, ids=lambda c: "N%d-K%d" % (c[1], c[2]))
def test_small_sizes_and_the_automatic_schedule(case):
    seed, N, K, iters = case
    y, prior, init = R.make_problem(seed, N, K)
    ref = _ref_single(y, prior, init, iters)
    stm = _single(y, prior, init, iters, "streamed")
    print("small", case, _hold(stm, ref))
    auto = _single(y, prior, init, iters, "auto")
    assert _same(stm, auto, ("a", "e", "f", "alpha", "fe", "resp"))         # auto IS the streamed schedule
    assert R.does_not_rise(stm["fe_total"], N, K)


def test_the_resident_schedule_is_refused():
    for N, K in ((250, 2), (3584, 8), (250, 16)):
        with pytest.raises(rxhip.RxHipError) as ei:
            rxhip.GammaMixtureEngine(N, K, (np.ones(K), np.ones(K)), (np.ones(K), np.ones(K)), np.ones(K), schedule="resident")
        assert ei.value.status == _lib.ERR_BADARG and "gammamix" in str(ei.value) and "resident" in str(ei.value)


# ---- 2. batches: different data and priors per problem; the bit-equality statements --------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.BATCH_CASES, ids=lambda c: "C%d-N%d-K%d-%s" % (c[1], c[2], c[3], SCHED[c[5]]))
def test_batches(case):
    seed, C, N, K, iters, sched = case
    Y, priors, inits = R.make_batch(seed, C, N, K)
    ref = R.run_batch(Y, priors, inits, iters)
    got = _run(Y, priors, inits, iters, SCHED[sched])
    print("batch", case, _hold(got, ref))
    again = _run(Y, priors, inits, iters, SCHED[sched])
    assert _same(got, again, ("a", "e", "f", "alpha", "fe", "fe_total", "last", "resp"))                      # two runs
    nofe = _run(Y, priors, inits, iters, SCHED[sched], fe=False)
    assert _same(got, nofe, ("a", "e", "f", "alpha", "resp"))                                             # with and without F
    for c in sorted({0, C // 2, C - 1}):                                                                  # a problem alone ≡ member 0 / middle / last of the batch
        alone = _run(Y[c:c + 1], [p[c:c + 1] for p in priors], [q[c:c + 1] for q in inits], iters, SCHED[sched])
        for k in ("a", "e", "f", "alpha", "fe"):
            assert np.array_equal(alone[k][:, 0], got[k][:, c]), (c, k)
        assert np.array_equal(alone["resp"][0], got["resp"][c]) and alone["last"][0] == got["last"][c]


@pytest.mark.parametrize("sched", ["streamed"])
def test_a_long_run_repeats_a_short_one(sched):
    y, prior, init = R.make_problem(601, 300, 3)
    long, short = _single(y, prior, init, 40, sched), _single(y, prior, init, 2, sched)
    for k in ("a", "e", "f", "alpha", "fe"):
        assert np.array_equal(long[k][:2], short[k]), k
    _hold(long, _ref_single(y, prior, init, 40))
    assert R.does_not_rise(long["fe_total"], 300, 3)


# ---- 3. data: missing points, refusals, transport ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.NAN_CASES, ids=lambda c: "seed%d" % c[0])
@pytest.mark.parametrize("sched", ["streamed"])
def test_nan_points_are_the_same_data_with_those_points_removed(case, sched):
    seed, N, K, iters, idx = case
    y, prior, init = R.make_problem(seed, N, K)
    y[idx] = np.nan
    ref = _ref_single(y, prior, init, iters)
    got = _single(y, prior, init, iters, sched)
    print("nan", case, sched, _hold(got, ref))
    kept = np.delete(y, idx)
    cut = _single(kept, prior, init, iters, sched)
    refc = _ref_single(kept, prior, init, iters)
    _hold(cut, refc)
    R.hold(dict(got, resp=np.delete(got["resp"], idx, axis=1)), cut)
    assert np.all(got["resp"][0, idx] == 0.0)
    counted = got["alpha"][-1, 0].sum() - np.sum(prior[4])
    assert abs(counted - (N - len(idx))) < 1e-9 * N and abs(cut["alpha"][-1, 0].sum() - np.sum(prior[4]) - (N - len(idx))) < 1e-9 * N   # equal counted N


def _refused(fn, status, text):
    with pytest.raises(rxhip.RxHipError) as ei:
        fn()
    assert ei.value.status == status and text in str(ei.value), str(ei.value)


def test_refused_observations():
    y, prior, init = R.make_problem(602, 100, 2)
    with rxhip.GammaMixtureEngine(100, 2, (prior[0], prior[1]), (prior[2], prior[3]), prior[4]) as eng:
        _refused(lambda: eng.run(1), _lib.ERR_STATE, "no observations")
        for bad in (0.0, -1.0, np.inf, -np.inf):
            yb = y.copy()
            yb[37] = bad
            _refused(lambda: eng.set_data(yb), _lib.ERR_BADARG, "gammamix")
            _refused(lambda: eng.run(1), _lib.ERR_STATE, "no observations")            # a refused array counts as not set
        eng.set_data(y)
        eng.run(2)
        eng.set_data(y)                                                                # the status word is clean again
        eng.run(2)


def test_device_data_equals_host_data_bit_for_bit():
    hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    for C, sched in ((3, "streamed"), (1, "streamed"), (1, "auto")):
        Y, priors, inits = R.make_batch(603, C, 200, 3)
        Y[0, 5] = np.nan
        host = _run(Y, priors, inits, 5, sched)
        for layout in ("time_chain", "chain_time"):
            a = np.ascontiguousarray(Y.T if layout == "time_chain" else Y)
            p = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
            with rxhip.GammaMixtureEngine(200, 3, (priors[0], priors[1]), (priors[2], priors[3]), priors[4], init_a=inits[0], init_b=(inits[1], inits[2]),
                                          init_s=inits[3], n_problems=C, schedule=sched, materialize=True) as eng:
                eng.set_data_device(p.value, a.size, layout=layout)
                dev = _collect(eng, 5)
            assert hip.hipFree(p) == 0
            assert _same(host, dev, ("a", "e", "f", "alpha", "fe", "fe_total", "last", "resp")), (C, sched, layout)
    bad = np.ascontiguousarray(Y[0])
    bad[3] = -2.0
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), bad.nbytes) == 0 and hip.hipMemcpy(p, bad.ctypes.data, bad.nbytes, 1) == 0
    with rxhip.GammaMixtureEngine(200, 3, (priors[0][0], priors[1][0]), (priors[2][0], priors[3][0]), priors[4][0]) as eng:
        _refused(lambda: eng.set_data_device(p.value, bad.size), _lib.ERR_BADARG, "gammamix")
    assert hip.hipFree(p) == 0


def test_stored_logarithms_are_the_same_bits():
    """the streamed pass on ln y read from memory against ln y recomputed: one function, one result"""
    Y, priors, inits = R.make_batch(604, 2, 5000, 4)
    a = _run(Y, priors, inits, 3, "streamed")
    with rxhip.GammaMixtureEngine(5000, 4, (priors[0], priors[1]), (priors[2], priors[3]), priors[4], init_a=inits[0], init_b=(inits[1], inits[2]), init_s=inits[3],
                                  n_problems=2, schedule="streamed", materialize=True) as eng:
        eng.set_stored_log(False)
        eng.set_data(Y, layout="chain_time")
        b = _collect(eng, 3)
        eng.set_stored_log(True)                                                         # switched on with the data in place
        c = _collect(eng, 3)
    assert _same(a, b, ("a", "e", "f", "alpha", "fe", "resp")) and _same(a, c, ("a", "e", "f", "alpha", "fe", "resp"))


# ---- 4. the reference's configuration, and infer ------------------------------------------------------------------------------------------------------------
def test_reference_configuration():
    """gamma_mixture_tests.jl's priors, initialisation, 250 points and 50 iterations on the recorded numpy draw: F[0] and F[-1] against RECORDED (this
    engine's own figures; the reference reports −146.8 ± 0.2 on its own draw with its own optimiser — an open item, gammamix_ref.RECORDED), F non-increasing."""
    y, prior = R.golden()
    for sched in ("auto", "streamed"):
        with rxhip.GammaMixtureEngine(250, 2, (prior[0], prior[1]), (prior[2], prior[3]), prior[4], schedule=sched) as eng:
            eng.set_data(y)
            got = _collect(eng, 50)
        fe = got["fe_total"]
        print("reference configuration", sched, fe[0], fe[-1])
        assert abs(fe[0] - R.RECORDED["fe_first"]) < R.TOL_FE * abs(R.RECORDED["fe_first"]) and abs(fe[-1] - R.RECORDED["fe_last"]) < R.TOL_FE * abs(R.RECORDED["fe_last"])
        assert R.does_not_rise(fe, 250, 2)
        means = got["a"][-1, 0] / (got["e"][-1, 0] / got["f"][-1, 0])
        assert np.allclose(means, R.RECORDED["means"], rtol=1e-6) and np.allclose(got["alpha"][-1, 0] / got["alpha"][-1, 0].sum(), R.RECORDED["mixing"], rtol=1e-6)


def test_infer_end_to_end():
    y, prior = R.golden()
    model = rxhip.gamma_mixture([rxhip.GammaShapeScale(1.0, 0.1), rxhip.GammaShapeScale(1.0, 1.0)], [rxhip.GammaShapeScale(10.0, 2.0), rxhip.GammaShapeScale(1.0, 3.0)],
                                rxhip.Dirichlet(prior[4]), init_b=[(1.0, 1.0), (1.0, 1.0)])
    res = rxhip.infer(model=model, data={"y": y}, iterations=50, free_energy=True)
    assert set(res.posteriors) == {"as", "bs", "s", "z"} and res.posteriors["as"].shape == (50, 2) and res.posteriors["bs"][0].shape == (50, 2)
    assert res.posteriors["s"].shape == (2,) and res.posteriors["z"].shape == (250, 2) and res.free_energy.shape == (50,)
    ref = R.run(y, prior, None, 50)
    assert np.allclose(res.posteriors["as"], ref["a"], rtol=1e-6) and abs(res.free_energy[-1] - ref["fe"][-1]) < 1e-8 * abs(ref["fe"][-1])
    assert np.allclose(res.posteriors["z"].sum(axis=1), 1.0)
    Y, priors, inits = R.make_batch(605, 4, 120, 3)
    model = rxhip.gamma_mixture(np.stack([priors[0], priors[1]], axis=-1), np.stack([priors[2], priors[3]], axis=-1), priors[4], init_a=inits[0],
                                init_b=np.stack([inits[1], inits[2]], axis=-1), init_s=inits[3])
    res = rxhip.infer(model=model, data={"y": Y}, iterations=6, free_energy=True)
    refb = R.run_batch(Y, priors, inits, 6)
    assert res.posteriors["as"].shape == (6, 4, 3) and res.posteriors["z"].shape == (4, 120, 3) and res.posteriors["s"].shape == (4, 3)
    assert np.allclose(res.posteriors["as"], refb["a"], rtol=1e-6) and np.allclose(res.posteriors["bs"][1], refb["f"], rtol=1e-6)
    assert np.allclose(res.free_energy, refb["fe_total"], rtol=1e-8)

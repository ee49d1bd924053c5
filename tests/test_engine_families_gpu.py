"""What the entry points shared by every engine family (rxhip_run, rxhip_run_filter, rxhip_set_data_device, the free-energy getters, the
RXHIP_VAR_X marginal getters, rxhip_destroy) do on ONE tiny engine per family: statuses, refusal texts, which buffer the free energy is read
from, and that a run longer than every initial per-iteration capacity (16 / 32 / first use) repeats the short run bit for bit.  The calls go
through ctypes on the handle wherever the Python classes do not expose an entry point for the family."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_X = "get_marginals: variable 1 is not random"
NO_TWIN = "run_filter: not a state-space engine with a streaming twin (the HGF engine is a filter already)"
NO_DATA = "run: no observations (call rxhip_set_data first)"
NO_DATA_BINREG = ("run: the binomial regression engine needs RXHIP_VAR_REGRESSORS, RXHIP_VAR_Y and RXHIP_VAR_TRIALS "
                  "(missing: regressors y n_trials)")


def _lgssm(rx):
    one = np.ones((1, 1))
    return rx.LGSSMEngine(0.9 * one, one, 0.1 * one, one, np.zeros(1), one, T=4, n_chains=2)


def _gmm(rx):
    m, o = np.array([-1.0, 1.0]), np.ones(2)
    return rx.GMMEngine(8, m, 10 * o, o, o, o, m, o, o, o, o)


def _mvgmm(d):
    def make(rx):
        mu = np.stack([-np.ones(d), np.ones(d)])
        eye = np.stack([np.eye(d)] * 2)
        nu = np.full(2, d + 1.0)
        return rx.MvGMMEngine(8, mu, 10 * eye, nu, eye / (d + 1.0), np.ones(2), mu, eye, nu, eye / (d + 1.0), np.ones(2))
    return make


def _binreg(rx):
    return rx.BinomialRegressionEngine(8, 1, np.zeros(1), np.eye(1))


def _feed_binreg(eng, y):
    eng.set_data(np.linspace(-1.0, 1.0, 8).reshape(1, 8, 1), y.reshape(1, 8), np.full((1, 8), 3.0))


def _feed_arreg(eng, y):
    eng.set_regressors(np.linspace(-1.0, 1.0, 8).reshape(1, 8, 1))
    eng.set_observations(y.reshape(1, 8))


# name -> (factory, n_chains, good observations, has RXHIP_VAR_X marginals, a value the family's check of device data refuses (or None))
_rng = np.random.default_rng(7)
FAMILIES = {
    "lgssm": (_lgssm, 2, _rng.standard_normal((4, 2, 1)), True, None),
    "drift": (lambda rx: rx.DriftChainEngine(4, 0.0, 1.0, 0.1, 1.0), 1, _rng.standard_normal((4, 1, 1)), True, None),
    "gmm": (_gmm, 1, _rng.standard_normal(8) + np.repeat([-1.0, 1.0], 4), False, None),
    "mvgmm2": (_mvgmm(2), 1, _rng.standard_normal((8, 2)) + np.repeat([[-1.0], [1.0]], 4, axis=0), False, None),
    "mvgmm5": (_mvgmm(5), 1, _rng.standard_normal((8, 5)) + np.repeat([[-1.0], [1.0]], 4, axis=0), False, None),
    "hgf": (lambda rx: rx.HGFEngine(4, 2, 1.0, -2.0, 1.0, 1.0), 2, _rng.standard_normal((4, 2)), False, None),
    "probit": (lambda rx: rx.ProbitEngine(4, 0.9, 0.0, 0.5, 0.0, 1.0), 1, np.array([[1.0], [0.0], [1.0], [1.0]]), True, 2.0),
    "hmm": (lambda rx: rx.HMMEngine(4, np.array([[3.0, 1.0], [1.0, 3.0]]), np.array([[4.0, 1.0], [1.0, 4.0]]), np.array([0.5, 0.5])), 1,
            np.array([[0.0], [1.0], [1.0], [0.0]]), False, 2.0),
    "lar": (lambda rx: rx.LAREngine(4, 1, 1.0), 1, _rng.standard_normal((4, 1)), False, np.inf),
    "binreg": (_binreg, 1, np.array([0.0, 1.0, 0.0, 2.0, 1.0, 3.0, 2.0, 3.0]), False, None),
    # one problem / series each at the smallest shapes: regression on regressors (N = 8, d = 1) and on the series' own lag (T = 8, order 1),
    # multinomial regression offline (N = 8, K = 3) and streamed (N = 4, K = 3), Gamma mixture (N = 8, K = 2)
    "arreg": (lambda rx: rx.ARRegressionEngine(8, 1), 1, _rng.standard_normal(8), False, None),
    "arreg_lagged": (lambda rx: rx.ARRegressionEngine(8, 1, lagged=True), 1, _rng.standard_normal((8, 1)), False, np.inf),
    "mnreg": (lambda rx: rx.MultinomialRegressionEngine(8, 3, np.zeros(2), np.eye(2)), 1, _rng.integers(0, 5, (1, 8, 3)).astype(np.float64), False, None),
    "mnreg_online": (lambda rx: rx.MultinomialRegressionEngine(4, 3, np.zeros(2), np.eye(2), online=True), 1,
                     _rng.integers(0, 5, (1, 4, 3)).astype(np.float64), False, None),
    "gammamix": (lambda rx: rx.GammaMixtureEngine(8, 2, (np.ones(2), np.ones(2)), (np.ones(2), np.ones(2)), np.ones(2), init_a=np.array([1.0, 3.0])), 1,
                 _rng.gamma(2.0, 1.0, (8, 1)), False, -1.0),
}
MIXTURES = ("gmm", "mvgmm2", "mvgmm5")
HOST_CHECKED = ("binreg", "arreg", "mnreg", "mnreg_online")   # families whose own set_data checks the arrays on the host: no device data
NO_DATA_MNREG = "run: no observations (the multinomial regression engine, mnreg, takes its counts through rxhip_set_data with RXHIP_VAR_Y)"
NO_DATA_OF = {"binreg": NO_DATA_BINREG, "arreg": "run: the regression engine needs RXHIP_VAR_REGRESSORS and RXHIP_VAR_Y (missing: regressors y)",
              "mnreg": NO_DATA_MNREG, "mnreg_online": NO_DATA_MNREG}
NAMES = list(FAMILIES)


def _L():
    from rxhip import _lib
    return _lib.lib()


def _feed(name, eng, y=None):
    y = FAMILIES[name][2] if y is None else y
    if name == "binreg":
        _feed_binreg(eng, y)
    elif name == "arreg":
        _feed_arreg(eng, y)
    else:
        eng.set_data(y)


def _err(eng):
    return _L().rxhip_last_error(eng._h).decode()


def _free_energy(eng, n):
    fe = np.full(n + 1, -7.0)   # one slot more than the getter may write
    assert _L().rxhip_get_free_energy(eng._h, fe.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0, _err(eng)
    assert fe[n] == -7.0
    return fe[:n]


@pytest.fixture(scope="module")
def hip():
    h = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")   # the runtime librxhip uses (torch, if loaded, carries its own copy)
    h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    h.hipFree.argtypes = [ctypes.c_void_p]
    return h


def _to_device(hip, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), a.nbytes) == 0
    assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
    return p


def _double_at(hip, ptr):
    out = np.empty(1)
    assert hip.hipMemcpy(out.ctypes.data, ptr, 8, 2) == 0
    return out[0]


@pytest.mark.parametrize("name", NAMES)
def test_run_refusals(name):
    import rxhip
    from rxhip import _lib
    L = _L()
    with FAMILIES[name][0](rxhip) as eng:
        assert L.rxhip_run(eng._h, 0, 1) == _lib.ERR_BADARG
        assert _err(eng) == "run: iterations must be positive"
        assert L.rxhip_run(eng._h, 2, 1) == _lib.ERR_STATE
        assert _err(eng) == NO_DATA_OF.get(name, NO_DATA)
        _feed(name, eng)
        if name == "lgssm":   # the one family with a streaming twin: a filtering run
            assert L.rxhip_run_filter(eng._h, 1) == _lib.OK, _err(eng)
            assert np.all(np.isfinite(_free_energy(eng, 1)))
        else:
            assert L.rxhip_run_filter(eng._h, 1) == _lib.ERR_BADARG
            assert _err(eng) == NO_TWIN
            assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, _err(eng)   # … and the refusal leaves the engine usable


@pytest.mark.parametrize("name", NAMES)
def test_free_energy_entry_points_and_capacity_growth(name, hip):
    import rxhip
    from rxhip import _lib
    L = _L()
    n_chains = FAMILIES[name][1]
    with FAMILIES[name][0](rxhip) as eng:
        _feed(name, eng)
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, _err(eng)
        short = _free_energy(eng, 2)
        assert np.all(np.isfinite(short))
        # the last entry, read through the two device-side entry points
        slot = _to_device(hip, np.zeros(1))
        assert L.rxhip_copy_free_energy_to_device(eng._h, slot) == _lib.OK, _err(eng)
        assert L.rxhip_sync(eng._h) == _lib.OK
        dev = ctypes.c_void_p()
        assert L.rxhip_get_free_energy_device(eng._h, ctypes.byref(dev)) == _lib.OK, _err(eng)
        assert _double_at(hip, slot) == short[1] and _double_at(hip, dev) == short[1]
        assert hip.hipFree(slot) == 0
        # per chain: not defined for the mixture engines, n_chains entries elsewhere
        pc = np.full(n_chains + 1, -7.0)
        st = L.rxhip_get_free_energy_per_chain(eng._h, pc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        if name in MIXTURES:
            assert st == _lib.ERR_BADARG and _err(eng) == "per-chain free energy is not defined for the mixture engine"
        else:
            assert st == _lib.OK, _err(eng)
            assert np.all(np.isfinite(pc[:n_chains])) and pc[n_chains] == -7.0
        # 40 iterations: more than every initial capacity (16, 32, or what the 2-iteration run reserved)
        assert L.rxhip_run(eng._h, 40, 1) == _lib.OK, _err(eng)
        long = _free_energy(eng, 40)
        assert np.all(np.isfinite(long))
        # The first two entries repeat the short run bit for bit, with two exceptions that are properties of the kernels, not of the buffers.  HGF: the
        # filter carries the belief after ALL iterations of a step into the next one, so every entry depends on the run's length.  HMM: the LAST sweep
        # of a run is another instance of the kernel (it also stores the posteriors), whose statistics differ in rounding: entry 1 was computed by
        # that instance in the short run only (8 log terms of size ≈ 1: a few ulp each, far inside 1e-13 of the sum).  The streamed multinomial
        # regression is the HGF's case: a row's prior is the posterior after ALL iterations of the row before, and entry i sums the rows' F after i + 1.
        if name == "hmm":
            assert long[0] == short[0] and long[1] == pytest.approx(short[1], rel=1e-13, abs=0)
        elif name not in ("hgf", "mnreg_online"):
            assert np.array_equal(long[:2], short)
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, _err(eng)
        assert np.array_equal(_free_energy(eng, 2), short)   # … and the grown buffers serve a short run as the first ones did
    with FAMILIES[name][0](rxhip) as eng:   # an engine whose FIRST run reserves 40 entries in one go gives the same 40 values
        _feed(name, eng)
        assert L.rxhip_run(eng._h, 40, 1) == _lib.OK, _err(eng)
        assert np.array_equal(_free_energy(eng, 40), long)


@pytest.mark.parametrize("name", NAMES)
def test_state_marginals_exist_or_are_refused(name):
    import rxhip
    from rxhip import _lib
    L = _L()
    dp = ctypes.POINTER(ctypes.c_double)
    factory, n_chains, _, has_x, _ = FAMILIES[name]
    with factory(rxhip) as eng:
        _feed(name, eng)
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, _err(eng)
        chains = np.zeros(1, dtype=np.int64)
        md, cd = ctypes.c_void_p(), ctypes.c_void_p()
        if not has_x:
            assert L.rxhip_get_marginals(eng._h, _lib.VAR_X, None, None, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG and _err(eng) == NO_X
            assert L.rxhip_get_marginals_device(eng._h, _lib.VAR_X, ctypes.byref(md), ctypes.byref(cd)) == _lib.ERR_BADARG and _err(eng) == NO_X
            assert L.rxhip_get_marginals_chains(eng._h, _lib.VAR_X, chains.ctypes.data_as(_lib.c_int64_p), 1, None, None) == _lib.ERR_BADARG
            assert _err(eng) == "get_marginals_chains: variable 1 is not random"
            return
        rows = 4 + (1 if name == "probit" else 0)   # the probit chain's x has T + 1 entries
        mean, one = np.full(rows * n_chains, np.nan), np.full(rows, np.nan)
        assert L.rxhip_get_marginals(eng._h, _lib.VAR_X, mean.ctypes.data_as(dp), None, _lib.LAYOUT_TIME_CHAIN) == _lib.OK, _err(eng)
        assert L.rxhip_get_marginals_device(eng._h, _lib.VAR_X, ctypes.byref(md), ctypes.byref(cd)) == _lib.OK and md.value and cd.value
        assert L.rxhip_get_marginals_chains(eng._h, _lib.VAR_X, chains.ctypes.data_as(_lib.c_int64_p), 1, one.ctypes.data_as(dp), None) == _lib.OK, _err(eng)
        assert np.all(np.isfinite(mean)) and np.array_equal(one, mean.reshape(rows, n_chains)[:, 0])


@pytest.mark.parametrize("name", [n for n in NAMES if n not in HOST_CHECKED])
def test_device_data_is_checked_and_runs_like_host_data(name, hip):
    import rxhip
    from rxhip import _lib
    L = _L()
    factory, _, y, _, bad = FAMILIES[name]
    with factory(rxhip) as eng:
        _feed(name, eng)
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, _err(eng)
        host = _free_energy(eng, 2)
    with factory(rxhip) as eng:
        if bad is not None:
            yb = y.copy()
            yb.flat[1] = bad
            pb = _to_device(hip, yb)
            assert L.rxhip_set_data_device(eng._h, _lib.VAR_Y, pb, yb.size, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG
            assert _err(eng) == {"probit": "set_data: a Probit observation is neither 0, 1 nor NaN (missing)",
                                 "hmm": "set_data: an observation is neither an integer symbol code 0 … 1 nor NaN (missing)",
                                 "lar": "set_data: an observation is infinite (finite values and NaN = missing are accepted)",
                                 "arreg_lagged": "set_data: an observation is infinite (finite values and NaN = missing are accepted)",
                                 "gammamix": "set_data: gammamix: an observation is zero, negative or infinite (positive finite values and NaN = missing "
                                             "are accepted)"}[name]
            assert L.rxhip_run(eng._h, 2, 1) == _lib.ERR_STATE and _err(eng) == NO_DATA   # a refused array counts as not set
            assert hip.hipFree(pb) == 0
        pg = _to_device(hip, y)
        assert L.rxhip_set_data_device(eng._h, _lib.VAR_Y, pg, y.size, _lib.LAYOUT_TIME_CHAIN) == _lib.OK, _err(eng)
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, _err(eng)
        assert np.array_equal(_free_energy(eng, 2), host)
    assert hip.hipFree(pg) == 0


def test_binreg_refuses_device_data(hip):
    import rxhip
    from rxhip import _lib
    with _binreg(rxhip) as eng:
        p = _to_device(hip, FAMILIES["binreg"][2])
        assert _L().rxhip_set_data_device(eng._h, _lib.VAR_Y, p, 8, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG
        assert _err(eng) == "set_data_device: the binomial regression engine checks its data on the host (rxhip_set_data)"
        assert hip.hipFree(p) == 0


@pytest.mark.parametrize("name, text", [
    ("arreg", "set_data_device: the regression engine checks X and y on the host (rxhip_set_data); the lagged mode takes device data"),
    ("mnreg", "set_data_device: the multinomial regression engine (mnreg) checks its counts on the host (rxhip_set_data)"),
    ("mnreg_online", "set_data_device: the multinomial regression engine (mnreg) checks its counts on the host (rxhip_set_data)")])
def test_host_checked_families_refuse_device_data(name, text, hip):
    import rxhip
    from rxhip import _lib
    factory, _, y, _, _ = FAMILIES[name]
    with factory(rxhip) as eng:
        p = _to_device(hip, y)
        assert _L().rxhip_set_data_device(eng._h, _lib.VAR_Y, p, y.size, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG
        assert _err(eng) == text
        assert hip.hipFree(p) == 0


@pytest.mark.parametrize("name", ["arreg", "arreg_lagged", "mnreg", "mnreg_online", "gammamix"])
def test_result_getters_refuse_before_a_run_and_without_free_energy(name):
    """the getters' shared preamble: "<entry point>: no run yet", then "<entry point>: free energy was not requested in the last run" """
    import rxhip
    from rxhip import RxHipError, _lib
    getter = {"arreg": "arreg_get_parameters", "arreg_lagged": "arreg_get_parameters", "mnreg": "mnreg_get_parameters", "mnreg_online": "mnreg_get_parameters",
              "gammamix": "gammamix_get_history"}[name]
    with FAMILIES[name][0](rxhip) as eng:
        _feed(name, eng)
        results = eng.history if name == "gammamix" else eng.parameters
        with pytest.raises(RxHipError) as exc:
            results()
        assert exc.value.status == _lib.ERR_STATE and str(exc.value).endswith(f"{getter}: no run yet")
        eng.run(2, free_energy=False)
        eng._fe = True   # ask for the free energies the run did not compute
        with pytest.raises(RxHipError) as exc:
            results()
        assert exc.value.status == _lib.ERR_STATE and str(exc.value).endswith(f"{getter}: free energy was not requested in the last run")
        eng._fe = False
        assert results() is not None   # … and both refusals leave the engine usable


def test_refused_creates_leave_a_handle_that_destroys_cleanly():
    from rxhip import _lib
    L = _L()
    hgf = _lib.HgfDesc(T=4, n_series=2, kappa=float("nan"), omega=-2.0, z_variance=1.0, y_variance=1.0, z0_mean=0.0, z0_var=5.0, x0_mean=0.0,
                       x0_var=5.0, n_gh=8, device=-1)
    probit = _lib.ProbitDesc(T=4, n_series=1, a=0.9, c=0.0, q=-1.0, m0=0.0, v0=1.0, n_gh=8, device=-1)
    hmm = _lib.HmmDesc(T=4, n_series=1, K=1, M=2, device=-1)
    lar = _lib.LarDesc(T=4, n_series=1, order=0, tau=1.0, prior_gamma_shape=1.0, prior_gamma_rate=1.0, device=-1)
    binreg = _lib.BinregDesc(N=8, n_problems=1, d=0, device=-1)
    arreg = _lib.ArregDesc(N=8, n_series=1, d=0, prior_gamma_shape=1.0, prior_gamma_rate=1.0, device=-1)
    mnreg = _lib.MnregDesc(N=8, n_problems=1, K=1, mode=_lib.MNREG_BATCH, device=-1)
    gammamix = _lib.GammaMixDesc(N=8, n_problems=1, K=0, device=-1)
    for create, desc, text in ((L.rxhip_arreg_create, arreg, "arreg: d must be 1 … 32 (got 0)"),
                               (L.rxhip_mnreg_create, mnreg, "mnreg: K must be 2 … 65 (got 1)"),
                               (L.rxhip_gammamix_create, gammamix, "gammamix: K must be 1 … 16 (got 0)"),
                               (L.rxhip_hgf_create, hgf, "hgf: kappa must be finite"),
                               (L.rxhip_probit_create, probit, "probit: the transition variance q must be positive and finite (got -1)"),
                               (L.rxhip_hmm_create, hmm, "hmm: K must be 2 … 16 states (got 1)"),
                               (L.rxhip_lar_create, lar, "lar: order must be 1 … 8 (got 0)"),
                               (L.rxhip_binreg_create, binreg, "binreg: d must be 1 … 32 (got 0)")):
        h = ctypes.c_void_p()
        assert create(ctypes.byref(desc), ctypes.byref(h)) == _lib.ERR_BADARG
        assert h.value and L.rxhip_last_error(h).decode() == text
        assert L.rxhip_destroy(h) == _lib.OK

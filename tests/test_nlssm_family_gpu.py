"""The entry points shared by every engine family on ONE tiny nonlinear state-space engine (T = 4, 2 series): the statuses and texts that
tests/test_engine_families_gpu.py checks for the other families (its list of families stays as it is)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_TWIN = "run_filter: not a state-space engine with a streaming twin (the HGF engine is a filter already)"
NO_DATA = "run: no observations (call rxhip_set_data first)"
Y = np.random.default_rng(7).standard_normal((4, 2, 1))
DP = ctypes.POINTER(ctypes.c_double)


def make(rx, **kw):
    return rx.NonlinearSSMEngine(lambda x: [x[0] + 0.1 * x[1], x[1] - 0.5 * np.sin(x[0])], 2, 4, np.zeros(2), np.eye(2), [1.0, 0.0], R=np.eye(1), Q=0.1 * np.eye(2),
                                 n_series=2, **kw)


def err(eng):
    import rxhip
    return rxhip.lib().rxhip_last_error(eng._h).decode()


def free_energy(eng, n):
    import rxhip
    fe = np.full(n + 1, -7.0)
    assert rxhip.lib().rxhip_get_free_energy(eng._h, fe.ctypes.data_as(DP)) == 0, err(eng)
    assert fe[n] == -7.0
    return fe[:n]


@pytest.fixture(scope="module")
def hip():
    h = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
    h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    h.hipFree.argtypes = [ctypes.c_void_p]
    return h


def to_device(hip, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
    return p


def double_at(hip, ptr):
    out = np.empty(1)
    assert hip.hipMemcpy(out.ctypes.data, ptr, 8, 2) == 0
    return out[0]


def test_run_refusals():
    import rxhip
    from rxhip import _lib
    L = rxhip.lib()
    with make(rxhip) as eng:
        assert L.rxhip_run(eng._h, 0, 1) == _lib.ERR_BADARG and err(eng) == "run: iterations must be positive"
        assert L.rxhip_run(eng._h, 2, 1) == _lib.ERR_STATE and err(eng) == NO_DATA
        eng.set_data(Y)
        assert L.rxhip_run_filter(eng._h, 1) == _lib.ERR_BADARG and err(eng) == NO_TWIN
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, err(eng)
        assert L.rxhip_nlssm_get_noise(eng._h, None, None) == _lib.ERR_BADARG and err(eng) == "nlssm_get_noise: the observation noise of this engine is known"


def test_free_energy_entry_points_and_capacity_growth(hip):
    import rxhip
    from rxhip import _lib
    L = rxhip.lib()
    with make(rxhip) as eng:
        eng.set_data(Y)
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, err(eng)
        short = free_energy(eng, 2)
        assert np.all(np.isfinite(short)) and short[0] == short[1]
        slot = to_device(hip, np.zeros(1))
        assert L.rxhip_copy_free_energy_to_device(eng._h, slot) == _lib.OK, err(eng)
        assert L.rxhip_sync(eng._h) == _lib.OK
        dev = ctypes.c_void_p()
        assert L.rxhip_get_free_energy_device(eng._h, ctypes.byref(dev)) == _lib.OK, err(eng)
        assert double_at(hip, slot) == short[1] and double_at(hip, dev) == short[1]
        assert hip.hipFree(slot) == 0
        pc = np.full(3, -7.0)
        assert L.rxhip_get_free_energy_per_chain(eng._h, pc.ctypes.data_as(DP)) == _lib.OK, err(eng)
        assert np.all(np.isfinite(pc[:2])) and pc[2] == -7.0 and pc[0] + pc[1] == short[0]
        assert L.rxhip_run(eng._h, 40, 1) == _lib.OK, err(eng)   # more than the initial capacity of 16
        long = free_energy(eng, 40)
        assert np.all(long == short[0])
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, err(eng)
        assert np.array_equal(free_energy(eng, 2), short)
        assert eng.counters()["rule_calls"] > 0
    with make(rxhip) as eng:
        eng.set_data(Y)
        assert L.rxhip_run(eng._h, 40, 1) == _lib.OK, err(eng)
        assert np.array_equal(free_energy(eng, 40), long)


def test_state_marginals_and_getters_before_a_run():
    import rxhip
    from rxhip import _lib
    L = rxhip.lib()
    with make(rxhip) as eng:
        eng.set_data(Y)
        mean, one = np.full(4 * 2 * 2, np.nan), np.full(4 * 2, np.nan)
        assert L.rxhip_get_marginals(eng._h, _lib.VAR_X, mean.ctypes.data_as(DP), None, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_STATE and err(eng) == "get_marginals: no run yet"
        assert L.rxhip_get_marginals(eng._h, _lib.VAR_Y, mean.ctypes.data_as(DP), None, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG
        assert err(eng) == "get_marginals: variable 0 is not random"
        assert L.rxhip_run(eng._h, 2, 0) == _lib.OK, err(eng)
        fe = np.zeros(2)
        assert L.rxhip_get_free_energy(eng._h, fe.ctypes.data_as(DP)) == _lib.ERR_STATE and err(eng) == "free energy was not requested in the last run"
        md, cd = ctypes.c_void_p(), ctypes.c_void_p()
        chains = np.zeros(1, dtype=np.int64)
        assert L.rxhip_get_marginals(eng._h, _lib.VAR_X, mean.ctypes.data_as(DP), None, _lib.LAYOUT_TIME_CHAIN) == _lib.OK, err(eng)
        assert L.rxhip_get_marginals(eng._h, _lib.VAR_X, mean.ctypes.data_as(DP), None, 7) == _lib.ERR_BADARG and err(eng) == "get_marginals: unknown layout 7"
        assert L.rxhip_get_marginals_device(eng._h, _lib.VAR_X, ctypes.byref(md), ctypes.byref(cd)) == _lib.OK and md.value and cd.value
        assert L.rxhip_get_marginals_chains(eng._h, _lib.VAR_X, chains.ctypes.data_as(_lib.c_int64_p), 1, one.ctypes.data_as(DP), None) == _lib.OK, err(eng)
        assert np.all(np.isfinite(mean)) and np.array_equal(one.reshape(4, 2), mean.reshape(4, 2, 2)[:, 0])
    with make(rxhip, noise_prior=None) as eng, pytest.raises(rxhip.RxHipError, match="nlssm_get_noise: the observation noise of this engine is known"):
        eng.noise()
    with rxhip.NonlinearSSMEngine(lambda x: [x[0]], 1, 4, [0.0], [[1.0]], [1.0], noise_prior=(1.0, 1.0), n_series=2) as eng:
        with pytest.raises(rxhip.RxHipError, match="nlssm_get_noise: no run yet"):
            eng.noise()


def test_device_data_runs_like_host_data(hip):
    import rxhip
    from rxhip import _lib
    L = rxhip.lib()
    with make(rxhip) as eng:
        eng.set_data(Y)
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, err(eng)
        host = free_energy(eng, 2)
    with make(rxhip) as eng:
        p = to_device(hip, Y)
        assert L.rxhip_set_data_device(eng._h, _lib.VAR_Y, p, Y.size, _lib.LAYOUT_TIME_CHAIN) == _lib.OK, err(eng)
        assert L.rxhip_set_data_device(eng._h, _lib.VAR_Y, p, Y.size - 1, _lib.LAYOUT_TIME_CHAIN) == _lib.ERR_BADARG and err(eng) == "set_data: expected 8 doubles, got 7"
        assert L.rxhip_run(eng._h, 2, 1) == _lib.OK, err(eng)
        assert np.array_equal(free_energy(eng, 2), host)
    assert hip.hipFree(p) == 0


def test_refused_create_leaves_a_handle_that_destroys_cleanly():
    import rxhip
    from rxhip import _lib
    L = rxhip.lib()
    desc = _lib.NlssmDesc(T=4, n_series=2, d=0, dy=1, device=-1)
    h = ctypes.c_void_p()
    assert L.rxhip_nlssm_create(ctypes.byref(desc), ctypes.byref(h)) == _lib.ERR_UNSUPPORTED
    assert h.value and L.rxhip_last_error(h).decode() == "nlssm: the state dimension d must be 1 … 4 (got 0)"
    assert L.rxhip_destroy(h) == _lib.OK

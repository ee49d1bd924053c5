"""CPU checks of the multinomial regression engine's boundary: rxhip_mnreg_desc is mirrored field for field by RxHip.jl and by the ctypes binding, no data
variable id was added, the refusals that need no device (they come before the first HIP call) carry a text that names mnreg, the schedule is a
function of N and K alone, and `infer` hands a MultinomialRegression model to the engine (the refusals of the DATA need an engine, hence a device:
tests/test_mnreg_gpu.py)."""
import re

import numpy as np
import pytest

import mnreg_ref as R
import rxhip
from rxhip import _lib
from test_julia_mirrors import HEADER, JULIA, c_fields, julia_fields


def test_descriptor_mirrors():
    want = c_fields("rxhip_mnreg_desc")
    assert want == ["N", "n_problems", "K", "mode", "n_trials", "prior_xi", "prior_precision", "init_mean", "init_cov", "keep_cov_history", "device", "stream"]
    assert julia_fields("MnregDesc") == want
    assert [f[0] for f in _lib.MnregDesc._fields_] == want
    modes = {k: int(v) for k, v in re.findall(r"RXHIP_MNREG_([A-Z]+)\s*=\s*(\d+)", HEADER)}
    assert modes == {"BATCH": 0, "ONLINE": 1} and (_lib.MNREG_BATCH, _lib.MNREG_ONLINE) == (0, 1)
    for name, v in modes.items():
        assert re.search(r"const RXHIP_MNREG_%s = Int32\(%d\)" % (name, v), JULIA), name
    for sym in ("rxhip_mnreg_create", "rxhip_mnreg_get_parameters", "rxhip_mnreg_get_history", "rxhip_mnreg_get_statistics", "rxhip_mnreg_schedule"):
        assert ":" + sym in JULIA, sym


def test_no_data_variable_id_was_added():
    ids = {k: int(v) for k, v in re.findall(r"RXHIP_VAR_([A-Z]+)\s*=\s*(\d+)", HEADER)}
    assert ids == {"Y": 0, "X": 1, "U": 2, "REGRESSORS": 3, "TRIALS": 4}


@pytest.mark.parametrize("online", [False, True])
def test_refusals_that_need_no_device(online):
    I2, z2 = np.eye(2), np.zeros(2)
    for args, kw in [((10, 66, np.zeros(65), np.eye(65)), {}), ((10, 1, np.zeros(0), np.zeros((0, 0))), {}), ((0, 3, z2, I2), {}),
                     ((10, 3, z2, I2), dict(n_problems=0)), ((10, 3, z2, I2), dict(n_problems=65536)), ((10, 3, z2, np.array([[1.0, 2.0], [2.0, 1.0]])), {}),
                     ((10, 3, z2, np.array([[1.0, 0.5], [0.0, 1.0]])), {}), ((10, 3, z2, np.array([[np.inf, 0.0], [0.0, 1.0]])), {}),
                     ((10, 3, z2, np.array([[np.nan, 0.0], [0.0, 1.0]])), {}), ((10, 3, np.array([np.nan, 0.0]), I2), {}),
                     ((10, 3, np.array([np.inf, 0.0]), I2), {}), ((10, 3, z2, I2), dict(init=(z2, -I2))), ((10, 3, z2, I2), dict(init=(np.array([np.nan, 0.0]), I2))),
                     ((10, 3, z2, I2), dict(n_trials=-1))]:
        with pytest.raises(rxhip.RxHipError) as ei:
            rxhip.MultinomialRegressionEngine(*args, online=online, **kw)
        assert ei.value.status == _lib.ERR_BADARG and "mnreg" in str(ei.value), (args[:2], kw, str(ei.value))
    desc = _lib.MnregDesc()
    desc.N, desc.n_problems, desc.K, desc.mode = 5, 1, 3, 2
    import ctypes
    h = ctypes.c_void_p()
    assert rxhip.lib().rxhip_mnreg_create(ctypes.byref(desc), ctypes.byref(h)) == _lib.ERR_BADARG and b"mnreg" in rxhip.lib().rxhip_last_error(h)
    assert rxhip.lib().rxhip_destroy(h) == _lib.OK


def test_schedule_values():
    S = rxhip.MultinomialRegressionEngine.schedule
    assert S(1000, 10) == (256, 4) and S(1000, 2) == (512, 2) and S(1000, 40) == (64, 16) and S(10 ** 7, 10) == (256, 1024) and S(1, 65) == (64, 1)
    for K in range(2, 66):
        assert S(12345, K)[0] == R.tile_rows(K) and S(10 ** 9, K)[1] == R.CHUNKS_CAP and R.tile_rows(K) * K <= 4160
    assert S(0, 5) == (0, 0) and S(10, 1) == (0, 0) and S(10, 66) == (0, 0)


@pytest.mark.skipif(rxhip.lib().rxhip_device_count() > 0, reason="checks the no-device error path")
def test_infer_reaches_the_engine():
    """a MultinomialRegression model is a device schedule of `infer` (it used to raise TypeError); without a device the engine says so"""
    Y, _, W0, N = R.golden()
    for kw in (dict(iterations=100), dict(iterations=1, autoupdates=True, keephistory=len(Y))):
        with pytest.raises(rxhip.RxHipError) as ei:
            rxhip.infer(model=rxhip.multinomial_regression(np.zeros(9), W0, n_trials=N), data={"y": Y}, free_energy=True, **kw)
        assert ei.value.status == _lib.ERR_NO_DEVICE
    res = rxhip.infer(model=rxhip.multinomial_regression(np.zeros(9), W0), data={"y": Y}, iterations=2, catch_exception=True)
    assert isinstance(res.error, rxhip.RxHipError) and res.posteriors == {}
    with pytest.raises(TypeError):
        rxhip.infer(model=object(), data={})

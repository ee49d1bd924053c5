"""CPU checks of the binomial regression engine's boundary: rxhip_binreg_desc is mirrored field for field by RxHip.jl and by the ctypes binding, the two
new data-variable ids are appended to the header's enum without moving the others, and the refusals that need no device (they come before the first
HIP call) carry a text."""
import re

import numpy as np
import pytest

import rxhip
from rxhip import _lib
from test_julia_mirrors import HEADER, JULIA, c_fields, julia_fields


def test_descriptor_mirrors():
    want = c_fields("rxhip_binreg_desc")
    assert want == ["N", "n_problems", "d", "prior_xi", "prior_precision", "init_mean", "init_cov", "device", "stream"]
    assert julia_fields("BinregDesc") == want
    assert [f[0] for f in _lib.BinregDesc._fields_] == want


def test_data_variable_ids_are_appended():
    ids = {k: int(v) for k, v in re.findall(r"RXHIP_VAR_([A-Z]+)\s*=\s*(\d+)", HEADER)}
    assert ids == {"Y": 0, "X": 1, "U": 2, "REGRESSORS": 3, "TRIALS": 4}
    assert (_lib.VAR_Y, _lib.VAR_X, _lib.VAR_U, _lib.VAR_REGRESSORS, _lib.VAR_TRIALS) == (0, 1, 2, 3, 4)
    for name, v in ids.items():
        assert re.search(r"const RXHIP_VAR_%s = Int32\(%d\)" % (name, v), JULIA), name


def test_refusals_that_need_no_device():
    I2 = np.eye(2)
    for args, kw in [((10, 33, np.zeros(33), np.eye(33)), {}), ((10, 0, np.zeros(0), np.zeros((0, 0))), {}), ((0, 2, np.zeros(2), I2), {}),
                     ((10, 2, np.zeros(2), I2), dict(n_problems=0)), ((10, 2, np.zeros(2), np.array([[1.0, 2.0], [2.0, 1.0]])), {}),
                     ((10, 2, np.zeros(2), np.array([[1.0, 0.5], [0.0, 1.0]])), {}), ((10, 2, np.zeros(2), np.array([[np.inf, 0.0], [0.0, 1.0]])), {}),
                     ((10, 2, np.array([np.nan, 0.0]), I2), {}), ((10, 2, np.zeros(2), I2), dict(init=(np.zeros(2), -I2)))]:
        with pytest.raises(rxhip.RxHipError) as ei:
            rxhip.BinomialRegressionEngine(*args, **kw)
        assert ei.value.status == _lib.ERR_BADARG and "binreg" in str(ei.value), (args[:2], kw, str(ei.value))
    assert rxhip.BinomialRegressionEngine.schedule(1000, 2) == (256, 4) and rxhip.BinomialRegressionEngine.schedule(1000, 17) == (128, 8)
    with pytest.raises(TypeError):
        rxhip.infer(model=object(), data={})

"""CPU checks of the regression / autoregression engine's boundary: every rxhip_arreg_* symbol the header declares is exported and bound,
rxhip_arreg_desc is mirrored field for field by RxHip.jl and by the ctypes binding, the engine and its two model constructors are part of the
package, and the refusals that need no device (they come before the first HIP call) carry a text."""
import re

import numpy as np
import pytest

import rxhip
from rxhip import _lib
from test_julia_mirrors import HEADER, JULIA, c_fields, julia_fields


def test_exported_symbols():
    declared = set(re.findall(r"\b(rxhip_arreg_[a-z_]+)\s*\(", HEADER))
    assert declared == {"rxhip_arreg_create", "rxhip_arreg_get_parameters", "rxhip_arreg_get_statistics", "rxhip_arreg_schedule"}
    L = _lib.lib()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in declared:
        assert name in bound and getattr(L, name) is not None, name
    for name in ("rxhip_arreg_create", "rxhip_arreg_get_parameters", "rxhip_arreg_get_statistics"):
        assert re.search(r":%s, librxhip" % name, JULIA), name


def test_descriptor_mirrors():
    want = c_fields("rxhip_arreg_desc")
    assert want == ["N", "n_series", "d", "lagged", "prior_theta_mean", "prior_theta_precision", "prior_gamma_shape", "prior_gamma_rate", "init_gamma_shape",
                    "init_gamma_rate", "share_parameters", "device", "stream"]
    assert julia_fields("ArregDesc") == want
    assert [f[0] for f in _lib.ArregDesc._fields_] == want


def test_public_names():
    assert rxhip.ARRegressionEngine.__name__ == "ARRegressionEngine"
    m = rxhip.autoregression(3, prior_gamma=(2, 3))
    assert m.order == 3 and m.prior_theta is None and m.prior_gamma == (2.0, 3.0) and m.init_gamma is None and m.share_parameters is False
    g = rxhip.gaussian_regression(np.zeros(2), np.eye(2), init_gamma=(1, 2), share_parameters=True)
    assert g.order is None and g.prior_theta[1].shape == (2, 2) and g.init_gamma == (1.0, 2.0) and g.share_parameters is True


def test_refusals_that_need_no_device():
    E, I2 = rxhip.ARRegressionEngine, np.eye(2)
    for args, kw in [((10, 33), {}), ((10, 0), {}), ((0, 2), {}), ((10, 2), dict(n_series=0)), ((10, 2), dict(prior_gamma=(0.0, 1.0))),
                     ((10, 2), dict(prior_gamma=(1.0, np.inf))), ((10, 2), dict(init_gamma=(-1.0, 1.0))), ((10, 2), dict(lagged=True, init_gamma=(1.0, np.nan))),
                     ((10, 2), dict(prior_theta=(np.zeros(2), np.array([[1.0, 2.0], [2.0, 1.0]])))), ((10, 2), dict(prior_theta=(np.zeros(2), np.array([[1.0, 0.5], [0.0, 1.0]])))),
                     ((10, 2), dict(prior_theta=(np.zeros(2), -I2), lagged=True)), ((10, 2), dict(prior_theta=(np.array([np.nan, 0.0]), I2)))]:
        with pytest.raises(rxhip.RxHipError) as ei:
            E(*args, **kw)
        assert ei.value.status == _lib.ERR_BADARG and "arreg" in str(ei.value), (args, kw, str(ei.value))
    with pytest.raises(ValueError):
        E(10, 2, prior_theta=(np.zeros(3), I2))
    S = E.schedule
    assert S(1000, 2) == (256, 4) and S(1000, 17) == (128, 8) and S(0, 5) == (128, 1) and S(995, 5) == (128, 8) and S(10, 33) == (0, 0)

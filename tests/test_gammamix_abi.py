"""CPU checks of the Gamma mixture engine's boundary: rxhip_gammamix_desc is mirrored field for field by RxHip.jl and by the ctypes binding, no data variable
id was added, the refusals that need no device (they come before the first HIP call) return RXHIP_ERR_BADARG with a text that names gammamix, the
schedule is a function of N and K alone, and `infer` hands a GammaMixture model to the engine (the refusals of the DATA need an engine, hence a device:
tests/test_gammamix_gpu.py)."""
import ctypes
import re

import numpy as np
import pytest

import gammamix_ref as R
import rxhip
from rxhip import _lib
from test_julia_mirrors import HEADER, JULIA, c_fields, julia_fields


def test_descriptor_mirrors():
    want = c_fields("rxhip_gammamix_desc")
    assert want == ["N", "n_problems", "K", "prior_a_shape", "prior_a_rate", "prior_b_shape", "prior_b_rate", "prior_alpha", "init_a", "init_b_shape", "init_b_rate",
                    "init_s_alpha", "schedule", "materialize_responsibilities", "device", "stream"]
    assert julia_fields("GammaMixDesc") == want
    assert [f[0] for f in _lib.GammaMixDesc._fields_] == want
    assert (_lib.GAMMAMIX_AUTO, _lib.GAMMAMIX_STREAMED, _lib.GAMMAMIX_RESIDENT) == (0, R.STREAMED, R.RESIDENT)
    for sym in ("rxhip_gammamix_create", "rxhip_gammamix_get_history", "rxhip_gammamix_get_responsibilities", "rxhip_gammamix_schedule", "rxhip_gammamix_set_stored_log"):
        assert ":" + sym in JULIA and sym + "(" in HEADER, sym


def test_no_data_variable_id_was_added():
    ids = {k: int(v) for k, v in re.findall(r"RXHIP_VAR_([A-Z]+)\s*=\s*(\d+)", HEADER)}
    assert ids == {"Y": 0, "X": 1, "U": 2, "REGRESSORS": 3, "TRIALS": 4}


def test_refusals_that_need_no_device():
    one = lambda K: (np.ones(K), np.ones(K))
    ok = dict(N=10, K=2, prior_a=one(2), prior_b=one(2), prior_alpha=np.ones(2))
    bad = [dict(K=0, prior_a=one(0), prior_b=one(0), prior_alpha=np.ones(0)), dict(K=17, prior_a=one(17), prior_b=one(17), prior_alpha=np.ones(17)), dict(N=0),
           dict(n_problems=0, prior_a=(np.ones((0, 2)), np.ones((0, 2))), prior_b=(np.ones((0, 2)), np.ones((0, 2))), prior_alpha=np.ones((0, 2))), dict(schedule=3),
           dict(schedule=-1), dict(schedule="resident"), dict(N=250, schedule=2), dict(prior_a=(np.array([0.5, 1.0]), np.ones(2))),
           dict(prior_a=(np.array([1.0, np.nan]), np.ones(2))), dict(prior_a=(np.ones(2), np.array([0.0, 1.0]))), dict(prior_a=(np.ones(2), np.array([np.inf, 1.0]))),
           dict(prior_b=(np.array([-1.0, 1.0]), np.ones(2))), dict(prior_b=(np.ones(2), np.array([np.nan, 1.0]))), dict(prior_alpha=np.array([0.0, 1.0])),
           dict(prior_alpha=np.array([np.inf, 1.0])), dict(init_a=np.array([0.0, 1.0])), dict(init_a=np.array([np.nan, 1.0])),
           dict(init_b=(np.array([1.0, -2.0]), np.ones(2))), dict(init_b=(np.ones(2), np.array([1.0, np.inf]))), dict(init_s=np.array([1.0, 0.0]))]
    for change in bad:
        kw = dict(ok, **change)
        with pytest.raises(rxhip.RxHipError) as ei:
            rxhip.GammaMixtureEngine(kw.pop("N"), kw.pop("K"), kw.pop("prior_a"), kw.pop("prior_b"), kw.pop("prior_alpha"), **kw)
        assert ei.value.status == _lib.ERR_BADARG and "gammamix" in str(ei.value), (change, str(ei.value))
    big = np.ones((65536, 1))
    with pytest.raises(rxhip.RxHipError) as ei:
        rxhip.GammaMixtureEngine(10, 1, (big, big), (big, big), big, n_problems=65536)
    assert ei.value.status == _lib.ERR_BADARG and "gammamix" in str(ei.value)
    desc = _lib.GammaMixDesc()                                   # the priors left NULL
    desc.N, desc.n_problems, desc.K = 5, 1, 2
    h = ctypes.c_void_p()
    assert rxhip.lib().rxhip_gammamix_create(ctypes.byref(desc), ctypes.byref(h)) == _lib.ERR_BADARG and b"gammamix" in rxhip.lib().rxhip_last_error(h)
    assert rxhip.lib().rxhip_destroy(h) == _lib.OK


def test_schedule_values():
    """one schedule, streamed, for every (N, K) of the engine's range: K alone never changes the kind, nor does N (the resident kernel is not part of the
    engine, and `schedule = 2` is refused: test_refusals_that_need_no_device)"""
    S = rxhip.GammaMixtureEngine.schedule
    for K in range(1, 17):
        for N in (1, 250, 3584, 3585, 10 ** 7, 10 ** 9):
            assert S(N, K) == R.schedule(N, K) == R.STREAMED
    assert S(0, 2) == 0 and S(-5, 2) == 0 and S(10, 0) == 0 and S(10, 17) == 0


@pytest.mark.skipif(rxhip.lib().rxhip_device_count() > 0, reason="checks the no-device error path")
def test_infer_reaches_the_engine():
    """a GammaMixture model is a device schedule of `infer`; without a device the engine says so"""
    y, prior = R.golden()
    model = rxhip.gamma_mixture([rxhip.GammaShapeScale(1.0, 0.1), rxhip.GammaShapeScale(1.0, 1.0)], [rxhip.GammaShapeRate(10.0, 0.5), (1.0, 1.0 / 3.0)],
                                rxhip.Dirichlet(prior[4]))
    assert np.allclose(model.prior_a[1], prior[1]) and np.allclose(model.prior_b[1], prior[3]) and np.allclose(model.prior_b[0], prior[2])
    with pytest.raises(rxhip.RxHipError) as ei:
        rxhip.infer(model=model, data={"y": y}, iterations=50, free_energy=True)
    assert ei.value.status == _lib.ERR_NO_DEVICE
    res = rxhip.infer(model=model, data={"y": y}, iterations=2, catch_exception=True)
    assert isinstance(res.error, rxhip.RxHipError) and res.posteriors == {}


def test_model_constructor_forms():
    a = rxhip.gamma_mixture([(1.0, 10.0), (1.0, 1.0)], [(10.0, 0.5), (1.0, 1 / 3)], [800.0, 200.0], init_a=[1.0, 1.0], init_b=[rxhip.GammaShapeRate(1.0, 1.0)] * 2)
    assert isinstance(a, rxhip.api.GammaMixture) and a.prior_a[0].tolist() == [1.0, 1.0] and a.prior_a[1].tolist() == [10.0, 1.0] and a.init_b[1].tolist() == [1.0, 1.0]
    assert a.prior_alpha.tolist() == [800.0, 200.0] and a.init_s is None
    assert issubclass(rxhip.GammaMixtureEngine, object) and rxhip.gamma_mixture is rxhip.api.gamma_mixture

"""What tests/test_python_surface_cpu.py checks for the classes defined in rxhip/engine.py, for NonlinearSSMEngine (defined in rxhip/nlssm.py and
re-exported by rxhip.engine, so that file's frozen list of classes does not see it): the one base class, its public surface, a refused creation
that leaves no handle behind, and the boundary of `infer` — what is checked before an engine exists propagates even with catch_exception, what the
engine refuses comes back as the result's error.  CPU only."""
import inspect

import numpy as np
import pytest

import rxhip
import rxhip.engine
from rxhip import _lib
from rxhip.engine import _Engine, _StateEngine

PEND = lambda x: [x[0] + 0.01 * x[1], x[1] - 0.0981 * np.sin(x[0])]
I2 = np.eye(2)

SURFACE = {
    "__init__": "(self, f, d, T, m0, V0, H, R=None, Q=None, noise_prior=None, method='linearization', unscented=None, mode='filter', n_series=1, "
                "per_series=False, device=-1, stream=None)",
    "noise": "(self)", "marginals": "(self, layout='time_chain', want_cov=True)", "marginals_of_chains": "(self, chains, want_cov=True)",
    "set_data": "(self, y, layout='time_chain')", "set_data_device": "(self, ptr, n, layout='time_chain', keepalive=None)",
    "run": "(self, iterations=1, free_energy=True)", "run_async": "(self, iterations=1, free_energy=True)", "sync": "(self)", "free_energy": "(self)",
    "free_energy_per_chain": "(self)", "counters": "(self)", "close": "(self)", "kernel_times": "(self)", "set_profiling": "(self, on=True)",
}


def test_the_class_is_one_object_under_both_names_and_inherits_the_one_base():
    cls = rxhip.NonlinearSSMEngine
    assert rxhip.engine.NonlinearSSMEngine is cls and cls.__module__ == "rxhip.nlssm"
    assert issubclass(cls, _StateEngine) and issubclass(cls, _Engine)


@pytest.mark.parametrize("attr", sorted(SURFACE))
def test_public_surface(attr):
    assert str(inspect.signature(getattr(rxhip.NonlinearSSMEngine, attr))) == SURFACE[attr]


def new_engine(made, *args, **kw):   # the object survives the constructor's exception
    made.append(rxhip.NonlinearSSMEngine.__new__(rxhip.NonlinearSSMEngine))
    made[0].__init__(*args, **kw)


@pytest.mark.skipif(rxhip.lib().rxhip_device_count() > 0, reason="checks the no-device error path")
def test_a_creation_refused_for_want_of_a_device_leaves_no_handle():
    made = []
    with pytest.raises(rxhip.RxHipError) as ei:
        new_engine(made, PEND, 2, 4, np.zeros(2), I2, [1.0, 0.0], R=[[1.0]])
    assert ei.value.status == _lib.ERR_NO_DEVICE
    assert str(ei.value)[len(f"rxhip status {_lib.ERR_NO_DEVICE}: "):].strip()   # a message of its own after the status
    eng, = made
    assert eng._h is None
    eng.close()
    eng.close()


def test_a_creation_refused_by_the_descriptor_leaves_no_handle():
    """with or without a device: the creator's own refusals come before the first HIP call"""
    made = []
    with pytest.raises(rxhip.RxHipError, match="nlssm: the prior covariance V0 of series 0") as ei:
        new_engine(made, PEND, 2, 4, np.zeros(2), -I2, [1.0, 0.0], R=[[1.0]])
    assert ei.value.status == _lib.ERR_NOT_POSDEF
    eng, = made
    assert eng._h is None
    eng.close()


KNOWN = rxhip.nonlinear_ssm(PEND, 2, np.zeros(2), I2, process_cov=0.1 * I2, obs_matrix=[1.0, 0.0], obs_cov=[[1.0]])
UNKNOWN = rxhip.nonlinear_ssm(PEND, 2, np.zeros(2), I2, obs_matrix=[1.0, 0.0], obs_precision_prior=rxhip.GammaShapeRate(1.0, 1.0), method=rxhip.Unscented())
CALLS = {"smooth": dict(model=KNOWN, data={"y": np.zeros(4)}), "filter": dict(model=UNKNOWN, data={"y": np.zeros(4)}, autoupdates=True, iterations=2)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_what_infer_checks_before_an_engine_exists_propagates_even_with_catch_exception(name):
    with pytest.raises(ValueError, match="Unknown option keys"):
        rxhip.infer(**CALLS[name], options={"nope": 1}, catch_exception=True)
    with pytest.raises(ValueError, match=r"y is \[T\]\[1\]"):
        rxhip.infer(**dict(CALLS[name], data={"y": np.zeros((4, 3))}), catch_exception=True)
    with pytest.raises(ValueError, match="keephistory must be 4"):
        rxhip.infer(**dict(CALLS["filter"], keephistory=3), catch_exception=True)


def test_what_the_engine_refuses_is_caught():
    """a refusal of the creator itself (smoothing with unknown noise: with or without a device) comes back as the result's error"""
    call = dict(model=UNKNOWN, data={"y": np.zeros(4)})
    res = rxhip.infer(**call, catch_exception=True)
    assert isinstance(res.error, rxhip.RxHipError) and res.error.status == _lib.ERR_UNSUPPORTED and "smoothing with unknown observation noise" in str(res.error)
    assert res.posteriors == {} and res.model is UNKNOWN
    with pytest.raises(rxhip.RxHipError):
        rxhip.infer(**call)


@pytest.mark.skipif(rxhip.lib().rxhip_device_count() > 0, reason="checks the no-device error path")
@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_missing_device_is_caught(name):
    res = rxhip.infer(**CALLS[name], options={"device": -1}, catch_exception=True)
    assert isinstance(res.error, rxhip.RxHipError) and res.error.status == _lib.ERR_NO_DEVICE
    assert res.posteriors == {} and res.model is CALLS[name]["model"]
    with pytest.raises(rxhip.RxHipError):
        rxhip.infer(**CALLS[name])

"""CPU checks of the nonlinear state-space engine's boundary: the symbols the header declares are exported and bound, rxhip_nlssm_desc and
rxhip_expr_program are mirrored field for field by the ctypes binding, the engine and its model constructor are part of the package, and every
refusal of the creator — they all come before the first HIP call — carries a text that names nlssm."""
import ctypes
import re

import numpy as np
import pytest

import rxhip
from rxhip import _lib
from test_julia_mirrors import HEADER, c_fields

I2 = np.eye(2)
PEND = lambda x: [x[0] + 0.01 * x[1], x[1] - 0.0981 * np.sin(x[0])]


def test_exported_symbols():
    declared = set(re.findall(r"\b(rxhip_(?:nlssm|expr)_[a-z_]+)\s*\(", HEADER))
    assert declared == {"rxhip_nlssm_create", "rxhip_nlssm_get_noise", "rxhip_expr_eval"}
    L = _lib.lib()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in declared:
        assert name in bound and getattr(L, name) is not None, name


def test_descriptor_mirrors():
    assert [f[0] for f in _lib.NlssmDesc._fields_] == c_fields("rxhip_nlssm_desc") == [
        "T", "n_series", "d", "dy", "f", "m0", "V0", "Q", "H", "R", "noise_shape", "noise_rate", "method", "alpha", "beta", "kappa", "mode", "per_series", "device",
        "stream"]
    assert [f[0] for f in _lib.ExprProgram._fields_] == c_fields("rxhip_expr_program") == ["n_code", "n_consts", "d", "n_slots", "code", "consts"]
    ops = dict(re.findall(r"RXHIP_OP_([A-Z]+) = (\d+)", HEADER))
    assert {k: int(v) for k, v in ops.items()} == {n: getattr(_lib, "OP_" + n) for n in rxhip.expr.OP_NAMES}


def test_public_names():
    assert rxhip.NonlinearSSMEngine.__name__ == "NonlinearSSMEngine"
    m = rxhip.nonlinear_ssm(PEND, 2, np.zeros(2), I2, obs_matrix=[1.0, 0.0], obs_precision_prior=rxhip.GammaShapeScale(1.0, 100.0))
    assert isinstance(m.f, rxhip.Program) and m.d == 2 and m.obs_matrix.shape == (1, 2) and isinstance(m.method, rxhip.Linearization) and m.process_cov is None
    u = rxhip.nonlinear_ssm(m.f, 2, np.zeros(2), I2, process_cov=0.1 * I2, obs_matrix=I2, obs_cov=I2, method=rxhip.Unscented(alpha=0.5))
    assert (u.method.alpha, u.method.beta, u.method.kappa) == (0.5, 2.0, 0.0) and u.f is m.f
    for kw in (dict(obs_cov=I2, obs_precision_prior=rxhip.GammaShapeRate(1.0, 1.0)), dict()):
        with pytest.raises(ValueError):
            rxhip.nonlinear_ssm(PEND, 2, np.zeros(2), I2, obs_matrix=I2, **kw)
    with pytest.raises(TypeError):
        rxhip.nonlinear_ssm(PEND, 2, np.zeros(2), I2, obs_matrix=I2, obs_cov=I2, method="unscented")
    for bad in (rxhip.Unscented(alpha=0.0, beta=5.0, kappa=1.0), rxhip.Unscented(alpha=-1.0), rxhip.Unscented(beta=np.nan)):
        with pytest.raises(ValueError, match="alpha > 0"):
            rxhip.nonlinear_ssm(PEND, 2, np.zeros(2), I2, obs_matrix=I2, obs_cov=I2, method=bad)
    assert float(re.search(r"RXHIP_NLSSM_DEFAULT_ALPHA (\S+)", HEADER).group(1)) == rxhip.Unscented().alpha


def refused(status, text, f=PEND, d=2, T=5, m0=np.zeros(2), V0=I2, H=np.array([[1.0, 0.0]]), **kw):
    with pytest.raises(rxhip.RxHipError) as ei:
        rxhip.NonlinearSSMEngine(f, d, T, m0, V0, H, **kw)
    assert ei.value.status == status and "nlssm" in str(ei.value) and text in str(ei.value), str(ei.value)


def test_refusals_that_need_no_device():
    B, U, N = _lib.ERR_BADARG, _lib.ERR_UNSUPPORTED, _lib.ERR_NOT_POSDEF
    R1 = np.eye(1)
    refused(N, "prior covariance V0 of series 0", V0=np.array([[1.0, 2.0], [2.0, 1.0]]), R=R1)
    refused(N, "prior covariance V0 of series 1", m0=np.zeros((2, 2)), V0=np.stack([I2, -I2]), R=R1, n_series=2, per_series=True)
    refused(N, "prior covariance V0", V0=np.array([[1.0, 0.5], [0.0, 1.0]]), R=R1)                      # not symmetric
    refused(N, "observation covariance R", R=np.zeros((1, 1)))
    refused(N, "process covariance Q", R=R1, Q=np.array([[1.0, 0.0], [0.0, -1e-3]]))
    refused(N, "process covariance Q", R=R1, Q=np.array([[1.0, 0.2], [0.1, 1.0]]))
    refused(B, "prior mean m0", m0=np.array([np.nan, 0.0]), R=R1)
    refused(B, "d_y must be 1 … d = 2 (got 3)", H=np.ones((3, 2)), R=np.eye(3))
    refused(B, "alpha must be positive", R=R1, method="unscented", unscented=(-1.0, 2.0, 0.0))
    refused(B, "alpha must be positive", R=R1, method="unscented", unscented=(0.0, 5.0, 1.0))
    refused(B, "d + lambda", R=R1, method="unscented", unscented=(1.0, 2.0, -2.0))
    refused(B, "known observation noise needs R")
    refused(U, "unknown observation noise needs d_y = 1 (got 2)", H=I2, noise_prior=(1.0, 1.0))
    refused(B, "positive finite shape and rate", noise_prior=(1.0, 0.0))
    refused(U, "smoothing with unknown observation noise", noise_prior=(1.0, 1.0), mode="smooth")
    # programs: the tracer refuses what is over the caps; a hand-made Program reaches the creator's own checks
    P = rxhip.Program
    refused(B, "program was traced for dimension 1", f=P([[_lib.OP_VAR, 0, 0, 0], [_lib.OP_OUT, 0, 0, 0]], [], 1, 1), R=R1)
    refused(B, "no OUT for output 1", f=P([[_lib.OP_VAR, 0, 0, 0], [_lib.OP_OUT, 0, 0, 0]], [], 2, 1), R=R1)
    refused(B, "1 … 128 instructions (got 129)", f=P([[_lib.OP_VAR, 0, 0, 0]] * 127 + [[_lib.OP_OUT, 0, 0, 0], [_lib.OP_OUT, 1, 0, 0]], [], 2, 1), R=R1)
    refused(B, "1 … 16 live slots (got 17)", f=P([[_lib.OP_VAR, 0, 0, 0], [_lib.OP_OUT, 0, 0, 0], [_lib.OP_OUT, 1, 0, 0]], [], 2, 17), R=R1)
    refused(B, "at most 32 constants (got 33)", f=P([[_lib.OP_VAR, 0, 0, 0], [_lib.OP_OUT, 0, 0, 0], [_lib.OP_OUT, 1, 0, 0]], np.ones(33), 2, 1), R=R1)
    refused(B, "reads slot 1 before it is written", f=P([[_lib.OP_VAR, 0, 0, 0], [_lib.OP_ADD, 0, 0, 1], [_lib.OP_OUT, 0, 0, 0], [_lib.OP_OUT, 1, 0, 0]], [], 2, 2), R=R1)
    refused(B, "unknown opcode 14", f=P([[14, 0, 0, 0], [_lib.OP_OUT, 0, 0, 0], [_lib.OP_OUT, 1, 0, 0]], [], 2, 1), R=R1)
    refused(B, "names input 2 of 2", f=P([[_lib.OP_VAR, 0, 2, 0], [_lib.OP_OUT, 0, 0, 0], [_lib.OP_OUT, 1, 0, 0]], [], 2, 1), R=R1)
    refused(B, "constant 0 is not finite", f=P([[_lib.OP_CONST, 0, 0, 0], [_lib.OP_OUT, 0, 0, 0], [_lib.OP_OUT, 1, 0, 0]], [np.inf], 2, 1), R=R1)
    # d outside 1 … 4: the tracer refuses it first; through the C ABI the creator does
    with pytest.raises(rxhip.ProgramError):
        rxhip.NonlinearSSMEngine(lambda x: x, 5, 5, np.zeros(5), np.eye(5), np.eye(5), R=np.eye(5))
    L, h, desc = _lib.lib(), ctypes.c_void_p(), _lib.NlssmDesc()
    desc.T, desc.n_series, desc.d, desc.dy = 5, 1, 5, 1
    assert L.rxhip_nlssm_create(ctypes.byref(desc), ctypes.byref(h)) == U and b"nlssm: the state dimension d must be 1" in L.rxhip_last_error(h)
    L.rxhip_destroy(h)
    desc.T = 0
    assert L.rxhip_nlssm_create(ctypes.byref(desc), ctypes.byref(h)) == B and not h.value
    with pytest.raises(ValueError):
        rxhip.NonlinearSSMEngine(PEND, 2, 5, np.zeros(2), I2, [1.0, 0.0], R=R1, method="cvi")


def test_expr_eval_refuses_a_malformed_program_with_a_text():
    p = rxhip.Program([[_lib.OP_VAR, 0, 0, 0]], [], 1, 1)
    with pytest.raises(rxhip.RxHipError, match="no OUT for output 0") as ei:
        rxhip.expr_eval(p, np.zeros((3, 1)))
    assert ei.value.status == _lib.ERR_BADARG

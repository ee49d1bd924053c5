"""The workgroup form of the reverse-filter sweep (k_forward0_ck, k_backward_sh_rev): W = 1, 2 or 4 waves per workgroup take W
adjacent 64-chain groups of one segment and share one double-buffered table stream, with one LDS-only workgroup barrier per chunk of four
steps.  A lane's arithmetic is the same in every arm, so RXHIP_SWEEP_WAVES = 1, 2 and 4 must agree bit for bit.

Shapes: `segments=` is a request — the engine takes L = ⌈(T − 1)/S⌉ and then S = ⌈(T − 1)/L⌉.  256 and 512 chains are one and two workgroups of
four waves per segment (two and four of two waves).  The segment lengths (last segment) below are 121 (117), 122 (120), 139 (137), 64 (62),
12 (11) and 111 (110): every remainder mod 4 of the chunk loop's tail, in the full segments and in the shorter last one; 64 is a multiple of
the stride 16 (the segment's end is a checkpoint of both rules), 12 is shorter than the stride (the end is the only checkpoint).  The stride is
forced, so every model takes the reverse-filter schedule at every shape."""
import os

import numpy as np
import pytest

import rxhip
import rxoracle
from rxhip import workloads

pytestmark = pytest.mark.gpu

MODELS = {
    (4, 4): workloads.c1_model,
    (3, 2): lambda: workloads.random_model(3, 2, 20),
    (2, 2): lambda: workloads.random_model(2, 2, 4),
    (1, 1): lambda: workloads.random_model(1, 1, 3),
}
#         chains, T, segments asked for, forced checkpoint stride
SHAPES = [(256, 602, 5, 8), (512, 365, 3, 16), (256, 694, 5, 16), (512, 191, 3, 16), (256, 60, 5, 16), (512, 333, 3, 8)]
ARMS = ("1", "2", "4")


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):   # a value of None removes the variable for the duration
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _env(waves, K=None, boundary_kernel=None):
    return _Env(RXHIP_TEST_HOOKS="1", RXHIP_ONE_PASS="1", RXHIP_Y_RING=None, RXHIP_SWEEP_WAVES=waves,
                RXHIP_MEAN_CHECKPOINT=str(K) if K else None, RXHIP_BOUNDARY_KERNEL=boundary_kernel)


def _engine(mdl, T, C, S):
    return rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C, segments=S, device=0)


def _results(eng, C, fe):
    mean, cov = eng.marginals_of_chains(np.arange(C))
    out = [np.array(mean), np.array(cov)]
    if fe:
        out += [np.array(eng.free_energy_per_chain()), np.array(eng.free_energy())]
    return out


def _two_sweeps(mdl, y, C, T, S, K, waves, fe, boundary_kernel):
    """(first sweep, second sweep) of one arm: the first sweep of a handle stores the per-chain covariances, the second does not"""
    with _env(waves, K, boundary_kernel):
        with _engine(mdl, T, C, S) as eng:
            assert eng.mean_checkpoint_stride() == K
            if waves is not None:
                assert eng.sweep_waves() == (int(waves), int(waves))
            eng.set_data(y)
            eng.run(iterations=1, free_energy=fe)
            first = _results(eng, C, fe)
            eng.run(iterations=1, free_energy=fe)
            return first, _results(eng, C, fe)


_data = {}


def _y(key, C, T):
    if (key, C, T) not in _data:
        _data[(key, C, T)] = workloads.generate_batch(MODELS[key](), T, C, seed0=17)
    return _data[(key, C, T)]


@pytest.mark.parametrize("boundary_kernel", [None, "1"], ids=["boundary_in_sweep", "boundary_kernel"])
@pytest.mark.parametrize("fe", [True, False], ids=["fe", "nofe"])
@pytest.mark.parametrize("key", list(MODELS), ids=lambda k: f"d{k[0]}dy{k[1]}")
@pytest.mark.parametrize("C,T,S,K", SHAPES, ids=lambda v: str(v))
def test_arms_agree_bit_for_bit(key, C, T, S, K, fe, boundary_kernel):
    mdl, y = MODELS[key](), _y(key, C, T)
    ref = _two_sweeps(mdl, y, C, T, S, K, "1", fe, boundary_kernel)
    for a in ref[0] + ref[1]:
        assert np.all(np.isfinite(a))
    for waves in ARMS[1:]:
        got = _two_sweeps(mdl, y, C, T, S, K, waves, fe, boundary_kernel)
        for sweep in (0, 1):
            for name, a, b in zip(("mean", "cov", "fe per chain", "fe"), ref[sweep], got[sweep]):
                assert np.array_equal(a, b), (waves, "first" if sweep == 0 else "second", name, float(np.max(np.abs(a - b))))


@pytest.mark.parametrize("C,T,S,K", SHAPES[:2], ids=lambda v: str(v))
def test_shipped_widths_agree_with_one_wave(C, T, S, K):
    """no hook: each kernel at the width it ships (they may differ), against one wave for both"""
    mdl, y = MODELS[(4, 4)](), _y((4, 4), C, T)
    ref = _two_sweeps(mdl, y, C, T, S, K, "1", True, None)
    got = _two_sweeps(mdl, y, C, T, S, K, None, True, None)
    for sweep in (0, 1):
        for a, b in zip(ref[sweep], got[sweep]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("waves", ARMS)
def test_oracle_parity(waves):
    """First and last chain of a (4, 4) batch against the CPU oracle, with the measures and bounds of the benchmark's parity check"""
    C, T, S, K = SHAPES[0]
    mdl, y = MODELS[(4, 4)](), _y((4, 4), C, T)
    (mean, cov, fec, _), _ = _two_sweeps(mdl, y, C, T, S, K, waves, True, None)
    for c in (0, C - 1):
        om, oc, ofe = rxoracle.lgssm_bp(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], np.ascontiguousarray(y[:, c]))[:3]
        sd = np.sqrt(np.einsum("tii->ti", oc))
        mean_rel = float(np.max(np.abs(mean[c] - om) / sd))
        cov_rel = float(np.max(np.abs(cov[c] - oc) / np.max(np.abs(oc), axis=(1, 2), keepdims=True)))
        fe_rel = float(abs(fec[c] - ofe) / abs(ofe))
        print(f"W = {waves}, chain {c}: mean {mean_rel:.2e} cov {cov_rel:.2e} fe {fe_rel:.2e}")
        assert mean_rel < 1e-6 and cov_rel < 1e-6 and fe_rel < 1e-8, (mean_rel, cov_rel, fe_rel)


@pytest.mark.parametrize("C,expect", [(320, (1, 1)), (128, (1, 2)), (256, (1, 2))])
def test_width_follows_the_batch(C, expect):
    """(forward, backward).  64·W chains of a workgroup sit in one segment: 320 = 5 · 64 leaves one wave, 128 two — the width the backward
    sweep ships; the forward kernel ships one wave (csrc/lgssm_plan.hpp SWEEP_WAVES_FORWARD / _BACKWARD)"""
    mdl = workloads.c1_model()
    with _env(None, 8):
        with _engine(mdl, 203, C, 5) as eng:
            assert eng.mean_checkpoint_stride() == 8
            assert eng.sweep_waves() == expect


def test_no_width_off_the_reverse_filter_schedule():
    mdl = workloads.c1_model()
    with _Env(RXHIP_TEST_HOOKS="1", RXHIP_ONE_PASS="0", RXHIP_SWEEP_WAVES=None, RXHIP_MEAN_CHECKPOINT=None):
        with _engine(mdl, 203, 128, 5) as eng:
            assert eng.mean_checkpoint_stride() == 0 and eng.sweep_waves() == (0, 0)


@pytest.mark.parametrize("C,waves", [(128, "4"), (320, "2"), (64, "2")])
def test_width_that_does_not_divide_the_batch_is_refused(C, waves):
    mdl = workloads.c1_model()
    with _env(waves, 8):
        with pytest.raises(rxhip.RxHipError, match="RXHIP_SWEEP_WAVES"):
            _engine(mdl, 203, C, 5).close()


@pytest.mark.parametrize("value", ["0", "3", "8", "-1", "x", "2x", ""])
def test_bad_value_is_refused_at_creation(value):
    mdl = workloads.c1_model()
    with _env(value, 8):
        with pytest.raises(rxhip.RxHipError, match="RXHIP_SWEEP_WAVES"):
            _engine(mdl, 203, 256, 5).close()


@pytest.mark.parametrize("first,second", [("1", "4"), ("4", "2")])
def test_pool_does_not_hand_back_another_width(first, second):
    """an engine of this size is parked when it is destroyed; the width is part of the pool's key (every hook is)"""
    C, T, S = 256, 203, 5
    mdl = workloads.c1_model()
    y = workloads.generate_batch(mdl, T, C, seed0=5)
    rxhip.lib().rxhip_release_cached_memory()   # no parked engine of an earlier test
    with _env(first, 8):
        with _engine(mdl, T, C, S) as eng:
            assert eng.sweep_waves() == (int(first), int(first))
            eng.set_data(y)
            eng.run(iterations=1, free_energy=True)
    with _env(second, 8):
        with _engine(mdl, T, C, S) as eng:
            assert eng.sweep_waves() == (int(second), int(second))

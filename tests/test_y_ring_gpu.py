"""The observation ring of the reverse-filter sweep (k_backward_sh_rev): y runs Y_RING_SHIPPED = 4 steps ahead of its use in a
register ring, the table rows one chunk ahead, both loaded unconditionally with the index clamped into the wave's own segment; whole chunks of
four steps run in a loop of their own and the last len mod 4 steps behind it.  RXHIP_Y_RING=1 selects the depth-1 instance of the same
loop; the arithmetic of a step is the same in both, so posteriors and free energy must agree bit for bit.

Shapes: `segments=` is a request — the engine takes L = ⌈(T − 1)/S⌉ and then S = ⌈(T − 1)/L⌉.  The segment lengths below are 1, 2 and 3
(shorter than the ring: every ring load past the first is clamped), 4 and 5 (the ring's depth and one more: one whole chunk, and a
whole chunk with a one-step tail), 36 (whole chunks only, across checkpoints), 18 (a tail of two steps), 41 with a last segment of 38
(tails of one and two steps, several checkpoints per segment at every stride), 9 with a last segment of 3, and 8.  tests/reverse_filter_ref.choose_stride
admits all of them for the three models (strides 8 … 32); a case whose engine disagrees skips loudly, and no (4, 4) case may."""
import os

import numpy as np
import pytest

import rxhip
import rxoracle
from rxhip import workloads

pytestmark = pytest.mark.gpu

# (the models of tests/test_boundary_in_sweep_gpu.py: the first seeds whose reverse filter stays inside its bound at these shapes)
MODELS = {
    (4, 4): workloads.c1_model,
    (2, 2): lambda: workloads.random_model(2, 2, 4),
    (3, 2): lambda: workloads.random_model(3, 2, 20),
}
#         chains, T, segments asked for, forced checkpoint stride (0: the engine's own)
SHAPES = [(64, 3, 2, 0), (64, 6, 5, 0), (64, 7, 3, 0), (64, 7, 2, 0), (64, 9, 2, 0), (64, 11, 2, 0), (64, 37, 1, 0), (64, 37, 2, 0),
          (128, 203, 5, 0), (64, 1030, 128, 0), (64, 1025, 128, 0), (128, 203, 5, 8)]
ORACLE_SHAPES = [(64, 7, 2, 0), (64, 11, 2, 0), (128, 203, 5, 0), (64, 1030, 128, 0), (128, 203, 5, 8)]


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


def _engine(mdl, T, C, S):
    return rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C, segments=S, device=0)


def _results(eng, C):
    mean, cov = eng.marginals_of_chains(np.arange(C))
    return np.array(mean), np.array(cov), np.array(eng.free_energy_per_chain()), np.array(eng.free_energy())


def _env(ring, K):
    kv = dict(RXHIP_TEST_HOOKS="1", RXHIP_ONE_PASS="1", RXHIP_Y_RING=ring)   # ring None: the default arm, whatever the caller exported
    if K:
        kv["RXHIP_MEAN_CHECKPOINT"] = str(K)
    return _Env(**kv)


_cache = {}


def _run(key, C, T, S, K, ring):
    """(stride, y, first run, second run) of one arm — a run is (mean, cov, fe per chain, fe); computed once per (model, shape, arm) and
    shared, never modified.  The first run of a handle stores the per-chain covariances, the second is the store-free variant."""
    k = (key, C, T, S, K, ring)
    if k not in _cache:
        mdl = MODELS[key]()
        y = workloads.generate_batch(mdl, T, C, seed0=17)
        with _env(ring, K):
            with _engine(mdl, T, C, S) as eng:
                stride = eng.mean_checkpoint_stride()
                eng.set_data(y)
                eng.run(iterations=1, free_energy=True)
                first = _results(eng, C)
                eng.run(iterations=1, free_energy=True)
                _cache[k] = (stride, y, first, _results(eng, C))
    return _cache[k]


def _skip_unless_reverse(key, stride, C, T, S):
    if stride == 0:
        assert key != (4, 4), "the headline model must take the reverse-filter schedule at every shape"
        pytest.skip(f"model {key}: no admissible checkpoint stride at {C} x {T}, S = {S}: the reverse-filter schedule is not taken")


@pytest.mark.parametrize("key", list(MODELS), ids=lambda k: f"d{k[0]}dy{k[1]}")
@pytest.mark.parametrize("C,T,S,K", SHAPES, ids=lambda v: str(v))
def test_bit_identical_to_depth_one(key, C, T, S, K):
    stride, _, (mean, cov, fec, fe), _ = _run(key, C, T, S, K, ring=None)
    _skip_unless_reverse(key, stride, C, T, S)
    if K:
        assert stride == K
    stride1, _, (mean1, cov1, fec1, fe1), _ = _run(key, C, T, S, K, ring="1")
    assert stride1 == stride
    assert np.array_equal(mean, mean1)
    assert np.array_equal(cov, cov1)
    assert np.array_equal(fec, fec1)
    assert np.array_equal(fe, fe1)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(cov)) and np.all(np.isfinite(fec)) and np.all(np.isfinite(fe))


@pytest.mark.parametrize("ring", [None, "1"], ids=["shipped", "depth1"])
@pytest.mark.parametrize("key", list(MODELS), ids=lambda k: f"d{k[0]}dy{k[1]}")
@pytest.mark.parametrize("C,T,S,K", SHAPES, ids=lambda v: str(v))
def test_second_run_repeats_the_first(key, C, T, S, K, ring):
    """the sweep that stores the covariances and the store-free one: same means, same free energy (and the array the first left is intact)"""
    stride, _, (mean, cov, fec, fe), (mean2, cov2, fec2, fe2) = _run(key, C, T, S, K, ring)
    _skip_unless_reverse(key, stride, C, T, S)
    assert np.array_equal(mean, mean2)
    assert np.array_equal(cov, cov2)
    assert np.array_equal(fec, fec2)
    assert np.array_equal(fe, fe2)
    assert np.all(np.isfinite(mean2)) and np.all(np.isfinite(fec2))


@pytest.mark.parametrize("key", list(MODELS), ids=lambda k: f"d{k[0]}dy{k[1]}")
@pytest.mark.parametrize("C,T,S,K", ORACLE_SHAPES, ids=lambda v: str(v))
def test_oracle_parity(key, C, T, S, K):
    """First and last chain against the CPU oracle, with the measures and bounds of the benchmark's parity check: rxoracle.lgssm_bp at
    dy = d, rxoracle.lgssm_kalman_rts at dy < d (tests/test_boundary_in_sweep_gpu.py says why)."""
    stride, y, (mean, cov, fec, _), _ = _run(key, C, T, S, K, ring=None)
    _skip_unless_reverse(key, stride, C, T, S)
    mdl = MODELS[key]()
    for c in (0, C - 1):
        args = (mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], np.ascontiguousarray(y[:, c]))
        om, oc, ofe = rxoracle.lgssm_bp(*args)[:3] if key[1] == key[0] else rxoracle.lgssm_kalman_rts(*args)
        sd = np.sqrt(np.einsum("tii->ti", oc))
        mean_rel = float(np.max(np.abs(mean[c] - om) / sd))
        cov_rel = float(np.max(np.abs(cov[c] - oc) / np.max(np.abs(oc), axis=(1, 2), keepdims=True)))
        fe_rel = float(abs(fec[c] - ofe) / abs(ofe))
        print(f"{key} {C}x{T} K={stride} chain {c}: mean {mean_rel:.2e} cov {cov_rel:.2e} fe {fe_rel:.2e}")
        assert mean_rel < 1e-6 and cov_rel < 1e-6 and fe_rel < 1e-8, (mean_rel, cov_rel, fe_rel)


@pytest.mark.parametrize("value", ["0", "2", "4", "3", "-1", "x", "1x", ""])
def test_bad_value_is_refused_at_creation(value):
    """1 and unset are the two arms; anything else — the shipped depth spelled out included — is an error, not a silent default"""
    mdl = workloads.c1_model()
    with _Env(RXHIP_TEST_HOOKS="1", RXHIP_ONE_PASS="1", RXHIP_Y_RING=value):
        with pytest.raises(rxhip.RxHipError, match="RXHIP_Y_RING"):
            _engine(mdl, 37, 64, 2).close()

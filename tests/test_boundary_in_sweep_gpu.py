"""The boundary recursion inside the reverse-filter sweep (boundary_in_sweep in k_backward_sh_rev): every wave of the sweep
computes the filtered mean at its segment start and the backward message at its segment end itself, so the schedule has no
k_boundary_scan_tab launch.  RXHIP_BOUNDARY_KERNEL=1 keeps that launch; both arms call the same step functions in the same order, so
posteriors and free energy must agree bit for bit.

Shapes: `segments=` is a request — the engine takes L = ⌈(T − 1)/S⌉ and then S = ⌈(T − 1)/L⌉, so no segment is ever empty and
64 × 1030 with 128 requested runs 115 segments of 9 steps (64 × 1025 is the shape with exactly 128 segments, of 8 steps).  Either is
many times the prologue's ring of 8 segments and its staging chunk; 5 and 2 segments are shorter than the ring, 1 has no recursion."""
import os

import numpy as np
import pytest

import rxhip
import rxoracle
from rxhip import workloads

pytestmark = pytest.mark.gpu

# Seeds: most of workloads.random_model's draws (A = 0.95 · orthogonal) amplify the reverse filter beyond its bound and take the records
# schedule, which is not the code under test.  4 and 20 are the first seeds whose model the numpy restatement of the stride choice
# (tests/reverse_filter_ref.choose_stride) admits at every shape below; a case whose engine disagrees skips loudly.
MODELS = {
    (4, 4): workloads.c1_model,
    (2, 2): lambda: workloads.random_model(2, 2, 4),
    (3, 2): lambda: workloads.random_model(3, 2, 20),
}
#         chains, T, segments asked for, segments the engine takes
SHAPES = [(64, 37, 1, 1), (64, 37, 2, 2), (128, 203, 5, 5), (64, 1030, 128, 115), (64, 1025, 128, 128)]
ORACLE_SHAPES = [(128, 203, 5), (64, 1030, 128)]


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

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


_cache = {}


def _run(key, C, T, S, kernel):
    """(stride, segments, mean, cov, fe per chain, fe) of one arm; computed once per (model, shape, arm) and shared, never modified."""
    k = (key, C, T, S, kernel)
    if k not in _cache:
        mdl = MODELS[key]()
        y = workloads.generate_batch(mdl, T, C, seed0=17)
        with _Env(RXHIP_TEST_HOOKS="1", RXHIP_ONE_PASS="1", RXHIP_BOUNDARY_KERNEL="1" if kernel else "0"):
            with _engine(mdl, T, C, S) as eng:
                K, seg = eng.mean_checkpoint_stride(), eng.schedule()["segments"]
                eng.set_data(y)
                eng.run(iterations=1, free_energy=True)
                _cache[k] = (K, seg, y) + _results(eng, C)
    return _cache[k]


@pytest.mark.parametrize("key", list(MODELS), ids=lambda k: f"d{k[0]}dy{k[1]}")
@pytest.mark.parametrize("C,T,S,S_engine", SHAPES, ids=lambda v: str(v))
def test_bit_identical_to_the_scan_kernel(key, C, T, S, S_engine):
    K, seg, _, mean, cov, fec, fe = _run(key, C, T, S, kernel=False)
    if K == 0:
        pytest.skip(f"model {key}: no admissible checkpoint stride at T = {T}, S = {S}: the reverse-filter schedule is not taken")
    assert seg == S_engine
    K1, seg1, _, mean1, cov1, fec1, fe1 = _run(key, C, T, S, kernel=True)
    assert (K1, seg1) == (K, seg)
    assert np.array_equal(mean, mean1)
    assert np.array_equal(cov, cov1)
    assert np.array_equal(fec, fec1)
    assert np.array_equal(fe, fe1)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(fec))


@pytest.mark.parametrize("key", list(MODELS), ids=lambda k: f"d{k[0]}dy{k[1]}")
@pytest.mark.parametrize("C,T,S", ORACLE_SHAPES, ids=lambda v: str(v))
def test_oracle_parity(key, C, T, S):
    """First and last chain against the CPU oracle, with the measures and bounds of the benchmark's parity check.

    The oracle is rxoracle.lgssm_bp where it is one: at dy = d.  At dy < d the reference schedule it restates converts the singular
    precision B'Q⁻¹B to a covariance on the backward edge (tests/test_oracle.py: it raises or, where the factorisation happens to go
    through, returns posteriors that are wrong — on the (3, 2) model here lgssm_bp and the textbook smoother differ by 6.9e-2 sd in the
    mean, 8.3e-3 in the covariance and 1.9e-5 in the free energy, on the CPU alone).  There the checker is rxoracle.lgssm_kalman_rts,
    as in test_random_shapes_gpu.py and the benchmark's own parity check for chains it cannot give to lgssm_bp; same measures, same bounds."""
    K, _, y, mean, cov, fec, _ = _run(key, C, T, S, kernel=False)
    if K == 0:
        pytest.skip(f"model {key}: the reverse-filter schedule is not taken")
    mdl = MODELS[key]()
    for c in (0, C - 1):
        args = (mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], np.ascontiguousarray(y[:, c]))
        om, oc, ofe = rxoracle.lgssm_bp(*args)[:3] if key[1] == key[0] else rxoracle.lgssm_kalman_rts(*args)
        sd = np.sqrt(np.einsum("tii->ti", oc))
        mean_rel = float(np.max(np.abs(mean[c] - om) / sd))
        cov_rel = float(np.max(np.abs(cov[c] - oc) / np.max(np.abs(oc), axis=(1, 2), keepdims=True)))
        fe_rel = float(abs(fec[c] - ofe) / abs(ofe))
        print(f"{key} {C}x{T} chain {c}: mean {mean_rel:.2e} cov {cov_rel:.2e} fe {fe_rel:.2e}")
        assert mean_rel < 1e-6 and cov_rel < 1e-6 and fe_rel < 1e-8, (mean_rel, cov_rel, fe_rel)


def test_no_stale_boundary():
    """A second run on other data equals a fresh engine on that data: no wave reads the boundary records of the run before."""
    mdl = workloads.c1_model()
    C, T, S = 128, 203, 5
    ya = workloads.generate_batch(mdl, T, C, seed0=101)
    K, _, yb, mean, cov, fec, fe = _run((4, 4), C, T, S, kernel=False)   # the fresh engine on B
    assert K > 0
    with _Env(RXHIP_TEST_HOOKS="1", RXHIP_ONE_PASS="1", RXHIP_BOUNDARY_KERNEL="0"):
        with _engine(mdl, T, C, S) as eng:
            eng.set_data(ya)
            eng.run(iterations=1, free_energy=True)
            ma = _results(eng, C)[0]
            eng.set_data(yb)
            eng.run(iterations=1, free_energy=True)
            m2, c2, f2, t2 = _results(eng, C)
    assert not np.array_equal(ma, mean)
    assert np.array_equal(m2, mean) and np.array_equal(c2, cov) and np.array_equal(f2, fec) and np.array_equal(t2, fe)

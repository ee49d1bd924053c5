"""GPU tests of the edges of the lane path of the multivariate mixture engine (d ≤ 4, csrc/mvgmm_kernels.hpp: k_mvg_init, k_mvg_pass,
k_mvg_reduce, k_mvg_update), beside the parity cases of tests/test_mvgmm_gpu.py.

Every case is one of mvgmm_ref.CASES (shown to be well conditioned by tests/test_mvgmm_ref_cpu.py) and is held at every iteration to the
contract mvgmm_ref.hold against the NumPy restatement, and against the C oracle below N = 1e4 (at the grid-stride size the oracle's
sequential sums are themselves 1.0e-7 posterior sd off the restatement in the means; see tests/test_mvgmm_ref_cpu.py)."""
import numpy as np
import pytest

import rxhip

import mvgmm_ref
from mvgmm_ref import CASES, Case, hold
from test_mvgmm_gpu import run_engine

pytestmark = pytest.mark.gpu

# k_mvg_pass runs workgroups of WG lanes, a point per lane, in a grid-stride loop over at most GRID_CAP workgroups (rxhip_mvgmm_create:
# nb = (N + 255) / 256, capped at 1024); the component tile KT is 4, 8 or 16 (mvg_kt), K ≤ KT components are real, the rest padding
WG, GRID_CAP = 256, 1024
assert (WG, GRID_CAP) == (mvgmm_ref.LANE_WG, mvgmm_ref.LANE_CAP)


def check(c, what, components=None):
    """runs the engine on the case and holds it to both references; returns the engine's result and the restatement's"""
    y, pri, init, ref = mvgmm_ref.case(c)
    got = run_engine(y, pri, init, c.iters)
    hold(got, ref, f"{what} vs restatement {tuple(c[:4])}", components)
    if c.N < 10 ** 4:
        hold(got, mvgmm_ref.oracle(c), f"{what} vs oracle {tuple(c[:4])}", components)
    return got, ref


@pytest.mark.parametrize("d,K,N,iters", [c[:4] for c in CASES["lane_instances"]])
def test_unvisited_instantiations(d, K, N, iters):
    """MVG_DISPATCH builds ten (D, KT); the parity cases launch six.  These reach k_mvg_{init,pass,update}<1,8>, <1,16>, <2,8> and <3,4>."""
    check(Case(d, K, N, iters), "instance")


def test_soft_responsibilities():
    """ring radius 6: the responsibilities are genuinely soft, so the softmax of k_mvg_pass is exercised away from 0/1 (KT = 8, K = 5)"""
    (c,) = CASES["lane_soft"]
    _, ref = check(c, "soft")
    assert np.sum((ref["resp"] > 0.05) & (ref["resp"] < 0.95)) > 10


@pytest.mark.parametrize("d,K,N", [c[:3] for c in CASES["lane_sizes"]])
def test_sizes_around_a_wavefront_and_a_workgroup(d, K, N):
    """N = 1, 63, 65 (a wavefront is 64 lanes: idle lanes enter wave_sum with zeros), 255, 256, 257 (a workgroup is WG: one full, one with a
    single point) at <4,4> and <3,8>; N = 1 at <2,4> with two of four components real"""
    (c,) = [c for c in CASES["lane_sizes"] if c[:3] == (d, K, N)]
    check(c, "size")


@pytest.mark.parametrize("d,K", [c[:2] for c in CASES["lane_stride"]])
def test_grid_stride(d, K):
    """N = GRID_CAP·WG + WG + 37: the grid-stride loop of k_mvg_pass<1,4> and k_mvg_pass<4,8> runs a second time — in full in workgroup 0,
    ragged (37 lanes) in workgroup 1, not at all in the others — and k_mvg_reduce sums GRID_CAP partials in four rounds of 256.  With the
    responsibilities materialised, `resp + i·K` is written for i beyond the first round as well."""
    (c,) = [c for c in CASES["lane_stride"] if c[:2] == (d, K)]
    assert c.N == GRID_CAP * WG + WG + 37
    check(c, "grid stride")


@pytest.mark.parametrize("K", [c.K for c in CASES["lane_padding"]])
def test_responsibilities_with_padding_components(K):
    """K = 3, 5, 9 in tiles of KT = 4, 8, 16: a row of the responsibilities has K entries (`r = p.resp + i * p.K`), a lane's statistics KT"""
    (c,) = [c for c in CASES["lane_padding"] if c.K == K]
    got, _ = check(c, "padding")
    assert got["resp"].shape == (c.N, K)
    assert np.max(np.abs(got["resp"].sum(axis=1) - 1.0)) < 1e-12


def test_starved_component():
    """the last component's prior and initial mean sit at 1e3 in every coordinate: every point's responsibility for it underflows, it keeps its
    prior (cov = S0 = 1e6·I next to the others' ≈ 0.1) — the two populated components hold the contract all the same"""
    (c,) = CASES["lane_starved"]
    _, pri, _, _ = mvgmm_ref.case(c)
    got, ref = check(c, "starved", components=[0, 1])
    assert got["nu"][-1, 2] - pri[2][2] < 1e-12 and ref["nu"][-1, 2] - pri[2][2] < 1e-12
    assert np.min(ref["nu"][-1, :2] - pri[2][:2]) > 50


BITS = Case(4, 8, 3000, 4)


def _bits(r):
    return r["raw"], r["fe"], r["resp"]


def test_determinism():
    """two runs of one engine and a fresh engine: the same bits in history, free energy and responsibilities (no floating-point atomics,
    fixed-shape reductions)"""
    y, pri, init, _ = mvgmm_ref.case(BITS)
    runs = []
    with rxhip.MvGMMEngine(BITS.N, *pri, *init, materialize_responsibilities=True) as eng:
        eng.set_data(y)
        for _ in range(2):
            eng.run(BITS.iters, True)
            runs.append((eng.history()["raw"].copy(), eng.free_energy().copy(), eng.responsibilities().copy()))
    runs.append(_bits(run_engine(y, pri, init, BITS.iters)))
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))


def test_split_phase_equals_run():
    """begin_run + (accumulate, update) × iterations — the multi-GPU split — equals run bit for bit; the statistics are KT·STAT + 1 numbers"""
    y, pri, init, _ = mvgmm_ref.case(BITS)
    d, K = BITS.d, BITS.K
    whole = _bits(run_engine(y, pri, init, BITS.iters))
    with rxhip.MvGMMEngine(BITS.N, *pri, *init, materialize_responsibilities=True) as eng:
        eng.set_data(y)
        eng.begin_run(BITS.iters)
        for _ in range(BITS.iters):
            eng.accumulate()
            eng.update(True)
        assert eng.statistics_device()[1] == K * (1 + d + d * (d + 1) // 2) + 1   # KT = K = 8 here
        split = (eng.history()["raw"], eng.free_energy(), eng.responsibilities())
    assert all(np.array_equal(a, b) for a, b in zip(whole, split))

"""The engine pool and the schedule hooks (csrc/lgssm_plan.hpp ScheduleHooks): a parked engine is handed out again only to a creation with the
same hooks.  RXHIP_BOUNDARY_KERNEL selects between two launch sequences of the same engine shape and was not part of the pool key while the
run re-read it; now every hook is fixed at creation, so the key has to tell the two engines apart.  Shape: the one at which
tests/test_boundary_in_sweep_gpu.py asserts an admissible stride (128 chains, T = 203, 5 segments, one-pass schedule)."""
import os

import pytest

import rxhip
from rxhip import workloads

pytestmark = pytest.mark.gpu

C, T, S = 128, 203, 5


def _engine(mdl):
    return rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C, segments=S, device=0)


@pytest.mark.parametrize("first, second, launches", [("0", "1", 1), ("1", "0", 0)])
def test_pool_does_not_hand_back_the_other_schedule(monkeypatch, first, second, launches):
    mdl = workloads.c1_model()
    y = workloads.generate_batch(mdl, T, C, seed0=5)
    monkeypatch.setenv("RXHIP_ONE_PASS", "1")
    rxhip.lib().rxhip_release_cached_memory()   # no parked engine of an earlier test
    monkeypatch.setenv("RXHIP_BOUNDARY_KERNEL", first)
    with _engine(mdl) as eng:
        assert eng.mean_checkpoint_stride() > 0   # the reverse-filter schedule: the only one with the boundary recursion inside the sweep
        eng.set_data(y)
        eng.run(iterations=1, free_energy=True)
    # destroyed without profiling and without an error: parked in the pool
    monkeypatch.setenv("RXHIP_BOUNDARY_KERNEL", second)
    with _engine(mdl) as eng:
        eng.set_profiling(True)
        eng.set_data(y)
        eng.run(iterations=1, free_energy=True)
        assert eng.kernel_times()["k_boundary_scan"]["launches"] == launches

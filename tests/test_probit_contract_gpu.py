"""The probit state-space engine (include/rxhip.h rxhip_probit_desc, csrc/probit_kernels.hpp) held to the project's contract across its parameter
range, against tests/probit_ref.py run_messages — which tests/test_probit_contract_cpu.py pins to a 60-digit restatement at 100× inside these
bounds at every point of the grid.  Per element, per iteration and per series: posterior means within 1e-6 posterior standard deviations (the
reference's own variance), variances within 1e-6 relative, free energy within 1e-8·max(1, |F_ref|) — the floor of 1 because at m0 = +40, y ≡ 1 the
true free energy is ~1e-19 and a pure relative bound means nothing there.  Then the launch arithmetic: every cubature order, batch widths around
the 64-lane sweep and the 256-lane energy / reduction blocks, chain lengths around the energy chunk, the longest chunk; and what needs no oracle:
mirror symmetry, position in the batch, the life of one handle."""
import functools
import importlib.util
import os
import time

import numpy as np
import pytest

import probit_mp
import probit_ref as R
import rxhip
from rxhip import _lib
from test_probit_gpu import _fe_per_series_and_iteration

pytestmark = pytest.mark.gpu

GRID = probit_mp.GRID   # (a, q, v0, m0, c)
T, ITERS = 20, 5        # T = 20: one full chunk of 16 Probit energies and a ragged one

_worst = {"mean": (0.0, None), "var": (0.0, None), "fe": (0.0, None)}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """after the module: the worst error per quantity that `_hold` / `_hold_fe` measured (-s shows it; DESIGN.md §3.5a quotes it)"""
    yield
    for q, (v, what) in _worst.items():
        if what is not None:
            print(f"\nworst {q}: {v:.3e} at {what}")


def _note(q, v, what):
    if v > _worst[q][0]:
        _worst[q] = (v, what)


def _hold(mean, var, ref_mean, ref_var, what=""):
    assert mean.shape == ref_mean.shape and var.shape == ref_var.shape, what
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)), what
    em = float(np.max(np.abs(mean - ref_mean) / np.sqrt(ref_var)))
    ev = float(np.max(np.abs(var - ref_var) / ref_var))
    _note("mean", em, what)
    _note("var", ev, what)
    assert em < 1e-6 and ev < 1e-6, (what, em, ev)


def _hold_fe(fe, ref, what=""):
    fe, ref = np.asarray(fe), np.asarray(ref)
    assert fe.shape == ref.shape and np.all(np.isfinite(fe)), what
    ef = float(np.max(np.abs(fe - ref) / np.maximum(1.0, np.abs(ref))))
    _note("fe", ef, what)
    assert ef < 1e-8, (what, ef)


def _make(T, model, C, n_gh=32):
    a, c, q, m0, v0 = model
    return lambda: rxhip.ProbitEngine(T, a, c, q, m0, v0, n_series=C, n_gh=n_gh)


def _engine(model, y, iters, want_fe=True, layout="time_chain", n_gh=32):
    """one fresh engine: mean, var [T+1][series], and with want_fe the per-iteration totals and the per-series values of the last iteration"""
    with _make(y.shape[0], model, y.shape[1], n_gh)() as eng:
        eng.set_data(y if layout == "time_chain" else np.ascontiguousarray(y.T), layout=layout)
        eng.run(iters, want_fe)
        mean, var = eng.marginals(layout=layout)
        fe = (eng.free_energy(), eng.free_energy_per_chain()) if want_fe else (None, None)
    if layout == "chain_time":
        mean, var = np.ascontiguousarray(mean.T), np.ascontiguousarray(var.T)
    return mean, var, fe[0], fe[1]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _ref(y, model, iters, n_gh=32):
    a, c, q, m0, v0 = model
    return R.run_batch(y, a, c, q, m0, v0, iters, n_gh)


# ---------------------------------------------------------------------------------------------------------------- the parameter grid
def test_the_grid_is_the_whole_grid():
    assert len(GRID) == 300 and len(set(GRID)) == 300 and {p[0] for p in GRID} == set(probit_mp.GRID_A)


@pytest.mark.parametrize("a", probit_mp.GRID_A)
def test_grid(a):
    """60 points per value of a, six series each (probit_ref.contract_series), the reference computed once per point.  The free energy of every
    iteration and series is read as tests/test_probit_gpu.py `_fe_per_series_and_iteration` does — the ABI returns per-series values of the LAST
    iteration, so one fresh engine per iteration count — and the per-iteration totals of the 5-iteration engine are held to the reference's sum."""
    y = R.contract_series(T)
    points = [p for p in GRID if p[0] == a]
    assert len(points) == 60
    for i, (_, q, v0, m0, c) in enumerate(points):
        model, what = (a, c, q, m0, v0), f"a={a:g} q={q:g} v0={v0:g} m0={m0:g} c={c:g}"
        rm, rv, rfe = _ref(y, model, ITERS)
        assert np.all(np.isfinite(rm)) and np.all(rv > 0) and np.all(np.isfinite(rfe)), what   # the reference alone, before the engine is consulted
        layout = "time_chain" if i % 2 == 0 else "chain_time"
        mean, var, fe_tot, fe_last = _engine(model, y, ITERS, layout=layout)
        _hold(mean, var, rm, rv, what)
        fe = _fe_per_series_and_iteration(_make(T, model, y.shape[1]), y, ITERS, layout)
        _hold_fe(fe, rfe, what + " per iteration and series")
        assert np.array_equal(fe[-1], fe_last), what
        _hold_fe(fe_tot, rfe.sum(axis=1), what + " totals")
        assert np.max(np.abs(fe[:, 5])) < 1e-12, (what, fe[:, 5])   # nothing observed: the free energy is exactly 0


# ---------------------------------------------------------------------------------------------------------------- cubature orders
ORDER_MODEL = (0.9, 0.2, 0.3, -0.5, 2.0)   # (a, c, q, m0, v0)
ORDER_Y = np.array([[1.0, 0.0, np.nan], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])


@pytest.mark.parametrize("n_gh", range(1, 33))
def test_cubature_orders(n_gh):
    """the library's own Gauss–Hermite table (Newton iteration on the host) at every order it accepts, against numpy's in the reference"""
    rm, rv, rfe = _ref(ORDER_Y, ORDER_MODEL, 3, n_gh)
    mean, var, fe_tot, fe_last = _engine(ORDER_MODEL, ORDER_Y, 3, n_gh=n_gh)
    _hold(mean, var, rm, rv, f"n_gh={n_gh}")
    _hold_fe(fe_last, rfe[-1], f"n_gh={n_gh} per series")
    _hold_fe(fe_tot, rfe.sum(axis=1), f"n_gh={n_gh} totals")


# ---------------------------------------------------------------------------------------------------------------- batch widths
WIDTH_MODEL, WIDTH_ITERS, WIDTH_GH, WIDTH_T = (0.8, -0.1, 0.4, 0.3, 1.5), 2, 8, 3


@functools.lru_cache(maxsize=None)
def _wide():
    """513 series of 3 steps, a tenth of the observations missing, and the reference on them"""
    rng = np.random.default_rng(513)
    y = (rng.random((WIDTH_T, 513)) < 0.5).astype(np.float64)
    y[rng.random((WIDTH_T, 513)) < 0.1] = np.nan
    y.setflags(write=False)
    return y, _ref(y, WIDTH_MODEL, WIDTH_ITERS, WIDTH_GH)


@functools.lru_cache(maxsize=None)
def _alone(s):
    return _engine(WIDTH_MODEL, np.ascontiguousarray(_wide()[0][:, s:s + 1]), WIDTH_ITERS, n_gh=WIDTH_GH)


@pytest.mark.parametrize("layout", ["time_chain", "chain_time"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 256, 257, 513])
def test_batch_widths(C, layout):
    """Around the 64 lanes of a sweep wavefront and the 256 lanes of an energy block and of the reduction's stride loop (C > 256: a second energy
    block, a second round of the stride loop).  A series' arithmetic does not depend on its place: series 0, 255, 256 and C − 1 have the bits of
    the same series run alone."""
    y_all, (rm, rv, rfe) = _wide()
    y = np.ascontiguousarray(y_all[:, :C])
    mean, var, fe_tot, fe_last = _engine(WIDTH_MODEL, y, WIDTH_ITERS, layout=layout, n_gh=WIDTH_GH)
    what = f"C={C} {layout}"
    _hold(mean, var, rm[:, :C], rv[:, :C], what)
    _hold_fe(fe_last, rfe[-1, :C], what + " per series")
    _hold_fe(fe_tot, rfe[:, :C].sum(axis=1), what + " totals")
    for s in sorted({0, 255, 256, C - 1}):
        if s < C:
            am, av, _, af = _alone(s)
            assert np.array_equal(mean[:, s], am[:, 0]) and np.array_equal(var[:, s], av[:, 0]) and fe_last[s] == af[0], (what, s)


# ---------------------------------------------------------------------------------------------------------------- chunk edges
@pytest.mark.parametrize("T_", [15, 16, 17, 32, 33])
def test_chunk_edges(T_):
    """chain lengths one below, at and one above a multiple of the 16 steps per partial sum of the Probit energies"""
    model = (0.95, 0.05, 0.2, -0.4, 3.0)
    y = np.ascontiguousarray(R.contract_series(T_)[:, :4])
    rm, rv, rfe = _ref(y, model, 4)
    mean, var, fe_tot, fe_last = _engine(model, y, 4)
    _hold(mean, var, rm, rv, f"T={T_}")
    _hold_fe(fe_last, rfe[-1], f"T={T_} per series")
    _hold_fe(fe_tot, rfe.sum(axis=1), f"T={T_} totals")


# ---------------------------------------------------------------------------------------------------------------- mirror symmetry
@pytest.mark.parametrize("m0", [0.7, 8.0, 40.0])
def test_mirror_symmetry(m0):
    """(y, m0, c) → (1 − y, −m0, −c) is the same model for −x.  Every operation of a sweep is odd or even under the flip and none is reordered, so
    the means are negated and the variances kept; the free energy differs only by the order of a 32-term Gauss–Hermite sum whose terms all have
    one sign (~32 ε), held to 1e-10·max(1, |F|), as the variances are to 1e-10 relative.  At m0 = 40 the all-ones series has its site precisions
    at the 1e-12 floor (upper tail) and its mirror sits in the lower tail, where Φ underflows."""
    a, c, q, v0 = 0.9, 0.2, 0.1, 0.5
    y = R.contract_series(T)
    mean, var, fe_tot, fe_last = _engine((a, c, q, m0, v0), y, ITERS)
    mean2, var2, fe_tot2, fe_last2 = _engine((a, -c, q, -m0, v0), 1.0 - y, ITERS)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(np.isfinite(fe_tot)) and np.all(np.isfinite(fe_last))
    assert np.array_equal(mean2, -mean)
    ev = float(np.max(np.abs(var2 - var) / var))
    ef = max(float(np.max(np.abs(f2 - f1) / np.maximum(1.0, np.abs(f1)))) for f1, f2 in ((fe_last, fe_last2), (fe_tot, fe_tot2)))
    print(f"m0={m0:g}: mirrored var rel {ev:.3e}, fe {ef:.3e}")
    assert ev < 1e-10 and ef < 1e-10, (m0, ev, ef)


# ---------------------------------------------------------------------------------------------------------------- one handle's life
def _snapshot(eng, want_fe=True):
    return eng.marginals() + ((eng.free_energy(), eng.free_energy_per_chain()) if want_fe else ())


def test_lifecycle_on_one_handle():
    """More iterations than the 16 the handle reserves at creation (its free-energy buffers grow, twice), fewer than before (stale rows stay behind
    the ones read), a run without the free energy, other data on the live handle: every result equals a fresh engine's, bit for bit."""
    model = (1.0, 0.1, 0.01, 0.0, 100.0)
    y = R.contract_series(T)
    y2 = np.ascontiguousarray((1.0 - y)[::-1])
    fresh = lambda data, n, fe=True: tuple(x for x in _engine(model, data, n, want_fe=fe) if x is not None)
    with _make(T, model, 6)() as eng:
        eng.set_data(y)
        eng.run(20, True)
        first = _snapshot(eng)
        assert _same(first, fresh(y, 20)) and first[2].shape == (20,)
        eng.run(3, True)
        assert _same(_snapshot(eng), fresh(y, 3)) and eng.free_energy().shape == (3,)
        eng.run(40, False)
        without = _snapshot(eng, False)
        assert _same(without, fresh(y, 40, False))
        for get in (eng.free_energy, eng.free_energy_per_chain):
            with pytest.raises(rxhip.RxHipError) as ei:
                get()
            assert ei.value.status == _lib.ERR_STATE and "not requested" in str(ei.value)
        eng.run(40, True)
        forty = _snapshot(eng)
        assert _same(forty, fresh(y, 40)) and forty[2].shape == (40,)
        assert _same(forty[:2], without)   # the free energy does not touch the posteriors
        eng.set_data(y2)
        eng.run(20, True)
        last = _snapshot(eng)
        assert _same(last, fresh(y2, 20)) and eng.free_energy().shape == (20,)
    for (mean, var, fe_tot, fe_last), data, what in ((first, y, "first run"), (last, y2, "after the second set_data")):
        rm, rv, rfe = _ref(data, model, 20)
        _hold(mean, var, rm, rv, what)
        _hold_fe(fe_last, rfe[-1], what + " per series")
        _hold_fe(fe_tot, rfe.sum(axis=1), what + " totals")


# ---------------------------------------------------------------------------------------------------------------- the longest chunk
def test_long_chain():
    """T = 524 289, one series, one iteration, 4-point rule: the smallest length at which the energy kernel takes 17 steps per partial sum instead
    of 16 (30 841 chunks in the grid's second dimension).  The reference is the fixture tests/golden/probit_long.npz (make_probit_long_golden.py:
    the Python restatement takes about a minute); the observations are regenerated from its seed.  Each of the engine's two sweeps is 5·10⁵
    dependent steps in one lane: measured 1.3 s on an MI355X for engine creation, set_data, run and read-back (printed below)."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_probit_long_golden", os.path.join(here, "make_probit_long_golden.py"))
    gold_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gold_mod)
    g = np.load(os.path.join(here, "probit_long.npz"))
    T_, n_gh, iters = int(g["T"]), int(g["n_gh"]), int(g["iterations"])
    assert T_ == 524289 and (T_ + 32767) // 32768 == 17 and (T_ - 1 + 32767) // 32768 == 16
    y = gold_mod.observations(T_, int(g["seed"]))[:, None]
    model = tuple(float(g[k]) for k in ("a", "c", "q", "m0", "v0"))
    t0 = time.perf_counter()
    mean, var, fe_tot, fe_last = _engine(model, y, iters, n_gh=n_gh)
    print(f"long chain: {time.perf_counter() - t0:.2f} s")
    k = g["steps"]
    assert mean.shape == (T_ + 1, 1) and k[-1] == T_ and k[0] == 0 and len(k) == len(g["mean"]) == 576
    _hold(mean[k, 0], var[k, 0], g["mean"], g["var"], "long chain")
    assert np.all(np.isfinite(mean)) and np.all(var > 0)
    _hold_fe(fe_tot, g["fe"], "long chain")
    assert fe_last[0] == fe_tot[-1]

"""The HGF engine (include/rxhip.h rxhip_hgf_desc, csrc/hgf_kernels.hpp) held to the project's contract across its parameter range, against the
C oracle — which tests/test_hgf_ref_cpu.py pins to a 60-digit restatement at 100× inside these bounds.  Per element: posterior means within 1e-6
posterior standard deviations (the reference's own variance), variances within 1e-6 relative, free energy within 1e-8 relative per iteration and
per series.  Then what needs no oracle: position in the wavefront, scale equivariance, the life of one handle, non-finite input, refusals."""
import functools

import numpy as np
import pytest

import hgf_ref as R
import rxhip
import rxoracle
from rxhip import _lib
from test_hgf_gpu import hgf_series

pytestmark = pytest.mark.gpu

T, ITERS, N_GH, S = 40, 18, 31, 5   # five series: one full wavefront of four 16-lane rows and a ragged one
FIRST_SEED = 11
NAMES = ("zm", "zv", "xm", "xv")
EXCLUDED = ()   # grid cases that tests/test_hgf_ref_cpu.py lists as ill-posed: none (its list holds n_gh = 3 only; the grid runs GH-31)

_worst = {"mean": (0.0, None), "var": (0.0, None), "fe": (0.0, None)}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """after the module: the worst error per quantity that `_hold` / `_hold_fe` measured (-s shows it; DESIGN.md's HGF table quotes it)"""
    yield
    for q, (v, what) in _worst.items():
        if what is not None:
            print(f"\nworst {q}: {v:.3e} at {what}")


def _note(q, v, what):
    if v > _worst[q][0]:
        _worst[q] = (v, what)


def _hold(got, ref, what=""):
    """got, ref: (zm, zv, xm, xv), arrays of one shape — every element at the contract"""
    for a in got:
        assert np.all(np.isfinite(a)), what
    em = max(float(np.max(np.abs(got[i] - ref[i]) / np.sqrt(ref[i + 1]))) for i in (0, 2))
    ev = max(float(np.max(np.abs(got[i] - ref[i]) / ref[i])) for i in (1, 3))
    print(f"{what}: mean err {em:.3e} sd, var rel {ev:.3e}")
    _note("mean", em, what)
    _note("var", ev, what)
    assert em < 1e-6 and ev < 1e-6, (what, em, ev)


def _hold_fe(fe, ref, what=""):
    assert np.all(np.abs(ref) >= 0.1), (what, float(np.min(np.abs(ref))))   # (a condition on the reference: the relative bound means something)
    ef = float(np.max(np.abs(fe - ref) / np.abs(ref)))
    print(f"{what}: fe rel {ef:.3e}")
    _note("fe", ef, what)
    assert np.all(np.isfinite(fe)) and ef < 1e-8, (what, ef)


def _hold_fe_total(fe_tot, ref_fe, what=""):
    """The per-iteration totals against the sum over the series.  The series' values differ in sign, so the sum can cancel (to 0.05 at one grid
    case): each series within 1e-8 relative puts the total within 1e-8 of Σ_series |reference|, which is the bound here."""
    ref, scale = ref_fe.sum(axis=1), np.abs(ref_fe).sum(axis=1)
    ef = float(np.max(np.abs(fe_tot - ref) / scale))
    print(f"{what}: fe totals rel {ef:.3e}")
    _note("fe", ef, what)
    assert fe_tot.shape == ref.shape and np.all(np.isfinite(fe_tot)) and ef < 1e-8, (what, ef)


@functools.lru_cache(maxsize=None)
def _reference(case, n=S, iters=ITERS, n_gh=N_GH, t=T, z0=(0.0, 5.0), x0=(0.0, 5.0)):
    """n series of the model's own generator at `case`, and the oracle on each: y [t][n], (zm, zv, xm, xv) each [t][n], fe [iters][n].
    Seeds FIRST_SEED, FIRST_SEED + 1, … in order; a seed is passed over (and printed) when the oracle refuses its series — the generated
    log-volatility walked out of the cubature range, which tests/test_hgf_gpu.py covers — or when some |free energy| of it is below 0.1."""
    k, w, zv, yv = case
    ys, outs, seed = [], [], FIRST_SEED
    while len(ys) < n:
        assert seed < FIRST_SEED + 4 * n, ("the grid is wrong, not the seeds", case)
        y = hgf_series(t, k, w, zv, yv, seed)[2]
        seed += 1
        try:
            o = rxoracle.hgf_filter(y, k, w, zv, yv, z0=z0, x0=x0, vmp_iters=iters, n_gh=n_gh)
        except RuntimeError as e:
            print(f"{case}: seed {seed - 1} passed over ({e})")
            continue
        if np.min(np.abs(o[4])) < 0.1:
            print(f"{case}: seed {seed - 1} passed over (|fe| {np.min(np.abs(o[4])):.3g} < 0.1)")
            continue
        ys.append(y)
        outs.append(o)
    y = np.stack(ys, axis=1)
    y.setflags(write=False)
    return y, tuple(np.stack([o[i] for o in outs], axis=1) for i in range(4)), np.stack([o[4] for o in outs], axis=1)


def _engine(case, y, iters, want_fe=True, layout="time_chain", **kw):
    """one fresh engine: posteriors [T][series], and with want_fe the per-iteration totals and the per-series values of the last iteration"""
    with rxhip.HGFEngine(y.shape[0], y.shape[1], *case, **kw) as eng:
        eng.set_data(y if layout == "time_chain" else np.ascontiguousarray(y.T), layout=layout)
        eng.run(iters, want_fe)
        post = eng.history(layout)
        fe = (eng.free_energy(), eng.free_energy_per_chain()) if want_fe else (None, None)
    if layout == "chain_time":
        post = tuple(np.ascontiguousarray(a.T) for a in post)
    return post, fe[0], fe[1]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- the parameter grid
def test_the_grid_is_the_whole_grid():
    assert len(R.GRID) == 112 and len(set(R.GRID)) == 112 and len(EXCLUDED) <= 10 and all(c in R.GRID for c in EXCLUDED)


@pytest.mark.parametrize("i", range(len(R.GRID)), ids=lambda i: "k%g_w%g_zv%g_yv%g" % R.GRID[i])
def test_grid(i):
    case = R.GRID[i]
    assert case not in EXCLUDED
    y, ref, ref_fe = _reference(case)
    assert all(np.all(np.isfinite(a)) for a in ref) and np.all(np.abs(ref_fe) >= 0.1)   # the reference alone, before the engine is consulted
    layout = "time_chain" if i % 2 == 0 else "chain_time"
    post, fe_tot, fe_last = _engine(case, y, ITERS, layout=layout)
    _hold(post, ref, f"{case} {layout}")
    _hold_fe(fe_last, ref_fe[-1], f"{case} per series")
    _hold_fe_total(fe_tot, ref_fe, f"{case} per iteration")


# ------------------------------------------------------------------------------------- free energy per (iteration, series)
FE_CASES = ((-1.5, -6.0, 1e-4, 1e2), R.CENTRE, (-0.3, 4.0, 1.0, 1e-6))   # a corner (the one the cancelling determinant hit hardest), the centre, a κ < 0


@pytest.mark.parametrize("case", FE_CASES, ids=lambda c: "k%g_w%g_zv%g_yv%g" % c)
def test_free_energy_per_series_and_iteration(case):
    """The ABI returns per-series values of the LAST iteration: one run per iteration count gives every (iteration, series).  A run of n iterations
    per observation is its own filter (the posteriors feed back), so the reference is the oracle at vmp_iters = n."""
    y = _reference(case)[0]
    got, ref = [], []
    for n in range(1, ITERS + 1):
        ref.append(np.array([rxoracle.hgf_filter(y[:, s], *case, vmp_iters=n, n_gh=N_GH)[4][-1] for s in range(S)]))
        got.append(_engine(case, y, n)[2])
    _hold_fe(np.array(got), np.array(ref), f"{case} n = 1 … {ITERS}")
    # inside one run: every iteration's total is the sum over the series (lanes 0 … 15 of a row, then the global accumulator)
    _, fe_tot, _ = _engine(case, y, ITERS)
    _hold_fe_total(fe_tot, _reference(case)[2], f"{case} totals")


@pytest.mark.parametrize("iters", [1, 16, 17, 33])
def test_iteration_counts(iters):
    """1: the pipelined loop body never runs, the epilogue alone evaluates the free energy; 16 | 17: the last lane-held iteration and the first
    one accumulated in global memory; 33: two passes beyond."""
    y, ref, ref_fe = _reference(R.CENTRE, iters=iters)
    post, fe_tot, fe_last = _engine(R.CENTRE, y, iters)
    _hold(post, ref, f"{iters} iterations")
    _hold_fe(fe_last, ref_fe[-1], f"{iters} iterations, per series")
    _hold_fe_total(fe_tot, ref_fe, f"{iters} iterations, per iteration")


# ---------------------------------------------------------------------------------------------------------------- cubature orders
@pytest.mark.parametrize("n_gh", [2, 3, 16, 17, 31, 32])
def test_cubature_orders(n_gh):
    y, ref, ref_fe = _reference(R.CENTRE, n_gh=n_gh)
    post, fe_tot, fe_last = _engine(R.CENTRE, y, ITERS, n_gh=n_gh)
    _hold(post, ref, f"GH-{n_gh}")
    _hold_fe(fe_last, ref_fe[-1], f"GH-{n_gh} per series")
    _hold_fe_total(fe_tot, ref_fe, f"GH-{n_gh} per iteration")


@pytest.mark.parametrize("want_fe", [True, False])
def test_one_point_rule_has_no_variance(want_fe):
    """n_gh = 1: q(zt) is a point, the oracle reports RXO_ERR_NONFINITE_FE — the engine the same class, not a posterior"""
    y = _reference(R.CENTRE)[0]
    with pytest.raises(RuntimeError, match="status 4"):
        rxoracle.hgf_filter(y[:, 0], *R.CENTRE, vmp_iters=3, n_gh=1, want_fe=want_fe)
    with pytest.raises(rxhip.RxHipError) as ei:
        _engine(R.CENTRE, y, 3, want_fe=want_fe, n_gh=1)
    assert ei.value.status == _lib.ERR_NONFINITE_FE and str(ei.value)


# ------------------------------------------------------------------------------------------------------- position in the wavefront
WAVE_CASE = (1.0, 0.0, 0.04, 0.01)


@functools.lru_cache(maxsize=None)
def _scaled_series():
    """nine series whose scales are decades apart: series s is multiplied by 10^(s mod 4 − 2); each alone in an S = 1 engine"""
    ys = [hgf_series(T, *WAVE_CASE, FIRST_SEED + s)[2] * 10.0 ** (s % 4 - 2) for s in range(9)]
    alone = [_engine(WAVE_CASE, y[:, None], ITERS) for y in ys]
    return ys, alone


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9])
def test_position_in_the_wavefront(n):
    """A series' arithmetic does not depend on the 16-lane row that owns it nor on its neighbours (the sums are row-local DPP, the free energy is
    accumulated per row and normalised per element): every series of a batch equals its run alone, bit for bit."""
    ys, alone = _scaled_series()
    post, _, fe_last = _engine(WAVE_CASE, np.stack(ys[:n], axis=1), ITERS)
    for s in range(n):
        for name, a, b in zip(NAMES, post, alone[s][0]):
            assert np.array_equal(a[:, s], b[:, 0]), (n, s, name)
        assert fe_last[s] == alone[s][2][0], (n, s)


# ---------------------------------------------------------------------------------------------------------------- scale equivariance
@pytest.mark.parametrize("s", [1e-6, 1e6])
@pytest.mark.parametrize("case", [R.CENTRE, (1.0, 0.0, 0.04, 0.01), (-1.5, -6.0, 1.0, 1e2), (2.0, 4.0, 1e-4, 1e2)], ids=lambda c: "k%g_w%g_zv%g_yv%g" % c)
def test_scale_equivariance(case, s):
    """y → s·y, y variance and x0 variance → s²·, x0 mean → s·, ω → ω + 2 ln s is the same model for x / s: q(z) is unchanged, the means of x scale
    by s and its variances by s².  The free energy is −log of a density of y, which the change of variable divides by s per observation: it GAINS
    ln s, being the mean over the observations.  (The oracle satisfies this at 1e±6 at 100× inside the contract: tests/test_hgf_ref_cpu.py.)"""
    k, w, zv, yv = case
    y = _reference(case)[0]
    x0 = (-0.2, 3.0)
    a, a_tot, a_last = _engine(case, y, ITERS, x0=x0)
    b, b_tot, b_last = _engine((k, w + 2.0 * np.log(s), zv, yv * s * s), y * s, ITERS, x0=(x0[0] * s, x0[1] * s * s))
    _hold((b[0], b[1], b[2] / s, b[3] / (s * s)), a, f"{case} scaled by {s:g}")
    ln_s = float(np.log(s))
    for got, base, shift, what in ((b_last, a_last, ln_s, "per series"), (b_tot, a_tot, S * ln_s, "per iteration")):
        ef = float(np.max(np.abs(got - (base + shift)) / np.minimum(np.abs(base), np.abs(base + shift))))   # relative to the smaller: the shift of ±13.8 buys no tolerance
        print(f"{case} scaled by {s:g}, {what}: fe rel {ef:.3e}")
        assert ef < 1e-8, (case, s, what, ef)


# ---------------------------------------------------------------------------------------------------------------- one handle's life
def _snapshot(eng, want_fe=True):
    return eng.history() + ((eng.free_energy(), eng.free_energy_per_chain()) if want_fe else ())


def test_lifecycle_on_one_handle():
    case = R.CENTRE
    y = _reference(case)[0]
    y2 = _reference((1.0, 0.0, 0.04, 0.01))[0]
    fresh = lambda data, n: _engine(case, data, n)
    flat = lambda r: r[0] + (r[1], r[2])
    with rxhip.HGFEngine(T, S, *case) as eng:
        eng.set_data(y)
        eng.run(20, True)
        first = _snapshot(eng)
        eng.run(20, True)
        assert _same(first, _snapshot(eng))                    # the same run twice
        assert _same(first, flat(fresh(y, 20)))
        eng.run(3, True)                                       # fewer: rows 3 … 19 of the accumulator are stale, only 0 … 2 are cleared and read
        assert _same(_snapshot(eng), flat(fresh(y, 3)))
        eng.run(40, True)                                      # more than ever before: the accumulator is reallocated
        assert _same(_snapshot(eng), flat(fresh(y, 40)))
        eng.set_data(y2)                                       # other data on the live engine
        eng.run(ITERS, True)
        assert _same(_snapshot(eng), flat(fresh(y2, ITERS)))
        assert eng.free_energy().shape == (ITERS,)


def test_run_without_free_energy():
    """The posteriors of run(n, False) hold the contract; free_energy() after it is RXHIP_ERR_STATE, as for every other engine of the library
    ("free energy was not requested in the last run") — not the values of an earlier run."""
    case = R.CENTRE
    y, ref, _ = _reference(case)
    with rxhip.HGFEngine(T, S, *case) as eng:
        eng.set_data(y)
        eng.run(ITERS, True)
        with_fe = eng.history()
        eng.run(ITERS, False)
        without = eng.history()
        for get in (eng.free_energy, eng.free_energy_per_chain):
            with pytest.raises(rxhip.RxHipError) as ei:
                get()
            assert ei.value.status == _lib.ERR_STATE and "not requested" in str(ei.value)
    _hold(without, ref, "run(n, False)")
    # (measured, not asserted: the two template instances of the kernel are compiled separately and the compiler is free to contract their
    # multiply-adds differently)
    print("run(n, False) bit-identical to run(n, True):", _same(with_fe, without),
          "; max difference in posterior sd:", max(float(np.max(np.abs(with_fe[i] - without[i]) / np.sqrt(with_fe[i + 1]))) for i in (0, 2)))


# ---------------------------------------------------------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_observation(bad):
    """One bad observation in one series of five.  The kernel's exponential clamps its argument and so swallows a NaN; what reports it is the
    check of the moments.  Neither run hands out posteriors with status OK, and the status is not sticky."""
    case = R.CENTRE
    y = _reference(case)[0]
    dirty = y.copy()
    dirty[7, 2] = bad
    with rxhip.HGFEngine(T, S, *case) as eng:
        for want_fe in (True, False):
            eng.set_data(dirty)
            with pytest.raises(rxhip.RxHipError) as ei:
                eng.run(ITERS, want_fe)
            assert ei.value.status == _lib.ERR_NONFINITE_FE and str(ei.value)
        eng.set_data(y)
        eng.run(ITERS, True)
        clean = _snapshot(eng)
    fresh = _engine(case, y, ITERS)
    assert _same(clean, fresh[0] + (fresh[1], fresh[2]))


# ---------------------------------------------------------------------------------------------------------------- refusals at creation
_GOOD = dict(kappa=1.0, omega=0.0, z_variance=0.04, y_variance=0.01, z0=(0.0, 5.0), x0=(0.0, 5.0), n_gh=31)


def _create(**kw):
    args = dict(_GOOD)
    args.update(kw)
    with pytest.raises(rxhip.RxHipError) as ei:
        rxhip.HGFEngine(4, 1, **args)
    return ei.value


@pytest.mark.parametrize("n_gh,status", [(0, _lib.ERR_BADARG), (33, _lib.ERR_UNSUPPORTED)])
def test_refused_cubature_order(n_gh, status):
    assert _create(n_gh=n_gh).status == status


@pytest.mark.parametrize("which", ["z_variance", "y_variance", "z0", "x0"])
@pytest.mark.parametrize("v", [0.0, -1.0, np.inf, np.nan])
def test_refused_variance(which, v):
    err = _create(**{which: (0.0, v) if which in ("z0", "x0") else v})
    if np.isinf(v):   # passed before: now a text names the field
        assert err.status == _lib.ERR_BADARG and (which if which.endswith("variance") else which + "_var") in str(err)
    else:
        assert err.status == _lib.ERR_NOT_POSDEF


@pytest.mark.parametrize("which", ["kappa", "omega", "z0", "x0"])
@pytest.mark.parametrize("v", [np.nan, np.inf, -np.inf])
def test_refused_non_finite_parameter(which, v):
    err = _create(**{which: (v, 5.0) if which in ("z0", "x0") else v})
    assert err.status == _lib.ERR_BADARG and (which + "_mean" if which in ("z0", "x0") else which) in str(err)


def test_a_refusal_leaves_the_library_usable():
    _create(kappa=np.nan)
    y, ref, _ = _reference(R.CENTRE)
    _hold(_engine(R.CENTRE, y, ITERS)[0], ref, "after a refusal")

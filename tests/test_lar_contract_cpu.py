"""The latent autoregressive engine's arithmetic held to a 50-digit restatement across its range, without a GPU: the double-precision restatement
tests/lar_ref.py — its dense form (numpy's inverse of the whole Λ) and, where T ≤ 300, its banded form, which walks the device's recursions in the
device's order — against tests/golden/lar_long.npz (tests/lar_mp.py at 50 digits, tests/golden/make_lar_long_golden.py) on every case of
lar_mp.GRID and lar_mp.SCAN.

The project's contract (lar_ref.contract_errors): state means within 1e-6 posterior standard deviations; (co)variances, θ and b within 1e-6
relative; a exact; the free energy within 1e-8·max(1, |F|) per iteration and per series.  This module holds the restatement to a TENTH of that
(lar_mp.TENTH), so that the device test, which holds the engine to the contract itself, has a decade to spare — the device has been seen up to 6×
away from the host build of the same arithmetic.  That rule is also what admits a case to the grid and what the envelope (lar_mp.ENVELOPE:
|m_i|/sd_i ≤ 1e8, cond Λ ≤ 1e8) was read from on the scan; the scan cases outside the envelope have their errors printed, not asserted.  The
50-digit restatement itself is checked here against its own independent form: the banded recursion against the `mp.matrix` inverse of the whole Λ
at 1e-40, on every case with T + p ≤ 48."""
import os

import numpy as np
import pytest

import lar_mp as MP
import lar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lar_long.npz")
SMALL = [s for s in MP.GRID + MP.SCAN if s.T + s.p <= 48]

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """after the module: the worst error per form and quantity, with its case (-s shows it; DESIGN.md §3.5c quotes it)"""
    yield
    for (who, q), (v, what) in sorted(_worst.items()):
        print(f"\nworst {who} {q}: {v:.3e} at {what}")


def _note(who, errs, what):
    for q, v in errs.items():
        if v > _worst.get((who, q), (-1.0, None))[0]:
            _worst[(who, q)] = (v, what)


@pytest.fixture(scope="module")
def golden():
    return MP.load(FIXTURE)


@pytest.fixture(scope="module")
def cases():
    """the inputs of every case, generated once"""
    return {s.name: MP.case(s) for s in MP.GRID + MP.SCAN}


def _restated(spec, case, banded):
    y, m, iters, share = case
    r = R.run_batch(y, **m, iterations=iters, share_parameters=share, banded=banded)
    return r, MP.pick(spec, r)


# ---- the fixture itself ------------------------------------------------------------------------------------------------------------------------------
def test_the_grid_is_the_whole_grid():
    names = [s.name for s in MP.GRID + MP.SCAN]
    assert len(MP.GRID) == 49 and len(MP.SCAN) == 47 and len(set(names)) == 96
    orders = [s for s in MP.GRID if s.name.startswith("orders")]
    assert [s.p for s in orders] == list(range(1, 9)) and all(s.T == 257 and s.iterations == 15 and s.missing == 0.1 for s in orders)
    assert [(s.T, s.p, s.C, s.iterations) for s in MP.GRID if s.name.startswith("long")] == [(4096, 1, 3, 2), (4096, 8, 3, 2)]
    assert sorted((s.p, s.T) for s in MP.GRID if s.name.startswith("boundary")) == sorted((p, T) for p in (5, 8) for T in (1, 2, p - 1, p, p + 1))
    assert {s.tau for s in MP.GRID} >= {1e-6, 1e-3, 1e3, 1e6} and {s.gamma for s in MP.GRID} >= {1e-3, 1e3, 1e6} and {s.theta for s in MP.GRID} >= {0.999, 1.0, 1.02, "last"}
    assert [(s.C, s.T, s.p, s.iterations) for s in MP.GRID if s.share] == [(65, 33, 3, 3), (70, 33, 3, 3)]
    assert all(2 <= s.C <= 3 for s in MP.GRID if not s.share) and all(s.C == 1 and s.T == 40 and s.missing == 0.0 for s in MP.SCAN)
    first = [s for s in MP.SCAN if s.iterations == 1]
    assert len(first) == 42 and [s.offset for s in MP.SCAN[42:]] == [1e2, 1e3, 1e4, 1e5, 1e6] and all(s.iterations == 3 and s.p == 2 for s in MP.SCAN[42:])
    assert {s.offset for s in first} == {10.0 ** k for k in range(2, 9)} and {(s.gamma, s.tau) for s in first} == {(1.0, 5.0), (1e4, 1e2), (1e6, 1e4)}


def test_fixture_matches_the_generators(golden, cases):
    """the inputs are regenerated from the specs: their CRCs are the ones the fixture was computed on; and the file respects its size limit"""
    assert os.path.getsize(FIXTURE) < 76773
    for s in MP.GRID + MP.SCAN:
        assert MP.checksum(*cases[s.name][:2]) == golden[s.name][1], s.name


def test_the_long_series_has_its_run_of_missing_steps(cases):
    for s in MP.GRID:
        if s.name.startswith("long"):
            y = cases[s.name][0]
            assert np.all(np.isnan(y[1000:1200, 1])) and not np.all(np.isnan(y[1000:1200, 0])) and 0.05 < np.mean(np.isnan(y[:, 0])) < 0.15


@pytest.mark.parametrize("spec", SMALL, ids=lambda s: s.name)
def test_banded_50_digits_equals_dense_50_digits(spec, golden, cases):
    """the two forms of lar_mp.run to 1e-40 in the contract's measures on every z mean, band entry, θ entry, b and F (a scan case outside the
    envelope: 1e-36 — in standard deviations a mean has 50 digits less those of |m|/sd, up to 1.6e11 there); the fixture is the banded one, bit
    for bit; and F does not rise, on the 50-digit values themselves"""
    y, m, iters, share = cases[spec.name]
    band, dense = MP.run(y, m, iters, share), MP.run(y, m, iters, share, form="dense")
    assert MP.raw_error(band["raw"], dense["raw"]) < (1e-40 if spec in MP.GRID or MP.in_envelope(golden[spec.name][2]) else 1e-36), spec.name
    assert np.array_equal(MP.flatten(MP.pick(spec, band)), golden[spec.name][0])
    assert np.allclose(band["gauges"], golden[spec.name][2], rtol=1e-6)
    for r in (band, dense):
        assert all(b <= a for a, b in zip(r["fe_mp"], r["fe_mp"][1:]))
        assert np.array_equal(r["gamma_shape"], np.broadcast_to(m["prior_gamma"][0] + 0.5 * y.size / r["gamma_shape"].shape[1], r["gamma_shape"].shape))


def test_free_energy_is_non_increasing_at_50_digits(golden):
    """on every case, as the fixture has it: the maker asserts it on the unrounded values, so here a rise can only be one of rounding"""
    for s in MP.GRID:
        fe = MP.free_energies(s, golden[s.name][0])
        assert fe.shape == (s.iterations,) and np.all(np.diff(fe) <= 2e-16 * np.abs(fe[1:])), (s.name, fe)


# ---- the admission rule: the restatement a tenth of the contract from 50 digits, the gauges inside the envelope -------------------------------------
def test_the_grid_is_admitted(golden, cases):
    misses = []
    for s in MP.GRID:
        flat, _, gauges = golden[s.name]
        print(f"{s.name}: |m|/sd ≤ {gauges[0]:.3g}, R/Szz ≥ {gauges[1]:.3g}, cond Λ ≤ {gauges[2]:.3g}")
        if not MP.in_envelope(gauges):
            misses.append((s.name, "outside the envelope", tuple(gauges)))
        for banded in (False, True) if s.T <= 300 else (False,):
            who = "lar_ref banded" if banded else "lar_ref dense"
            r, picked = _restated(s, cases[s.name], banded)
            errs = MP.errors(s, picked, flat)
            _note(who, errs, s.name)
            misses += [(s.name, who, q, v) for q, v in errs.items() if not v <= MP.TENTH[q]]
            if not np.all(np.diff(r["fe"]) <= 1e-9 * np.abs(r["fe"][1:])):
                misses.append((s.name, who, "F rises", r["fe"]))
    assert not misses, misses


def test_the_scan_gives_the_envelope(golden, cases):
    """inside the envelope both forms of the restatement are within a tenth of the contract; outside, the figures are printed.  And the bounds are
    not slack by more than the stated margins: the first case whose means the banded form misses lies within two decades of the bound on
    |m|/sd, and on the iterated part of the scan (the last five cases) b or F have left the tenth of the contract where R/Szz is below 3e-8."""
    misses, first_miss = [], np.inf
    for s in MP.SCAN:
        flat, _, gauges = golden[s.name]
        inside = MP.in_envelope(gauges)
        line = f"{s.name}: |m|/sd {gauges[0]:.2e}, R/Szz {gauges[1]:.1e}, cond Λ {gauges[2]:.1f}, {'inside ' if inside else 'OUTSIDE'}"
        for banded in (True, False):
            who = "lar_ref banded" if banded else "lar_ref dense"
            r, picked = _restated(s, cases[s.name], banded)
            errs = MP.errors(s, picked, flat)
            line += f" | {'banded' if banded else 'dense'}: mean {errs['mean']:.1e} sd, par {errs['par']:.1e}, F {errs['fe']:.1e}"
            if banded:                                              # printed only: the means at EVERY step against a fresh 50-digit run (DESIGN's table)
                y, m, iters, share = cases[s.name]
                line += f", mean over all steps {R.contract_errors(r, MP.run(y, m, iters, share))['mean']:.1e}"
            if inside:
                _note(who + " (scan, inside)", errs, s.name)
                misses += [(s.name, who, q, v) for q, v in errs.items() if not v <= MP.TENTH[q]]
            elif banded and errs["mean"] > MP.TENTH["mean"]:
                first_miss = min(first_miss, gauges[0])
            if banded and s.iterations == 3 and gauges[1] < 3e-8:
                assert errs["fe"] > MP.TENTH["fe"] or errs["par"] > MP.TENTH["par"], (s.name, errs)
        print(line)
    assert not misses, misses
    assert MP.ENVELOPE["ratio"] < first_miss <= 100.0 * MP.ENVELOPE["ratio"], first_miss
    assert sum(MP.in_envelope(golden[s.name][2]) for s in MP.SCAN) >= 25           # and most of the scan is inside: the envelope is not empty

"""The hidden Markov model engine (include/rxhip.h rxhip_hmm_desc, csrc/hmm_kernels.hpp) held to the project's contract across its count range,
against 50 digits: γ within 1e-9 absolute, counts within 1e-9 relative, free energy within 1e-8·max(1, |F|), per series and per iteration, on
every point of hmm_mp.GRID — prior scales 1e-3 … 1e9, default and scaled initial counts, uniform and sticky data, a symbol that never occurs,
one symbol throughout, nothing observed, mixed magnitudes inside one table, the widest, narrowest and a partial row, T = 1, 2 and 4096, shared
parameters.  Two references, both 50-digit: the fixture tests/golden/hmm_long.npz (a stated subset of every case, hmm_mp.pick: it has a size
limit) and, for everything but the widest and the longest cases, hmm_mp.run itself, computed once for the module (under 3 s), which gives
γ and the counts in full for EVERY iteration; on the widest and longest cases the iterations before the last are held to tests/hmm_ref.py, whose
γ and counts tests/test_hmm_contract_cpu.py pins to the fixture at 1e-11.

Cases of equal (T, K, M) run as ONE engine with a parameter set per series, so the grid is a handful of launches and every point is also
checked as a member of a batch; the ABI returns posteriors and per-series free energies of the last iteration, so a group runs once per iteration
count, as tests/test_hmm_gpu.py `_check_every_iteration` does.  Then the small-initial-count scans (hmm_mp.SCAN), one engine per case: answered
within the contract or refused with RXHIP_ERR_NONFINITE_FE and a text that says why, nothing in between; which cases must be answered and which
must be refused is decided by hmm_ref.min_normaliser."""
import collections
import os

import numpy as np
import pytest

import hmm_mp as MP
import hmm_ref as R
import rxhip
from rxhip import _lib

pytestmark = pytest.mark.gpu

CONTRACT = {"gamma": 1e-9, "counts": 1e-9, "fe": 1e-8}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hmm_long.npz")

_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """after the module: the worst error per quantity with its case (-s shows it; DESIGN.md §3.5b quotes it)"""
    yield
    for q, (v, what) in sorted(_worst.items()):
        print(f"\nworst {q}: {v:.3e} at {what}")


def _hold(errs, what):
    for q, v in errs.items():
        if v > _worst.get(q, (-1.0, None))[0]:
            _worst[q] = (v, what)
    assert all(v < CONTRACT[q] for q, v in errs.items()), (what, errs)


def _errors(gamma, a, b, fe, ref_gamma, ref_a, ref_b, ref_fe):
    """the contract's three measures of one series (fe / ref_fe: any shape, or None)"""
    assert np.all(np.isfinite(gamma)) and np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    out = {"gamma": float(np.max(np.abs(gamma - ref_gamma))),
           "counts": max(float(np.max(np.abs(a - ref_a) / ref_a)), float(np.max(np.abs(b - ref_b) / ref_b)))}
    if fe is not None:
        fe, ref_fe = np.asarray(fe, dtype=np.float64), np.asarray(ref_fe, dtype=np.float64)
        assert np.all(np.isfinite(fe))
        out["fe"] = float(np.max(np.abs(fe - ref_fe) / np.maximum(1.0, np.abs(ref_fe))))
    return out


@pytest.fixture(scope="module")
def golden():
    g = np.load(FIXTURE)
    ends = np.cumsum(g["sizes"].astype(np.int64))
    return {s.name: (g["values"][e - n:e] if n else None) for s, e, n in zip(MP.GRID + MP.SCAN, ends, g["sizes"])}


@pytest.fixture(scope="module")
def cases(golden):
    """the inputs of every case, generated once and checked against the CRCs the fixture was computed on"""
    crc = np.load(FIXTURE)["crc"]
    out = {s.name: MP.case(s) for s in MP.GRID + MP.SCAN}
    for s, c in zip(MP.GRID + MP.SCAN, crc):
        assert MP.checksum(*out[s.name]) == int(c), s.name
    return out


def _in_full(spec):
    return not (spec.name.startswith("widest") or spec.name.startswith("long"))


@pytest.fixture(scope="module")
def full(cases):
    """hmm_mp.run on every grid case but the widest and longest: γ, counts and free energy of every iteration at 50 digits"""
    return {s.name: MP.run(cases[s.name][0], **cases[s.name][1], iterations=s.iterations, share=s.share) for s in MP.GRID if _in_full(s)}


def _groups():
    """the single-series grid cases by shape: one engine each (the two T = 4096 chains are two series of one engine)"""
    g = collections.OrderedDict()
    for s in MP.GRID:
        if not s.share:
            g.setdefault((s.T, s.K, s.M, s.iterations), []).append(s)
    return g


GROUPS = _groups()


def _stack(specs, cases):
    x = np.stack([cases[s.name][0] for s in specs], axis=1)
    m = {k: np.stack([cases[s.name][1][k] for s in specs]) for k in ("prior_A", "prior_B", "init_A", "init_B")}
    return x, m


def _run(x, m, pi, iters, layout="time_chain", want_fe=True, **kw):
    """(γ [T+1][series][K], A counts, B counts, fe [iters], per-series fe of the last iteration)"""
    with rxhip.HMMEngine(x.shape[0], m["prior_A"], m["prior_B"], pi, m["init_A"], m["init_B"], n_series=x.shape[1], **kw) as eng:
        eng.set_data(x if layout == "time_chain" else np.ascontiguousarray(x.T), layout=layout)
        eng.run(iters, want_fe)
        g = eng.states(layout)
        a, b = eng.parameters()
        fe = (eng.free_energy(), eng.free_energy_per_chain()) if want_fe else (None, None)
    return (g if layout == "time_chain" else np.ascontiguousarray(g.transpose(1, 0, 2))), a, b, fe[0], fe[1]


def _pi(specs, cases):
    """the one π of an engine: the cases of a shape share it (hmm_mp.shared_pi)"""
    pi = cases[specs[0].name][1]["prior_s0"]
    assert all(np.array_equal(cases[s.name][1]["prior_s0"], pi) for s in specs)
    return pi


# ---- the grid --------------------------------------------------------------------------------------------------------------------------------------
def test_the_groups_are_the_grid():
    assert sorted(GROUPS) == sorted([(24, 3, 4, 4), (8, 16, 64, 4), (24, 2, 2, 4), (12, 9, 3, 4), (1, 3, 4, 4), (2, 3, 4, 4), (4096, 3, 3, 3)])
    assert [len(GROUPS[k]) for k in ((24, 3, 4, 4), (8, 16, 64, 4), (24, 2, 2, 4), (4096, 3, 3, 3))] == [41, 3, 3, 2]
    assert sum(len(v) for v in GROUPS.values()) + sum(s.share for s in MP.GRID) == len(MP.GRID) == 56


@pytest.mark.parametrize("shape", list(GROUPS), ids=lambda k: "T%d-K%d-M%d" % k[:3])
def test_grid(shape, golden, cases, full):
    """One engine per shape, a parameter set per series, one run per iteration count n: the n-th iterate of every series against 50 digits (γ and
    counts in full from hmm_mp.run where `full` has the case, else hmm_ref before the last iteration), its free energy of iteration n against the
    fixture's; the last iterate against the fixture's subset; the totals of every iteration of the longest run against the series' sum."""
    specs = GROUPS[shape]
    iters = shape[3]
    x, m = _stack(specs, cases)
    pi = _pi(specs, cases)
    fe_fix = {s.name: golden[s.name][-iters:] for s in specs}                        # (hmm_mp.pick puts the free energies last)
    for n in range(1, iters + 1):
        g, a, b, fe_tot, fe_last = _run(x, m, pi, n)
        assert fe_tot.shape == (n,) and fe_last.shape == (len(specs),)
        for k, s in enumerate(specs):
            what = f"{s.name}, iteration {n}"
            if s.name in full:
                r = full[s.name]
                ref = (r["gamma"][n - 1], r["A"][n - 1], r["B"][n - 1])
                assert abs(r["fe"][n - 1] - fe_fix[s.name][n - 1]) <= 1e-15 * max(1.0, abs(r["fe"][n - 1]))   # the fixture is this restatement
            else:
                ref = R.run(cases[s.name][0], **cases[s.name][1], iterations=n)[:3]
            _hold(_errors(g[:, k], a[k], b[k], fe_last[k], *ref, fe_fix[s.name][n - 1]), what)
            if n == iters:
                _hold(MP.errors(MP.pick(s, g[:, k], a[k], b[k], np.concatenate([fe_fix[s.name][:-1], fe_last[k:k + 1]])), golden[s.name]), what + " (fixture)")
        if n == iters:
            want = np.sum([fe_fix[s.name] for s in specs], axis=0)
            _hold({"fe": float(np.max(np.abs(fe_tot - want) / np.maximum(1.0, np.abs(want))))}, f"totals of {shape}")


@pytest.mark.parametrize("name", [s.name for s in MP.GRID if s.share])
def test_grid_shared_parameters(name, golden, cases, full):
    """5 series under one q(A), q(B): every iteration against hmm_mp.run, the last against the fixture"""
    s = next(v for v in MP.GRID if v.name == name)
    x, m = cases[name]
    r = full[name]
    for n in range(1, s.iterations + 1):
        g, a, b, fe_tot, _ = _run(x, m, m["prior_s0"], n, share_parameters=True)
        assert a.shape == (1, s.K, s.K) and b.shape == (1, s.M, s.K)
        _hold(_errors(g, a[0], b[0], fe_tot, r["gamma"][n - 1], r["A"][n - 1], r["B"][n - 1], r["fe"][:n]), f"{name}, iteration {n}")
    _hold(MP.errors(MP.pick(s, g, a[0], b[0], fe_tot), golden[name]), name + " (fixture)")


POINTS_ALONE = ("scale p=0.001 init=default uniform", "scale p=1e+09 init=1e+09 sticky", "row 2 of B × 1e-3 p=1 init=1 uniform")


def test_a_series_alone_has_the_bits_of_the_series_in_its_batch(cases):
    """the smallest and the largest count scale and a mixed-magnitude point: 41 series of wildly different magnitudes share four wavefronts, and
    none of them sees the others"""
    specs = GROUPS[(24, 3, 4, 4)]
    names = [s.name for s in specs]
    assert all(p in names for p in POINTS_ALONE)
    x, m = _stack(specs, cases)
    pi = _pi(specs, cases)
    g, a, b, _, fe_last = _run(x, m, pi, 4)
    for p in POINTS_ALONE:
        k = names.index(p)
        g1, a1, b1, fe1, _ = _run(x[:, k:k + 1], {key: v[k:k + 1] for key, v in m.items()}, pi, 4)
        assert np.array_equal(g1[:, 0], g[:, k]) and np.array_equal(a1[0], a[k]) and np.array_equal(b1[0], b[k]) and fe1[-1] == fe_last[k], p


def test_both_layouts_on_one_batch(cases):
    specs = GROUPS[(24, 3, 4, 4)]
    x, m = _stack(specs, cases)
    pi = _pi(specs, cases)
    one, two = _run(x, m, pi, 4), _run(x, m, pi, 4, layout="chain_time")
    for u, v in zip(one, two):
        assert np.array_equal(u, v)


# ---- the guard: small initial counts are answered within the contract or refused -----------------------------------------------------------------
def _refusal(ei):
    text = str(ei.value)
    assert ei.value.status == _lib.ERR_NONFINITE_FE and "underflow" in text and "counts are too small" in text, text


def test_scan(golden, cases):
    """One engine per case.  hmm_ref's smallest normaliser decides what is required: ≥ 10·kMinNormaliser must be answered, ≤ kMinNormaliser / 10 must be
    refused (the fixture holds no answer for those); in between either, but never a wrong answer."""
    wrong, refused_n, refused_first = [], 0, 0
    for s in MP.SCAN:
        x, m = cases[s.name]
        small = R.min_normaliser(x, **m, iterations=s.iterations)
        try:
            g, a, b, fe_tot, _ = _run(x[:, None], {k: v[None] for k, v in m.items() if k != "prior_s0"}, m["prior_s0"], s.iterations)
        except rxhip.RxHipError as err:
            assert err.status == _lib.ERR_NONFINITE_FE and "underflow" in str(err) and "counts are too small" in str(err), (s.name, str(err))
            refused_n += 1
            refused_first += s.name.startswith("scan ")
            if small >= 10 * R.K_MIN_NORMALISER:
                wrong.append((s.name, "refused, but must be answered", small))
            continue
        if small <= R.K_MIN_NORMALISER / 10:
            wrong.append((s.name, "answered, but must be refused", small))
            continue
        errs = MP.errors(MP.pick(s, g[:, 0], a[0], b[0], fe_tot), golden[s.name])
        for q, v in errs.items():
            if v > _worst.get(q + " (scan)", (-1.0, None))[0]:
                _worst[q + " (scan)"] = (v, s.name)
        wrong += [(s.name, q, v, small) for q, v in errs.items() if not v < CONTRACT[q]]
    print(f"{refused_n} of {len(MP.SCAN)} scan cases refused")
    assert not wrong, wrong
    assert refused_first <= 49           # of the first scan's 110: tests/test_hmm_contract_cpu.py derives the cap from the reference


def test_a_refused_run_leaves_the_engine_usable(cases):
    """s = 1e-3: with its data the sweep underflows and the run is refused; with nothing observed (factors of 1, B̃ out of the products) the same
    engine answers, within the contract of the 50-digit restatement; with the data back it refuses again"""
    s = next(v for v in MP.SCAN if v.name == "scan s=0.001 seed=0")
    x, m = cases[s.name]
    blank = np.full_like(x, np.nan)
    assert R.min_normaliser(x, **m, iterations=2) <= R.K_MIN_NORMALISER / 10 and R.min_normaliser(blank, **m, iterations=2) >= 1e50 * R.K_MIN_NORMALISER
    r = MP.run(blank, **m, iterations=2)
    for layout in ("time_chain", "chain_time"):
        put = lambda eng, v: eng.set_data(v[:, None] if layout == "time_chain" else v[None, :], layout=layout)
        with rxhip.HMMEngine(s.T, m["prior_A"], m["prior_B"], m["prior_s0"], m["init_A"], m["init_B"]) as eng:
            for _ in range(2):
                put(eng, x)
                for want_fe in (True, False):
                    with pytest.raises(rxhip.RxHipError) as ei:
                        eng.run(2, want_fe)
                    _refusal(ei)
                put(eng, blank)
                eng.run(2, True)
                g = eng.states(layout)
                a, b = eng.parameters()
                _hold(_errors(g[:, 0] if layout == "time_chain" else g[0], a[0], b[0], eng.free_energy(), r["gamma"][-1], r["A"][-1], r["B"][-1], r["fe"]),
                      "nothing observed after a refusal")

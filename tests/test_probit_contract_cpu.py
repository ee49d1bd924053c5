"""tests/probit_ref.py `run_messages` — what tests/test_probit_contract_gpu.py holds the probit engine to — pinned to the 60-digit restatement
tests/probit_mp.py at 100× inside the engine's contract: means within 1e-8 posterior standard deviations, variances within 1e-8 relative, the
free energy of every iteration within 1e-10·max(1, |F|).  At EVERY point of probit_mp.GRID (300 points; none excluded), two series per point:
all ones, and a mixed series whose first and last steps are missing.  T = 8 and 3 iterations keep the 600 sixty-digit runs near a minute; the
arithmetic that can go wrong in double — the tails of the tilted moments, the nearly singular pair marginals at q = 1e-8, the vague prior —
does so at any length."""
import numpy as np
import pytest

import probit_mp as M
import probit_ref as R

NAN = float("nan")
T, ITERS = 8, 3
SERIES = {"ones": np.ones(T), "mixed": np.array([NAN, 1.0, 0.0, NAN, 1.0, 1.0, 0.0, NAN])}


def test_the_grid_is_the_whole_grid():
    assert len(M.GRID) == 300 and len(set(M.GRID)) == 300
    assert {p[0] for p in M.GRID} == {0.0, -0.9, 0.5, 1.0, 1.05} and {p[1] for p in M.GRID} == {1e-8, 1e-4, 1e-2, 1.0, 1e3}
    assert {p[2] for p in M.GRID} == {1e-4, 1.0, 1e6} and {(p[3], p[4]) for p in M.GRID} == {(0.0, 0.0), (3.0, -0.5), (-8.0, 0.3), (40.0, 0.0)}


@pytest.mark.parametrize("a", M.GRID_A)
def test_run_messages_equals_the_60_digit_restatement(a):
    points = [p for p in M.GRID if p[0] == a]
    assert len(points) == 60
    worst, failures = [0.0, 0.0, 0.0], []
    for _, q, v0, m0, c in points:
        for name, y in SERIES.items():
            got = R.run_messages(y, a, c, q, m0, v0, ITERS)
            finite = all(np.all(np.isfinite(x)) for x in got)
            em, ev, ef = M.errors(got, M.run(y, a, c, q, m0, v0, ITERS)) if finite else (np.inf,) * 3
            worst = [max(w, e) for w, e in zip(worst, (em, ev, ef))]
            if not (finite and em < 1e-8 and ev < 1e-8 and ef < 1e-10):
                failures.append((dict(a=a, q=q, v0=v0, m0=m0, c=c, series=name), em, ev, ef))
    print(f"a = {a}: worst mean {worst[0]:.3e} sd, var {worst[1]:.3e} rel, fe {worst[2]:.3e} of max(1, |F|)")
    assert not failures, failures


def test_the_restatement_itself_on_the_reference_case():
    """the 60-digit iteration reaches the reference's golden free energy (probit_tests.jl:77) at its fixed point"""
    _, y = R.reference_data()
    mean, var, fe = M.run(y, **R.REFERENCE_MODEL, iterations=10)
    assert abs(float(fe[-1]) - R.GOLDEN_FE) < 1e-8 * R.GOLDEN_FE

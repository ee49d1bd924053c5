"""The probit engine's kernels on the HOST: tests/host_emul/probit_main.cpp compiles csrc/probit_kernels.hpp with g++ through the stand-in
<hip/hip_runtime.h> of tests/host_emul/ and runs its sweeps one "thread" at a time — the same __host__ __device__ functions, loops and indexing
as on the device.  Held to tests/probit_ref.py at the tolerances of tests/test_probit_gpu.py (means 1e-6 posterior standard deviations,
variances 1e-6 relative, free energy 1e-8 relative per iteration and series): the check of this arithmetic that needs no GPU.  The corners and
the whole grid of tests/test_probit_contract_gpu.py run here too, with that test's free-energy bound of 1e-8·max(1, |F|)."""
import os
import subprocess

import numpy as np
import pytest

import probit_mp as M
import probit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("probit_host") / "probit_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC, "-o", out,
                    os.path.join(EMUL, "probit_main.cpp")], check=True)
    return out


def _case_text(y, a, c, q, m0, v0, n_gh, iters):
    T, C = y.shape
    gx, gw = R.gauss_hermite(n_gh)
    nums = list(y.ravel()) + list(gx) + list(gw)
    return " ".join([f"{T} {C} {a!r} {c!r} {q!r} {m0!r} {v0!r} {n_gh} {iters}"] + [repr(float(v)) for v in nums])


def _cases():
    _, y = R.reference_data()
    out = [(y[:, None], 1.0, 0.1, 0.01, 0.0, 100.0, 32, 10)]
    for seed, (T, C) in ((1, (37, 70)), (2, (5, 3))):   # more than one "wavefront", a ragged last one; a chunk of the energy sum that is not full
        rng = np.random.default_rng(seed)
        yy = (rng.random((T, C)) < 0.5).astype(np.float64)
        yy[rng.random((T, C)) < 0.2] = np.nan
        yy[:, 0] = 0.0
        yy[:, 1] = 1.0
        yy[0, 2] = yy[-1, 2] = np.nan
        out.append((yy, float(rng.uniform(0.7, 1.0)), float(rng.normal(0, 0.2)), float(rng.uniform(0.05, 1.0)), float(rng.normal()), float(rng.uniform(0.5, 10)),
                    int(rng.integers(5, 33)), 4))
    out.append((np.ones((5, 1)), 1.0, 0.0, 1e-4, -40.0, 0.01, 32, 5))   # the tail: every cavity sits at z ≈ −40, where Φ underflows
    return out


def _corners():
    """Corners of the contract grid (tests/probit_mp.py GRID) on the six series of tests/test_probit_contract_gpu.py: a nearly deterministic chain
    (q = 1e-8), a vague prior (v0 = 1e6), no coupling (a = 0), a sign-flipping chain (a = −0.9), the upper tail (m0 = +40: the site precision sits
    at its floor and the free energy of the all-ones series is ~1e-19, hence the floor of 1 under the free-energy bound)."""
    y = R.contract_series(20)
    return [(y, 1.0, 0.0, 1e-8, 0.0, 1e6, 32, 5), (y, 0.0, 0.3, 1.0, -8.0, 1e-4, 32, 5), (y, -0.9, -0.5, 1e-4, 3.0, 1.0, 32, 5), (y, 1.05, 0.0, 1e3, 40.0, 1e6, 32, 5),
            (y, 0.5, 0.0, 1e-8, 40.0, 1e-4, 32, 5), (y, -0.9, 0.3, 1e-8, -8.0, 1e6, 32, 5)]


def _run(exe, cases):
    text = f"{len(cases)}\n" + "\n".join(_case_text(*c) for c in cases) + "\n"
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()


def _hold(lines, cases, fe_floor):
    """every series of every case at the contract; the free energy relative to |F|, or to max(1, |F|) with `fe_floor`"""
    i = 0
    for y, a, c, q, m0, v0, n_gh, iters in cases:
        mean, var, fe = R.run_batch(y, a, c, q, m0, v0, iters, n_gh)
        for s in range(y.shape[1]):
            gm, gv, gf = (np.array(lines[i + j].split(), dtype=np.float64) for j in range(3))
            i += 3
            what = (a, c, q, m0, v0, s)
            assert np.all(np.isfinite(gm)) and np.all(np.isfinite(gv)) and np.all(np.isfinite(gf)), what
            assert np.max(np.abs(gm - mean[:, s]) / np.sqrt(var[:, s])) < 1e-6, what
            assert np.max(np.abs(gv - var[:, s]) / var[:, s]) < 1e-6, what
            scale = np.maximum(1.0, np.abs(fe[:, s])) if fe_floor else np.abs(fe[:, s])
            assert np.max(np.abs(gf - fe[:, s]) / scale) < 1e-8, (what, gf, fe[:, s])
            if np.all(np.isnan(y[:, s])):   # nothing observed: the free energy is exactly 0
                assert np.max(np.abs(gf)) < 1e-12, (what, gf)
    assert i == len(lines)


def test_host_build_of_the_kernels_equals_the_restatement(exe):
    cases = _cases()
    lines = _run(exe, cases)
    _hold(lines, cases, fe_floor=False)
    # the reference case reaches the reference's own number
    assert abs(float(lines[2].split()[-1]) - R.GOLDEN_FE) < 1e-8 * R.GOLDEN_FE


def test_host_build_at_the_corners_of_the_contract_grid(exe):
    cases = _corners()
    _hold(_run(exe, cases), cases, fe_floor=True)


@pytest.mark.parametrize("a", M.GRID_A)
def test_host_build_on_the_contract_grid(exe, a):
    """the kernels' arithmetic at every point of the grid that tests/test_probit_contract_gpu.py runs on the device, same series, same bounds"""
    y = R.contract_series(20)
    cases = [(y, a, c, q, m0, v0, 32, 5) for a_, q, v0, m0, c in M.GRID if a_ == a]
    assert len(cases) == 60
    _hold(_run(exe, cases), cases, fe_floor=True)


def test_host_build_refuses_an_observation_that_is_not_binary(exe):
    y = np.array([[0.0], [0.5], [1.0]])
    text = "1\n" + _case_text(y, 1.0, 0.0, 0.1, 0.0, 1.0, 8, 2) + "\n"
    assert subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split() == ["bad_y"]


def test_tail_functions_of_the_header(exe):
    """r(z), log Φ and the site update of the header at the points where the naive forms break: z = ∓40 (Φ underflows / saturates), the switch points of
    the erfcx evaluation (t = 4 ⇔ z = −4√2) and ordinary arguments."""
    pts = [(-40.0, 0.01, 1.0), (40.0, 0.01, -1.0), (-4.0 * np.sqrt(2.0) - 1e-9, 0.5, 1.0), (-4.0 * np.sqrt(2.0) + 1e-9, 0.5, 1.0), (0.3, 2.0, 1.0), (-1.0, 1.0, 1.0),
           (3.0, 0.5, -1.0), (-12.0, 4.0, 1.0), (0.0, 1.0, 1.0)]
    text = "0\n" + "\n".join(f"{float(m)!r} {float(v)!r} {float(s)!r}" for m, v, s in pts) + "\n"
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(pts)
    for (m, v, s), ln in zip(pts, lines):
        mt, vt, xi, w, lphi, r = (float(x) for x in ln.split())
        assert all(np.isfinite(x) for x in (mt, vt, xi, w, lphi, r)) and w > 0 and vt > 0
        assert abs(lphi - R.log_ndtr(m)) <= 1e-13 * max(1.0, abs(R.log_ndtr(m)))
        assert abs(r - float(R.mills(m))) <= 1e-13 * max(float(R.mills(m)), 1e-300) or float(R.mills(m)) < 1e-300
        rm, rv = R.tilted(m, v, 0.5 * (s + 1.0))
        assert abs(mt - rm) <= 1e-12 * max(1.0, abs(rm)) and abs(vt - rv) <= 1e-10 * rv

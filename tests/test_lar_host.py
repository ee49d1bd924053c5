"""The latent autoregressive engine's `__host__ __device__` helpers on the HOST: tests/host_emul/lar_main.cpp compiles csrc/lar_kernels.hpp with g++
through the stand-in <hip/hip_runtime.h> of tests/host_emul/ and drives the band entry, the LDLᵀ row step, the back-substitution and
selected-inverse step, the statistics and the θ/γ update serially in the order of the device's run.  Held to the dense restatement of
tests/lar_ref.py at the project's contract (lar_ref.hold: means 1e-6 standard deviations, parameters and (co)variances 1e-6 relative, free energy
1e-8 relative per iteration): the check of this arithmetic that needs no GPU.  And held, at the same contract, to the 50-digit fixture
tests/golden/lar_long.npz on every case of lar_mp.GRID with (T + p)·series ≤ 3000 and every lar_mp.SCAN case inside the envelope: every order over
257 steps and 15 iterations, the boundary shapes at p = 5 and 8, τ and γ over twelve and nine decades, unit roots, extreme priors, offsets."""
import os
import subprocess

import numpy as np
import pytest

import lar_mp as MP
import lar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rxinfer.jl_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "host_emul")
FIXTURE = os.path.join(ROOT, "tests", "golden", "lar_long.npz")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lar_host") / "lar_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", EMUL, "-I", CSRC, "-o", out,
                    os.path.join(EMUL, "lar_main.cpp")], check=True)
    return out


def case_text(y, m, iters, shared):
    T, C = y.shape
    nums = np.concatenate([[m["tau"], *m["prior_gamma"], *m["init_gamma"]], m["prior_theta"][0], m["prior_theta"][1].ravel(), m["prior_x0"][0],
                           m["prior_x0"][1].ravel(), m["init_theta"][0], m["init_theta"][1].ravel(),
                           [np.linalg.slogdet(m["prior_theta"][1])[1], np.linalg.slogdet(m["prior_x0"][1])[1]], y.ravel()])
    return f"{T} {C} {m['order']} {iters} {int(shared)} " + " ".join(repr(float(v)) for v in nums)


def parse(lines, T, C, p, iters, shared):
    G = 1 if shared else C
    v = [np.array(ln.split(), dtype=np.float64) for ln in lines]
    gam = v[4].reshape(iters, G, 2)
    return dict(x_mean=v[0].reshape(T, C, p), x_cov=v[1].reshape(T, C, p, p), theta_mean=v[2].reshape(iters, G, p), theta_cov=v[3].reshape(iters, G, p, p),
                gamma_shape=gam[..., 0], gamma_rate=gam[..., 1], fe=v[5])


def contract_specs():
    """the cases of lar_mp that are held to the fixture here"""
    golden = MP.load(FIXTURE)
    return [s for s in MP.GRID if (s.T + s.p) * s.C <= 3000] + [s for s in MP.SCAN if MP.in_envelope(golden[s.name][2])], golden


def all_cases():
    y, _ = R.reference_data()
    return [(y[:, None], R.model(p, 5.0), 15, False) for p in (1, 5)] + [R.case(spec) for spec in R.CASES["host"]] + [MP.case(s) for s in contract_specs()[0]]


def test_host_build_of_the_helpers_equals_the_restatement(exe):
    cases = all_cases()
    text = f"{len(cases)}\n" + "\n".join(case_text(*c) for c in cases) + "\n"
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 6 * len(cases)
    worst = {}
    specs, golden = contract_specs()
    assert len(specs) >= 47 + 27 and sum(s.share for s in specs) == 2 and {s.p for s in specs if s.T == 257} == set(range(1, 9))
    first = len(cases) - len(specs)
    fixture_worst = {}
    for spec, (y, m, iters, shared), n in zip(specs, cases[first:], range(first, len(cases))):       # the 50-digit fixture, at the contract
        got = parse(lines[6 * n:6 * n + 6], *y.shape, m["order"], iters, shared)
        assert MP.checksum(y, m) == golden[spec.name][1], spec.name
        errs = MP.errors(spec, MP.pick(spec, got), golden[spec.name][0])
        for k, v in errs.items():
            if v >= fixture_worst.get(k, (-1.0, None))[0]:
                fixture_worst[k] = (v, spec.name)
        assert all(v <= MP.CONTRACT[k] for k, v in errs.items()), (spec.name, errs)
        assert np.all(np.diff(got["fe"]) <= 1e-9 * np.abs(got["fe"][1:])), (spec.name, got["fe"])
    print("worst against the 50-digit fixture:", fixture_worst)
    for n, (y, m, iters, shared) in enumerate(cases[:first]):
        ref = R.run_batch(y, **m, iterations=iters, share_parameters=shared)
        got = parse(lines[6 * n:6 * n + 6], *y.shape, m["order"], iters, shared)
        for k, v in R.hold(got, ref).items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert np.all(np.diff(got["fe"]) <= 1e-9 * np.abs(got["fe"][1:]))
        if n < 2:                                                                 # the reference data at p = 1 and p = 5
            assert abs(got["fe"][-1] - R.GOLDEN_FE[m["order"]]) < 0.01
            for it, want in zip((0, 14), R.RECORDED_FE[m["order"]]):
                assert abs(got["fe"][it] - want) < 1e-8 * want
    print("worst:", worst)

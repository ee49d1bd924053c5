"""What pins tests/gammamix_ref.py (the CPU restatement the Gamma mixture engine is held to) independently of the engine, and the conditions on the inputs
of every case the CPU and GPU tests use.
 1. the restatement against the 50-digit statement tests/gammamix_mp.py at 1e-10 (â, e, f, α relative; F relative to max(1, |F|)) over gammamix_ref.CPU_CASES;
 2. F never rises (gammamix_ref.does_not_rise: a rounding allowance reasoned there);
 3. at the last iterate every coordinate is at its minimum: moving â_k (against the q(b) it was solved with), (e_k, f_k) or α raises F;
 4. K = 1: q(z) ≡ 1 and the fixed point satisfies the two stationarity equations of iid Gamma data with a MAP shape and a conjugate rate;
 5. N = 3, K = 2 with every ψ and lnΓ replaced by its closed form by hand: one iteration equals the hand computation;
 6. the conditions: S0_k ≥ 1 for every component at every iteration, and the history moves by less than 1e-10 under a permutation of y — over EVERY case;
 7. the reference test's own configuration on the recorded numpy draw: RECORDED (not the reference's −146.8: gammamix_ref.RECORDED)."""
import math

import numpy as np
import pytest
from scipy.special import digamma

import gammamix_mp as MP
import gammamix_ref as R

TOL = 1e-10


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_restatement_against_50_digits():
    assert len(R.CPU_CASES) >= 20 and {K for _, _, K, _ in R.CPU_CASES} == {1, 2, 3, 5, 16}
    assert max(N for _, N, _, _ in R.CPU_CASES) <= 300 and max(it for *_, it in R.CPU_CASES) <= 30
    worst = {}
    for seed, N, K, it in R.CPU_CASES:
        it = min(it, 12) if N * K > 1500 else it          # (the 50-digit run of the largest cases is kept to 12 iterations)
        y, prior, init = R.make_problem(seed, N, K)
        ref, mp = R.run(y, prior, init, it), MP.run(y, prior, init, it)
        for key in ("a", "e", "f", "alpha"):
            worst[key] = max(worst.get(key, 0.0), _rel(ref[key], mp[key]))
        worst["fe"] = max(worst.get("fe", 0.0), float(np.max(np.abs(ref["fe"] - mp["fe"]) / np.maximum(1.0, np.abs(mp["fe"])))))
    print("restatement against 50 digits, worst:", worst)
    assert max(worst.values()) < TOL, worst


def test_default_initialisation_against_50_digits():
    y, prior = R.golden()
    ref, mp = R.run(y, prior, None, 10), MP.run(y, prior, None, 10)
    assert max(_rel(ref[k], mp[k]) for k in ("a", "e", "f", "alpha")) < TOL and float(np.max(np.abs(ref["fe"] - mp["fe"]) / np.abs(mp["fe"]))) < TOL


def test_free_energy_never_rises():
    for seed, N, K, it in R.CPU_CASES + R.STREAMED_CASES[:8] + R.SMALL_CASES[:4]:
        y, prior, init = R.make_problem(seed, N, K)
        fe = R.run(y, prior, init, it)["fe"]
        assert R.does_not_rise(fe, N, K), (seed, N, K, np.diff(fe).max())
    y, prior = R.golden()
    assert R.does_not_rise(R.run(y, prior, None, 50)["fe"], 250, 2)


def test_every_coordinate_is_at_its_minimum():
    rng = np.random.default_rng(7)
    n = 0
    extra = [(700 + i, N, K, 6) for i, (N, K) in enumerate([(40, 1), (90, 2), (120, 3), (200, 5), (240, 16), (77, 2), (150, 3), (260, 5)])]   # (conditions: below)
    for seed, N, K, it in R.CPU_CASES + R.STREAMED_CASES[:8] + R.SMALL_CASES[:4] + extra:
        y, prior, init = R.make_problem(seed, N, K)
        r = R.run(y, prior, init, min(it, 6))
        L = r["last"]
        a, e, f, al = r["a"][-1], r["e"][-1], r["f"][-1], r["alpha"][-1]
        F = lambda a_, e_, f_, al_: R.free_energy(L["S0"], L["S1"], L["SL"], L["H"], a_, e_, f_, al_, prior)
        base = F(a, e, f, al)
        assert abs(base - r["fe"][-1]) <= 1e-12 * max(1.0, abs(base))
        k = int(rng.integers(K))
        for step in (1e-3, -1e-3, 0.05, -0.05):
            d = np.zeros(K)
            d[k] = step
            assert F(a, e * (1 + d), f, al) > base and F(a, e, f * (1 + d), al) > base and F(a, e * (1 + d), f * (1 - d), al) > base     # q(b_k)
            assert K == 1 or F(a, e, f, al * (1 + d)) > base                                            # q(s) (K = 1: F does not depend on α)
            # â_k was solved against the OLD q(b): the objective it maximises is g(a) = ln p(a) + a (S0 E ln b_old + SL) − S0 lnΓ(a)
            g = lambda x: (prior[0][k] - 1) * math.log(x) - prior[1][k] * x + x * (L["S0"][k] * L["Elnb_old"][k] + L["SL"][k]) - L["S0"][k] * math.lgamma(x)
            assert g(a[k] * (1 + step)) < g(a[k])
        n += 1
    assert n >= 40


def test_one_component_is_iid_gamma_data():
    y, prior, init = R.make_problem(9, 80, 1)
    r = R.run(y, prior, init, 400)
    assert np.all(r["resp"] == 1.0) and np.all(r["S0"] == 80.0)
    a, e, f = r["a"][-1, 0], r["e"][-1, 0], r["f"][-1, 0]
    c0, d0, e0, f0 = prior[0][0], prior[1][0], prior[2][0], prior[3][0]
    # conjugate rate: e = e⁰ + N â, f = f⁰ + Σ y;   MAP shape: (c⁰ − 1)/â − d⁰ + N (ψ(e) − ln f) + Σ ln y − N ψ(â) = 0
    assert e == pytest.approx(e0 + 80 * a, rel=1e-14) and f == pytest.approx(f0 + y.sum(), rel=1e-14)
    terms = [(c0 - 1) / a, d0, 80 * (digamma(e) - np.log(f)), np.log(y).sum(), 80 * digamma(a)]
    assert abs(terms[0] - terms[1] + terms[2] + terms[3] - terms[4]) < 1e-9 * max(abs(t) for t in terms)


def test_one_iteration_by_hand():
    """N = 3, K = 2 from â = (1, 2), q(b) = Gamma(1, 1), Gamma(2, 1), q(s) = Dir(1, 2): ψ(1) = −γ, ψ(2) = 1 − γ, ψ(3) = 3/2 − γ, lnΓ(1) = lnΓ(2) = 0, so
    logit_1 = −3/2 − γ − y,   logit_2 = −1/2 + 2(1 − γ) + ln y − 2y."""
    g = 0.5772156649015329
    y = np.array([0.5, 1.0, 2.5])
    prior = (np.array([1.5, 2.0]), np.array([0.5, 0.25]), np.array([1.0, 3.0]), np.array([2.0, 1.0]), np.array([1.0, 2.0]))
    init = (np.array([1.0, 2.0]), np.array([1.0, 2.0]), np.array([1.0, 1.0]), np.array([1.0, 2.0]))
    r = R.run(y, prior, init, 1)
    l1, l2 = -1.5 - g - y, -0.5 + 2 * (1 - g) + np.log(y) - 2 * y
    r1 = 1 / (1 + np.exp(l2 - l1))
    resp = np.stack([r1, 1 - r1], axis=1)
    assert np.allclose(r["resp"], resp, rtol=1e-13, atol=0)
    S0, S1, SL = resp.sum(0), (resp * y[:, None]).sum(0), (resp * np.log(y)[:, None]).sum(0)
    assert np.allclose(r["alpha"][0], prior[4] + S0, rtol=1e-14) and np.allclose(r["f"][0], prior[3] + S1, rtol=1e-14)
    a = r["a"][0]
    assert np.allclose(r["e"][0], prior[2] + S0 * a, rtol=1e-14)
    Elnb_old = np.array([-g, 1 - g])                       # ψ(1) − ln 1, ψ(2) − ln 1
    resid = (prior[0] - 1) / a - prior[1] + S0 * Elnb_old + SL - S0 * digamma(a)
    assert np.all(np.abs(resid) < 1e-12 * (1 + S0 * np.abs(digamma(a))))
    # F with its terms written out for this case
    al, e, f = r["alpha"][0], r["e"][0], r["f"][0]
    Elns, Elnb = digamma(al) - digamma(al.sum()), digamma(e) - np.log(f)
    lg = lambda v: np.array([math.lgamma(x) for x in np.atleast_1d(v)])
    H = -float(np.sum(resp * np.log(resp)))
    F = -np.sum(S0 * (Elns + a * Elnb - lg(a)) + (a - 1) * SL - e / f * S1) - H
    F += math.lgamma(al.sum()) - math.lgamma(3.0) - np.sum(lg(al) - lg(prior[4])) + np.sum((al - prior[4]) * Elns)
    F += np.sum((e - prior[2]) * digamma(e) - lg(e) + lg(prior[2]) + prior[2] * (np.log(f) - np.log(prior[3])) + e * (prior[3] - f) / f)
    F -= np.sum(prior[0] * np.log(prior[1]) - lg(prior[0]) + (prior[0] - 1) * np.log(a) - prior[1] * a)
    assert r["fe"][0] == pytest.approx(F, rel=1e-13)


def _conditions(y, prior, init, it, tag):
    r = R.run(y, prior, init, it)
    assert r["S0"].min() >= 1.0, (tag, r["S0"].min())
    ok = ~np.isnan(y)
    p = np.random.default_rng(11).permutation(len(y))
    r2 = R.run(y[p], prior, init, it)
    moved = max(_rel(r2[k], r[k]) for k in ("a", "e", "f", "alpha"))
    moved = max(moved, float(np.max(np.abs(r2["fe"] - r["fe"]) / np.maximum(1.0, np.abs(r["fe"])))))
    assert moved < 1e-10, (tag, moved)
    assert r["n"] == ok.sum()
    return moved


def test_conditions_on_every_case():
    worst = 0.0
    extra = [(700 + i, N, K, 6) for i, (N, K) in enumerate([(40, 1), (90, 2), (120, 3), (200, 5), (240, 16), (77, 2), (150, 3), (260, 5)])]
    for seed, N, K, it in R.CPU_CASES + R.STREAMED_CASES + R.SMALL_CASES + R.OTHER_SINGLE + extra:
        worst = max(worst, _conditions(*R.make_problem(seed, N, K), it, (seed, N, K)))
    for seed, N, K, it, idx in R.NAN_CASES:
        y, prior, init = R.make_problem(seed, N, K)
        y[idx] = np.nan
        worst = max(worst, _conditions(y, prior, init, it, (seed, "nan")))
        worst = max(worst, _conditions(np.delete(y, idx), prior, init, it, (seed, "cut")))
    for seed, C, N, K, it, *_ in R.BATCH_CASES + R.OTHER_BATCH:
        Y, priors, inits = R.make_batch(seed, C, N, K)
        if seed == 603:
            Y[0, 5] = np.nan
        for c in range(C):
            worst = max(worst, _conditions(Y[c], [p[c] for p in priors], [q[c] for q in inits], it, (seed, c)))
    y, prior = R.golden()
    worst = max(worst, _conditions(y, prior, None, 50, "golden"))
    print("largest move of a history under a permutation of y: %.2e" % worst)


def test_reference_configuration_recorded():
    """the reference's priors, initialisation, 250 points, 50 iterations on the recorded numpy draw (tests/golden/make_gammamix_golden.py).  RECORDED holds
    THIS iteration's figures; the reference's test reports F = −146.8 ± 0.2, means 0.32, 0.33 and mixing (0.8, 0.2) on its own draw with its own point-mass
    optimiser, neither of which is on hand: the difference is recorded as an open item and nothing is tuned towards it."""
    y, prior = R.golden()
    y2, prior2 = R.recipe(43, 250)
    assert np.array_equal(y, y2) and all(np.array_equal(a, b) for a, b in zip(prior, prior2))
    r = R.run(y, prior, None, 50)
    means, mixing = r["a"][-1] / (r["e"][-1] / r["f"][-1]), r["alpha"][-1] / r["alpha"][-1].sum()
    print("reference configuration: F[0] %.6f F[-1] %.6f means %s mixing %s (the reference: -146.8, 0.32 / 0.33, 0.8 / 0.2)" % (r["fe"][0], r["fe"][-1], means, mixing))
    assert r["fe"][0] == pytest.approx(R.RECORDED["fe_first"], rel=1e-10) and r["fe"][-1] == pytest.approx(R.RECORDED["fe_last"], rel=1e-10)
    assert np.allclose(means, R.RECORDED["means"], rtol=1e-9) and np.allclose(mixing, R.RECORDED["mixing"], rtol=1e-9)

"""GPU tests of the dense path of the multivariate mixture engine (d = 5 … 32, K = 1 … 16, csrc/mvgmm_dense_kernels.hpp).

References: the C oracle rxo_mvgmm_vmp where it runs (d ≤ 8) and its NumPy restatement tests/mvgmm_ref.py at every d (pinned to the
oracle by tests/test_mvgmm_ref_cpu.py).  The contract is mvgmm_ref.hold, per (iteration, component): means 1e-6 posterior standard deviations
(and 1e-6 of the largest mean), cov and V 1e-6 relative to √(ref_aa · ref_bb), nu and alpha 1e-6 relative, free energy 1e-8 relative,
responsibilities 1e-9 absolute.  Cases: the dense groups of mvgmm_ref.CASES (shown to be well conditioned by tests/test_mvgmm_ref_cpu.py)."""
import numpy as np
import pytest

import rxhip
import rxoracle
from rxhip import graph

import mvgmm_ref
from mvgmm_ref import CASES, KEYS, Case, contract_errors, hold

pytestmark = pytest.mark.gpu

# the pass takes tiles of TILE points in a grid-stride loop over at most GRID_CAP workgroups (MVD_TP, MVD_GRID_CAP)
TILE, GRID_CAP = mvgmm_ref.DENSE_TILE, mvgmm_ref.DENSE_CAP


def case(d, K, N, iters, L=50.0, offset=0.0):
    """inputs and the NumPy reference of one ring case of the table, computed once and shared (read only): y, priors, init, reference"""
    c = Case(d, K, N, iters, L, offset)
    assert any(c in group for group in CASES.values()), c   # only cases whose conditioning the host tests have asserted
    return mvgmm_ref.case(c)


def run_engine(y, pri, init, iters, resp=True):
    with rxhip.MvGMMEngine(y.shape[0], *pri, *init, materialize_responsibilities=resp) as eng:
        eng.set_data(y)
        eng.run(iters, True)
        return eng.history(), eng.free_energy(), eng.responsibilities() if resp else None


def check_parity(h, fe, resp, ref, d, what):
    """the contract against a reference in the layout of mvgmm_ref.result(); every key, the free energy and the responsibilities must be there"""
    assert fe is not None and resp is not None and ref["fe"] is not None and ref["resp"] is not None
    return hold(dict(h, fe=fe, resp=resp), ref, what)


PARITY = [c[:4] for c in CASES["dense"]]   # what the shapes are chosen for: see the table


@pytest.mark.parametrize("d,K,N,iters", PARITY)
def test_parity_every_iteration(d, K, N, iters):
    y, pri, init, ref = case(d, K, N, iters)
    h, fe, resp = run_engine(y, pri, init, iters)
    check_parity(h, fe, resp, ref, d, f"vs restatement d={d} K={K} N={N}")
    if d <= 8:
        check_parity(h, fe, resp, mvgmm_ref.oracle(Case(d, K, N, iters)), d, f"vs oracle d={d} K={K} N={N}")
    print("fe", fe, "diff", np.diff(fe))
    assert np.all(np.diff(fe) < 1e-6 * np.abs(fe[-1]))   # free energy non-increasing (gmm_multivariate_tests.jl:139)


@pytest.mark.parametrize("d,K,N", [c[:3] for c in CASES["dense_soft"]])
def test_overlapping_clusters(d, K, N):
    """ring radius 6 instead of 50: the responsibilities are genuinely soft (radius 50 gives 0/1 assignments)"""
    y, pri, init, ref = case(d, K, N, 5, L=6.0)
    assert np.sum((ref["resp"] > 0.05) & (ref["resp"] < 0.95)) > 10
    h, fe, resp = run_engine(y, pri, init, 5)
    check_parity(h, fe, resp, ref, d, f"overlapping d={d} K={K}")


def test_offset_data():
    """1e4 added to every coordinate of data and prior means: the logits are formed from y − m̄ BEFORE the product, so nothing cancels there.
    The reference itself keeps the parity bounds at this offset (checked here against its own unshifted run: the statistics Σπyy' lose
    ≈ 2e-8 relative in V, 1e-10 in the free energy), so the offset is not lowered."""
    d, K, N, iters, off = 16, 4, 600, 5, 1e4
    y, pri, init, ref = case(d, K, N, iters, offset=off)
    _, _, _, ref0 = case(d, K, N, iters)
    hold(dict(ref, mean=ref["mean"] - off), ref0, "the reference, offset 1e4 against unshifted")
    h, fe, resp = run_engine(y, pri, init, iters)
    check_parity(h, fe, resp, ref, d, "offset 1e4")


def test_grid_stride():
    """more points than one pass of the grid covers: GRID_CAP workgroups × TILE points"""
    d, K, iters = 5, 2, 2
    N = GRID_CAP * TILE + 3 * TILE + 37
    c = Case(d, K, N, iters, kind="axis")   # two clusters on the first axis
    assert c in CASES["dense_stride"]
    y, pri, init, ref = mvgmm_ref.case(c)
    h, fe, resp = run_engine(y, pri, init, iters)
    check_parity(h, fe, resp, ref, d, f"grid stride N={N}")


def test_determinism():
    y, pri, init, _ = case(17, 16, 1500, 4)
    runs = []
    with rxhip.MvGMMEngine(y.shape[0], *pri, *init, materialize_responsibilities=True) as eng:
        eng.set_data(y)
        for _ in range(2):
            eng.run(4, True)
            runs.append((eng.history()["raw"].copy(), eng.free_energy().copy(), eng.responsibilities().copy()))
    h2, f2, r2 = run_engine(y, pri, init, 4)
    runs.append((h2["raw"], f2, r2))
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], other))


SPLIT = (17, 3, 1500, 4)


def _two_engine_worker(rank, out_dir):
    """Child process: two engines on halves of the data, B's statistics added into A's through statistics_tensor() before the update.
    torch adopts the device buffers, so it has to bring the GPU up itself, before the library does: hence a process of its own
    (as tests/test_gmm_gpu.py::_mp_worker)."""
    import os

    import torch

    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")   # brings torch's runtime up now
    d, K, N, iters = SPLIT
    y, pri, init, _ = case(d, K, N, iters)
    half = N // 2
    with rxhip.MvGMMEngine(half, *pri, *init, device=0) as A, rxhip.MvGMMEngine(N - half, *pri, *init, device=0) as B:
        A.set_data(np.ascontiguousarray(y[:half]))
        B.set_data(np.ascontiguousarray(y[half:]))
        A.begin_run(iters)
        B.begin_run(iters)
        ta, tb = A.statistics_tensor(), B.statistics_tensor()
        for _ in range(iters):
            A.accumulate()
            B.accumulate()
            A.sync()   # the statistics are produced on the engines' streams, the sum runs on torch's
            B.sync()
            ta += tb
            tb.copy_(ta)
            torch.cuda.synchronize()
            A.update(True)
            B.update(True)
        np.savez(os.path.join(out_dir, "split.npz"), ha=A.history()["raw"], fa=A.free_energy(), hb=B.history()["raw"], fb=B.free_energy(),
                 n=A.statistics_device()[1])


def test_split_phase(tmp_path):
    d, K, N, iters = SPLIT
    y, pri, init, _ = case(d, K, N, iters)
    h0, f0, r0 = run_engine(y, pri, init, iters)
    nq = K * (1 + d + d * (d + 1) // 2) + 1
    with rxhip.MvGMMEngine(N, *pri, *init, materialize_responsibilities=True) as eng:
        eng.set_data(y)
        eng.begin_run(iters)
        for _ in range(iters):
            eng.accumulate()
            eng.update(True)
        assert eng.statistics_device()[1] == nq
        assert np.array_equal(eng.history()["raw"], h0["raw"]) and np.array_equal(eng.free_energy(), f0) and np.array_equal(eng.responsibilities(), r0)
    import torch.multiprocessing as mp

    mp.spawn(_two_engine_worker, args=(str(tmp_path),), nprocs=1, join=True)
    r = np.load(tmp_path / "split.npz")
    assert int(r["n"]) == nq
    e = contract_errors(rxoracle.mvgmm_unpack(r["ha"], d), h0)
    print("two engines", " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    # engine against engine, not parity: the bound of 1e-12 on the norm over the whole history stays for every key as it was (the per-component
    # norm at a bound the summation order allows would not imply it); per (iteration, component) the halves' other summation order gets what the
    # host reference shows between two orders on this case (1.1e-13 in V, 2.7e-11 sd in the means) with a decade and a half over it
    ha = rxoracle.mvgmm_unpack(r["ha"], d)
    assert all(mvgmm_ref.rel(ha[key], h0[key]) < 1e-12 for key in KEYS), e
    assert e["mean"] < 1e-9 and all(e[key] < 1e-10 for key in KEYS[1:]), e
    efe = float(np.max(np.abs(r["fa"] - f0) / np.abs(f0)))
    print(f"two engines fe rel {efe:.2e}")
    assert efe < 1e-12
    assert np.array_equal(r["ha"], r["hb"]) and np.array_equal(r["fa"], r["fb"])


def test_through_the_graph():
    d, K, N, iters = 12, 3, 200, 4
    y, pri, init, _ = case(d, K, N, iters)
    mu0, S0, nu0, V0, al0 = pri
    gb, ys = graph.mv_mixture_graph(N, mu0, S0, nu0, V0, al0, init=dict(m=(init[0], init[1]), w=(init[2], init[3]), s=init[4]))
    e1 = graph.create_vmp_engine_from_graph(gb.tables()[0])
    e1.set_data(y)
    e1.run(iters, True)
    h1, f1 = e1.history()["raw"], e1.free_energy()
    e1.close()
    h2, f2, _ = run_engine(y, pri, init, iters, resp=False)
    assert np.array_equal(h1, h2["raw"]) and np.array_equal(f1, f2)
    # the K = 1 iid form (mv_iid_precision_tests.jl:11-15) at d = 6
    d, n = 6, 300
    rng = np.random.default_rng(5)
    Lm = rng.standard_normal((d, d))
    yi = rng.multivariate_normal(rng.random(d), Lm @ Lm.T + np.eye(d), size=n)
    gb, ys = graph.mv_iid_graph(n, np.zeros(d), 100.0 * np.eye(d), d + 1.0, np.eye(d), init=dict(m=(np.zeros(d), np.eye(d)), w=(float(d + 1), np.eye(d))))
    e = graph.create_vmp_engine_from_graph(gb.tables()[0])
    e.set_data(yi)
    e.run(5, True)
    hi, fi = e.history(), e.free_energy()
    e.close()
    one = lambda a: np.asarray(a)[None]
    c = Case(d, 1, n, 5, kind="iid")
    assert c in CASES["dense_other"] and np.array_equal(mvgmm_ref.inputs(c)[0], yi)
    o = mvgmm_ref.oracle(c)
    hold(dict(hi, fe=fi), dict(o, resp=None), "iid d = 6 through the graph")


def _create(d, K, N=10, **over):
    a = dict(mu0=np.zeros((K, d)), S0=np.tile(np.eye(d), (K, 1, 1)), nu0=np.full(K, d + 1.0), V0=np.tile(np.eye(d), (K, 1, 1)), al0=np.ones(K))
    a.update(over)
    pri = (a["mu0"], a["S0"], a["nu0"], a["V0"], a["al0"])
    init = (np.zeros((K, d)), np.tile(np.eye(d), (K, 1, 1)), np.full(K, d + 1.0), np.tile(np.eye(d), (K, 1, 1)), np.ones(K))
    return rxhip.MvGMMEngine(N, *pri, *init)


def test_error_paths():
    for d, K in ((33, 2), (5, 17)):
        with pytest.raises(rxhip.RxHipError) as ei:
            _create(d, K)
        assert ei.value.status == 2   # UNSUPPORTED
    with pytest.raises(rxhip.RxHipError) as ei:   # Wishart degrees of freedom must exceed d − 1
        _create(9, 2, nu0=np.full(2, 8.0))
    assert ei.value.status == 3       # NOT_POSDEF
    bad = np.eye(9)
    bad[0, 1] = bad[1, 0] = 2.0
    with pytest.raises(rxhip.RxHipError) as ei:   # indefinite prior covariance
        _create(9, 2, S0=np.tile(bad, (2, 1, 1)))
    assert ei.value.status == 3

    def nan_status(d):
        rng = np.random.default_rng(d)
        y = rng.standard_normal((40, d)) + 5.0 * rng.integers(0, 2, (40, 1))
        y[7, 1] = np.nan
        try:
            with _create(d, 2, N=40) as e:
                e.set_data(y)
                e.run(2, True)
                e.free_energy()
            return 0
        except rxhip.RxHipError as ex:
            return ex.status

    s4, s5 = nan_status(4), nan_status(5)
    assert s5 == s4 and s5 != 0

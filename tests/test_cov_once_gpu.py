"""The per-chain covariance array of a shared-model batch is stored once, not per sweep (rxhip_set_covariance_mode mode 0).

k_backward_sh / k_backward_sh_rev and the split schedule of the MFMA path do not compute posterior covariances: they copy a per-model table
that is built at creation.  A smoothing sweep stores the array only when it does not already hold that broadcast
(rxhip_engine_life::cov_current); means and free energy are recomputed every sweep.  RXHIP_COV_EVERY_SWEEP=1 keeps a store per sweep and is
the comparison arm: everything a caller can read must agree with it bit for bit, and rxhip_get_covariance_writes shows that the stores
were in fact skipped — or, after a filtering run, a setter or a new owner of a pooled engine, that they were not.

Models, seeds and the oracle's measures are those of tests/test_boundary_in_sweep_gpu.py (see there for the seeds)."""
import os

import numpy as np
import pytest

import rxhip
import rxoracle
from rxhip import workloads

pytestmark = pytest.mark.gpu

MODELS = {
    (4, 4): workloads.c1_model,
    (2, 2): lambda: workloads.random_model(2, 2, 4),
    (3, 2): lambda: workloads.random_model(3, 2, 20),
}
# chains, T, segments: one segment; fewer segments than the prologue's ring; a ragged last segment; many short segments
SHAPES = [(64, 37, 1), (64, 37, 2), (128, 203, 5), (64, 1025, 128)]
ORACLE_SHAPES = [(128, 203, 5), (64, 1025, 128)]
POOL_SHAPE = (128, 203, 5)   # T · chains ≤ 65 536: rxhip_destroy parks the engine
SEEDS = (17, 101, 17)        # data a, b, a

_keys = pytest.mark.parametrize("key", list(MODELS), ids=lambda k: f"d{k[0]}dy{k[1]}")
_shapes = pytest.mark.parametrize("C,T,S", SHAPES, ids=lambda v: str(v))
_records = pytest.mark.parametrize("records", [False, True], ids=["reverse_filter", "mean_records"])


class _Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _env(records=False, every=False, **more):
    return _Env(RXHIP_TEST_HOOKS="1", RXHIP_ONE_PASS="1", RXHIP_MEAN_RECORDS="1" if records else "0",
                RXHIP_COV_EVERY_SWEEP="1" if every else "0", **more)


def _engine(mdl, T, C, S, **kw):
    return rxhip.LGSSMEngine(mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], T=T, n_chains=C, segments=S, device=0, **kw)


def _results(eng):
    mean, cov = eng.marginals_of_chains(np.arange(eng.n_chains))
    return np.array(mean), np.array(cov), np.array(eng.free_energy_per_chain()), np.array(eng.free_energy())


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


_data, _cache = {}, {}


def _y(key, T, C, seed):
    k = (key, T, C, seed)
    if k not in _data:
        _data[k] = workloads.generate_batch(MODELS[key](), T, C, seed0=seed)
    return _data[k]


def _sequence(key, C, T, S, records, every):
    """One engine runs data a, b, a: (stride, [results after each run], covariance_writes).  Computed once per arm and shared, never modified."""
    k = ("seq", key, C, T, S, records, every)
    if k not in _cache:
        with _env(records, every):
            with _engine(MODELS[key](), T, C, S) as eng:
                K, out = eng.mean_checkpoint_stride(), []
                for seed in SEEDS:
                    eng.set_data(_y(key, T, C, seed))
                    eng.run(iterations=1, free_energy=True)
                    out.append(_results(eng))
                _cache[k] = (K, out, eng.covariance_writes())
    return _cache[k]


def _skip_without_stride(key, C, T, S, records):
    if not records and _sequence(key, C, T, S, False, False)[0] == 0:
        pytest.skip(f"model {key}: no admissible checkpoint stride at T = {T}, S = {S}: the reverse-filter schedule is not taken")


@_keys
@_shapes
@_records
def test_bit_identical_to_a_store_per_sweep(key, C, T, S, records):
    _skip_without_stride(key, C, T, S, records)
    K, new, n_new = _sequence(key, C, T, S, records, every=False)
    K1, ref, n_ref = _sequence(key, C, T, S, records, every=True)
    assert K1 == K and (K == 0) == records
    for run, (a, b) in enumerate(zip(new, ref)):
        assert _same(a, b), run
        assert all(np.all(np.isfinite(x)) for x in a)
    assert not np.array_equal(new[0][0], new[1][0]) and np.array_equal(new[0][0], new[2][0])   # the means follow the data
    assert np.array_equal(new[0][1], new[1][1])                                                 # the covariances do not
    assert (n_new, n_ref) == (1, 3)


@_keys
@_shapes
@_records
def test_iterations_of_one_run(key, C, T, S, records):
    _skip_without_stride(key, C, T, S, records)
    out = []
    for every in (False, True):
        with _env(records, every):
            with _engine(MODELS[key](), T, C, S) as eng:
                eng.set_data(_y(key, T, C, 17))
                eng.run(iterations=3, free_energy=True)
                out.append((_results(eng), eng.covariance_writes()))
    assert _same(out[0][0], out[1][0])
    assert out[0][0][3].shape == (3,)
    assert (out[0][1], out[1][1]) == (1, 3)
    assert _same(out[0][0][:3], _sequence(key, C, T, S, records, every=True)[1][0][:3])


def _filter_steps(eng, key, T, C):
    y = _y(key, T, C, 17)
    eng.filter_step(y[0])
    eng.filter_step(y[1])


@_keys
@_shapes
@_records
@pytest.mark.parametrize("between", ["run_filter", "set_covariance_mode", "set_fixed_point_exits", "filter_step"])
def test_invalidation(key, C, T, S, records, between):
    """Whatever may have changed the array, or is documented to ask for a rewrite, costs the next smoothing sweep its stores — and only that one."""
    _skip_without_stride(key, C, T, S, records)
    ref = _sequence(key, C, T, S, records, every=True)[1]
    with _env(records):
        with _engine(MODELS[key](), T, C, S) as eng:
            eng.set_data(_y(key, T, C, 17))
            eng.run(iterations=1, free_energy=True)
            assert _same(_results(eng), ref[0]) and eng.covariance_writes() == 1
            if between == "run_filter":
                eng.run_filter(True)
                cov_f = np.array(eng.marginals_of_chains(np.arange(C))[1])
                assert not np.array_equal(cov_f, ref[0][1])   # the filtered covariances are in the array now: the case bites
                assert eng.covariance_writes() == 1           # (a filtering run is no smoothing sweep)
            elif between == "set_covariance_mode":
                eng.set_covariance_mode(0)
            elif between == "set_fixed_point_exits":
                eng.set_fixed_point_exits(1)
            else:
                _filter_steps(eng, key, T, C)
            eng.set_data(_y(key, T, C, 101))
            eng.run(iterations=1, free_energy=True)
            assert _same(_results(eng), ref[1])
            assert eng.covariance_writes() == 2
            eng.set_data(_y(key, T, C, 17))
            eng.run(iterations=1, free_energy=True)        # … and the run after it skips them again
            assert _same(_results(eng), ref[2])
            assert eng.covariance_writes() == 2


@_keys
def test_a_pooled_engine_starts_over(key):
    """rxhip_destroy parks the engine with the first owner's covariances in its array; the next owner of the same descriptor gets a fresh
    life (rxhip_engine_life) and stores them itself."""
    C, T, S = POOL_SHAPE
    _skip_without_stride(key, C, T, S, False)
    mdl = MODELS[key]()
    with _env(every=True, RXHIP_ENGINE_POOL="0"):   # never parked, never revived, a store per sweep
        with _engine(mdl, T, C, S) as eng:
            eng.set_data(_y(key, T, C, 101))
            eng.run(iterations=1, free_energy=True)
            want = _results(eng)
    with _env():
        with _engine(mdl, T, C, S) as eng:
            eng.set_data(_y(key, T, C, 17))
            eng.run(iterations=1, free_energy=True)
            assert eng.covariance_writes() == 1
        with _engine(mdl, T, C, S) as eng:
            assert eng.covariance_writes() == 0
            eng.set_data(_y(key, T, C, 101))
            eng.run(iterations=1, free_energy=True)
            assert _same(_results(eng), want)
            assert eng.covariance_writes() == 1


@_keys
@pytest.mark.parametrize("C,T,S", ORACLE_SHAPES, ids=lambda v: str(v))
@_records
def test_oracle_parity_of_a_sweep_without_stores(key, C, T, S, records):
    """The second run of the sequence (data b: its sweep stored no covariance), first and last chain against the CPU oracle with the measures
    and bounds of the benchmark's parity check; lgssm_bp at dy = d, lgssm_kalman_rts at dy < d (tests/test_boundary_in_sweep_gpu.py says why)."""
    _skip_without_stride(key, C, T, S, records)
    _, runs, n = _sequence(key, C, T, S, records, every=False)
    assert n == 1
    mean, cov, fec, _ = runs[1]
    mdl, y = MODELS[key](), _y(key, T, C, 101)
    for c in (0, C - 1):
        args = (mdl["A"], mdl["B"], mdl["P"], mdl["Q"], mdl["m0"], mdl["V0"], np.ascontiguousarray(y[:, c]))
        om, oc, ofe = rxoracle.lgssm_bp(*args)[:3] if key[1] == key[0] else rxoracle.lgssm_kalman_rts(*args)
        sd = np.sqrt(np.einsum("tii->ti", oc))
        mean_rel = float(np.max(np.abs(mean[c] - om) / sd))
        cov_rel = float(np.max(np.abs(cov[c] - oc) / np.max(np.abs(oc), axis=(1, 2), keepdims=True)))
        fe_rel = float(abs(fec[c] - ofe) / abs(ofe))
        print(f"{key} {C}x{T} chain {c}: mean {mean_rel:.2e} cov {cov_rel:.2e} fe {fe_rel:.2e}")
        assert mean_rel < 1e-6 and cov_rel < 1e-6 and fe_rel < 1e-8, (mean_rel, cov_rel, fe_rel)


def _outside(kind):
    """(constructor, data a, data b) of an engine the rule does not apply to: its covariances are computed in the sweep, or its array has rows
    the table does not cover."""
    mdl = workloads.c1_model()
    T, S = 203, 5
    C = 65 if kind == "65_chains" else 64
    ya, yb = (workloads.generate_batch(mdl, T, C, seed0=s) for s in (17, 101))
    kw = {}
    if kind == "chain_model":
        mdl = {k: np.repeat(np.asarray(v)[None], C, 0) for k, v in mdl.items()}
        kw = dict(chain_model=np.arange(C, dtype=np.int32))
    elif kind == "allow_missing":
        ya, yb = ya.copy(), yb.copy()
        ya[5, 3], yb[7, 2] = np.nan, np.nan
        kw = dict(allow_missing=True)
    elif kind == "horizon":
        kw = dict(horizon=3)
    if kind == "noise":
        dy = 4
        make = lambda: rxhip.LGSSMNoiseEngine(mdl["A"], mdl["B"], mdl["P"], mdl["m0"], mdl["V0"], T, dy + 2.0, np.eye(dy), n_chains=C, segments=S, device=0)
    else:
        make = lambda: _engine(mdl, T, C, S, **kw)
    return make, ya, yb


@pytest.mark.parametrize("kind", ["65_chains", "chain_model", "allow_missing", "horizon", "noise"])
def test_engines_outside_the_rule_store_every_sweep(kind):
    make, ya, yb = _outside(kind)
    with _env():
        with make() as eng:
            eng.set_data(yb)
            eng.run(iterations=1, free_energy=True)
            want = _results(eng)
            assert eng.covariance_writes() == 1
        with make() as eng:
            eng.set_data(ya)
            eng.run(iterations=1, free_energy=True)
            first = _results(eng)
            eng.set_data(yb)
            eng.run(iterations=1, free_energy=True)
            assert eng.covariance_writes() == 2   # both sweeps wrote covariances
            assert _same(_results(eng), want)
            assert not np.array_equal(first[0], want[0])


def _split(mode, every):
    """d = 8, dy = 4, 64 chains, T = 200 on the model / data split of the MFMA path: two runs on different data, the getter after each."""
    k = ("split", mode, every)
    if k not in _cache:
        d, dy, C, T = 8, 4, 64, 200
        m = workloads.random_model(d, dy, seed=5)
        with _Env(RXHIP_TEST_HOOKS="1", RXHIP_DENSE_SPLIT="1", RXHIP_COV_EVERY_SWEEP="1" if every else "0"):
            with rxhip.LGSSMEngine(m["A"], m["B"], m["P"], m["Q"], m["m0"], m["V0"], T=T, n_chains=C, device=0) as eng:
                eng.set_covariance_mode(mode)
                out = []
                for seed in (3, 77):
                    eng.set_data(workloads.generate_batch(m, T, C, seed0=seed))
                    eng.run(iterations=1, free_energy=True)
                    out.append(_results(eng))
                _cache[k] = (out, eng.covariance_writes())
    return _cache[k]


def test_split_schedule_stores_once():
    new, n_new = _split(0, every=False)
    ref, n_ref = _split(0, every=True)
    assert _same(new[0], ref[0]) and _same(new[1], ref[1])
    assert not np.array_equal(new[0][0], new[1][0]) and np.array_equal(new[0][1], new[1][1])
    assert (n_new, n_ref) == (1, 2)


def test_split_schedule_on_request_is_unchanged():
    """Mode 1 followed by a getter: one materialisation, whatever the hook says; the same arrays as mode 0."""
    new, n_new = _split(1, every=False)
    ref, n_ref = _split(1, every=True)
    assert _same(new[0], ref[0]) and _same(new[1], ref[1])
    assert (n_new, n_ref) == (1, 1)
    mode0 = _split(0, every=True)[0]
    assert _same(new[0], mode0[0]) and _same(new[1], mode0[1])

"""The Python classes over a handle: their public surface may only grow, every one inherits the one base class, a refused creation leaves no handle
behind, and `infer` keeps its boundary — what it checks before an engine exists propagates even with catch_exception, what the engine refuses comes
back as the result's error.  No device is needed (the construction checks run only where none is visible, as the *_abi tests do).

PARENT is the surface at the commit before the engine classes got a base class, written by

    import inspect, pprint, rxhip, rxhip.tree
    classes = [c for c in vars(rxhip).values() if inspect.isclass(c) and c.__module__ == "rxhip.engine"] + [rxhip.tree.TreeEngine]
    table = {}
    for c in classes:
        names = sorted(n for n in dir(c) if not n.startswith("_"))
        table[c.__name__] = {n: str(inspect.signature(getattr(c, n))) if callable(getattr(c, n)) else None for n in ["__init__"] + names}
    pprint.pprint(table, width=150, sort_dicts=True)

(None: a public attribute that is not callable)."""
import inspect

import numpy as np
import pytest

import rxhip
from rxhip import _lib, graph
from rxhip.engine import _Engine
from rxhip.tree import TreeEngine

PARENT = \
{'ARRegressionEngine': {'__init__': '(self, N, d, prior_theta=None, prior_gamma=(1.0, 1.0), init_gamma=None, n_series=1, lagged=False, '
                                    'share_parameters=False, device=-1, stream=None)',
                        'close': '(self)',
                        'counters': '(self)',
                        'free_energy': '(self)',
                        'free_energy_per_chain': '(self)',
                        'parameters': '(self)',
                        'run': '(self, iterations=1, free_energy=True)',
                        'run_async': '(self, iterations=1, free_energy=True)',
                        'schedule': '(n_rows, d)',
                        'set_data': "(self, y, layout='time_chain')",
                        'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
                        'set_observations': '(self, y)',
                        'set_regressors': '(self, X)',
                        'statistics': '(self)',
                        'stream': '(self)',
                        'sync': '(self)'},
 'BinomialRegressionEngine': {'__init__': '(self, N, d, prior_xi, prior_precision, init=None, n_problems=1, device=-1, stream=None)',
                              'close': '(self)',
                              'counters': '(self)',
                              'free_energy': '(self)',
                              'free_energy_per_chain': '(self)',
                              'parameters': '(self)',
                              'run': '(self, iterations=1, free_energy=True)',
                              'run_async': '(self, iterations=1, free_energy=True)',
                              'schedule': '(N, d)',
                              'set_data': '(self, X, y, n_trials)',
                              'set_observations': '(self, y)',
                              'set_regressors': '(self, X)',
                              'set_trials': '(self, n_trials)',
                              'stream': '(self)',
                              'sync': '(self)'},
 'Communicator': {'__init__': '(self, nranks, unique_id, rank, device=-1)', 'close': '(self)', 'unique_id': '()'},
 'DriftChainEngine': {'__init__': '(self, T, m0, v0, c, obs_var, n_chains=1, prior_through_transition=True, device=-1, stream=None)',
                      'allreduce_free_energy': '(self, comm)',
                      'close': '(self)',
                      'counters': '(self)',
                      'free_energy': '(self)',
                      'free_energy_per_chain': '(self)',
                      'kernel_times': '(self)',
                      'marginals': "(self, layout='time_chain', want_cov=True)",
                      'marginals_of_chains': '(self, chains, want_cov=True)',
                      'reset_kernel_times': '(self)',
                      'run': '(self, iterations=1, free_energy=True)',
                      'run_async': '(self, iterations=1, free_energy=True)',
                      'set_data': "(self, y, layout='time_chain')",
                      'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
                      'set_profiling': '(self, on=True)',
                      'stream': '(self)',
                      'sync': '(self)'},
 'GMMEngine': {'__init__': '(self, N, mu0, v0, a0, b0, alpha0, init_m_mean, init_m_var, init_p_shape, init_p_rate, init_s_alpha, '
                           'materialize_responsibilities=False, device=-1, stream=None)',
               'accumulate': '(self)',
               'allreduce_free_energy': '(self, comm)',
               'allreduce_statistics': '(self, comm)',
               'begin_run': '(self, iterations)',
               'close': '(self)',
               'counters': '(self)',
               'free_energy': '(self)',
               'free_energy_device': '(self)',
               'history': '(self)',
               'kernel_times': '(self)',
               'reset_kernel_times': '(self)',
               'responsibilities': '(self)',
               'run': '(self, iterations=1, free_energy=True)',
               'run_async': '(self, iterations=1, free_energy=True)',
               'set_data': '(self, y)',
               'set_data_device': '(self, ptr, n, keepalive=None)',
               'set_profiling': '(self, on=True)',
               'statistics_device': '(self)',
               'statistics_tensor': '(self)',
               'stream': '(self)',
               'sync': '(self)',
               'update': '(self, free_energy=True)'},
 'GammaMixtureEngine': {'SCHEDULES': None,
                        '__init__': '(self, N, K, prior_a, prior_b, prior_alpha, init_a=None, init_b=None, init_s=None, n_problems=1, '
                                    "schedule='auto', materialize=False, device=-1, stream=None)",
                        'close': '(self)',
                        'counters': '(self)',
                        'free_energy': '(self)',
                        'free_energy_per_chain': '(self)',
                        'history': '(self)',
                        'kernel_times': '(self)',
                        'responsibilities': '(self)',
                        'run': '(self, iterations=1, free_energy=True)',
                        'run_async': '(self, iterations=1, free_energy=True)',
                        'schedule': '(N, K)',
                        'set_data': "(self, y, layout='time_chain')",
                        'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
                        'set_profiling': '(self, on=True)',
                        'set_stored_log': '(self, stored)',
                        'stream': '(self)',
                        'sync': '(self)'},
 'HGFEngine': {'__init__': '(self, T, n_series, kappa, omega, z_variance, y_variance, z0=(0.0, 5.0), x0=(0.0, 5.0), n_gh=31, device=-1, stream=None)',
               'allreduce_free_energy': '(self, comm)',
               'close': '(self)',
               'copy_free_energy_to_device': '(self, dst_ptr)',
               'counters': '(self)',
               'free_energy': '(self)',
               'free_energy_device': '(self)',
               'free_energy_per_chain': '(self)',
               'history': "(self, layout='time_chain')",
               'kernel_times': '(self)',
               'reset_kernel_times': '(self)',
               'run': '(self, iterations=1, free_energy=True)',
               'run_async': '(self, iterations=1, free_energy=True)',
               'set_data': "(self, y, layout='time_chain')",
               'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
               'set_profiling': '(self, on=True)',
               'stream': '(self)',
               'sync': '(self)'},
 'HMMEngine': {'__init__': '(self, T, prior_A, prior_B, prior_s0, init_A=None, init_B=None, n_series=1, share_parameters=False, device=-1, '
                           'stream=None)',
               'close': '(self)',
               'counters': '(self)',
               'free_energy': '(self)',
               'free_energy_per_chain': '(self)',
               'parameters': '(self)',
               'run': '(self, iterations=1, free_energy=True)',
               'run_async': '(self, iterations=1, free_energy=True)',
               'set_data': "(self, y, layout='time_chain')",
               'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
               'states': "(self, layout='time_chain')",
               'stream': '(self)',
               'sync': '(self)'},
 'LAREngine': {'__init__': '(self, T, order, tau, prior_theta=None, prior_gamma=(1.0, 1.0), prior_x0=None, init_theta=None, init_gamma=None, '
                           'n_series=1, share_parameters=False, device=-1, stream=None)',
               'close': '(self)',
               'counters': '(self)',
               'free_energy': '(self)',
               'free_energy_per_chain': '(self)',
               'parameters': '(self)',
               'run': '(self, iterations=1, free_energy=True)',
               'run_async': '(self, iterations=1, free_energy=True)',
               'set_data': "(self, y, layout='time_chain')",
               'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
               'states': "(self, layout='time_chain')",
               'stream': '(self)',
               'sync': '(self)'},
 'LGSSMEngine': {'__init__': '(self, A, B, P, Q, m0, V0, T, n_chains=1, chain_model=None, prior_through_transition=False, segments=0, device=-1, '
                             'stream=None, horizon=0, allow_missing=False, step_model=None, state_offset=None, obs_offset=None)',
                 'allreduce_free_energy': '(self, comm)',
                 'close': '(self)',
                 'copy_free_energy_to_device': '(self, dst_ptr)',
                 'counters': '(self)',
                 'covariance_writes': '(self)',
                 'create_stages': '(self)',
                 'filter_reset': '(self)',
                 'filter_step': '(self, y, want_cov=True, free_energy=True)',
                 'free_energy': '(self)',
                 'free_energy_device': '(self)',
                 'free_energy_per_chain': '(self)',
                 'infer': '(self, y, iterations=1, free_energy=True, want_cov=True, filtering=False)',
                 'kernel_times': '(self)',
                 'marginals': "(self, layout='time_chain', want_cov=True)",
                 'marginals_device': '(self)',
                 'marginals_of_chains': '(self, chains, want_cov=True)',
                 'mean_checkpoint_stride': '(self)',
                 'model_tables_ms': '(self)',
                 'node_marginals': "(self, layout='time_chain')",
                 'predictions': "(self, layout='time_chain', want_cov=True)",
                 'reset_kernel_times': '(self)',
                 'run': '(self, iterations=1, free_energy=True)',
                 'run_async': '(self, iterations=1, free_energy=True)',
                 'run_filter': '(self, free_energy=True)',
                 'run_filter_async': '(self, free_energy=True)',
                 'schedule': '(self)',
                 'set_chain_offsets': "(self, state_offset=None, obs_offset=None, layout='time_chain')",
                 'set_covariance_mode': '(self, mode)',
                 'set_data': "(self, y, layout='time_chain')",
                 'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
                 'set_fixed_point_exits': '(self, enabled)',
                 'set_inputs': "(self, u, layout='time_chain')",
                 'set_offsets': '(self, state_offset=None, obs_offset=None)',
                 'set_profiling': '(self, on=True)',
                 'stream': '(self)',
                 'sync': '(self)'},
 'LGSSMNoiseEngine': {'__init__': '(self, A, B, P, m0, V0, T, nu0, S0, init_nu=None, init_V=None, n_chains=1, prior_through_transition=False, '
                                  'segments=0, device=-1, stream=None)',
                      'allreduce_free_energy': '(self, comm)',
                      'close': '(self)',
                      'continue_runs': '(self, on=True)',
                      'copy_free_energy_to_device': '(self, dst_ptr)',
                      'counters': '(self)',
                      'covariance_writes': '(self)',
                      'create_stages': '(self)',
                      'filter_reset': '(self)',
                      'filter_step': '(self, y, want_cov=True, free_energy=True)',
                      'free_energy': '(self)',
                      'free_energy_device': '(self)',
                      'free_energy_per_chain': '(self)',
                      'infer': '(self, y, iterations=1, free_energy=True, want_cov=True, filtering=False)',
                      'kernel_times': '(self)',
                      'marginals': "(self, layout='time_chain', want_cov=True)",
                      'marginals_device': '(self)',
                      'marginals_of_chains': '(self, chains, want_cov=True)',
                      'mean_checkpoint_stride': '(self)',
                      'model_tables_ms': '(self)',
                      'node_marginals': "(self, layout='time_chain')",
                      'noise_posterior': '(self)',
                      'predictions': "(self, layout='time_chain', want_cov=True)",
                      'reset_kernel_times': '(self)',
                      'run': '(self, iterations=1, free_energy=True)',
                      'run_async': '(self, iterations=1, free_energy=True)',
                      'run_filter': '(self, free_energy=True)',
                      'run_filter_async': '(self, free_energy=True)',
                      'schedule': '(self)',
                      'set_chain_offsets': "(self, state_offset=None, obs_offset=None, layout='time_chain')",
                      'set_covariance_mode': '(self, mode)',
                      'set_data': "(self, y, layout='time_chain')",
                      'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
                      'set_fixed_point_exits': '(self, enabled)',
                      'set_inputs': "(self, u, layout='time_chain')",
                      'set_offsets': '(self, state_offset=None, obs_offset=None)',
                      'set_profiling': '(self, on=True)',
                      'stream': '(self)',
                      'sync': '(self)'},
 'MultinomialRegressionEngine': {'__init__': '(self, N, K, prior_xi, prior_precision, n_trials=None, init=None, n_problems=1, online=False, '
                                             'keep_cov_history=False, device=-1, stream=None)',
                                 'close': '(self)',
                                 'counters': '(self)',
                                 'free_energy': '(self)',
                                 'free_energy_per_chain': '(self)',
                                 'history': '(self)',
                                 'kernel_times': '(self)',
                                 'parameters': '(self)',
                                 'run': '(self, iterations=1, free_energy=True)',
                                 'run_async': '(self, iterations=1, free_energy=True)',
                                 'schedule': '(N, K)',
                                 'set_data': '(self, Y)',
                                 'set_profiling': '(self, on=True)',
                                 'statistics': '(self)',
                                 'stream': '(self)',
                                 'sync': '(self)'},
 'MvGMMEngine': {'__init__': '(self, N, mu0, S0, nu0, V0, alpha0, init_m_mean, init_m_cov, init_w_nu, init_w_V, init_s_alpha, '
                             'materialize_responsibilities=False, device=-1, stream=None)',
                 'accumulate': '(self)',
                 'allreduce_free_energy': '(self, comm)',
                 'allreduce_statistics': '(self, comm)',
                 'begin_run': '(self, iterations)',
                 'close': '(self)',
                 'counters': '(self)',
                 'free_energy': '(self)',
                 'free_energy_device': '(self)',
                 'history': '(self)',
                 'kernel_times': '(self)',
                 'reset_kernel_times': '(self)',
                 'responsibilities': '(self)',
                 'run': '(self, iterations=1, free_energy=True)',
                 'run_async': '(self, iterations=1, free_energy=True)',
                 'set_data': '(self, y)',
                 'set_data_device': '(self, ptr, n, keepalive=None)',
                 'set_profiling': '(self, on=True)',
                 'statistics_device': '(self)',
                 'statistics_tensor': '(self)',
                 'stream': '(self)',
                 'sync': '(self)',
                 'update': '(self, free_energy=True)'},
 'ProbitEngine': {'__init__': '(self, T, a, c, q, m0, v0, n_series=1, n_gh=32, device=-1, stream=None)',
                  'allreduce_free_energy': '(self, comm)',
                  'close': '(self)',
                  'counters': '(self)',
                  'free_energy': '(self)',
                  'free_energy_per_chain': '(self)',
                  'kernel_times': '(self)',
                  'marginals': "(self, layout='time_chain')",
                  'reset_kernel_times': '(self)',
                  'run': '(self, iterations=1, free_energy=True)',
                  'run_async': '(self, iterations=1, free_energy=True)',
                  'set_data': "(self, y, layout='time_chain')",
                  'set_data_device': "(self, ptr, n, layout='time_chain', keepalive=None)",
                  'set_profiling': '(self, on=True)',
                  'stream': '(self)',
                  'sync': '(self)'},
 'TreeEngine': {'__init__': '(self, gb, n_replicas=1, device=-1, stream=None, force_executor=True, allow_missing=False)',
                'allreduce_free_energy': '(self, comm)',
                'close': '(self)',
                'continue_runs': '(self, on=True)',
                'counters': '(self)',
                'discrete': '(self, variable)',
                'free_energy': '(self)',
                'free_energy_per_replica': '(self)',
                'last_iteration_ms': '(self)',
                'marginals': '(self, variables)',
                'precision': '(self, variable)',
                'run': '(self, iterations=1, free_energy=True)',
                'set_autoupdates': '(self, table)',
                'set_data': '(self, variables, values)',
                'stream': '(self, variables, series, iterations=1, free_energy=True, history=())'}}


def _classes():
    found = [c for c in vars(rxhip).values() if inspect.isclass(c) and c.__module__ == "rxhip.engine"] + [TreeEngine]
    return {c.__name__: c for c in found}


def test_exported_classes_are_the_parents():
    assert set(_classes()) == set(PARENT)


@pytest.mark.parametrize("name", sorted(PARENT))
def test_public_surface_only_grew(name):
    cls = _classes()[name]
    for attr, signature in PARENT[name].items():
        assert hasattr(cls, attr), f"{name}.{attr} is gone"
        if signature is not None:
            assert str(inspect.signature(getattr(cls, attr))) == signature, f"{name}.{attr}"


def test_every_engine_class_inherits_the_one_base():
    for name, cls in _classes().items():
        assert issubclass(cls, _Engine) == (name != "Communicator"), name


_one, _o, _m = np.ones((1, 1)), np.ones(2), np.array([-1.0, 1.0])
_mu2, _eye2, _nu2 = np.stack([-np.ones(2), np.ones(2)]), np.stack([np.eye(2)] * 2), np.full(2, 3.0)
SMALLEST = {   # every engine class with its smallest valid arguments
    "LGSSMEngine": lambda new: new(rxhip.LGSSMEngine, 0.9 * _one, _one, 0.1 * _one, _one, np.zeros(1), _one, T=4),
    "LGSSMNoiseEngine": lambda new: new(rxhip.LGSSMNoiseEngine, 0.9 * _one, _one, 0.1 * _one, np.zeros(1), _one, 4, 3.0, _one),
    "GMMEngine": lambda new: new(rxhip.GMMEngine, 8, _m, 10 * _o, _o, _o, _o, _m, _o, _o, _o, _o),
    "MvGMMEngine": lambda new: new(rxhip.MvGMMEngine, 8, _mu2, 10 * _eye2, _nu2, _eye2 / 3.0, _o, _mu2, _eye2, _nu2, _eye2 / 3.0, _o),
    "HGFEngine": lambda new: new(rxhip.HGFEngine, 4, 1, 1.0, -2.0, 1.0, 1.0),
    "DriftChainEngine": lambda new: new(rxhip.DriftChainEngine, 4, 0.0, 1.0, 0.1, 1.0),
    "ProbitEngine": lambda new: new(rxhip.ProbitEngine, 4, 0.9, 0.0, 0.5, 0.0, 1.0),
    "HMMEngine": lambda new: new(rxhip.HMMEngine, 4, np.array([[3.0, 1.0], [1.0, 3.0]]), np.array([[4.0, 1.0], [1.0, 4.0]]), np.array([0.5, 0.5])),
    "LAREngine": lambda new: new(rxhip.LAREngine, 4, 1, 1.0),
    "BinomialRegressionEngine": lambda new: new(rxhip.BinomialRegressionEngine, 8, 1, np.zeros(1), np.eye(1)),
    "ARRegressionEngine": lambda new: new(rxhip.ARRegressionEngine, 8, 1),
    "MultinomialRegressionEngine": lambda new: new(rxhip.MultinomialRegressionEngine, 8, 3, np.zeros(2), np.eye(2)),
    "GammaMixtureEngine": lambda new: new(rxhip.GammaMixtureEngine, 8, 2, (_o, _o), (_o, _o), _o),
    "TreeEngine": lambda new: new(TreeEngine, graph.lgssm_graph(2, 0.9 * _one, _one, 0.1 * _one, _one, np.zeros(1), _one)[0]),
}


def test_smallest_arguments_cover_every_engine_class():
    assert set(SMALLEST) == set(PARENT) - {"Communicator"}


@pytest.mark.skipif(rxhip.lib().rxhip_device_count() > 0, reason="checks the no-device error path")
@pytest.mark.parametrize("name", sorted(SMALLEST))
def test_a_refused_creation_leaves_no_handle(name):
    made = []

    def new(cls, *args, **kw):   # the object survives the constructor's exception
        made.append(cls.__new__(cls))
        made[0].__init__(*args, **kw)

    with pytest.raises(rxhip.RxHipError) as ei:
        SMALLEST[name](new)
    assert ei.value.status == _lib.ERR_NO_DEVICE
    assert str(ei.value)[len(f"rxhip status {_lib.ERR_NO_DEVICE}: "):].strip()   # a message of its own after the status
    eng, = made
    assert type(eng).__name__ == name and eng._h is None
    eng.close()
    eng.close()


_rng = np.random.default_rng(3)
_gm = rxhip.gaussian_mixture(_m, 10 * _o, _o, _o)
_mvgm = rxhip.multivariate_gaussian_mixture(_mu2, 10 * _eye2, _nu2, _eye2 / 3.0)
_ssm = (0.9 * _one, _one, 0.1 * _one, _one, np.zeros(1), _one)
_counts = _rng.integers(0, 5, (8, 3)).astype(np.float64)
CALLS = {   # one model of each family of `infer`, with the keywords it needs
    "mixture": dict(model=_gm, data={"y": _rng.standard_normal(8)},
                    initialization={"m": rxhip.NormalMeanVariance(_m, _o), "p": rxhip.GammaShapeRate(_o, _o)}),
    "mv_mixture": dict(model=_mvgm, data={"y": _rng.standard_normal((8, 2))},
                       initialization={"m": rxhip.MvNormalMeanCovariance(_mu2, _eye2), "w": rxhip.Wishart(_nu2, _eye2 / 3.0)}),
    "hgf": dict(model=rxhip.hierarchical_gaussian_filter(1.0, -2.0, 1.0, 1.0), data={"y": _rng.standard_normal(4)}),
    "drift": dict(model=rxhip.univariate_drift_chain(0.0, 1.0, 0.1, 1.0), data={"y": _rng.standard_normal(4)}),
    "probit": dict(model=rxhip.probit_ssm(0.9, 0.0, 0.5, 0.0, 1.0), data={"y": np.array([1.0, 0.0, 1.0, 1.0])}),
    "hmm": dict(model=rxhip.hidden_markov_model([[3.0, 1.0], [1.0, 3.0]], [[4.0, 1.0], [1.0, 4.0]], [0.5, 0.5]), data={"x": np.array([0.0, 1.0, 1.0, 0.0])}),
    "lar": dict(model=rxhip.latent_autoregressive(1, 1.0), data={"y": _rng.standard_normal(4)}),
    "binreg": dict(model=rxhip.binomial_regression(np.zeros(1), np.eye(1)),
                   data={"X": np.linspace(-1.0, 1.0, 8).reshape(8, 1), "y": np.array([0.0, 1.0, 0.0, 2.0, 1.0, 3.0, 2.0, 3.0]), "n_trials": np.full(8, 3.0)}),
    "arreg_lagged": dict(model=rxhip.autoregression(1), data={"y": _rng.standard_normal(8)}),
    "arreg": dict(model=rxhip.gaussian_regression(np.zeros(1), np.eye(1)), data={"x": np.linspace(-1.0, 1.0, 8).reshape(8, 1), "y": _rng.standard_normal(8)}),
    "mnreg": dict(model=rxhip.multinomial_regression(np.zeros(2), np.eye(2)), data={"y": _counts}),
    "mnreg_online": dict(model=rxhip.multinomial_regression(np.zeros(2), np.eye(2)), data={"y": _counts}, autoupdates=True),
    "gammamix": dict(model=rxhip.gamma_mixture([(1.0, 1.0), (1.0, 1.0)], [(1.0, 1.0), (1.0, 1.0)], _o), data={"y": _rng.gamma(2.0, 1.0, 8)}),
    "lgssm": dict(model=rxhip.linear_gaussian_ssm(*_ssm), data={"y": _rng.standard_normal((4, 1))}),
    "lgssm_filtering": dict(model=rxhip.linear_gaussian_ssm(*_ssm), data={"y": _rng.standard_normal((4, 1))}, autoupdates=True),
    "lgssm_noise": dict(model=rxhip.linear_gaussian_ssm(_ssm[0], _ssm[1], _ssm[2], None, _ssm[4], _ssm[5], noise_precision_prior=rxhip.Wishart(3.0, _one)),
                        data={"y": _rng.standard_normal((4, 1))}, iterations=2, initialization={"W": rxhip.Wishart(3.0, _one)}),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_unknown_options_propagate_even_with_catch_exception(name):
    with pytest.raises(ValueError, match="Unknown option keys"):
        rxhip.infer(**CALLS[name], options={"nope": 1}, catch_exception=True)


def test_a_missing_initialization_propagates_even_with_catch_exception():
    for name in ("mixture", "mv_mixture"):
        call = dict(CALLS[name], initialization=None)
        with pytest.raises(ValueError, match="needs `initialization`"):
            rxhip.infer(**call, catch_exception=True)
    with pytest.raises(ValueError, match="keephistory must be 8"):
        rxhip.infer(**CALLS["mnreg_online"], keephistory=3, catch_exception=True)


def test_an_unknown_model_type_is_a_type_error():
    with pytest.raises(TypeError, match="no device schedule for this model type"):
        rxhip.infer(model=object(), data={"y": np.zeros(4)}, catch_exception=True)


@pytest.mark.skipif(rxhip.lib().rxhip_device_count() > 0, reason="checks the no-device error path")
@pytest.mark.parametrize("name", sorted(CALLS))
def test_what_the_engine_refuses_is_caught(name):
    res = rxhip.infer(**CALLS[name], options={"device": -1}, catch_exception=True)
    assert isinstance(res.error, rxhip.RxHipError) and res.error.status == _lib.ERR_NO_DEVICE
    assert res.posteriors == {} and res.model is CALLS[name]["model"]
    with pytest.raises(rxhip.RxHipError):
        rxhip.infer(**CALLS[name])

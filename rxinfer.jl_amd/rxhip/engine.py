"""The engine classes — thin object wrappers over the rxhip C ABI (one handle = one batch of chains / series / problems).  `_Engine` owns what is
true of every handle; a family's class adds its descriptor and its own getters."""
import ctypes

import numpy as np

from . import _lib
from ._lib import RxHipError, c_double_p


def _c(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _p(a):
    return a.ctypes.data_as(c_double_p)


def _lay(layout):
    return _lib.LAYOUT_TIME_CHAIN if layout == "time_chain" else _lib.LAYOUT_CHAIN_TIME


class _Engine:
    """One `rxhip_engine*` and what the C ABI answers for every kind of it: creation failure, lifecycle, runs, free energies, counters and
    measurement.  A family's class fills its descriptor, calls its creator into `self._h = ctypes.c_void_p()` and hands the status to `_created`;
    what exists only for some kinds (marginals, the filtering twin, a family's getters and `schedule`) stays on the classes that have it."""

    n_chains = 1   # free_energy_per_chain: the engines without a batch axis are one chain

    def _created(self, st, text=""):
        """The end of every constructor.  A refused creation leaves no handle behind and raises with `text` (the graph entry points report
        through rxhip_lowering_error), else the handle's own message, else the name of the status."""
        if st != _lib.OK:
            L = _lib.lib()
            msg = text or (self._last_error() if self._h else "") or L.rxhip_status_string(st).decode()
            if self._h:
                L.rxhip_destroy(self._h)
            self._h = None
            raise RxHipError(st, msg)
        self._iters, self._fe, self._data_ref = 0, False, None

    def _last_error(self):
        return _lib.lib().rxhip_last_error(self._h).decode()

    def _chk(self, st):
        if st != _lib.OK:
            raise RxHipError(st, self._last_error())

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().rxhip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- inference --------------------------------------------------------------------------
    def run(self, iterations=1, free_energy=True):
        self._chk(_lib.lib().rxhip_run(self._h, int(iterations), int(bool(free_energy))))
        self._iters, self._fe = int(iterations), bool(free_energy)

    def run_async(self, iterations=1, free_energy=True):
        self._chk(_lib.lib().rxhip_run_async(self._h, int(iterations), int(bool(free_energy))))
        self._iters, self._fe = int(iterations), bool(free_energy)

    def sync(self):
        self._chk(_lib.lib().rxhip_sync(self._h))

    def free_energy(self):
        out = np.empty(self._iters)
        self._chk(_lib.lib().rxhip_get_free_energy(self._h, _p(out)))
        return out

    def free_energy_per_chain(self):
        out = np.empty(self.n_chains)
        self._chk(_lib.lib().rxhip_get_free_energy_per_chain(self._h, _p(out)))
        return out

    def free_energy_device(self):
        p = ctypes.c_void_p()
        self._chk(_lib.lib().rxhip_get_free_energy_device(self._h, ctypes.byref(p)))
        return p.value

    def copy_free_energy_to_device(self, dst_ptr):
        self._chk(_lib.lib().rxhip_copy_free_energy_to_device(self._h, ctypes.c_void_p(dst_ptr)))

    def allreduce_free_energy(self, comm):
        """Sum the free energies of the last run over all ranks of the RCCL communicator `comm` (a `Communicator` or a raw
        ncclComm_t address), in place on the device, on the engine's stream."""
        self._chk(_lib.lib().rxhip_allreduce_free_energy(self._h, ctypes.c_void_p(int(getattr(comm, "handle", comm) or 0))))

    def counters(self):
        r, p, m = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(_lib.lib().rxhip_counters(self._h, ctypes.byref(r), ctypes.byref(p), ctypes.byref(m)))
        return {"rule_calls": r.value, "products": p.value, "marginals": m.value}

    # -- measurement ------------------------------------------------------------------------
    def set_profiling(self, on=True):
        self._chk(_lib.lib().rxhip_set_profiling(self._h, int(bool(on))))

    def reset_kernel_times(self):
        self._chk(_lib.lib().rxhip_reset_kernel_times(self._h))

    def kernel_times(self):
        ms = (ctypes.c_double * _lib.K_COUNT)()
        n = (ctypes.c_uint64 * _lib.K_COUNT)()
        self._chk(_lib.lib().rxhip_get_kernel_times(self._h, ms, n))
        return {name: {"ms_avg": ms[i], "launches": n[i]} for i, name in enumerate(_lib.KERNEL_NAMES)}

    def stream(self):
        p = ctypes.c_void_p()
        self._chk(_lib.lib().rxhip_get_stream(self._h, ctypes.byref(p)))
        return p.value


class _SeriesEngine(_Engine):
    """The engines whose observations are one series per chain through the common ingest, from the host or from device memory."""

    def set_data(self, y, layout="time_chain"):
        """y: [T][chain] (layout='time_chain') or [chain][T] ('chain_time'), with a trailing [dy] where observations are vectors; host array."""
        y = _c(y)
        self._chk(_lib.lib().rxhip_set_data(self._h, _lib.VAR_Y, _p(y), y.size, _lay(layout)))

    def set_data_device(self, ptr, n, layout="time_chain", keepalive=None):
        """Observations already in device memory (e.g. a torch tensor's data_ptr())."""
        self._data_ref = keepalive
        self._chk(_lib.lib().rxhip_set_data_device(self._h, _lib.VAR_Y, ctypes.c_void_p(ptr), n, _lay(layout)))


class _StateEngine(_SeriesEngine):
    """The families with posteriors of a latent state x[t] in the common arrays (d_mean / d_cov: the rows of the family table with has_x)."""

    def marginals(self, layout="time_chain", want_cov=True):
        d, T, C = self.d, self.T + getattr(self, "horizon", 0), self.n_chains
        shp = (T, C) if layout == "time_chain" else (C, T)
        mean = np.empty(shp + (d,))
        cov = np.empty(shp + (d, d)) if want_cov else None
        self._chk(_lib.lib().rxhip_get_marginals(self._h, _lib.VAR_X, _p(mean), _p(cov) if want_cov else None, _lay(layout)))
        return mean, cov

    def marginals_of_chains(self, chains, want_cov=True):
        """Posteriors of the selected chains only, chain-major: mean [n][T][d], cov [n][T][d][d] (strided gather on the
        device + one copy; rxhip_get_marginals_chains)."""
        ch = np.ascontiguousarray(chains, dtype=np.int64).ravel()
        T = self.T + getattr(self, "horizon", 0)
        mean = np.empty((ch.size, T, self.d))
        cov = np.empty((ch.size, T, self.d, self.d)) if want_cov else None
        self._chk(_lib.lib().rxhip_get_marginals_chains(self._h, _lib.VAR_X, ch.ctypes.data_as(_lib.c_int64_p), ch.size,
                                                         _p(mean), _p(cov) if want_cov else None))
        return mean, cov


class LGSSMEngine(_StateEngine):
    """Batch of linear Gaussian state-space factor graphs on one MI355X.

    A, B, P, Q, m0, V0 may carry a leading model axis ([n_models, ...]); chain_model maps chains
    to models.  P is the state-noise covariance, Q the observation-noise covariance (the
    benchmark notebook's naming; test/models/statespace/mlgssm_test.jl swaps the two names).
    """

    def __init__(self, A, B, P, Q, m0, V0, T, n_chains=1, chain_model=None, prior_through_transition=False,
                 segments=0, device=-1, stream=None, horizon=0, allow_missing=False, step_model=None, state_offset=None, obs_offset=None):
        L = _lib.lib()
        A = _c(A)
        B = _c(B)
        if A.ndim == 2:
            A, B, P, Q, m0, V0 = (np.asarray(x, dtype=np.float64)[None] for x in (A, B, P, Q, m0, V0))
        self.n_models = A.shape[0]
        self.d = A.shape[-1]
        self.dy = _c(B).shape[-2]
        self.T = int(T)
        self.horizon = int(horizon)
        self.n_chains = int(n_chains)
        d, dy, M = self.d, self.dy, self.n_models
        self._keep = [_c(A, (M, d, d)), _c(B, (M, dy, d)), _c(P, (M, d, d)), _c(Q, (M, dy, dy)), _c(m0, (M, d)),
                      _c(V0, (M, d, d))]
        desc = _lib.LgssmDesc()
        desc.d, desc.dy, desc.T, desc.n_chains, desc.n_models = d, dy, self.T, self.n_chains, M
        desc.prior_through_transition = int(bool(prior_through_transition))
        desc.A, desc.B, desc.P, desc.Q, desc.m0, desc.V0 = (_p(x) for x in self._keep)
        if chain_model is not None:
            cm = np.ascontiguousarray(chain_model, dtype=np.int32)
            if cm.shape != (self.n_chains,):
                raise ValueError("chain_model must have one entry per chain")
            self._keep.append(cm)
            desc.chain_model = cm.ctypes.data_as(_lib.c_int32_p)
        desc.segments = int(segments)
        desc.device = int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        desc.horizon = self.horizon
        desc.allow_missing = int(bool(allow_missing))
        if step_model is not None:  # time-varying constants: the model of every time index
            sm = np.ascontiguousarray(step_model, dtype=np.int32)
            if sm.shape != (self.T + self.horizon,):
                raise ValueError("step_model must have one entry per time index (T + horizon)")
            self._keep.append(sm)
            desc.step_model = sm.ctypes.data_as(_lib.c_int32_p)
        # known inputs: x[t] ~ N(A x[t-1] + c[t], P), y[t] ~ N(B x[t] + d[t], Q); a single vector is the same offset at every step
        for name, off, k in (("state_offset", state_offset, d), ("obs_offset", obs_offset, dy)):
            if off is not None:
                a = _c(np.broadcast_to(np.asarray(off, dtype=np.float64), (self.T + self.horizon, k)))
                self._keep.append(a)
                setattr(desc, name, _p(a))
        self._h = ctypes.c_void_p()
        st = self._create(L, desc)
        # without a handle, an unsupported model was refused by the graph lowering, which reports through its own channel
        self._created(st, L.rxhip_lowering_error().decode() if st == _lib.ERR_UNSUPPORTED and not self._h else "")

    def _create(self, L, desc):
        return L.rxhip_lgssm_create(ctypes.byref(desc), ctypes.byref(self._h))

    def set_inputs(self, u, layout="time_chain"):
        """Data inputs u[t] of `A * x[t-1] + B_u * u[t]` (engines built from a graph with such inputs): [T][chain][du] / [chain][T][du]."""
        u = _c(u)
        self._chk(_lib.lib().rxhip_set_data(self._h, _lib.VAR_U, _p(u), u.size, _lay(layout)))

    def infer(self, y, iterations=1, free_energy=True, want_cov=True, filtering=False):
        """set_data + run + marginals (+ per-chain free energy) in one round trip (rxhip_lgssm_infer); y: [T][chain][dy].
        Returns mean [T+H][chain][d], cov | None, fe [chain] | None."""
        y = _c(y)
        To, C, d = self.T + self.horizon, self.n_chains, self.d
        mean = np.empty((To, C, d))
        cov = np.empty((To, C, d, d)) if want_cov else None
        fe = np.empty(C) if free_energy else None
        self._chk(_lib.lib().rxhip_lgssm_infer(self._h, _p(y), y.size, int(iterations), int(bool(free_energy)), int(bool(filtering)), _p(mean),
                                               _p(cov) if want_cov else None, _p(fe) if free_energy else None))
        self._iters = int(iterations)
        return mean, cov, fe

    def run_filter(self, free_energy=True):
        """Streaming / filtering run (rxhip_run_filter): afterwards `marginals()` holds q(x_t | y_1..t) and
        `free_energy()` ONE value — Σ_chains of the mean-over-observations free energy."""
        self._chk(_lib.lib().rxhip_run_filter(self._h, int(bool(free_energy))))
        self._iters = 1

    def run_filter_async(self, free_energy=True):
        self._chk(_lib.lib().rxhip_run_filter_async(self._h, int(bool(free_energy))))
        self._iters = 1

    def filter_step(self, y, want_cov=True, free_energy=True):
        """One observation of every chain (y: [chain][dy]; NaN = missing) through the streaming driver (rxhip_filter_step):
        returns the posterior mean [chain][d], covariance [chain][d][d] | None, −log p(y_k | y_<k) [chain] | None."""
        y = _c(y, (self.n_chains, self.dy))
        mean = np.empty((self.n_chains, self.d))
        cov = np.empty((self.n_chains, self.d, self.d)) if want_cov else None
        fe = np.empty(self.n_chains) if free_energy else None
        self._chk(_lib.lib().rxhip_filter_step(self._h, _p(y), _p(mean), _p(cov) if want_cov else None, _p(fe) if free_energy else None))
        return mean, cov, fe

    def set_offsets(self, state_offset=None, obs_offset=None):
        """New known inputs (rxhip_lgssm_set_offsets); the engine must have been created with offsets."""
        To = self.T + self.horizon
        cx = None if state_offset is None else _c(np.broadcast_to(np.asarray(state_offset, dtype=np.float64), (To, self.d)))
        cy = None if obs_offset is None else _c(np.broadcast_to(np.asarray(obs_offset, dtype=np.float64), (To, self.dy)))
        self._chk(_lib.lib().rxhip_lgssm_set_offsets(self._h, _p(cx) if cx is not None else None, _p(cy) if cy is not None else None))

    def set_chain_offsets(self, state_offset=None, obs_offset=None, layout="time_chain"):
        """Known inputs per chain (rxhip_lgssm_set_chain_offsets): [T+horizon][chain][d] / [..][dy] ('time_chain') or
        [chain][T+horizon][·] ('chain_time')."""
        To, C = self.T + self.horizon, self.n_chains
        shp = (lambda k: (To, C, k)) if layout == "time_chain" else (lambda k: (C, To, k))
        cx = None if state_offset is None else _c(state_offset, shp(self.d))
        cy = None if obs_offset is None else _c(obs_offset, shp(self.dy))
        lay = _lay(layout)
        self._chk(_lib.lib().rxhip_lgssm_set_chain_offsets(self._h, _p(cx) if cx is not None else None,
                                                           _p(cy) if cy is not None else None, lay))

    def filter_reset(self):
        self._chk(_lib.lib().rxhip_filter_reset(self._h))

    def predictions(self, layout="time_chain", want_cov=True):
        """Messages toward y[1..T+horizon] (`predictvars`): mean [T+H][chain][dy], cov [...][dy][dy] (rxhip_get_predictions)."""
        dy, T, C = self.dy, self.T + getattr(self, "horizon", 0), self.n_chains
        lay = _lay(layout)
        shp = (T, C) if layout == "time_chain" else (C, T)
        mean = np.empty(shp + (dy,))
        cov = np.empty(shp + (dy, dy)) if want_cov else None
        self._chk(_lib.lib().rxhip_get_predictions(self._h, _lib.VAR_Y, _p(mean), _p(cov) if want_cov else None, lay))
        return mean, cov

    def node_marginals(self, layout="time_chain"):
        """Node-local joints q(x[t], A x[t-1]) of the transition nodes (rxhip_get_node_marginals): mean [T-1][chain][2d],
        cov [T-1][chain][2d][2d] in (out, μ) order."""
        d2, T, C = 2 * self.d, self.T - 1, self.n_chains
        lay = _lay(layout)
        shp = (T, C) if layout == "time_chain" else (C, T)
        mean, cov = np.empty(shp + (d2,)), np.empty(shp + (d2, d2))
        self._chk(_lib.lib().rxhip_get_node_marginals(self._h, _lib.NODE_MVNORMAL_MEAN_COV, _p(mean), _p(cov), lay))
        return mean, cov

    def marginals_device(self):
        m, c = ctypes.c_void_p(), ctypes.c_void_p()
        self._chk(_lib.lib().rxhip_get_marginals_device(self._h, _lib.VAR_X, ctypes.byref(m), ctypes.byref(c)))
        return m.value, c.value

    # -- measurement ------------------------------------------------------------------------
    def model_tables_ms(self):
        """device time of the once-per-engine kernels (tables that depend on the model only); 0 without such tables"""
        ms = ctypes.c_double()
        self._chk(_lib.lib().rxhip_get_model_tables_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def mean_checkpoint_stride(self):
        """checkpoint stride K of the reverse-filter backward sweep; 0: a filtered-mean record per time index
        (rxhip_get_mean_checkpoint_stride)"""
        k = ctypes.c_int32()
        self._chk(_lib.lib().rxhip_get_mean_checkpoint_stride(self._h, ctypes.byref(k)))
        return k.value

    def sweep_waves(self):
        """(forward, backward): wavefronts per workgroup of the two sweep kernels of the reverse-filter schedule; (0, 0) for an
        engine on another schedule (rxhip_get_sweep_waves)"""
        f, b = ctypes.c_int32(), ctypes.c_int32()
        self._chk(_lib.lib().rxhip_get_sweep_waves(self._h, ctypes.byref(f), ctypes.byref(b)))
        return f.value, b.value

    def create_stages(self):
        """host milliseconds of the engine's creation by stage (rxhip_get_create_stages)"""
        ms = (ctypes.c_double * 4)()
        self._chk(_lib.lib().rxhip_get_create_stages(self._h, ms))
        return {"tables_host_ms": ms[0], "tables_device_ms": ms[1], "upload_ms": ms[2], "alloc_ms": ms[3]}

    def set_fixed_point_exits(self, enabled):
        """False: every recursion of this engine's later sweeps runs in full — no frozen stretches, no early exits (rxhip_set_fixed_point_exits)"""
        self._chk(_lib.lib().rxhip_set_fixed_point_exits(self._h, 1 if enabled else 0))

    def set_covariance_mode(self, mode):
        """0: after every sweep the array holds the covariance of every chain (default; batches sharing one model store it when it is not
        already there); 1: shared-model batches on the MFMA path write the per-chain array when it is asked for (rxhip_set_covariance_mode)"""
        self._chk(_lib.lib().rxhip_set_covariance_mode(self._h, int(mode)))

    def covariance_writes(self):
        """how many times in this handle's life the per-chain covariance array was stored (rxhip_get_covariance_writes)"""
        n = ctypes.c_uint64()
        self._chk(_lib.lib().rxhip_get_covariance_writes(self._h, ctypes.byref(n)))
        return n.value

    def schedule(self):
        s, l = ctypes.c_int32(), ctypes.c_int64()
        self._chk(_lib.lib().rxhip_get_schedule(self._h, ctypes.byref(s), ctypes.byref(l)))
        return {"segments": s.value, "segment_len": l.value}


class LGSSMNoiseEngine(LGSSMEngine):
    """State-space chains with an UNKNOWN observation-noise precision, `W ~ Wishart(nu0, S0); y[t] ~ MvNormal(μ = B * x[t], Λ = W)` with
    `q(x, W) = q(x) q(W)` (include/rxhip.h rxhip_lgssm_noise_create): every chain its own W.  run(iterations, free_energy) alternates one
    belief-propagation sweep of all chains with the Wishart update of all chains, on the device; free_energy() per iteration,
    noise_posterior() -> (nu [chains], V [chains][dy][dy]) after the last one."""

    def __init__(self, A, B, P, m0, V0, T, nu0, S0, init_nu=None, init_V=None, n_chains=1, prior_through_transition=False, segments=0,
                 device=-1, stream=None):
        dy = _c(B).shape[-2]
        self._pri = _lib.NoisePrior()
        self._pri_keep = [_c(S0, (dy, dy)), _c(S0 if init_V is None else init_V, (dy, dy))]
        self._pri.nu0, self._pri.init_nu = float(nu0), float(nu0 if init_nu is None else init_nu)
        self._pri.S0, self._pri.init_V = _p(self._pri_keep[0]), _p(self._pri_keep[1])
        super().__init__(A, B, P, np.eye(dy), m0, V0, T, n_chains=n_chains, prior_through_transition=prior_through_transition,
                         segments=segments, device=device, stream=stream)

    def _create(self, L, desc):
        return L.rxhip_lgssm_noise_create(ctypes.byref(desc), ctypes.byref(self._pri), ctypes.byref(self._h))

    def continue_runs(self, on=True):
        """later run() calls go on from the current q(W) instead of the initial marginal (rxhip_lgssm_noise_continue)"""
        self._chk(_lib.lib().rxhip_lgssm_noise_continue(self._h, int(bool(on))))

    def noise_posterior(self):
        nu, V = np.empty(self.n_chains), np.empty((self.n_chains, self.dy, self.dy))
        self._chk(_lib.lib().rxhip_lgssm_noise_get(self._h, _p(nu), _p(V)))
        return nu, V


class GMMEngine(_Engine):
    """Mean-field VMP for the univariate Gaussian mixture on one MI355X (see include/rxhip.h rxhip_gmm_desc).
    K = 1 is the iid Gaussian with unknown mean and precision."""

    def __init__(self, N, mu0, v0, a0, b0, alpha0, init_m_mean, init_m_var, init_p_shape, init_p_rate, init_s_alpha,
                 materialize_responsibilities=False, device=-1, stream=None):
        L = _lib.lib()
        arrs = [_c(a).ravel() for a in (mu0, v0, a0, b0, alpha0, init_m_mean, init_m_var, init_p_shape, init_p_rate,
                                        init_s_alpha)]
        self.K = arrs[0].size
        if any(a.size != self.K for a in arrs):
            raise ValueError("all prior / initialisation arrays must have K entries")
        self.N = int(N)
        self._keep = arrs
        desc = _lib.GmmDesc()
        desc.N, desc.K = self.N, self.K
        for name, a in zip(("mu0", "v0", "a0", "b0", "alpha0", "init_m_mean", "init_m_var", "init_p_shape", "init_p_rate",
                            "init_s_alpha"), arrs):
            setattr(desc, name, _p(a))
        desc.materialize_responsibilities = int(bool(materialize_responsibilities))
        desc.device = int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_gmm_create(ctypes.byref(desc), ctypes.byref(self._h)))

    def set_data(self, y):
        y = _c(y).ravel()
        self._chk(_lib.lib().rxhip_set_data(self._h, _lib.VAR_Y, _p(y), y.size, _lib.LAYOUT_TIME_CHAIN))

    def set_data_device(self, ptr, n, keepalive=None):
        self._data_ref = keepalive
        self._chk(_lib.lib().rxhip_set_data_device(self._h, _lib.VAR_Y, ctypes.c_void_p(ptr), n, _lib.LAYOUT_TIME_CHAIN))

    # split-phase iteration (several GPUs: all-reduce the statistics between accumulate and update)
    def begin_run(self, iterations):
        self._chk(_lib.lib().rxhip_gmm_begin_run(self._h, int(iterations)))
        self._iters = int(iterations)

    def accumulate(self):
        self._chk(_lib.lib().rxhip_gmm_accumulate(self._h))

    def statistics_device(self):
        p, n = ctypes.c_void_p(), ctypes.c_int32()
        self._chk(_lib.lib().rxhip_gmm_statistics_device(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def statistics_tensor(self):
        """torch tensor ALIASING the device statistics buffer (3K'+1 doubles) — what the multi-GPU host hands to
        `torch.distributed.all_reduce` in place (RCCL) between accumulate() and update()."""
        import torch

        ptr, n = self.statistics_device()

        class _View:  # zero-copy: torch adopts foreign device memory through the array interface
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        self._stats_view = _View()  # keep the descriptor object alive as long as the engine
        return torch.as_tensor(self._stats_view, device=f"cuda:{torch.cuda.current_device()}")

    def allreduce_statistics(self, comm):
        """Sum the statistics of this iteration over all ranks of the RCCL communicator (between accumulate and update)."""
        self._chk(_lib.lib().rxhip_gmm_allreduce_statistics(self._h, ctypes.c_void_p(int(getattr(comm, "handle", comm) or 0))))

    def update(self, free_energy=True):
        self._chk(_lib.lib().rxhip_gmm_update(self._h, int(bool(free_energy))))

    def history(self):
        """[iterations][5][K]: mean m, var m, shape p, rate p, alpha s after every iteration (KeepEach)."""
        h = np.empty((self._iters, 5, self.K))
        self._chk(_lib.lib().rxhip_gmm_get_history(self._h, _p(h)))
        return h

    def responsibilities(self):
        r = np.empty((self.N, self.K))
        self._chk(_lib.lib().rxhip_gmm_get_responsibilities(self._h, _p(r)))
        return r


class MvGMMEngine(GMMEngine):
    """Mean-field VMP for the multivariate Gaussian mixture (include/rxhip.h rxhip_mvgmm_desc): d = 1…4 (K ≤ 16 at d ≤ 2, K ≤ 8 at d = 3, 4)
    and d = 5…32 with K ≤ 16 on the fp64 matrix cores.
    priors: mu0 [K][d], S0 [K][d][d], nu0 [K], V0 [K][d][d], alpha0 [K]; init: the same five blocks of the initial marginals."""

    def __init__(self, N, mu0, S0, nu0, V0, alpha0, init_m_mean, init_m_cov, init_w_nu, init_w_V, init_s_alpha,
                 materialize_responsibilities=False, device=-1, stream=None):
        L = _lib.lib()
        arrs = [_c(a) for a in (mu0, S0, nu0, V0, alpha0, init_m_mean, init_m_cov, init_w_nu, init_w_V, init_s_alpha)]
        self.K, self.d = arrs[0].shape
        K, d = self.K, self.d
        shapes = [(K, d), (K, d, d), (K,), (K, d, d), (K,)] * 2
        if any(a.shape != sh for a, sh in zip(arrs, shapes)):
            raise ValueError("prior / initialisation arrays have inconsistent shapes")
        self.N = int(N)
        self._keep = arrs
        desc = _lib.MvGmmDesc()
        desc.N, desc.K, desc.d = self.N, K, d
        for name, a in zip(("mu0", "S0", "nu0", "V0", "alpha0", "init_m_mean", "init_m_cov", "init_w_nu", "init_w_V", "init_s_alpha"), arrs):
            setattr(desc, name, _p(a))
        desc.materialize_responsibilities = int(bool(materialize_responsibilities))
        desc.device = int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_mvgmm_create(ctypes.byref(desc), ctypes.byref(self._h)))

    def set_data(self, y):
        y = _c(y)
        if y.shape != (self.N, self.d):
            raise ValueError(f"observations must be [N][d] = {(self.N, self.d)}")
        self._chk(_lib.lib().rxhip_set_data(self._h, _lib.VAR_Y, _p(y), y.size, _lib.LAYOUT_TIME_CHAIN))

    def history(self):
        """dict of arrays over (iteration, component): mean [.., d], cov [.., d, d], nu, V [.., d, d], alpha (KeepEach)."""
        d, dd = self.d, self.d * self.d
        h = np.empty((self._iters, self.K, 2 + d + 2 * dd))
        self._chk(_lib.lib().rxhip_gmm_get_history(self._h, _p(h)))
        return dict(mean=h[..., :d], cov=h[..., d:d + dd].reshape(h.shape[:-1] + (d, d)), nu=h[..., d + dd],
                    V=h[..., d + dd + 1:d + 2 * dd + 1].reshape(h.shape[:-1] + (d, d)), alpha=h[..., -1], raw=h)


class HGFEngine(_SeriesEngine):
    """Online hierarchical Gaussian filter (GCV node) for n_series independent series (include/rxhip.h rxhip_hgf_desc)."""

    def __init__(self, T, n_series, kappa, omega, z_variance, y_variance, z0=(0.0, 5.0), x0=(0.0, 5.0), n_gh=31,
                 device=-1, stream=None):
        L = _lib.lib()
        desc = _lib.HgfDesc()
        desc.T, desc.n_series = int(T), int(n_series)
        desc.kappa, desc.omega, desc.z_variance, desc.y_variance = float(kappa), float(omega), float(z_variance), float(y_variance)
        desc.z0_mean, desc.z0_var, desc.x0_mean, desc.x0_var = float(z0[0]), float(z0[1]), float(x0[0]), float(x0[1])
        desc.n_gh, desc.device = int(n_gh), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.T, self.n_series, self.n_chains = int(T), int(n_series), int(n_series)
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_hgf_create(ctypes.byref(desc), ctypes.byref(self._h)))

    def history(self, layout="time_chain"):
        """(z_mean, z_var, x_mean, x_var), each [T][series] (or [series][T])."""
        lay = _lay(layout)
        shp = (self.T, self.n_series) if layout == "time_chain" else (self.n_series, self.T)
        outs = [np.empty(shp) for _ in range(4)]
        self._chk(_lib.lib().rxhip_hgf_get_history(self._h, *[_p(o) for o in outs], lay))
        return tuple(outs)


class DriftChainEngine(_StateEngine):
    """Noise-free drift chain `x_prior ~ Normal(m0, v0); x[t] ~ x[t-1] + c; y[t] ~ Normal(x[t], obs_var)`
    (test/models/statespace/ulgssm_tests.jl:8-15) for n_chains independent chains (include/rxhip.h rxhip_drift_chain_desc)."""

    def __init__(self, T, m0, v0, c, obs_var, n_chains=1, prior_through_transition=True, device=-1, stream=None):
        L = _lib.lib()
        desc = _lib.DriftChainDesc()
        desc.T, desc.n_chains = int(T), int(n_chains)
        desc.m0, desc.v0, desc.c, desc.obs_var = float(m0), float(v0), float(c), float(obs_var)
        desc.prior_through_transition = int(bool(prior_through_transition))
        desc.device = int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.T, self.n_chains, self.d, self.dy, self.n_models = int(T), int(n_chains), 1, 1, 1
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_drift_chain_create(ctypes.byref(desc), ctypes.byref(self._h)))
        self._keep = []


class ProbitEngine(_StateEngine):
    """Scalar Gaussian chain observed through Probit, `x[1] ~ Normal(m0, v0); x[k] ~ Normal(a x[k-1] + c, q); y[k-1] ~ Probit(x[k])`
    (test/models/statespace/probit_tests.jl:11-18), for n_series independent series: batched parallel EP (include/rxhip.h rxhip_probit_desc).
    `run(iterations)`: that many parallel-EP updates from empty sites; `marginals()`: mean / variance of x[1 … T+1]."""

    def __init__(self, T, a, c, q, m0, v0, n_series=1, n_gh=32, device=-1, stream=None):
        L = _lib.lib()
        desc = _lib.ProbitDesc()
        desc.T, desc.n_series = int(T), int(n_series)
        desc.a, desc.c, desc.q, desc.m0, desc.v0 = float(a), float(c), float(q), float(m0), float(v0)
        desc.n_gh, desc.device = int(n_gh), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.T, self.n_series, self.n_chains, self.d, self.dy, self.horizon = int(T), int(n_series), int(n_series), 1, 1, 1
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_probit_create(ctypes.byref(desc), ctypes.byref(self._h)))

    def marginals(self, layout="time_chain"):
        """(mean, var) of x[1 … T+1]: [T+1][series] ('time_chain') or [series][T+1] ('chain_time')."""
        mean, cov = super().marginals(layout)
        return mean[..., 0], cov[..., 0, 0]


class HMMEngine(_SeriesEngine):
    """Hidden Markov model with unknown transition and observation matrices (test/models/statespace/hmm_tests.jl:8-24) for n_series independent
    series: batched forward–backward VMP (include/rxhip.h rxhip_hmm_desc).  prior_A [K][K] and prior_B [M][K] are Dirichlet counts per COLUMN
    (A[i, j] = p(s_t = i | s_{t-1} = j), B[m, i] = p(x_t = m | s_t = i)), prior_s0 [K] probabilities; init_A / init_B the initial q (None: ones).
    Priors and initial counts may carry a leading [n_series] axis (one set per series; not with share_parameters).
    `run(iterations)`: that many iterations from the initial q; `states()`: q(s_0 … s_T); `parameters()`: the counts of q(A), q(B)."""

    def __init__(self, T, prior_A, prior_B, prior_s0, init_A=None, init_B=None, n_series=1, share_parameters=False, device=-1, stream=None):
        L = _lib.lib()
        arrs = [None if v is None else _c(v) for v in (prior_A, prior_B, prior_s0, init_A, init_B)]
        pA, pB, ps0, iA, iB = arrs
        if pA.ndim not in (2, 3) or pB.ndim != pA.ndim or pA.shape[-1] != pA.shape[-2] or pB.shape[-1] != pA.shape[-1] or ps0.shape != (pA.shape[-1],):
            raise ValueError("prior_A must be [K][K], prior_B [M][K], prior_s0 [K] (A and B optionally with a leading series axis)")
        for name, v, ref in (("init_A", iA, pA), ("init_B", iB, pB)):
            if v is not None and v.shape != ref.shape:
                raise ValueError(f"{name} must have the shape of its prior, {ref.shape}")
        per_series = pA.ndim == 3
        if per_series and (pA.shape[0] != int(n_series) or pB.shape[0] != int(n_series)):
            raise ValueError("per-series priors need a leading axis of n_series sets")
        desc = _lib.HmmDesc()
        desc.T, desc.n_series, desc.K, desc.M = int(T), int(n_series), int(pA.shape[-1]), int(pB.shape[-2])
        desc.prior_A, desc.prior_B, desc.prior_s0 = _p(pA), _p(pB), _p(ps0)
        desc.init_A, desc.init_B = (None if iA is None else _p(iA)), (None if iB is None else _p(iB))
        desc.share_parameters, desc.per_series, desc.device = int(bool(share_parameters)), int(per_series), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.T, self.n_series, self.n_chains, self.K, self.M = int(T), int(n_series), int(n_series), desc.K, desc.M
        self.share_parameters = bool(share_parameters)
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_hmm_create(ctypes.byref(desc), ctypes.byref(self._h)))

    def states(self, layout="time_chain"):
        """q(s_t), t = 0 … T: [T+1][series][K] ('time_chain') or [series][T+1][K] ('chain_time')."""
        lay = _lay(layout)
        out = np.empty((self.T + 1, self.n_series, self.K) if layout == "time_chain" else (self.n_series, self.T + 1, self.K))
        self._chk(_lib.lib().rxhip_hmm_get_states(self._h, _p(out), lay))
        return out

    def parameters(self):
        """(A counts [series or 1][K][K], B counts [series or 1][M][K]); 1 with shared parameters."""
        G = 1 if self.share_parameters else self.n_series
        a, b = np.empty((G, self.K, self.K)), np.empty((G, self.M, self.K))
        self._chk(_lib.lib().rxhip_hmm_get_parameters(self._h, _p(a), _p(b)))
        return a, b


class LAREngine(_SeriesEngine):
    """Latent autoregressive model of order p = 1 … 8 with unknown coefficients θ and driving-noise precision γ
    (test/models/autoregressive/lar_tests.jl:51-76) for n_series independent series: batched banded structured VMP (include/rxhip.h
    rxhip_lar_desc).  prior_theta / prior_x0: (mean [p], precision [p][p]) or None = zero mean and identity precision; prior_gamma: (shape, rate);
    init_theta: (mean [p], covariance [p][p]) and init_gamma: (shape, rate), None = the prior's own values.
    `run(iterations)`: that many iterations from the initial q; `states()`: q(x[1 … T]) of the last one; `parameters()`: q(θ), q(γ) after every one."""

    def __init__(self, T, order, tau, prior_theta=None, prior_gamma=(1.0, 1.0), prior_x0=None, init_theta=None, init_gamma=None, n_series=1,
                 share_parameters=False, device=-1, stream=None):
        L = _lib.lib()
        p = int(order)
        shape_p = max(p, 0)

        def pair(v, name):
            if v is None:
                return _c(np.zeros(shape_p)), _c(np.eye(shape_p))
            m, w = _c(v[0]), _c(v[1])
            if m.shape != (shape_p,) or w.shape != (shape_p, shape_p):
                raise ValueError(f"{name} must be (mean [p], matrix [p][p]) with p = {p}")
            return m, w

        pt, px = pair(prior_theta, "prior_theta"), pair(prior_x0, "prior_x0")
        it = None if init_theta is None else pair(init_theta, "init_theta")
        desc = _lib.LarDesc()
        desc.T, desc.n_series, desc.order, desc.tau = int(T), int(n_series), p, float(tau)
        desc.prior_theta_mean, desc.prior_theta_precision = _p(pt[0]), _p(pt[1])
        desc.prior_gamma_shape, desc.prior_gamma_rate = float(prior_gamma[0]), float(prior_gamma[1])
        desc.prior_x0_mean, desc.prior_x0_precision = _p(px[0]), _p(px[1])
        if it is not None:
            desc.init_theta_mean, desc.init_theta_cov = _p(it[0]), _p(it[1])
        ig = None if init_gamma is None else _c([float(init_gamma[0]), float(init_gamma[1])])
        if ig is not None:
            desc.init_gamma_shape = _p(ig[0:1])
            desc.init_gamma_rate = _p(ig[1:2])
        desc.share_parameters, desc.device = int(bool(share_parameters)), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.T, self.n_series, self.n_chains, self.order = int(T), int(n_series), int(n_series), p
        self.share_parameters = bool(share_parameters)
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_lar_create(ctypes.byref(desc), ctypes.byref(self._h)))

    def states(self, layout="time_chain"):
        """q(x[t]), t = 1 … T, x[t] = (z_t … z_{t-p+1}): (mean [T][series][p], cov [T][series][p][p]) ('time_chain') or [series][T][…] ('chain_time')."""
        lay = _lay(layout)
        lead = (self.T, self.n_series) if layout == "time_chain" else (self.n_series, self.T)
        mean, cov = np.empty(lead + (self.order,)), np.empty(lead + (self.order, self.order))
        self._chk(_lib.lib().rxhip_lar_get_states(self._h, _p(mean), _p(cov), lay))
        return mean, cov

    def parameters(self):
        """q(θ), q(γ) after every iteration of the last run: (θ mean [iterations][G][p], θ covariance [iterations][G][p][p], γ shape
        [iterations][G], γ rate [iterations][G]); G = n_series, or 1 with shared parameters."""
        G, n, p = (1 if self.share_parameters else self.n_series), max(int(self._iters), 0), self.order
        tm, tc, ga, gb = np.empty((n, G, p)), np.empty((n, G, p, p)), np.empty((n, G)), np.empty((n, G))
        self._chk(_lib.lib().rxhip_lar_get_parameters(self._h, _p(tm), _p(tc), _p(ga), _p(gb)))
        return tm, tc, ga, gb


class BinomialRegressionEngine(_Engine):
    """Bayesian binomial (logistic) regression `β ~ MvNormalWeightedMeanPrecision(ξ0, W0); y[i] ~ BinomialPolya(X[i], n_trials[i], β)`
    (test/models/regression/binomialreg_tests.jl) for n_problems independent regressions of N points and d = 1 … 32 features: batched
    Pólya-Gamma VMP (include/rxhip.h rxhip_binreg_desc).  init: (mean [d], covariance [d][d]) or None = the prior's W0⁻¹ξ0, W0⁻¹.
    `set_data(X, y, n_trials)`; `run(iterations)`: that many iterations from the initial q(β); `parameters()`: q(β) after every one."""

    def __init__(self, N, d, prior_xi, prior_precision, init=None, n_problems=1, device=-1, stream=None):
        L = _lib.lib()
        d = int(d)
        xi, w0 = _c(prior_xi), _c(prior_precision)
        if xi.shape != (max(d, 0),) or w0.shape != (max(d, 0), max(d, 0)):
            raise ValueError(f"prior_xi must be [d] and prior_precision [d][d] with d = {d}")
        desc = _lib.BinregDesc()
        desc.N, desc.n_problems, desc.d = int(N), int(n_problems), d
        desc.prior_xi, desc.prior_precision = _p(xi), _p(w0)
        if init is not None:
            im, iv = _c(init[0]), _c(init[1])
            if im.shape != xi.shape or iv.shape != w0.shape:
                raise ValueError(f"init must be (mean [d], covariance [d][d]) with d = {d}")
            desc.init_mean, desc.init_cov = _p(im), _p(iv)
        desc.device = int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.N, self.d, self.n_problems, self.n_chains = int(N), d, int(n_problems), int(n_problems)
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_binreg_create(ctypes.byref(desc), ctypes.byref(self._h)))

    @staticmethod
    def schedule(N, d):
        """(points per tile, workgroups per problem) of the pass for N points of d features: a function of N and d only."""
        tp, ch = ctypes.c_int32(), ctypes.c_int32()
        _lib.lib().rxhip_binreg_schedule(int(N), int(d), ctypes.byref(tp), ctypes.byref(ch))
        return tp.value, ch.value

    def _set(self, var, a, shape, name):
        a = _c(a)
        if a.shape != shape and not (self.n_problems == 1 and a.shape == shape[1:]):
            raise ValueError(f"{name} must be {list(shape)} (the problem axis may be left out for one problem), got {list(a.shape)}")
        self._chk(_lib.lib().rxhip_set_data(self._h, var, _p(a), a.size, _lib.LAYOUT_TIME_CHAIN))

    def set_regressors(self, X):
        self._set(_lib.VAR_REGRESSORS, X, (self.n_problems, self.N, self.d), "X")

    def set_observations(self, y):
        """y [problems][N]; NaN = missing."""
        self._set(_lib.VAR_Y, y, (self.n_problems, self.N), "y")

    def set_trials(self, n_trials):
        self._set(_lib.VAR_TRIALS, n_trials, (self.n_problems, self.N), "n_trials")

    def set_data(self, X, y, n_trials):
        self.set_regressors(X)
        self.set_trials(n_trials)
        self.set_observations(y)

    def parameters(self):
        """q(β) after every iteration of the last run: (mean [iterations][problems][d], covariance [iterations][problems][d][d], free energy
        [iterations][problems] or None when the run was without it)."""
        n, C, d = max(int(self._iters), 0), self.n_problems, self.d
        mean, cov = np.empty((n, C, d)), np.empty((n, C, d, d))
        fe = np.empty((n, C)) if self._fe else None
        self._chk(_lib.lib().rxhip_binreg_get_parameters(self._h, _p(mean), _p(cov), _p(fe) if self._fe else None))
        return mean, cov, fe


class ARRegressionEngine(_SeriesEngine):
    """Bayesian linear regression with unknown coefficients θ and noise precision γ, `γ ~ Gamma(a0, b0); θ ~ MvNormal(m0, Λ0⁻¹); y[i] ~
    Normal(dot(x[i], θ), γ⁻¹)` with `q(γ, θ) = q(γ)q(θ)` (test/models/autoregressive/ar_tests.jl:17-46) for n_series independent problems or one
    θ, γ for all of them, d = 1 … 32: batched Normal-Gamma VMP from the statistics G, h, s, n (include/rxhip.h rxhip_arreg_desc).
    lagged=False: `set_regressors(X [series][N][d])`, `set_observations(y [series][N])`, a NaN y drops the row.  lagged=True: N is the length T of
    a series and d the order p; `set_data(z, layout)` takes the raw series ([T][series] or [series][T]) and row t has y = z_t, x = (z_{t−1} … z_{t−p});
    no regressor matrix is formed.  prior_theta: (mean [d], precision [d][d]) or None = zero mean and identity precision; prior_gamma, init_gamma:
    (shape, rate), init None = the prior's.  `run(iterations)`: that many iterations from the initial q(γ), ONE launch after the pass over the data;
    `parameters()`: q(θ), q(γ), F after every one; `statistics()`: G, h, s, n per series."""

    def __init__(self, N, d, prior_theta=None, prior_gamma=(1.0, 1.0), init_gamma=None, n_series=1, lagged=False, share_parameters=False, device=-1,
                 stream=None):
        L = _lib.lib()
        d = int(d)
        sd = max(d, 0)
        if prior_theta is None:
            m0, l0 = _c(np.zeros(sd)), _c(np.eye(sd))
        else:
            m0, l0 = _c(prior_theta[0]), _c(prior_theta[1])
            if m0.shape != (sd,) or l0.shape != (sd, sd):
                raise ValueError(f"prior_theta must be (mean [d], precision [d][d]) with d = {d}")
        desc = _lib.ArregDesc()
        desc.N, desc.n_series, desc.d, desc.lagged = int(N), int(n_series), d, int(bool(lagged))
        desc.prior_theta_mean, desc.prior_theta_precision = _p(m0), _p(l0)
        desc.prior_gamma_shape, desc.prior_gamma_rate = float(prior_gamma[0]), float(prior_gamma[1])
        ig = None if init_gamma is None else _c([float(init_gamma[0]), float(init_gamma[1])])
        if ig is not None:
            desc.init_gamma_shape = _p(ig[0:1])
            desc.init_gamma_rate = _p(ig[1:2])
        desc.share_parameters, desc.device = int(bool(share_parameters)), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.N, self.T, self.d, self.n_series, self.n_chains = int(N), int(N), d, int(n_series), int(n_series)
        self.lagged, self.share_parameters = bool(lagged), bool(share_parameters)
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_arreg_create(ctypes.byref(desc), ctypes.byref(self._h)))

    @staticmethod
    def schedule(n_rows, d):
        """(rows per tile, workgroups per series) of the pass for n_rows rows (N, or max(T − p, 0) in lagged mode) of d regressors."""
        tp, ch = ctypes.c_int32(), ctypes.c_int32()
        _lib.lib().rxhip_arreg_schedule(int(n_rows), int(d), ctypes.byref(tp), ctypes.byref(ch))
        return tp.value, ch.value

    def _set(self, var, a, shape, name):
        a = _c(a)
        if a.shape != shape and not (self.n_series == 1 and a.shape == shape[1:]):
            raise ValueError(f"{name} must be {list(shape)} (the series axis may be left out for one series), got {list(a.shape)}")
        self._chk(_lib.lib().rxhip_set_data(self._h, var, _p(a), a.size, _lib.LAYOUT_TIME_CHAIN))

    def set_regressors(self, X):
        """regressor mode: X [series][N][d]."""
        self._set(_lib.VAR_REGRESSORS, X, (self.n_series, self.N, self.d), "X")

    def set_observations(self, y):
        """regressor mode: y [series][N]; NaN drops the row."""
        self._set(_lib.VAR_Y, y, (self.n_series, self.N), "y")

    def parameters(self):
        """after every iteration of the last run: (θ mean [iterations][G][d], θ covariance [iterations][G][d][d], γ shape [iterations][G], γ rate
        [iterations][G], free energy [iterations][G] or None when the run was without it); G = n_series, or 1 with shared parameters."""
        G, n, d = (1 if self.share_parameters else self.n_series), max(int(self._iters), 0), self.d
        tm, tc, ga, gb = np.empty((n, G, d)), np.empty((n, G, d, d)), np.empty((n, G)), np.empty((n, G))
        fe = np.empty((n, G)) if self._fe else None
        self._chk(_lib.lib().rxhip_arreg_get_parameters(self._h, _p(tm), _p(tc), _p(ga), _p(gb), _p(fe) if self._fe else None))
        return tm, tc, ga, gb, fe

    def statistics(self):
        """the pass alone: (G [series][d][d], h [series][d], s [series], n [series]) of the data in place."""
        C, d = self.n_series, self.d
        G, h, s, n = np.empty((C, d, d)), np.empty((C, d)), np.empty(C), np.empty(C)
        self._chk(_lib.lib().rxhip_arreg_get_statistics(self._h, _p(G), _p(h), _p(s), _p(n)))
        return G, h, s, n


class MultinomialRegressionEngine(_Engine):
    """Bayesian multinomial regression `ψ ~ MvNormalWeightedMeanPrecision(ξ0, W0); y[i] ~ MultinomialPolya(N_i, ψ)`
    (test/models/regression/multinomialreg_tests.jl) for n_problems independent problems of N count vectors with K = 2 … 65 categories, d = K − 1:
    batched stick-breaking Pólya-Gamma VMP from the column sums (include/rxhip.h rxhip_mnreg_desc).  online=True streams the N rows of each
    series one at a time with the posterior fed back as the next prior (`run(iterations)`: that many per step; `history()`).  n_trials: every
    observed row must sum to it (None: not checked).  init (offline): (mean [d], covariance [d][d]) or None = the prior's W0⁻¹ξ0, W0⁻¹.
    `set_data(Y [problems][N][K])`, a row with any NaN is missing; `parameters()`: q(ψ) after every iteration (online: after the last step);
    `statistics()`: Y, S, lc, n per problem."""

    def __init__(self, N, K, prior_xi, prior_precision, n_trials=None, init=None, n_problems=1, online=False, keep_cov_history=False, device=-1,
                 stream=None):
        L = _lib.lib()
        K = int(K)
        d = max(K - 1, 0)
        xi, w0 = _c(prior_xi), _c(prior_precision)
        if xi.shape != (d,) or w0.shape != (d, d):
            raise ValueError(f"prior_xi must be [K − 1] and prior_precision [K − 1][K − 1] with K = {K}")
        desc = _lib.MnregDesc()
        desc.N, desc.n_problems, desc.K = int(N), int(n_problems), K
        desc.mode = _lib.MNREG_ONLINE if online else _lib.MNREG_BATCH
        desc.n_trials = 0 if n_trials is None else int(n_trials)
        desc.prior_xi, desc.prior_precision = _p(xi), _p(w0)
        if init is not None:
            im, iv = _c(init[0]), _c(init[1])
            if im.shape != xi.shape or iv.shape != w0.shape:
                raise ValueError(f"init must be (mean [K − 1], covariance [K − 1][K − 1]) with K = {K}")
            desc.init_mean, desc.init_cov = _p(im), _p(iv)
        desc.keep_cov_history, desc.device = int(bool(keep_cov_history)), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.N, self.T, self.K, self.d, self.n_problems, self.n_chains = int(N), int(N), K, d, int(n_problems), int(n_problems)
        self.online, self.keep_cov_history = bool(online), bool(keep_cov_history)
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_mnreg_create(ctypes.byref(desc), ctypes.byref(self._h)))

    @staticmethod
    def schedule(N, K):
        """(rows per tile, workgroups per problem) of the statistics pass for N rows of K categories: a function of N and K only."""
        tr, ch = ctypes.c_int32(), ctypes.c_int32()
        _lib.lib().rxhip_mnreg_schedule(int(N), int(K), ctypes.byref(tr), ctypes.byref(ch))
        return tr.value, ch.value

    def set_data(self, Y):
        """Y [problems][N][K] (the problem axis may be left out for one problem): counts as doubles; a row with any NaN is missing."""
        a = _c(Y)
        shape = (self.n_problems, self.N, self.K)
        if a.shape != shape and not (self.n_problems == 1 and a.shape == shape[1:]):
            raise ValueError(f"Y must be {list(shape)} (the problem axis may be left out for one problem), got {list(a.shape)}")
        self._chk(_lib.lib().rxhip_set_data(self._h, _lib.VAR_Y, _p(a), a.size, _lib.LAYOUT_TIME_CHAIN))

    def parameters(self):
        """offline: q(ψ) after every iteration of the last run: (mean [iterations][problems][d], covariance [iterations][problems][d][d], free
        energy [iterations][problems] or None).  online: the last step's (mean [series][d], covariance [series][d][d], F_T [series] or None)."""
        C, d = self.n_problems, self.d
        lead = (C,) if self.online else (max(int(self._iters), 0), C)
        mean, cov = np.empty(lead + (d,)), np.empty(lead + (d, d))
        fe = np.empty(lead) if self._fe else None
        self._chk(_lib.lib().rxhip_mnreg_get_parameters(self._h, _p(mean), _p(cov), _p(fe) if self._fe else None))
        return mean, cov, fe

    def history(self):
        """online: q(ψ) after every step: (mean [T][series][d], variances [T][series][d], covariance [T][series][d][d] or None without
        keep_cov_history, F_t [T][series] or None when the run was without the free energy)."""
        T, C, d = self.N, self.n_problems, self.d
        mean, var = np.empty((T, C, d)), np.empty((T, C, d))
        cov = np.empty((T, C, d, d)) if self.keep_cov_history else None
        fe = np.empty((T, C)) if self._fe else None
        self._chk(_lib.lib().rxhip_mnreg_get_history(self._h, _p(mean), _p(var), _p(cov) if cov is not None else None, _p(fe) if self._fe else None))
        return mean, var, cov, fe

    def statistics(self):
        """offline, the pass alone: (Y [problems][K], S [problems][K], lc [problems], n [problems]) of the data in place."""
        C, K = self.n_problems, self.K
        Y, S, lc, n = np.empty((C, K)), np.empty((C, K)), np.empty(C), np.empty(C)
        self._chk(_lib.lib().rxhip_mnreg_get_statistics(self._h, _p(Y), _p(S), _p(lc), _p(n)))
        return Y, S, lc, n


class GammaMixtureEngine(_SeriesEngine):
    """Gamma mixture with a point-mass shape, `s ~ Dirichlet(α⁰); a[k] ~ Gamma(c⁰_k, d⁰_k); b[k] ~ Gamma(e⁰_k, f⁰_k); z[i] ~ Categorical(s); y[i] ~
    GammaMixture(switch = z[i], a = a, b = b)` with `q = q(s) Π q(z_i) Π q(b_k) Π δ(a_k − â_k)` (test/models/mixtures/gamma_mixture_tests.jl:7-40)
    for n_problems independent mixtures of N points and K = 1 … 16 components (include/rxhip.h rxhip_gammamix_desc).  prior_a, prior_b: (shape,
    rate), each [K] (every problem the same) or [problems][K]; prior_alpha the same; init_a (default 1.0), init_b (default (1, 1)), init_s (default
    the prior's α⁰) alike.  schedule: 'auto' or 'streamed' (the same; 'resident' is a value of the C descriptor that the library refuses).  `set_data(y, layout)`: [N][problems] ('time_chain')
    or [problems][N] ('chain_time'), NaN = a missing point; `run(iterations)`; `history()`: â, b shape, b rate, α after every iteration;
    `responsibilities()`: q(z) of the last one (materialize=True)."""

    SCHEDULES = {"auto": _lib.GAMMAMIX_AUTO, "streamed": _lib.GAMMAMIX_STREAMED, "resident": _lib.GAMMAMIX_RESIDENT}

    def __init__(self, N, K, prior_a, prior_b, prior_alpha, init_a=None, init_b=None, init_s=None, n_problems=1, schedule="auto", materialize=False,
                 device=-1, stream=None):
        L = _lib.lib()
        K, C = int(K), int(n_problems)
        shape = (max(C, 0), max(K, 0))

        def full(v, name):
            a = _c(v)
            if a.shape == shape[1:]:
                a = np.ascontiguousarray(np.broadcast_to(a, shape))
            if a.shape != shape:
                raise ValueError(f"{name} must be [K] or [problems][K] = {list(shape)}, got {list(a.shape)}")
            return a

        keep = [full(prior_a[0], "prior_a shape"), full(prior_a[1], "prior_a rate"), full(prior_b[0], "prior_b shape"), full(prior_b[1], "prior_b rate"),
                full(prior_alpha, "prior_alpha")]
        desc = _lib.GammaMixDesc()
        desc.N, desc.n_problems, desc.K = int(N), C, K
        desc.prior_a_shape, desc.prior_a_rate, desc.prior_b_shape, desc.prior_b_rate, desc.prior_alpha = [_p(a) for a in keep]
        if init_a is not None:
            keep.append(full(init_a, "init_a"))
            desc.init_a = _p(keep[-1])
        if init_b is not None:
            keep += [full(init_b[0], "init_b shape"), full(init_b[1], "init_b rate")]
            desc.init_b_shape, desc.init_b_rate = _p(keep[-2]), _p(keep[-1])
        if init_s is not None:
            keep.append(full(init_s, "init_s"))
            desc.init_s_alpha = _p(keep[-1])
        desc.schedule = self.SCHEDULES[schedule] if isinstance(schedule, str) else int(schedule)
        desc.materialize_responsibilities, desc.device = int(bool(materialize)), int(device)
        desc.stream = ctypes.c_void_p(stream) if stream else None
        self.N, self.T, self.K, self.n_problems, self.n_chains, self.materialize = int(N), int(N), K, C, C, bool(materialize)
        self._h = ctypes.c_void_p()
        self._created(L.rxhip_gammamix_create(ctypes.byref(desc), ctypes.byref(self._h)))

    @staticmethod
    def schedule(N, K):
        """1: streamed, for every N and K of the engine's range; 0: outside it."""
        return int(_lib.lib().rxhip_gammamix_schedule(int(N), int(K)))

    def set_stored_log(self, stored):
        """the streamed pass reads ln y from memory (True, the default) or recomputes it (False): the same bits, a measurement switch."""
        self._chk(_lib.lib().rxhip_gammamix_set_stored_log(self._h, int(bool(stored))))

    def history(self):
        """after every iteration of the last run: dict of a, b_shape, b_rate, alpha, each [iterations][problems][K], and fe [iterations][problems] (None
        when the run was without the free energy)."""
        n = max(int(self._iters), 0)
        h = np.empty((n, self.n_problems, 4, self.K))
        fe = np.empty((n, self.n_problems)) if self._fe else None
        self._chk(_lib.lib().rxhip_gammamix_get_history(self._h, _p(h), _p(fe) if self._fe else None))
        return dict(a=h[:, :, 0], b_shape=h[:, :, 1], b_rate=h[:, :, 2], alpha=h[:, :, 3], fe=fe)

    def responsibilities(self):
        """q(z) of the last iteration: [problems][N][K] (a missing point's row is 0)."""
        r = np.empty((self.n_problems, self.N, self.K))
        self._chk(_lib.lib().rxhip_gammamix_get_responsibilities(self._h, _p(r)))
        return r


class Communicator:
    """RCCL communicator made through the C ABI (rxhip_comm_*): rank 0 calls `Communicator.unique_id()`, the 128 bytes
    travel to the other ranks by any host-side means, every rank constructs `Communicator(nranks, id, rank)`."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        st = _lib.lib().rxhip_comm_unique_id(buf)
        if st != _lib.OK:
            raise RxHipError(st, _lib.lib().rxhip_comm_last_error().decode())
        return buf.raw

    def __init__(self, nranks, unique_id, rank, device=-1):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of Communicator.unique_id()")
        self.nranks, self.rank = int(nranks), int(rank)
        h = ctypes.c_void_p()
        st = _lib.lib().rxhip_comm_init_rank(ctypes.byref(h), self.nranks, unique_id, self.rank, int(device))
        if st != _lib.OK:
            raise RxHipError(st, _lib.lib().rxhip_comm_last_error().decode())
        self.handle = h.value

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib().rxhip_comm_destroy(ctypes.c_void_p(self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# the nonlinear state-space engine's class lives in a module of its own (next to the expression tracer it needs) and is part of this one's namespace
from .nlssm import NonlinearSSMEngine  # noqa: E402,F401

// engine.hpp — what every translation unit behind the C ABI shares: the engine object, its family table, the error path, the device guards and the
// helpers every creator, run and result getter uses.  A new family writes its descriptor checks, its buffers, its kernels' launches and one row of the
// family table; it gets for free the handle and its refusal path (new_handle, count_devices, open_device, finish_create), the start and the bookkeeping
// of a run (run_preamble, reserve, finish_run), the check of ingested observations (check_observations), the preamble of its getters (results_ready,
// open_results, sum_chunk_partials) and every entry point common to all engines.
//   rxhip.hip       runtime (pools, arenas), the state-space and drift-chain engines, the entry points common to all engines, the shared helpers
//   vmp_engines.hip the mixture, HGF, probit, HMM, latent-AR, binomial-, linear- and multinomial-regression and Gamma-mixture engines and their family rows
//   graph_abi.hip   the graph entry points: host-only lowering (graph_lowering.hpp), rxhip_create, the node-array executor's rxhip_tree_* wrappers
//   rccl_abi.hip    the RCCL exchange entry points (rxhip_comm_*, rxhip_allreduce_free_energy, rxhip_gmm_allreduce_statistics)
//   tree_engine.hip the node-array executor itself (behind tree_engine.hpp)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/rxhip.h"
#include "lgssm_plan.hpp"
#include "tree_engine.hpp"

namespace rxhip {
struct LgssmVtbl;    // launch_tables.hpp
struct DenseModel;   // dense_kernels.hpp
}
struct DenseTables;  // rxhip.hip: shared per-model tables of the MFMA path
using rxhip::DenseModel;
using rxhip::LgssmVtbl;

// ------------------------------------------------------------------------------------------
// What a handle's OWNER changes after creation — data, runs, modes, counters.  One value-initialised sub-object: rxhip_lgssm_create hands a parked engine
// (engine pool, rxhip.hip) to its next owner by assigning a fresh rxhip_engine_life, so a field added here can never leak from one life to the next.
// Everything that describes the MODEL and its device tables stays in rxhip_engine proper.
struct rxhip_engine_life {
    bool have_data = false;
    long long stream_k = 0;        // rxhip_filter_step: observations seen
    bool have_inputs = false;      // engines with data inputs u[t] (du > 0): rxhip_set_data(RXHIP_VAR_U) has been called
    double stage_ms[4] = {0.0, 0.0, 0.0, 0.0};  // creation stages (rxhip_get_create_stages): tables host | tables device | upload | alloc (zero: nothing was built for this owner)
    bool records_hold_gains = false; // the last run was a smoothing sweep of kd_forward_info / kd_backward_info with one chain per tile: d_filt holds G_t′
    bool records_tinv = false;       // the last smoothing run left mean-only forward records behind the fixed point of V_f (Params::tinv_records)
    bool m_wave8_last = false;       // the last masked sweep ran on the in-wave d ≤ 8 kernels
    int cov_mode = 0;                // rxhip_set_covariance_mode (see below)
    // cov_current: rows 0 … T−1 of d_cov hold what a smoothing sweep of this engine would store — the broadcast of the per-model covariance table
    // (d_gtab row VS at d, dy ≤ 4; d_vstab on the split schedule of the MFMA path).  A smoothing run of a shared-model batch that finds it set stores
    // no covariances (run_impl `cov_once`; mode 1 of rxhip_set_covariance_mode: no materialisation).  The state lives HERE and nowhere else: a parked
    // engine's next owner gets a fresh rxhip_engine_life and pays for its first sweep's stores.  cov_pending: mode 1, the last run left the array to
    // be materialised (ensure_cov).  Who stores into d_cov, and what keeps the state true:
    //   run_impl                    clears the flag at the top of EVERY run (smoothing, filtering, any family) and sets it only after the loop of an
    //                               eligible smoothing run ended without error; every writer below that runs inside run_impl is covered by that
    //   k_backward_sh(_rev)         the eligible sweep itself: rows 0 … T of its table, the same bits every time
    //   kd_split_broadcast          the split schedule's copy of d_vstab (run_dense, ensure_cov); its model pass (full MFMA kernels on workgroup chain 0,
    //                               once per engine, before kd_split_save) runs in the engine's first smoothing sweep, which always stores
    //   k_boundary_scan(_tab), k_forward, k_small_sweep, k_backward, k_forward0
    //                               filtering runs, T == 1 and the per-chain schedules: inside run_impl, never eligible (no backward_sh / filter)
    //   kd_* / km_* / k8_* / k_gseq_*  the other MFMA-path and sequential families: inside run_impl, never eligible
    //   k_forecast, k_forecast_generic  rows ≥ T, engines with a horizon: never eligible (H == 0 is part of the rule)
    //   noise engines               compute V_t in the sweep (skip_marginals): never eligible
    //   rxhip_filter_step           writes its own staging block (d_stream), not d_cov; clears the flag all the same
    //   k_predict, k_joint(_generic), k_predict_generic, kd_cross_from_records, k_gather_chains, noise moments
    //                               read d_cov; the getters' sequential re-run (k_gseq_*) writes scratch arrays of its own
    //   drift / probit / HGF / mixture engines  other kinds: their own run paths, no shared-model sweep
    // No kernel of a run uses d_cov as scratch, and the arena never overlays it with another buffer (ArenaPlan).  Setters: rxhip_set_covariance_mode and
    // rxhip_set_fixed_point_exits clear the flag; rxhip_set_data(_device), rxhip_lgssm_set_chain_offsets and the known inputs do not — none enters the table.
    bool cov_pending = false, cov_current = false;
    uint64_t cov_writes = 0;         // rxhip_get_covariance_writes: smoothing sweeps (and mode-1 materialisations) that stored the per-chain covariance array
    bool noise_continue = false;     // rxhip_lgssm_noise_continue: runs go on from the current q(W) (iteration-at-a-time drivers)
    bool full_recursions = false;    // rxhip_set_fixed_point_exits(e, 0): every recursion of a sweep in full (no frozen stretches, full records)
    // results bookkeeping
    int last_iterations = 0;
    bool last_want_fe = false;
    bool ran = false, last_filter = false;
    uint64_t rule_calls = 0, products = 0, marginals = 0;
    // per-kernel device times (rxhip_set_profiling)
    double k_ms[RXHIP_K_COUNT] = {};
    uint64_t k_n[RXHIP_K_COUNT] = {};
};
// The family of an engine: one row of the family table each (EngineFamily below).
enum class EngineKind : int {
    Lgssm = 0,    // linear Gaussian state-space model: every schedule of rxhip.hip's run_impl
    Mixture = 1,  // uni- and multivariate Gaussian mixture (gmm_kernels.hpp, mvgmm_kernels.hpp, mvgmm_dense_kernels.hpp)
    Hgf = 2,      // hierarchical Gaussian filter (hgf_kernels.hpp)
    Drift = 3,    // noise-free drift chain (drift_kernels.hpp)
    Probit = 4,   // probit chain, batched EP (probit_kernels.hpp)
    Tree = 5,     // the level-scheduled node-array executor (tree_engine.hip; everything lives behind `tree`)
    Hmm = 6,      // hidden Markov model, batched forward–backward VMP (hmm_kernels.hpp)
    Lar = 7,      // latent autoregressive model, batched banded structured VMP (lar_kernels.hpp)
    Binreg = 8,   // binomial regression, batched Pólya-Gamma VMP (binreg_kernels.hpp)
    Arreg = 9,    // regression / autoregression with unknown coefficients and noise precision, batched Normal-Gamma VMP from the statistics
                  // (arreg_kernels.hpp), regressor mode: X and y through the family's own set_data, host arrays only
    ArregLagged = 10,   // … lagged mode: the raw series through the common ingest, host or device (the same run, release and getters; the two rows
                        // differ in how the data arrive, which is what a row of the family table says)
    Mnreg = 11,         // multinomial regression, batched stick-breaking Pólya-Gamma VMP from the column sums (mnreg_kernels.hpp), offline: every
                        // iteration of a run in one resident launch
    MnregOnline = 12,   // … streamed one row at a time with the posterior fed back as the next prior (the same plumbing, release and getters)
    GammaMix = 13,      // Gamma mixture with a point-mass shape, batched VMP (gammamix_kernels.hpp): a streamed pass and an update launch per iteration
    Nlssm = 14,         // nonlinear state-space model, batched extended / unscented filtering and smoothing (nlssm_kernels.hpp, expr.hpp)
};
struct rxhip_engine : rxhip_engine_life {
    // one device allocation holds every buffer of a state-space engine (creation / destruction cost two driver calls
    // instead of ≈40: 2.9 ms -> see DESIGN §6c); pointers inside it are never freed individually
    char* arena = nullptr;
    size_t arena_bytes = 0;
    bool in_arena(const void* q) const { return arena && (const char*)q >= arena && (const char*)q < arena + arena_bytes; }
    // description
    rxhip::plan::ScheduleHooks hooks;   // state-space engines: the test hooks as rxhip_lgssm_create found them — every schedule decision of the engine's life reads these
    int d = 0, dy = 0;
    int dpad = 0;  // dense path: d rounded up to a multiple of 16 (kernel dimension); == d otherwise
    long long T = 0, n_chains = 0;
    long long H = 0;     // time indices without an observation after the T observed ones (rxhip_lgssm_desc.horizon)
    long long Tout() const { return T + H; }  // rows of the posterior / prediction arrays
    std::vector<double> h_bq;  // per model B | Q (row-major): the prediction kernel needs them, the sweep does not
    double* d_bq = nullptr;
    int n_models = 1;
    int ptt = 0;
    int S = 0;
    long long L = 0, Llast = 0;
    bool uniform = true;
    const LgssmVtbl* vt = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // device memory
    double* d_y = nullptr;
    bool own_y = false;
    double *d_filt = nullptr, *d_mean = nullptr, *d_cov = nullptr, *d_cst = nullptr, *d_tab = nullptr,
           *d_vtab = nullptr, *d_scan = nullptr, *d_agg = nullptr, *d_elem = nullptr, *d_fstart = nullptr, *d_beta = nullptr, *d_fe_part = nullptr,
           *d_fe_chain = nullptr, *d_fe_total = nullptr;
    int* d_chain_model = nullptr;
    int* d_status = nullptr;
    double* d_fe_blocks = nullptr;
    EngineKind kind = EngineKind::Lgssm;
    rxhip::tree::Engine* tree = nullptr;
    // one sub-object per family with state of its own (the state-space engine's lives in the fields around them)
    struct Drift { double m0 = 0, v0 = 1, c = 0, obs_var = 1; } dr;
    struct Hgf {
        rxhip_hgf_desc ds;
        double *d_out = nullptr, *d_fe_series = nullptr, *d_gh = nullptr, *d_fe_total = nullptr;
        int fe_cap = 0;
    } h;
    struct Probit {   // one block (sites | forward messages | free-energy scratch) next to d_mean / d_cov / d_fe_chain / d_fe_total
        rxhip_probit_desc ds;
        double *d_block = nullptr, *d_gh = nullptr, *d_fe_series = nullptr;
        int fe_cap = 0;
    } pb;
    struct Hmm {      // parameter block (π | prior | init | counts | log tables ×2 | Ã B̃ | KL | statistics | their sum | log Z̃), α̂ and γ, free energies
        int K = 0, M = 0, shared = 0;
        double *d_par = nullptr, *d_alpha = nullptr, *d_gamma = nullptr, *d_fe_series = nullptr;
        int fe_cap = 0;
    } hm;
    struct Lar {      // constants, parameter block (initial q | G per set | KL | statistics | their sum), parameter history, row records, m and the Σ band, free energies
        int P = 0, shared = 0;
        double *d_cst = nullptr, *d_par = nullptr, *d_hist = nullptr, *d_rec = nullptr, *d_out = nullptr, *d_fe_series = nullptr;
        int fe_cap = 0, hist_cap = 0;
    } la;
    struct Breg {     // X, n_eff, κ, constants, ξ, lc, S, the pass's partials, ξ partials, parameter history, free energies; y and n_trials stay on the host for the checks
        int d = 0, nchunk = 0, nchunk_xi = 0, hist_cap = 0;
        double *d_X = nullptr, *d_neff = nullptr, *d_kappa = nullptr, *d_cst = nullptr, *d_xi = nullptr, *d_lc = nullptr, *d_S = nullptr, *d_part = nullptr,
               *d_xi_part = nullptr, *d_hist = nullptr, *d_fe_prob = nullptr;
        bool have_X = false, have_y = false, have_n = false, ready = false;
        std::vector<double> h_y, h_n;
    } br;
    struct Arreg {    // kinds 9 and 10: X and y (regressor mode; lagged mode reads d_y), constants, the pass's partials (kept: the statistics of the data in place), history, free energies
        int d = 0, lagged = 0, shared = 0, nchunk = 0, hist_cap = 0;
        long long rows = 0;   // rows per series as the pass counts them
        double *d_X = nullptr, *d_yreg = nullptr, *d_cst = nullptr, *d_part = nullptr, *d_hist = nullptr, *d_fe = nullptr;
        bool have_X = false, have_y = false, stats_ready = false;
    } ar;
    struct Mnreg {    // kinds 11 and 12: the counts, constants, the pass's partials (kept: the statistics of the data in place), offline history and free energies;
                      // online: mean | variance history, F_t, per-iteration sums, the last step's mean | covariance, the covariance history on request
        int K = 0, d = 0, online = 0, keep_cov = 0, nchunk = 0, hist_cap = 0;
        long long n_trials = 0;
        double *d_data = nullptr, *d_cst = nullptr, *d_part = nullptr, *d_hist = nullptr, *d_fe = nullptr, *d_on = nullptr, *d_oncov = nullptr, *d_feit = nullptr;
        bool have = false, stats_ready = false;
        uint64_t stats_launches = 0;
    } mn;
    struct GammaMix {  // kind 13: priors, the state every run starts from, the current state and the pass's partials, history, free energies, q(z) on request,
                       // the problem-major copy of a batch's data and (pass on stored logarithms) ln y
        int K = 0, KT = 0, sched = 0, nchunk = 0, hist_cap = 0, materialize = 0, stored_log = 0;
        double *d_prior = nullptr, *d_init = nullptr, *d_state = nullptr, *d_part = nullptr, *d_hist = nullptr, *d_fe = nullptr, *d_resp = nullptr, *d_yt = nullptr,
               *d_ly = nullptr;
    } gx;
    struct Nlssm {     // kind 14: the descriptor's scalars, the expression program, the priors, q(τ) history, the smoothing records, free energies, the first non-finite event
        int method = 0, unknown = 0, per_series = 0, smooth = 0;
        double Q[16] = {}, Hm[16] = {}, R[16] = {}, a0 = 1, b0 = 1, sc = 1, wm0 = 0, wc0 = 0, wi = 0;
        size_t lds_bytes = 0;
        double *d_prog = nullptr, *d_prior = nullptr, *d_noise = nullptr, *d_rec = nullptr, *d_fe_series = nullptr, *d_where = nullptr;
    } nl;
    struct Gmm {
        long long N = 0;
        int K = 0, KT = 0, materialize = 0, nblocks = 0, it = 0, iterations = 0, hist_cap = 0;
        int mvd = 0;          // 0: univariate engine; d ≥ 1: multivariate engine (mvgmm_kernels.hpp) of that dimension
        int nq = 0;           // statistics per iteration (the multi-GPU all-reduce payload)
        int hist_stride = 0;  // doubles of history per iteration
        int state_size = 0;   // doubles of the marginal block (d_par / d_init)
        double *d_resp = nullptr, *d_par = nullptr, *d_drv = nullptr, *d_prior = nullptr, *d_init = nullptr,
               *d_partial = nullptr, *d_totals = nullptr, *d_hist = nullptr, *d_fe = nullptr;
    } g;
    // dense (d = 16·NT) path
    bool dense = false;
    int nt = 0;
    double *d_scanm = nullptr, *d_fstart_m = nullptr, *d_beta_xi = nullptr, *d_vend = nullptr, *d_qtab = nullptr, *d_loc = nullptr, *d_bnd = nullptr;
    const int* d_canon = nullptr;  // canonical indices of the boundary maps (DenseParams::canon), inside the shared table block
    int scan_sg = 1, scan_ng = 1;  // two-level boundary scan of the dense path: group size, groups
    int agg_oc = 1, agg_kc = 1;    // dense aggregation product: offsets per K-chunk, K-chunks
    double* d_aggpart = nullptr;   // [chain][agg_kc][S][2·dpad] partial sums of kd_agg_gemm
    // shared-model smoothing in one pass over the observations (k_forward0): tables, see lgssm_kernels.hpp
    bool fused = false;
    double *d_ftab = nullptr, *d_mtab = nullptr, *d_ntab = nullptr, *d_pos = nullptr, *d_fseg = nullptr;
    double fe_const = 0.0;
    double *d_gtab = nullptr, *d_segend = nullptr, *d_sblk = nullptr;
    // reverse-filter schedule (k_backward_sh_rev): checkpoint stride 2^ck_log2 of the z records, 0: a record per time index
    int ck_log2 = 0;
    int sweep_waves_fwd = 1, sweep_waves_bwd = 1;   // wavefronts per workgroup of k_forward0_ck / k_backward_sh_rev (plan::sweep_waves)
    long long nck = 0;
    double *d_amp = nullptr, *d_ainv = nullptr;
    int* d_ckfail = nullptr;
    hipEvent_t ev_tab0 = nullptr, ev_tab1 = nullptr;  // around the once-per-engine table kernels (rxhip_get_model_tables_ms)  // table-driven backward sweep (k_backward_sh): batches of a multiple of 64 chains
    bool sequential = false;  // no per-position tables: missing observations / per-step constants (per-chain records; the segment
                              // elements are computed in the lane, k_seg_elements, or the chain is ONE segment)
    double* d_elemx = nullptr;
    double* h_io = nullptr;       // pinned staging of rxhip_lgssm_infer (pooled)
    size_t h_io_bytes = 0;
    double* h_stream = nullptr;   // its pinned host staging block
    double* d_stream = nullptr;   // rxhip_filter_step: belief per chain | staging of y, mean, cov, fe (allocated on first use)
    double *d_mu = nullptr, *d_nu = nullptr, *d_cx = nullptr, *d_cy_raw = nullptr;  // known inputs: μ[t] [Tout][d], ν[t] = B μ[t] + d[t] [Tout][dy], c[t], d[t]
    std::vector<double> h_mu, h_nu, h_cx, h_cy, h_offA, h_offB;
    std::vector<double> h_cx_const, h_cy_const;  // the offsets the engine was created with (graph constants), for RXHIP_VAR_U
    std::vector<int> h_offsm;
    int du = 0;                    // graph engines with data inputs `+ B_u * u[t]`: dimension of u, B_u [d][du], which steps have one
    std::vector<double> h_Bu;
    std::vector<char> h_umask;
    bool off_chain = false;        // the device offset arrays carry a chain axis (rxhip_lgssm_set_chain_offsets)
    double* d_off_chain = nullptr; // their block: μ | ν | c | d with a chain axis, and A | B of every model
    std::vector<double> h_user;  // MFMA path: user-level A | P | B | Q | Q⁻¹ of every model (generic_kernels.hpp)
    double* d_user = nullptr;
    int* d_step_model = nullptr;
    // MFMA path, a batch that shares one model: matrices once per engine, vectors per sweep (dense_split_kernels.hpp)
    bool split = false, split_ready = false;
    // rxhip_set_covariance_mode: 0 = every sweep writes the covariance of every chain; 1 = shared-model batches on the split schedule write
    // the per-chain array on request (the values do not depend on the data: one [T][d][d] table per model).  cov_pending / cov_current: rxhip_engine_life
    int m_dpad = 0, m_nt = 0;        // masked schedule: tile dimension 16·⌈max(d, dy)/16⌉ (the engine's own dpad pads d only)
    int m_sg = 0, m_ng = 0;          // masked schedule: groups of the two-level boundary recursion (0: one level)
    int m_models = 1;                // masked schedule: constant blocks (per-step constants: desc.n_models, else 1)
    bool m_stepm = false;            // per-step constants on the masked schedule
    bool m_chainm = false;           // one model per chain on the masked schedule
    DenseModel* m_modtab = nullptr;  // [m_models] constant-block pointers for the sweep kernels (one model per chain)
    double* m_feconst = nullptr;
    double *m_grp = nullptr, *m_gvec = nullptr;
    int m_hs = 0, m_hs_rounds = 0;   // masked schedule: log-depth boundary recursion (km_compose / km_apply)
    int m_hs_n = 0, m_hs_g = 1;      // … over m_hs_n entries of m_hs_g segments each (km_fold / km_inner when m_hs_g > 1)
    double *m_hsel = nullptr, *m_hsvec = nullptr;
    double *d_dtab = nullptr, *d_vlast = nullptr, *d_vstab = nullptr, *d_fe_const = nullptr;
    bool gseq = false;        // d > 4 with `missing` observations or per-step constants: sequential schedule (gseq_kernels.hpp)
    // … and, for `missing` observations under ONE model, the time-parallel schedule of dense_mseg_kernels.hpp for smoothing runs
    bool mseg = false;
    int mS = 0;               // its segments / segment length
    long long mL = 1;
    char* mseg_block = nullptr;   // one allocation: padded model | constants workspace | cst | obs | nobs | elements | boundaries | records | scratch
    double *m_in = nullptr, *m_cw = nullptr, *m_cst = nullptr, *m_obs = nullptr, *m_nobs = nullptr, *m_el = nullptr, *m_vec = nullptr,
           *m_bnd = nullptr, *m_lb = nullptr, *m_ws = nullptr, *m_fe_part = nullptr;
    double* d_prior = nullptr;  // gseq: [n_models][m0 | V0]
    bool masked = false;      // NaN observations are `missing` (rxhip_lgssm_desc.allow_missing): per-chain records, one segment
    int pack = 1;             // 2: pairs of chains share a 16×16 tile as a block-diagonal model (d ≤ 8), see dense_kernels.hpp
    long long wg_chains = 0;  // chains (or pairs) the kernels' grids run over
    int dyk = 0;              // observation dimension at kernel level (2·dy when packed)
    std::vector<struct DenseTables*> dts;  // shared per-model device tables of the MFMA path (d_cst, d_tab, … point into model 0's)
    struct DenseModel* d_models = nullptr;  // [n_models] table pointers on the device (several models per engine)
    std::vector<double> h_cst0;  // model 0's constant block (kernel argument when all chains share it)
    int fe_total_cap = 0;
    // profiling
    bool profiling = false;
    double* h_stage = nullptr;   // pinned staging block of the creation upload (arena_commit), kept until destruction
    size_t h_stage_bytes = 0;
    // unknown observation-noise precision (rxhip_lgssm_noise_create, noise_kernels.hpp): one block B | prior | state | history
    bool noise = false;
    char* noise_block = nullptr;
    double *n_B = nullptr, *n_prior = nullptr, *n_state = nullptr, *n_hist = nullptr, *n_part = nullptr;
    int n_hist_cap = 0, n_slices = 1;
    struct Pending { int k; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    std::string err = "";
    std::string pool_key;   // non-empty: this engine may be parked by rxhip_destroy and handed out again by rxhip_lgssm_create (engine pool below)
    // scratch of the cross-GPU sums (rxhip_allreduce_free_energy / rxhip_gmm_allreduce_statistics): [nranks][n]
    double* d_coll = nullptr;
    size_t coll_cap = 0;
};

inline rxhip_status fail(rxhip_engine* e, rxhip_status s, const char* fmt, ...) {
    if (e) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        e->err = buf;
    }
    return s;
}
// entry points of the state-space / mixture engines, called on an engine of the node-array executor
#define TREE_GUARD(e) do { if ((e) && (e)->tree) return fail((e), RXHIP_ERR_UNSUPPORTED, "%s: not available on an engine of the node-array executor (rxhip_tree_* entry points)", __func__); } while (0)
// a temporary device block that is freed on every path out of its scope (early HIPCHK returns included)
struct DevTmp {
    void* p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp&) = delete;
    DevTmp& operator=(const DevTmp&) = delete;
    ~DevTmp() { if (p) (void)hipFree(p); }
};
#define HIPCHK(e, call)                                                                              \
    do {                                                                                             \
        hipError_t _err = (call);                                                                    \
        if (_err != hipSuccess)                                                                      \
            return fail((e), RXHIP_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_err), \
                        __FILE__, __LINE__);                                                         \
    } while (0)


// Every entry point runs on the engine's device and leaves the CALLER's current device as it found it (a host that drives
// several GPUs from one thread — torch, the Julia shim — must not be left on another device after a destroy / getter).
struct DevGuard {
    int prev = -1;
    bool changed = false;
    hipError_t set(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == dev) return hipSuccess;
        hipError_t err = hipSetDevice(dev);
        changed = err == hipSuccess;
        return err;
    }
    ~DevGuard() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
};
#define SET_DEVICE(e) DevGuard _dev_guard; HIPCHK((e), _dev_guard.set((e)->device))

// One row per EngineKind: what the entry points common to all engines (rxhip_run, rxhip_set_data(_device), the free-energy and marginal getters,
// rxhip_destroy) need to know about a family.  Plain function pointers and flags, like the launch tables (launch_tables.hpp).  The rows of the
// families in vmp_engines.hip are defined there (vmp_family), the state-space and drift rows in rxhip.hip (family_of); the node-array executor's
// row is empty (every entry point hands an engine with `tree` to tree_engine.hip before it looks at the row).  The rows are function-local
// statics: a namespace-scope constant would also be emitted for the device, where the host functions it points to do not exist.
struct EngineFamily {
    rxhip_status (*run)(rxhip_engine* e, int32_t iterations, int32_t want_fe);   // rxhip_run_async
    bool filter_twin;                                      // rxhip_run_filter is meaningful: a state-space engine with a streaming twin
    rxhip_status (*check_data)(rxhip_engine* e);           // after a successful ingest of observations, host or device (null: any double is data)
    rxhip_status (*set_data)(rxhip_engine* e, int32_t var_id, const double* host, size_t n);   // replaces rxhip_set_data (null: the common ingest)
    const char* no_device_data;                            // text of rxhip_set_data_device's refusal (null: accepted)
    double* (*fe_total)(const rxhip_engine* e);            // the per-iteration free-energy buffer (null: d_fe_total)
    bool has_x;                                            // RXHIP_VAR_X marginals exist (d_mean / d_cov)
    void (*release)(rxhip_engine* e);                      // frees the family's sub-object (null: nothing beyond the common buffers)
};

// destruction: device buffers of an engine that are freed unless they are part of its arena (free_all and the families' release hooks)
inline void free_buffers(rxhip_engine* e, std::initializer_list<double**> bufs) {
    for (double** b : bufs)
        if (*b) { if (!e->in_arena(*b)) (void)hipFree(*b); *b = nullptr; }
}

// what the translation units of the engines share with the runtime in rxhip.hip
namespace rxhip {
// status bit of k_hmm_sweep (hmm_kernels.hpp; next to ST_NOT_POSDEF = 1, ST_NONFINITE = 2, ST_PROBIT_BAD_Y = 4, ST_HMM_BAD_X = 8, ST_LAR_BAD_Y = 16): a normaliser of
// the forward–backward sweep underflowed.  rxhip_sync reports it as RXHIP_ERR_NONFINITE_FE with a text of its own.
constexpr int ST_HMM_UNDERFLOW = 32;
// status bit of k_nlssm_forward (nlssm_kernels.hpp): a value of f, of its Jacobian or of the predicted moments was not finite; the engine's `where`
// word holds the first (step, series).  rxhip_sync reports it as RXHIP_ERR_NONFINITE_FE with a text of its own.
constexpr int ST_NLSSM_NONFINITE = 64;
const EngineFamily& family_of(const rxhip_engine* e);   // the row of the engine's kind
const EngineFamily* vmp_family(EngineKind kind);        // … of a family of vmp_engines.hip (null: not one of them)
inline double* fe_total_of(const rxhip_engine* e) { const auto f = family_of(e).fe_total; return f ? f(e) : e->d_fe_total; }
// an idle stream of the device (pooled: creating one costs milliseconds on this runtime)
hipError_t stream_acquire(int device, hipStream_t* out);
// the HIP-event pair around a kernel of an engine that is being profiled
rxhip_status prof_begin(rxhip_engine* e, int k);
rxhip_status prof_end(rxhip_engine* e);
bool host_chol_inv(int n, const double* A, double* out, double* logdet);   // host Cholesky inverse + log-determinant of an SPD matrix
// rxhip_expr_eval (vmp_engines.hip, next to the engine that runs programs): a refusal leaves its text in err
rxhip_status expr_eval(const rxhip_expr_program* f, const double* x, int64_t n, double* value, double* jac, int device, std::string& err);

// ---- creators -------------------------------------------------------------------------------------------------------------------
// A handle-first creator is: new_handle, the family's own refusals (each with a text), count_devices, the description, open_device, the family's
// buffers, finish_create.
// The head: `out` and the descriptor are checked (a null `out`, or desc_ok false: a bare RXHIP_ERR_BADARG with *out == nullptr), then *out is a
// fresh handle of `kind` with device = -1, so that every later refusal of the creator can leave its text in it (fail; the caller reads it with
// rxhip_last_error and destroys the handle).
rxhip_status new_handle(bool desc_ok, rxhip_engine** out, EngineKind kind);
// the number of visible devices, or the refusal "no HIP device visible"
rxhip_status count_devices(rxhip_engine* e, int* ndev);
// The device and stream of a new engine: desc.device (≥ 0: checked against the `ndev` visible ones; else the caller's current device) becomes e->device and
// is SELECTED through the creator's own guard — declared before the call, so that it covers the rest of the creator and hands the caller its device
// back on every way out — then desc.stream is adopted or a pooled one acquired.
rxhip_status open_device(rxhip_engine* e, DevGuard& guard, int device, void* stream, int ndev);
// The tail: the common free-energy buffers — d_fe_chain [chains], zeroed, and d_fe_total with room for `fe_capacity` iterations (runs grow it
// with reserve) — and the zeroed status word of the kernels.
rxhip_status finish_create(rxhip_engine* e, size_t chains, int fe_capacity);
// ---- runs -----------------------------------------------------------------------------------------------------------------------
// "iterations must be positive", "no observations": the refusals every run starts with (need_data false: the family has a data check of its own)
rxhip_status run_preamble(rxhip_engine* e, int32_t iterations, bool need_data = true);
// Per-iteration device buffers that share one capacity: grown (never shrunk) to `iterations` entries of `per_iteration` doubles each.  Growing waits for
// the stream, frees what is not part of the arena and leaves the capacity at 0 if an allocation fails.
struct IterBuf { double** p; size_t per_iteration; };
rxhip_status reserve(rxhip_engine* e, int* cap, int iterations, std::initializer_list<IterBuf> bufs);
// the result bookkeeping of a finished run
inline void finish_run(rxhip_engine* e, int iterations, bool want_fe, bool filter = false) {
    e->last_iterations = iterations;
    e->last_want_fe = want_fe;
    e->ran = true;
    e->last_filter = filter;
}
// A family's check of freshly ingested observations, on the device copy, whichever way it arrived: `launch` enqueues the kernel that raises `bit` of
// d_status over the n = T · chains values (nb blocks of 256); a refused array counts as not set.
rxhip_status check_observations(rxhip_engine* e, void (*launch)(rxhip_engine* e, long long n, unsigned nb), int bit, const char* message);
// The refusals of a result getter, in this order: "<name>: no run yet", then — a free-energy array was passed — "<name>: free energy was not
// requested in the last run".  `name` is the entry point's without the rxhip_ prefix.
rxhip_status results_ready(rxhip_engine* e, const char* name, bool wants_fe);
// The whole preamble of a result getter: a bare RXHIP_ERR_BADARG unless kind_ok (the family's predicate; false for a null handle), results_ready, then
// the engine's device selected through the getter's own guard (declared before the call, as for open_device) and its stream drained.  A getter with
// refusals of its own that come before "no run yet" has tested the kind for them and passes true.
rxhip_status open_results(rxhip_engine* e, DevGuard& guard, bool kind_ok, const char* name, bool wants_fe);
// tot[q] = Σ_c part[c · n + q], q < n, over the nchunk partials of one chain in ascending chunk order: the order in which the iterate kernels add them
void sum_chunk_partials(const double* part, size_t nchunk, size_t n, double* tot);
}  // namespace rxhip

// vmp_engines.hip — the engines of the pattern-matched families other than the state-space ones, behind the C ABI.  Per family: its creator, its
// getters, its run and its row of the family table (engine.hpp EngineFamily), through which the entry points common to all engines reach it.
//   mixture   uni- and multivariate Gaussian mixture (gmm_kernels.hpp, mvgmm_kernels.hpp, mvgmm_dense_kernels.hpp)
//   HGF       hierarchical Gaussian filter (hgf_kernels.hpp; a11)
//   probit    probit chain, batched EP (probit_kernels.hpp)
//   HMM       hidden Markov model, forward–backward VMP (hmm_kernels.hpp)
//   LAR       latent autoregressive model, banded structured VMP (lar_kernels.hpp)
//   binreg    binomial regression, Pólya-Gamma VMP (binreg_kernels.hpp)
//   arreg     regression / autoregression with unknown coefficients and noise precision, Normal-Gamma VMP from the statistics (arreg_kernels.hpp): two
//             rows, X and y from the host or the raw series through the common ingest
//   mnreg     multinomial regression, stick-breaking Pólya-Gamma VMP from the column sums (mnreg_kernels.hpp): two rows, offline and online
//   gammamix  Gamma mixture with a point-mass shape (gammamix_kernels.hpp): a streamed pass and an update launch per iteration
//   nlssm     nonlinear state-space model, extended / unscented filtering and smoothing (nlssm_kernels.hpp) with f as an expression program (expr.hpp)
// The runtime they share with the state-space engines — streams, profiling events, the engine handle, the creation and run helpers — is rxhip.hip's
// (engine.hpp).  No kernels of the state-space path live here.
#include "../../include/rxhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "gmm_kernels.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Warray-bounds"   // (k_hgf_filter<FE = false> indexes its FE-sized scratch inside `if (FE)` branches that are dead in that instance)
#include "hgf_kernels.hpp"
#pragma clang diagnostic pop
#include "mvgmm_kernels.hpp"
#include "mvgmm_dense_kernels.hpp"
#include "probit_kernels.hpp"
#include "hmm_kernels.hpp"
#include "lar_kernels.hpp"
#include "binreg_kernels.hpp"
#include "arreg_kernels.hpp"
#include "mnreg_kernels.hpp"
#include "gammamix_kernels.hpp"
#include "nlssm_kernels.hpp"
#include "engine.hpp"

using namespace rxhip;

// ------------------------------------------------------------------------------------------
// Gaussian-mixture VMP engine
static int gmm_kt(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }
static MvgParams mvg_params(rxhip_engine* e) {
    MvgParams p;
    p.N = e->g.N; p.K = e->g.K; p.y = e->d_y; p.resp = e->g.d_resp; p.state = e->g.d_par; p.drv = e->g.d_drv;
    p.prior = e->g.d_prior; p.partial = e->g.d_partial; p.totals = e->g.d_totals; p.hist = e->g.d_hist; p.fe = e->g.d_fe;
    p.iteration = e->g.it; p.nblocks = e->g.nblocks; p.write_resp = 0; p.status = e->d_status;
    return p;
}
template <int D, int KT>
struct MvgLaunch {
    static void init(const MvgParams& p, hipStream_t s) { hipLaunchKernelGGL((k_mvg_init<D, KT>), dim3(1), dim3(64), 0, s, p); }
    static void pass(const MvgParams& p, bool resp, hipStream_t s) {
        if (resp) hipLaunchKernelGGL((k_mvg_pass<D, KT, true>), dim3(p.nblocks), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((k_mvg_pass<D, KT, false>), dim3(p.nblocks), dim3(256), 0, s, p);
    }
    static void reduce(const MvgParams& p, hipStream_t s) {
        hipLaunchKernelGGL(k_mvg_reduce, dim3(KT * MvgDim<D>::STAT + 1), dim3(256), 0, s, p, KT * MvgDim<D>::STAT + 1);
    }
    static void update(const MvgParams& p, bool fe, hipStream_t s) {
        if (fe) hipLaunchKernelGGL((k_mvg_update<D, KT, true>), dim3(1), dim3(64), 0, s, p);
        else hipLaunchKernelGGL((k_mvg_update<D, KT, false>), dim3(1), dim3(64), 0, s, p);
    }
};
// component tile: the statistics of a lane live in registers, KT·(1 + d + d(d+1)/2) ≤ 128 doubles
static int mvg_kt(int d, int K) {
    const int cap = d <= 2 ? 16 : 8;
    const int kt = K <= 4 ? 4 : K <= 8 ? 8 : 16;
    return kt <= cap ? kt : 0;
}
#define MVG_DISPATCH(d, kt, CALL)                                                    \
    switch ((d) * 100 + (kt)) {                                                      \
        case 104: MvgLaunch<1, 4>::CALL; break;  case 108: MvgLaunch<1, 8>::CALL; break;  case 116: MvgLaunch<1, 16>::CALL; break; \
        case 204: MvgLaunch<2, 4>::CALL; break;  case 208: MvgLaunch<2, 8>::CALL; break;  case 216: MvgLaunch<2, 16>::CALL; break; \
        case 304: MvgLaunch<3, 4>::CALL; break;  case 308: MvgLaunch<3, 8>::CALL; break;                                          \
        case 404: MvgLaunch<4, 4>::CALL; break;  default: MvgLaunch<4, 8>::CALL; break;                                           \
    }
// d = 5…32 (mvgmm_dense_kernels.hpp): d and K are runtime values, the pass is templated on the tile count ⌈d/16⌉ only
struct MvdLaunch {
    static void init(const MvgParams& p, int d, hipStream_t s) { hipLaunchKernelGGL(k_mvgd_init, dim3(p.K), dim3(64), 0, s, p, d); }
    static void pass(MvgParams p, int d, bool resp, hipStream_t s) {
        p.write_resp = resp ? 1 : 0;
        if (mvd_tiles(d) == 1) hipLaunchKernelGGL((k_mvgd_pass<1>), dim3(p.nblocks), dim3(256), 0, s, p, d);
        else hipLaunchKernelGGL((k_mvgd_pass<2>), dim3(p.nblocks), dim3(256), 0, s, p, d);
    }
    static void reduce(const MvgParams& p, int nq, hipStream_t s) { hipLaunchKernelGGL(k_mvg_reduce, dim3(nq), dim3(256), 0, s, p, nq); }
    static void update(const MvgParams& p, int d, bool fe, hipStream_t s) {
        if (fe) {
            hipLaunchKernelGGL((k_mvgd_update<true>), dim3(p.K), dim3(64), 0, s, p, d);
            hipLaunchKernelGGL(k_mvgd_fe, dim3(1), dim3(64), 0, s, p, d);
        } else
            hipLaunchKernelGGL((k_mvgd_update<false>), dim3(p.K), dim3(64), 0, s, p, d);
    }
};


static GmmParams gmm_params(rxhip_engine* e) {
    GmmParams p;
    p.N = e->g.N; p.K = e->g.K; p.y = e->d_y; p.resp = e->g.d_resp; p.par = e->g.d_par; p.drv = e->g.d_drv;
    p.prior = e->g.d_prior; p.partial = e->g.d_partial; p.totals = e->g.d_totals; p.hist = e->g.d_hist; p.fe = e->g.d_fe;
    p.iteration = e->g.it; p.nblocks = e->g.nblocks; p.write_resp = 0; p.status = e->d_status;
    return p;
}
template <int KT>
struct GmmLaunch {
    static void init(const GmmParams& p, hipStream_t s) { hipLaunchKernelGGL((k_gmm_init<KT>), dim3(1), dim3(256), 0, s, p); }
    static void pass(const GmmParams& p, bool resp, hipStream_t s) {
        if (resp) hipLaunchKernelGGL((k_gmm_pass<KT, true>), dim3(p.nblocks), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((k_gmm_pass<KT, false>), dim3(p.nblocks), dim3(256), 0, s, p);
    }
    static void reduce(const GmmParams& p, hipStream_t s) { hipLaunchKernelGGL((k_gmm_reduce<KT>), dim3(3 * KT + 1), dim3(256), 0, s, p); }
    static void update(const GmmParams& p, bool fe, hipStream_t s) {
        if (fe) hipLaunchKernelGGL((k_gmm_update<KT, true>), dim3(1), dim3(64), 0, s, p);
        else hipLaunchKernelGGL((k_gmm_update<KT, false>), dim3(1), dim3(64), 0, s, p);
    }
};
#define GMM_DISPATCH(kt, CALL)                   \
    switch (kt) {                                \
        case 1: GmmLaunch<1>::CALL; break;       \
        case 2: GmmLaunch<2>::CALL; break;       \
        case 4: GmmLaunch<4>::CALL; break;       \
        case 8: GmmLaunch<8>::CALL; break;       \
        default: GmmLaunch<16>::CALL; break;     \
    }

// One stage of an iteration on the kernels of the engine's shape: the matrix-core ones (d > 4), the lane ones (d ≤ 4) or the univariate ones.
// `flag`: the pass also writes the responsibilities / the update also evaluates the free energy.
enum class GmmStage { Init, Pass, Reduce, Update };
static void gmm_launch(rxhip_engine* e, GmmStage stage, bool flag = false) {
    const int d = e->g.mvd, kt = e->g.KT;
    hipStream_t s = e->stream;
    if (d > 4) {
        const MvgParams p = mvg_params(e);
        switch (stage) {
            case GmmStage::Init: MvdLaunch::init(p, d, s); break;
            case GmmStage::Pass: MvdLaunch::pass(p, d, flag, s); break;
            case GmmStage::Reduce: MvdLaunch::reduce(p, e->g.nq, s); break;
            case GmmStage::Update: MvdLaunch::update(p, d, flag, s); break;
        }
    } else if (d) {
        const MvgParams p = mvg_params(e);
        switch (stage) {
            case GmmStage::Init: MVG_DISPATCH(d, kt, init(p, s)); break;
            case GmmStage::Pass: MVG_DISPATCH(d, kt, pass(p, flag, s)); break;
            case GmmStage::Reduce: MVG_DISPATCH(d, kt, reduce(p, s)); break;
            case GmmStage::Update: MVG_DISPATCH(d, kt, update(p, flag, s)); break;
        }
    } else {
        const GmmParams p = gmm_params(e);
        switch (stage) {
            case GmmStage::Init: GMM_DISPATCH(kt, init(p, s)); break;
            case GmmStage::Pass: GMM_DISPATCH(kt, pass(p, flag, s)); break;
            case GmmStage::Reduce: GMM_DISPATCH(kt, reduce(p, s)); break;
            case GmmStage::Update: GMM_DISPATCH(kt, update(p, flag, s)); break;
        }
    }
}


extern "C" {

rxhip_status rxhip_gmm_create(const rxhip_gmm_desc* ds, rxhip_engine** out) {
    if (!out) return RXHIP_ERR_BADARG;
    *out = nullptr;
    if (!ds || ds->N <= 0 || ds->K <= 0 || !ds->mu0 || !ds->v0 || !ds->a0 || !ds->b0 || !ds->alpha0 || !ds->init_m_mean ||
        !ds->init_m_var || !ds->init_p_shape || !ds->init_p_rate || !ds->init_s_alpha)
        return RXHIP_ERR_BADARG;
    if (ds->K > 16) return RXHIP_ERR_UNSUPPORTED;
    for (int k = 0; k < ds->K; ++k)
        if (!(ds->v0[k] > 0) || !(ds->a0[k] > 0) || !(ds->b0[k] > 0) || !(ds->alpha0[k] > 0) || !(ds->init_m_var[k] > 0) ||
            !(ds->init_p_shape[k] > 0) || !(ds->init_p_rate[k] > 0) || !(ds->init_s_alpha[k] > 0))
            return RXHIP_ERR_NOT_POSDEF;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RXHIP_ERR_NO_DEVICE;
    rxhip_engine* e = new rxhip_engine();
    *out = e;
    e->kind = EngineKind::Mixture;
    e->g.N = ds->N;
    e->g.K = ds->K;
    e->g.KT = gmm_kt(ds->K);
    e->g.materialize = ds->materialize_responsibilities ? 1 : 0;
    e->n_chains = 1;
    e->T = ds->N;
    e->dy = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    const int KT = e->g.KT, K = e->g.K;
    e->g.nq = 3 * KT + 1;
    e->g.hist_stride = 5 * K;
    e->g.state_size = 5 * KT;
    long long nb = (e->g.N + 255) / 256;
    if (nb > 1024) nb = 1024;  // 4 workgroups per CU, grid-stride over the observations
    e->g.nblocks = (int)nb;
    std::vector<double> prior(5 * KT, 1.0), init(5 * KT, 1.0);
    const double* pr[5] = {ds->mu0, ds->v0, ds->a0, ds->b0, ds->alpha0};
    const double* in[5] = {ds->init_m_mean, ds->init_m_var, ds->init_p_shape, ds->init_p_rate, ds->init_s_alpha};
    for (int f = 0; f < 5; ++f)
        for (int k = 0; k < K; ++k) {
            prior[f * KT + k] = pr[f][k];
            init[f * KT + k] = in[f][k];
        }
    HIPCHK(e, hipMalloc(&e->g.d_prior, sizeof(double) * 5 * KT));
    HIPCHK(e, hipMalloc(&e->g.d_init, sizeof(double) * 5 * KT));
    HIPCHK(e, hipMalloc(&e->g.d_par, sizeof(double) * 5 * KT));
    HIPCHK(e, hipMalloc(&e->g.d_drv, sizeof(double) * 3 * KT));
    HIPCHK(e, hipMalloc(&e->g.d_partial, sizeof(double) * (size_t)nb * (3 * KT + 1)));
    HIPCHK(e, hipMalloc(&e->g.d_totals, sizeof(double) * (3 * KT + 1)));
    HIPCHK(e, hipMemcpy(e->g.d_prior, prior.data(), sizeof(double) * 5 * KT, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->g.d_init, init.data(), sizeof(double) * 5 * KT, hipMemcpyHostToDevice));
    if (e->g.materialize) HIPCHK(e, hipMalloc(&e->g.d_resp, sizeof(double) * (size_t)e->g.N * K));
    HIPCHK(e, hipMalloc(&e->d_status, sizeof(int)));
    HIPCHK(e, hipMemset(e->d_status, 0, sizeof(int)));
    return RXHIP_OK;
}

rxhip_status rxhip_mvgmm_create(const rxhip_mvgmm_desc* ds, rxhip_engine** out) {
    if (!out) return RXHIP_ERR_BADARG;
    *out = nullptr;
    if (!ds || ds->N <= 0 || ds->K <= 0 || ds->d <= 0 || !ds->mu0 || !ds->S0 || !ds->nu0 || !ds->V0 || !ds->alpha0 ||
        !ds->init_m_mean || !ds->init_m_cov || !ds->init_w_nu || !ds->init_w_V || !ds->init_s_alpha)
        return RXHIP_ERR_BADARG;
    const bool dense = ds->d > 4;   // d = 5…32 on the matrix cores (mvgmm_dense_kernels.hpp): no component padding, K ≤ 16
    if (dense ? (ds->d > MVD_DMAX || ds->K > MVD_KMAX) : mvg_kt(ds->d, ds->K) == 0) return RXHIP_ERR_UNSUPPORTED;
    const int d = ds->d, dd = d * d, K = ds->K, KT = dense ? K : mvg_kt(d, K);
    const int SZ = 2 + d + 2 * dd, PRI = d + 2 * dd + 4, STAT = 1 + d + d * (d + 1) / 2, DRV = dense ? mvd_drv_stride(d) : 1 + d * (d + 1) / 2 + d;
    for (int k = 0; k < K; ++k)
        if (!(ds->nu0[k] > d - 1) || !(ds->init_w_nu[k] > d - 1) || !(ds->alpha0[k] > 0) || !(ds->init_s_alpha[k] > 0)) return RXHIP_ERR_NOT_POSDEF;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RXHIP_ERR_NO_DEVICE;
    rxhip_engine* e = new rxhip_engine();
    *out = e;
    e->kind = EngineKind::Mixture;
    e->g.mvd = d;
    e->g.N = ds->N; e->g.K = K; e->g.KT = KT;
    e->g.materialize = ds->materialize_responsibilities ? 1 : 0;
    e->g.nq = KT * STAT + 1; e->g.hist_stride = K * SZ; e->g.state_size = K * SZ;
    e->n_chains = 1; e->T = ds->N; e->dy = d; e->d = d;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    long long nb = dense ? (e->g.N + MVD_TP - 1) / MVD_TP : (e->g.N + 255) / 256;
    const long long nb_cap = dense ? MVD_GRID_CAP : 1024;
    if (nb > nb_cap) nb = nb_cap;
    e->g.nblocks = (int)nb;
    // prior block per component: mu0 | S0⁻¹ | nu0 | V0⁻¹ | alpha0 | log|S0| | log|V0|   (inverses / log-determinants once, here)
    std::vector<double> prior((size_t)K * PRI), init((size_t)K * SZ), tmp(dd);
    for (int k = 0; k < K; ++k) {
        double* pr = prior.data() + (size_t)k * PRI;
        double ldS = 0, ldV = 0;
        for (int a = 0; a < d; ++a) pr[a] = ds->mu0[k * d + a];
        if (!host_chol_inv(d, ds->S0 + (size_t)k * dd, pr + d, &ldS)) return fail(e, RXHIP_ERR_NOT_POSDEF, "prior covariance of m[%d] is not positive definite", k);
        pr[d + dd] = ds->nu0[k];
        if (!host_chol_inv(d, ds->V0 + (size_t)k * dd, pr + d + dd + 1, &ldV)) return fail(e, RXHIP_ERR_NOT_POSDEF, "Wishart scale of w[%d] is not positive definite", k);
        pr[d + 2 * dd + 1] = ds->alpha0[k];
        pr[d + 2 * dd + 2] = ldS;
        pr[d + 2 * dd + 3] = ldV;
        double* in = init.data() + (size_t)k * SZ;
        for (int a = 0; a < d; ++a) in[a] = ds->init_m_mean[k * d + a];
        for (int q = 0; q < dd; ++q) in[d + q] = ds->init_m_cov[(size_t)k * dd + q];
        in[d + dd] = ds->init_w_nu[k];
        for (int q = 0; q < dd; ++q) in[d + dd + 1 + q] = ds->init_w_V[(size_t)k * dd + q];
        in[SZ - 1] = ds->init_s_alpha[k];
        if (!host_chol_inv(d, in + d, tmp.data(), nullptr) || !host_chol_inv(d, in + d + dd + 1, tmp.data(), nullptr))
            return fail(e, RXHIP_ERR_NOT_POSDEF, "initial marginal of component %d is not positive definite", k);
    }
    HIPCHK(e, hipMalloc(&e->g.d_prior, sizeof(double) * prior.size()));
    HIPCHK(e, hipMalloc(&e->g.d_init, sizeof(double) * init.size()));
    HIPCHK(e, hipMalloc(&e->g.d_par, sizeof(double) * init.size()));
    HIPCHK(e, hipMalloc(&e->g.d_drv, sizeof(double) * (size_t)KT * DRV));
    HIPCHK(e, hipMalloc(&e->g.d_partial, sizeof(double) * (size_t)nb * e->g.nq));
    HIPCHK(e, hipMalloc(&e->g.d_totals, sizeof(double) * (e->g.nq + (dense ? K : 0))));   // dense: the components' free-energy terms behind the statistics
    HIPCHK(e, hipMemcpy(e->g.d_prior, prior.data(), sizeof(double) * prior.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->g.d_init, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice));
    if (e->g.materialize) HIPCHK(e, hipMalloc(&e->g.d_resp, sizeof(double) * (size_t)e->g.N * K));
    HIPCHK(e, hipMalloc(&e->d_status, sizeof(int)));
    HIPCHK(e, hipMemset(e->d_status, 0, sizeof(int)));
    return RXHIP_OK;
}

rxhip_status rxhip_gmm_begin_run(rxhip_engine* e, int32_t iterations) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Mixture) return RXHIP_ERR_BADARG;
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    if (rxhip_status st = reserve(e, &e->g.hist_cap, iterations, {{&e->g.d_hist, (size_t)e->g.hist_stride}, {&e->g.d_fe, 1}})) return st;
    HIPCHK(e, hipMemsetAsync(e->g.d_fe, 0, sizeof(double) * iterations, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->g.d_par, e->g.d_init, sizeof(double) * e->g.state_size, hipMemcpyDeviceToDevice, e->stream));
    e->g.it = 0;
    e->g.iterations = iterations;
    gmm_launch(e, GmmStage::Init);
    HIPCHK(e, hipGetLastError());
    e->rule_calls = e->products = e->marginals = 0;
    return RXHIP_OK;
}
rxhip_status rxhip_gmm_accumulate(rxhip_engine* e) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Mixture) return RXHIP_ERR_BADARG;
    if (e->g.it >= e->g.iterations) return fail(e, RXHIP_ERR_STATE, "accumulate: no iteration left (call rxhip_gmm_begin_run)");
    SET_DEVICE(e);
    const bool resp = e->g.materialize && e->g.it == e->g.iterations - 1;
    rxhip_status st;
    if ((st = prof_begin(e, RXHIP_K_GMM_PASS))) return st;
    gmm_launch(e, GmmStage::Pass, resp);
    if ((st = prof_end(e))) return st;
    if ((st = prof_begin(e, RXHIP_K_GMM_REDUCE))) return st;
    gmm_launch(e, GmmStage::Reduce);
    if ((st = prof_end(e))) return st;
    HIPCHK(e, hipGetLastError());
    return RXHIP_OK;
}
rxhip_status rxhip_gmm_statistics_device(rxhip_engine* e, double** stats_dev, int32_t* n) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Mixture) return RXHIP_ERR_BADARG;
    if (stats_dev) *stats_dev = e->g.d_totals;
    if (n) *n = e->g.nq;
    return RXHIP_OK;
}
rxhip_status rxhip_gmm_update(rxhip_engine* e, int32_t want_fe) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Mixture) return RXHIP_ERR_BADARG;
    if (e->g.it >= e->g.iterations) return fail(e, RXHIP_ERR_STATE, "update: no iteration left");
    SET_DEVICE(e);
    rxhip_status st;
    if ((st = prof_begin(e, RXHIP_K_GMM_UPDATE))) return st;
    gmm_launch(e, GmmStage::Update, want_fe != 0);
    if ((st = prof_end(e))) return st;
    HIPCHK(e, hipGetLastError());
    e->g.it++;
    finish_run(e, e->g.it, want_fe != 0);
    // reference-equivalent event counts per iteration (the oracle counts its own invocations the same way)
    const uint64_t N = (uint64_t)e->g.N, K = (uint64_t)e->g.K;
    e->rule_calls += N * (2 + 3 * K);
    e->products += N * (1 + 3 * K);
    e->marginals += N + 3 * K;
    return RXHIP_OK;
}
rxhip_status rxhip_gmm_get_history(rxhip_engine* e, double* hist) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Mixture || !hist) return RXHIP_ERR_BADARG;
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, true, "get_history", false)) return st;
    HIPCHK(e, hipMemcpy(hist, e->g.d_hist, sizeof(double) * (size_t)e->g.it * e->g.hist_stride, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}
rxhip_status rxhip_gmm_get_responsibilities(rxhip_engine* e, double* resp) {
    TREE_GUARD(e);
    if (!e || e->kind != EngineKind::Mixture || !resp) return RXHIP_ERR_BADARG;
    if (!e->g.materialize) return fail(e, RXHIP_ERR_STATE, "responsibilities were not materialised (desc.materialize_responsibilities)");
    if (!e->ran || e->g.it < e->g.iterations) return fail(e, RXHIP_ERR_STATE, "get_responsibilities: run not finished");
    SET_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(resp, e->g.d_resp, sizeof(double) * (size_t)e->g.N * e->g.K, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}


// Gauss–Hermite nodes / weights (Newton iteration on the orthonormal recurrence)
static void gauss_hermite_host(int n, double* x, double* w) {
    const double PIM4 = 0.7511255444649425;
    const int m = (n + 1) / 2;
    double z = 0.0, pp = 0.0;
    for (int i = 0; i < m; ++i) {
        if (i == 0) z = std::sqrt((double)(2 * n + 1)) - 1.85575 * std::pow((double)(2 * n + 1), -0.16667);
        else if (i == 1) z -= 1.14 * std::pow((double)n, 0.426) / z;
        else if (i == 2) z = 1.86 * z - 0.86 * x[0];
        else if (i == 3) z = 1.91 * z - 0.91 * x[1];
        else z = 2.0 * z - x[i - 2];
        for (int its = 0; its < 100; ++its) {
            double p1 = PIM4, p2 = 0.0;
            for (int j = 0; j < n; ++j) {
                const double p3 = p2;
                p2 = p1;
                p1 = z * std::sqrt(2.0 / (j + 1)) * p2 - std::sqrt((double)j / (j + 1)) * p3;
            }
            pp = std::sqrt(2.0 * n) * p2;
            const double z1 = z;
            z = z1 - p1 / pp;
            if (std::fabs(z - z1) <= 1e-15 * (1.0 + std::fabs(z))) break;
        }
        x[i] = z;
        x[n - 1 - i] = -z;
        w[i] = 2.0 / (pp * pp);
        w[n - 1 - i] = w[i];
    }
}
// … and their device table as the HGF and probit kernels read it: nodes [32] | weights / √π [32]
static rxhip_status gauss_hermite_upload(rxhip_engine* e, int n_gh, double** d_gh) {
    double gh[64] = {0}, gx[32], gw[32];
    gauss_hermite_host(n_gh, gx, gw);
    for (int i = 0; i < n_gh; ++i) {
        gh[i] = gx[i];
        gh[32 + i] = gw[i] / 1.7724538509055160273;
    }
    HIPCHK(e, hipMalloc(d_gh, sizeof(gh)));
    HIPCHK(e, hipMemcpy(*d_gh, gh, sizeof(gh), hipMemcpyHostToDevice));
    return RXHIP_OK;
}

// steps per partial sum of k_probit_energy: PROBIT_ECHUNK unless that would be more chunks than a grid dimension holds
static long long probit_echunk(long long T) { return std::max<long long>(PROBIT_ECHUNK, (T + 32767) / 32768); }

rxhip_status rxhip_hgf_create(const rxhip_hgf_desc* ds, rxhip_engine** out) {
    if (!out) return RXHIP_ERR_BADARG;
    *out = nullptr;
    if (!ds || ds->T <= 0 || ds->n_series <= 0 || ds->n_gh < 1) return RXHIP_ERR_BADARG;
    if (ds->n_gh > 32) return RXHIP_ERR_UNSUPPORTED;
    if (!(ds->z_variance > 0) || !(ds->y_variance > 0) || !(ds->z0_var > 0) || !(ds->x0_var > 0)) return RXHIP_ERR_NOT_POSDEF;
    // non-finite parameters: the kernel's exponential clamps its argument (a NaN included), so nothing downstream would report them
    const char* nonfinite = !std::isfinite(ds->z_variance) ? "z_variance" : !std::isfinite(ds->y_variance) ? "y_variance" : !std::isfinite(ds->z0_var) ? "z0_var"
                          : !std::isfinite(ds->x0_var) ? "x0_var" : !std::isfinite(ds->kappa) ? "kappa" : !std::isfinite(ds->omega) ? "omega"
                          : !std::isfinite(ds->z0_mean) ? "z0_mean" : !std::isfinite(ds->x0_mean) ? "x0_mean" : nullptr;
    if (nonfinite) {   // (a handle that carries the text, nothing else: the caller destroys it)
        rxhip_engine* e = new rxhip_engine();
        *out = e;
        e->kind = EngineKind::Hgf;
        e->device = -1;
        return fail(e, RXHIP_ERR_BADARG, "hgf: %s must be finite", nonfinite);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RXHIP_ERR_NO_DEVICE;
    rxhip_engine* e = new rxhip_engine();
    *out = e;
    e->kind = EngineKind::Hgf;
    e->h.ds = *ds;
    e->T = ds->T;
    e->n_chains = ds->n_series;
    e->dy = 1;
    e->d = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    if (rxhip_status st = gauss_hermite_upload(e, ds->n_gh, &e->h.d_gh)) return st;
    HIPCHK(e, hipMalloc(&e->h.d_out, sizeof(double) * 4 * (size_t)ds->T * ds->n_series));
    HIPCHK(e, hipMalloc(&e->d_fe_chain, sizeof(double) * (size_t)ds->n_series));
    HIPCHK(e, hipMalloc(&e->d_status, sizeof(int)));
    HIPCHK(e, hipMemset(e->d_status, 0, sizeof(int)));
    return RXHIP_OK;
}

rxhip_status rxhip_probit_create(const rxhip_probit_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds && ds->T > 0 && ds->n_series > 0, out, EngineKind::Probit)) return st;
    rxhip_engine* e = *out;
    if (!(ds->q > 0) || !std::isfinite(ds->q)) return fail(e, RXHIP_ERR_BADARG, "probit: the transition variance q must be positive and finite (got %g)", ds->q);
    if (!(ds->v0 > 0) || !std::isfinite(ds->v0)) return fail(e, RXHIP_ERR_BADARG, "probit: the prior variance v0 must be positive and finite (got %g)", ds->v0);
    if (ds->n_gh < 1 || ds->n_gh > 32) return fail(e, RXHIP_ERR_BADARG, "probit: n_gh must be 1 … 32 Gauss-Hermite points (got %d)", ds->n_gh);
    if (!std::isfinite(ds->a) || !std::isfinite(ds->c) || !std::isfinite(ds->m0)) return fail(e, RXHIP_ERR_BADARG, "probit: a, c and m0 must be finite");
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    e->pb.ds = *ds;
    e->T = ds->T;
    e->H = 1;   // x has T + 1 entries: the posterior arrays carry one row beyond the observations
    e->n_chains = ds->n_series;
    e->d = e->dy = e->dpad = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    const size_t C = (size_t)ds->n_series, R = (size_t)ds->T + 1;
    const size_t chunks = (size_t)((ds->T + probit_echunk(ds->T) - 1) / probit_echunk(ds->T));
    if (rxhip_status st = gauss_hermite_upload(e, ds->n_gh, &e->pb.d_gh)) return st;
    // sites ξ | w, forward messages pm | pv ([T+1][series] each), Gaussian free-energy part [series], Probit energies [chunks][series]
    HIPCHK(e, hipMalloc(&e->pb.d_block, sizeof(double) * (4 * R * C + C + chunks * C)));
    HIPCHK(e, hipMalloc(&e->d_mean, sizeof(double) * R * C));
    HIPCHK(e, hipMalloc(&e->d_cov, sizeof(double) * R * C));
    return finish_create(e, C, 16);
}

// the hidden Markov model's parameter block (doubles): π | prior | init | counts | log tables ×2 | Ã B̃ | KL | statistics | their sum | log Z̃
static HmmParams hmm_params(const rxhip_engine* e) {
    const size_t C = (size_t)e->n_chains, K = (size_t)e->hm.K, M = (size_t)e->hm.M, KM = (K + M) * K, G = e->hm.shared ? 1 : C;
    HmmParams p;
    p.T = e->T; p.n_series = e->n_chains; p.K = e->hm.K; p.M = e->hm.M; p.shared = e->hm.shared;
    p.x = e->d_y;
    double* q = e->hm.d_par;
    p.pi = q; q += 16;
    p.prior = q; q += G * KM;
    p.init = q; q += G * KM;
    p.counts = q; q += G * KM;
    p.ltab = q; q += 2 * G * KM;
    p.ttab = q; q += G * KM;
    p.kl = q; q += G * 2 * K;
    p.stat = q; q += C * KM;
    p.stat_sum = q; q += KM;
    p.logz = q;
    p.alpha = e->hm.d_alpha; p.gamma = e->hm.d_gamma; p.fe_series = e->hm.d_fe_series; p.status = e->d_status;
    return p;
}
static size_t hmm_param_doubles(size_t C, size_t K, size_t M, bool shared) {
    const size_t KM = (K + M) * K, G = shared ? 1 : C;
    return 16 + 6 * G * KM + G * 2 * K + C * KM + KM + C;
}

rxhip_status rxhip_hmm_create(const rxhip_hmm_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds != nullptr, out, EngineKind::Hmm)) return st;
    rxhip_engine* e = *out;
    if (ds->T < 1) return fail(e, RXHIP_ERR_BADARG, "hmm: T must be at least 1 (got %lld)", (long long)ds->T);
    if (ds->n_series < 1) return fail(e, RXHIP_ERR_BADARG, "hmm: n_series must be at least 1 (got %lld)", (long long)ds->n_series);
    if (ds->K < 2 || ds->K > hmm::kMaxK) return fail(e, RXHIP_ERR_BADARG, "hmm: K must be 2 … %d states (got %d)", hmm::kMaxK, ds->K);
    if (ds->M < 2 || ds->M > hmm::kMaxM) return fail(e, RXHIP_ERR_BADARG, "hmm: M must be 2 … %d symbols (got %d)", hmm::kMaxM, ds->M);
    if (!ds->prior_A || !ds->prior_B || !ds->prior_s0) return fail(e, RXHIP_ERR_BADARG, "hmm: prior_A, prior_B and prior_s0 are required");
    if (ds->per_series && ds->share_parameters) return fail(e, RXHIP_ERR_BADARG, "hmm: shared parameters have one prior and one initial q, not one per series");
    const size_t C = (size_t)ds->n_series, K = (size_t)ds->K, M = (size_t)ds->M, KM = (K + M) * K, G = ds->share_parameters ? 1 : C;
    const size_t sets = ds->per_series ? C : 1;
    auto positive = [](const double* v, size_t n) {
        for (size_t i = 0; i < n; ++i)
            if (!(v[i] > 0.0) || !std::isfinite(v[i])) return false;
        return true;
    };
    if (!positive(ds->prior_A, sets * K * K)) return fail(e, RXHIP_ERR_BADARG, "hmm: every count of prior_A must be positive and finite");
    if (!positive(ds->prior_B, sets * M * K)) return fail(e, RXHIP_ERR_BADARG, "hmm: every count of prior_B must be positive and finite");
    if (ds->init_A && !positive(ds->init_A, sets * K * K)) return fail(e, RXHIP_ERR_BADARG, "hmm: every count of init_A must be positive and finite");
    if (ds->init_B && !positive(ds->init_B, sets * M * K)) return fail(e, RXHIP_ERR_BADARG, "hmm: every count of init_B must be positive and finite");
    double psum = 0.0;
    for (size_t i = 0; i < K; ++i) psum += ds->prior_s0[i];
    if (!positive(ds->prior_s0, K) || !(std::fabs(psum - 1.0) <= 1e-12))
        return fail(e, RXHIP_ERR_BADARG, "hmm: prior_s0 must be positive probabilities summing to 1 within 1e-12 (sum − 1 = %g)", psum - 1.0);
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    e->hm.K = ds->K; e->hm.M = ds->M; e->hm.shared = ds->share_parameters ? 1 : 0;
    e->T = ds->T;
    e->H = 1;   // s has T + 1 entries
    e->n_chains = ds->n_series;
    e->d = e->dy = e->dpad = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    // host image of π | prior | init: one set per parameter set g, the K×K block of A and then the M×K block of B
    std::vector<double> host(16 + 2 * G * KM, 0.0);
    for (size_t i = 0; i < K; ++i) host[i] = ds->prior_s0[i];
    for (size_t g = 0; g < G; ++g) {
        const size_t src = ds->per_series ? g : 0;
        double *pr = &host[16 + g * KM], *in = &host[16 + G * KM + g * KM];
        std::memcpy(pr, ds->prior_A + src * K * K, sizeof(double) * K * K);
        std::memcpy(pr + K * K, ds->prior_B + src * M * K, sizeof(double) * M * K);
        for (size_t i = 0; i < KM; ++i) in[i] = 1.0;
        if (ds->init_A) std::memcpy(in, ds->init_A + src * K * K, sizeof(double) * K * K);
        if (ds->init_B) std::memcpy(in + K * K, ds->init_B + src * M * K, sizeof(double) * M * K);
    }
    const size_t R = (size_t)ds->T + 1;
    HIPCHK(e, hipMalloc(&e->hm.d_par, sizeof(double) * hmm_param_doubles(C, K, M, e->hm.shared != 0)));
    HIPCHK(e, hipMemcpy(e->hm.d_par, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&e->hm.d_alpha, sizeof(double) * R * C * K));
    HIPCHK(e, hipMalloc(&e->hm.d_gamma, sizeof(double) * R * C * K));
    return finish_create(e, C, 32);
}

rxhip_status rxhip_hmm_get_states(rxhip_engine* e, double* probs, int32_t layout) {
    if (!e || e->kind != EngineKind::Hmm) return RXHIP_ERR_BADARG;
    if (!probs) return fail(e, RXHIP_ERR_BADARG, "hmm_get_states: no output array");
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME) return fail(e, RXHIP_ERR_BADARG, "hmm_get_states: unknown layout %d", layout);
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, true, "hmm_get_states", false)) return st;
    const size_t C = (size_t)e->n_chains, K = (size_t)e->hm.K, R = (size_t)e->T + 1;
    if (layout == RXHIP_LAYOUT_TIME_CHAIN || C == 1) {
        HIPCHK(e, hipMemcpy(probs, e->hm.d_gamma, sizeof(double) * R * C * K, hipMemcpyDeviceToHost));
        return RXHIP_OK;
    }
    std::vector<double> tmp(R * C * K);
    HIPCHK(e, hipMemcpy(tmp.data(), e->hm.d_gamma, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < R; ++t)
        for (size_t s = 0; s < C; ++s) std::memcpy(probs + (s * R + t) * K, &tmp[(t * C + s) * K], sizeof(double) * K);
    return RXHIP_OK;
}

rxhip_status rxhip_hmm_get_parameters(rxhip_engine* e, double* A_counts, double* B_counts) {
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, e && e->kind == EngineKind::Hmm, "hmm_get_parameters", false)) return st;
    const size_t C = (size_t)e->n_chains, K = (size_t)e->hm.K, M = (size_t)e->hm.M, KM = (K + M) * K, G = e->hm.shared ? 1 : C;
    std::vector<double> tmp(G * KM);
    HIPCHK(e, hipMemcpy(tmp.data(), hmm_params(e).counts, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < G; ++g) {
        if (A_counts) std::memcpy(A_counts + g * K * K, &tmp[g * KM], sizeof(double) * K * K);
        if (B_counts) std::memcpy(B_counts + g * M * K, &tmp[g * KM + K * K], sizeof(double) * M * K);
    }
    return RXHIP_OK;
}

}  // extern "C"

// the latent autoregressive model's parameter block (doubles): initial q | G, mγ per set | KL per set | statistics [ns][series] | their sum
static LarParams lar_params(const rxhip_engine* e) {
    const size_t C = (size_t)e->n_chains, G = e->la.shared ? 1 : C;
    const int P = e->la.P;
    LarParams p;
    p.T = e->T; p.n_series = e->n_chains; p.P = P; p.shared = e->la.shared; p.want_fe = 0;
    p.y = e->d_y;
    p.cst = e->la.d_cst;
    double* q = e->la.d_par;
    p.init = q; q += lar::nq(P);
    p.gm = q; q += G * (size_t)lar::ng(P);
    p.kl = q; q += G;
    p.stat = q; q += C * (size_t)lar::ns(P);
    p.stat_sum = q;
    p.hist = e->la.d_hist; p.rec = e->la.d_rec; p.zmean = e->la.d_out; p.band = e->la.d_out + ((size_t)e->T + P) * C;
    p.fe_series = e->la.d_fe_series; p.status = e->d_status;
    return p;
}

// a symmetric positive definite p×p matrix (symmetric within 1e-12 of its largest entry, Cholesky succeeds): its symmetrised copy, inverse and ln det
static bool spd_inverse(int p, const double* a, std::vector<double>& sym, std::vector<double>& inv, double* logdet) {
    double big = 0.0;
    for (int i = 0; i < p * p; ++i) {
        if (!std::isfinite(a[i])) return false;
        big = std::max(big, std::fabs(a[i]));
    }
    sym.assign((size_t)p * p, 0.0);
    inv.assign((size_t)p * p, 0.0);
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) {
            if (std::fabs(a[i * p + j] - a[j * p + i]) > 1e-12 * big) return false;
            sym[(size_t)(i * p + j)] = 0.5 * (a[i * p + j] + a[j * p + i]);
        }
    return host_chol_inv(p, sym.data(), inv.data(), logdet);
}

extern "C" {

rxhip_status rxhip_lar_create(const rxhip_lar_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds != nullptr, out, EngineKind::Lar)) return st;
    rxhip_engine* e = *out;
    if (ds->order < 1 || ds->order > lar::kMaxP) return fail(e, RXHIP_ERR_BADARG, "lar: order must be 1 … %d (got %d)", lar::kMaxP, ds->order);
    if (ds->T < 1) return fail(e, RXHIP_ERR_BADARG, "lar: T must be at least 1 (got %lld)", (long long)ds->T);
    if (ds->n_series < 1) return fail(e, RXHIP_ERR_BADARG, "lar: n_series must be at least 1 (got %lld)", (long long)ds->n_series);
    auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!positive(ds->tau)) return fail(e, RXHIP_ERR_BADARG, "lar: tau must be positive and finite (got %g)", ds->tau);
    if (!positive(ds->prior_gamma_shape) || !positive(ds->prior_gamma_rate))
        return fail(e, RXHIP_ERR_BADARG, "lar: prior_gamma shape and rate must be positive and finite (got %g, %g)", ds->prior_gamma_shape, ds->prior_gamma_rate);
    const double ia = ds->init_gamma_shape ? *ds->init_gamma_shape : ds->prior_gamma_shape, ib = ds->init_gamma_rate ? *ds->init_gamma_rate : ds->prior_gamma_rate;
    if (!positive(ia) || !positive(ib)) return fail(e, RXHIP_ERR_BADARG, "lar: init_gamma shape and rate must be positive and finite (got %g, %g)", ia, ib);
    if (!ds->prior_theta_mean || !ds->prior_theta_precision || !ds->prior_x0_mean || !ds->prior_x0_precision)
        return fail(e, RXHIP_ERR_BADARG, "lar: prior_theta_mean, prior_theta_precision, prior_x0_mean and prior_x0_precision are required");
    const int P = ds->order;
    const size_t C = (size_t)ds->n_series, G = ds->share_parameters ? 1 : C, n = (size_t)ds->T + (size_t)P;
    auto finite = [](const double* v, int cnt) {
        for (int i = 0; i < cnt; ++i)
            if (!std::isfinite(v[i])) return false;
        return true;
    };
    if (!finite(ds->prior_theta_mean, P)) return fail(e, RXHIP_ERR_BADARG, "lar: prior_theta_mean must be finite");
    if (!finite(ds->prior_x0_mean, P)) return fail(e, RXHIP_ERR_BADARG, "lar: prior_x0_mean must be finite");
    if (ds->init_theta_mean && !finite(ds->init_theta_mean, P)) return fail(e, RXHIP_ERR_BADARG, "lar: init_theta_mean must be finite");
    std::vector<double> wth0, vth0, w0, v0, vinit, winit;
    double ld_wth0 = 0.0, ld_w0 = 0.0, ld = 0.0;
    if (!spd_inverse(P, ds->prior_theta_precision, wth0, vth0, &ld_wth0))
        return fail(e, RXHIP_ERR_BADARG, "lar: prior_theta_precision is not symmetric positive definite");
    if (!spd_inverse(P, ds->prior_x0_precision, w0, v0, &ld_w0)) return fail(e, RXHIP_ERR_BADARG, "lar: prior_x0_precision is not symmetric positive definite");
    if (ds->init_theta_cov) {
        if (!spd_inverse(P, ds->init_theta_cov, vinit, winit, &ld)) return fail(e, RXHIP_ERR_BADARG, "lar: init_theta_cov is not symmetric positive definite");
    } else
        vinit = vth0;   // the prior's own covariance
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    e->la.P = P; e->la.shared = ds->share_parameters ? 1 : 0;
    e->T = ds->T;
    e->n_chains = ds->n_series;
    e->d = e->dy = e->dpad = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    // host images: the constants (lar::consts) and the initial q
    std::vector<double> cst((size_t)lar::nconst(P), 0.0), init((size_t)lar::nq(P), 0.0);
    {
        double* c = cst.data();
        double *cw0 = c, *cm0 = c + P * P, *ch0 = cm0 + P, *cwth0 = ch0 + P, *cmth0 = cwth0 + P * P, *cwm0 = cmth0 + P, *sc = cwm0 + P;
        for (int i = 0; i < P; ++i) {
            cm0[i] = ds->prior_x0_mean[i];
            cmth0[i] = ds->prior_theta_mean[i];
            for (int j = 0; j < P; ++j) {
                cw0[i * P + j] = w0[(size_t)(i * P + j)];
                cwth0[i * P + j] = wth0[(size_t)(i * P + j)];
            }
        }
        for (int i = 0; i < P; ++i) {
            double s0 = 0.0, s1 = 0.0;
            for (int j = 0; j < P; ++j) { s0 += cw0[i * P + j] * cm0[j]; s1 += cwth0[i * P + j] * cmth0[j]; }
            ch0[i] = s0;
            cwm0[i] = s1;
        }
        sc[0] = ds->prior_gamma_shape; sc[1] = ds->prior_gamma_rate; sc[2] = ld_w0; sc[3] = ld_wth0; sc[4] = ds->tau;
        sc[5] = std::lgamma(ds->prior_gamma_shape); sc[6] = std::log(ds->prior_gamma_rate); sc[7] = std::log(ds->tau);
        for (int i = 0; i < P; ++i) init[(size_t)i] = ds->init_theta_mean ? ds->init_theta_mean[i] : ds->prior_theta_mean[i];
        for (int i = 0; i < P * P; ++i) init[(size_t)(P + i)] = vinit[(size_t)i];
        init[(size_t)(P + P * P)] = ia;
        init[(size_t)(P + P * P + 1)] = ib;
    }
    const size_t par = (size_t)lar::nq(P) + G * (size_t)lar::ng(P) + G + (C + 1) * (size_t)lar::ns(P);
    HIPCHK(e, hipMalloc(&e->la.d_cst, sizeof(double) * cst.size()));
    HIPCHK(e, hipMemcpy(e->la.d_cst, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&e->la.d_par, sizeof(double) * par));
    HIPCHK(e, hipMemcpy(e->la.d_par, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&e->la.d_rec, sizeof(double) * n * (size_t)(P + 2) * C));
    HIPCHK(e, hipMalloc(&e->la.d_out, sizeof(double) * n * (size_t)(P + 2) * C));   // m [n][series] | band [n][P + 1][series]
    return finish_create(e, C, 32);
}

rxhip_status rxhip_lar_get_states(rxhip_engine* e, double* mean, double* cov, int32_t layout) {
    if (!e || e->kind != EngineKind::Lar) return RXHIP_ERR_BADARG;
    if (layout != RXHIP_LAYOUT_TIME_CHAIN && layout != RXHIP_LAYOUT_CHAIN_TIME) return fail(e, RXHIP_ERR_BADARG, "lar_get_states: unknown layout %d", layout);
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, true, "lar_get_states", false)) return st;
    const size_t C = (size_t)e->n_chains, T = (size_t)e->T, P = (size_t)e->la.P, n = T + P;
    std::vector<double> tmp(n * (P + 2) * C);
    HIPCHK(e, hipMemcpy(tmp.data(), e->la.d_out, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    const double *zm = tmp.data(), *band = zm + n * C;
    // x[t] = (z_t … z_{t-P+1}): component a is the scalar of index t + P − 1 − a; Σ(i, j) with i ≤ j sits at band[i][j − i]
    for (size_t t = 1; t <= T; ++t)
        for (size_t s = 0; s < C; ++s) {
            const size_t o = layout == RXHIP_LAYOUT_TIME_CHAIN ? (t - 1) * C + s : s * T + (t - 1);
            for (size_t a = 0; a < P; ++a) {
                const size_t ia = t + P - 1 - a;
                if (mean) mean[o * P + a] = zm[ia * C + s];
                if (cov)
                    for (size_t b = 0; b < P; ++b) {
                        const size_t ib = t + P - 1 - b, lo = std::min(ia, ib), lag = std::max(ia, ib) - lo;
                        cov[(o * P + a) * P + b] = band[(lo * (P + 1) + lag) * C + s];
                    }
            }
        }
    return RXHIP_OK;
}

rxhip_status rxhip_lar_get_parameters(rxhip_engine* e, double* theta_mean, double* theta_cov, double* gamma_shape, double* gamma_rate) {
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, e && e->kind == EngineKind::Lar, "lar_get_parameters", false)) return st;
    const size_t C = (size_t)e->n_chains, P = (size_t)e->la.P, G = e->la.shared ? 1 : C, NQ = (size_t)lar::nq((int)P), rows = (size_t)e->last_iterations * G;
    std::vector<double> tmp(rows * NQ);
    HIPCHK(e, hipMemcpy(tmp.data(), e->la.d_hist, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        const double* q = &tmp[r * NQ];
        if (theta_mean) std::memcpy(theta_mean + r * P, q, sizeof(double) * P);
        if (theta_cov) std::memcpy(theta_cov + r * P * P, q + P, sizeof(double) * P * P);
        if (gamma_shape) gamma_shape[r] = q[P + P * P];
        if (gamma_rate) gamma_rate[r] = q[P + P * P + 1];
    }
    return RXHIP_OK;
}

}  // extern "C"

// every observation of a latent autoregressive engine is finite or NaN
static rxhip_status lar_check_data(rxhip_engine* e) {
    return check_observations(e, [](rxhip_engine* e, long long n, unsigned nb) {
        hipLaunchKernelGGL(k_lar_check_y, dim3(nb), dim3(256), 0, e->stream, (const double*)e->d_y, n, e->d_status);
    }, ST_LAR_BAD_Y, "set_data: an observation is infinite (finite values and NaN = missing are accepted)");
}

template <int P>
static void lar_launch_sweep(const LarParams& p, bool out, hipStream_t stream) {
    const unsigned grid = (unsigned)((p.n_series + 63) / 64);
    if (out) hipLaunchKernelGGL((k_lar_sweep<P, true>), dim3(grid), dim3(64), 0, stream, p);
    else hipLaunchKernelGGL((k_lar_sweep<P, false>), dim3(grid), dim3(64), 0, stream, p);
}

static rxhip_status lar_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains, G = e->la.shared ? 1 : C;
    rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}});
    if (!rs && want_fe) rs = reserve(e, &e->la.fe_cap, iterations, {{&e->la.d_fe_series, C}});
    if (!rs) rs = reserve(e, &e->la.hist_cap, iterations, {{&e->la.d_hist, G * (size_t)lar::nq(e->la.P)}});   // the parameter history: every iteration of the run
    if (rs) return rs;
    LarParams p = lar_params(e);
    p.want_fe = want_fe ? 1 : 0;
    const unsigned ggrid = (unsigned)((G + 255) / 256), sgrid = (unsigned)((C + 255) / 256);
    // every run starts from the initial q
    hipLaunchKernelGGL(k_lar_init, dim3(ggrid), dim3(256), 0, e->stream, p);
    for (int i = 0; i < iterations; ++i) {
        const bool last = i == iterations - 1;
        switch (p.P) {
            case 1: lar_launch_sweep<1>(p, last, e->stream); break;
            case 2: lar_launch_sweep<2>(p, last, e->stream); break;
            case 3: lar_launch_sweep<3>(p, last, e->stream); break;
            case 4: lar_launch_sweep<4>(p, last, e->stream); break;
            case 5: lar_launch_sweep<5>(p, last, e->stream); break;
            case 6: lar_launch_sweep<6>(p, last, e->stream); break;
            case 7: lar_launch_sweep<7>(p, last, e->stream); break;
            default: lar_launch_sweep<8>(p, last, e->stream); break;
        }
        if (p.shared) hipLaunchKernelGGL(k_lar_reduce, dim3(1), dim3(256), 0, e->stream, p);
        hipLaunchKernelGGL(k_lar_update, dim3(ggrid), dim3(256), 0, e->stream, p, i);
        if (want_fe) {
            hipLaunchKernelGGL(k_lar_fe, dim3(sgrid), dim3(256), 0, e->stream, p, i);
            hipLaunchKernelGGL(k_lar_fe_total, dim3(1), dim3(256), 0, e->stream, p, i, e->d_fe_total);
        }
    }
    if (want_fe)
        HIPCHK(e, hipMemcpyAsync(e->d_fe_chain, e->la.d_fe_series + (size_t)(iterations - 1) * C, sizeof(double) * C, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per series and iteration: per step the AR node's messages toward x[t], x[t-1], θ and γ and the observation
    // message; products and marginals at the T + 1 states and the two parameters
    const uint64_t Cs = (uint64_t)C, T = (uint64_t)e->T, I = (uint64_t)iterations;
    e->rule_calls = I * Cs * (5 * T + 1);
    e->products = I * Cs * (4 * T + 2);
    e->marginals = I * Cs * (T + 3);
    return RXHIP_OK;
}

// the binomial regression's kernel arguments
static BregParams breg_params(const rxhip_engine* e) {
    const int d = e->br.d;
    BregParams p;
    p.N = e->T; p.C = e->n_chains; p.d = d; p.nchunk = e->br.nchunk; p.nchunk_xi = e->br.nchunk_xi; p.want_fe = 0;
    p.X = e->br.d_X; p.neff = e->br.d_neff; p.kappa = e->br.d_kappa; p.cst = e->br.d_cst; p.xi = e->br.d_xi; p.lc = e->br.d_lc;
    p.S = e->br.d_S; p.part = e->br.d_part; p.xi_part = e->br.d_xi_part;
    p.hist_m = e->br.d_hist; p.hist_v = e->br.d_hist + (size_t)e->br.hist_cap * (size_t)e->n_chains * (size_t)d;
    p.fe_prob = e->br.d_fe_prob; p.status = e->d_status;
    return p;
}

extern "C" {

void rxhip_binreg_schedule(int64_t N, int32_t d, int32_t* tile_points, int32_t* chunks) {
    const bool ok = N >= 1 && d >= 1 && d <= breg::kMaxD;
    if (tile_points) *tile_points = ok ? breg::tile_points(d) : 0;
    if (chunks) *chunks = ok ? breg::chunks(N, d) : 0;
}

rxhip_status rxhip_binreg_create(const rxhip_binreg_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds != nullptr, out, EngineKind::Binreg)) return st;
    rxhip_engine* e = *out;
    if (ds->d < 1 || ds->d > breg::kMaxD) return fail(e, RXHIP_ERR_BADARG, "binreg: d must be 1 … %d (got %d)", breg::kMaxD, ds->d);
    if (ds->N < 1) return fail(e, RXHIP_ERR_BADARG, "binreg: N must be at least 1 (got %lld)", (long long)ds->N);
    if (ds->n_problems < 1) return fail(e, RXHIP_ERR_BADARG, "binreg: n_problems must be at least 1 (got %lld)", (long long)ds->n_problems);
    if (!ds->prior_xi || !ds->prior_precision) return fail(e, RXHIP_ERR_BADARG, "binreg: prior_xi and prior_precision are required");
    const int d = ds->d;
    for (int i = 0; i < d; ++i) {
        if (!std::isfinite(ds->prior_xi[i])) return fail(e, RXHIP_ERR_BADARG, "binreg: prior_xi must be finite");
        if (ds->init_mean && !std::isfinite(ds->init_mean[i])) return fail(e, RXHIP_ERR_BADARG, "binreg: init_mean must be finite");
    }
    std::vector<double> w0, v0, vinit, winit;
    double ld_w0 = 0.0, ld = 0.0;
    if (!spd_inverse(d, ds->prior_precision, w0, v0, &ld_w0)) return fail(e, RXHIP_ERR_BADARG, "binreg: prior_precision is not symmetric positive definite");
    if (ds->init_cov) {
        if (!spd_inverse(d, ds->init_cov, vinit, winit, &ld)) return fail(e, RXHIP_ERR_BADARG, "binreg: init_cov is not symmetric positive definite");
    } else
        vinit = v0;   // the prior's own covariance
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    e->br.d = d;
    e->T = ds->N;
    e->n_chains = ds->n_problems;
    e->d = e->dy = e->dpad = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    // constants: ξ0 | W0 | m0 = W0⁻¹ξ0 | ln det W0 | initial m | initial V
    std::vector<double> cst((size_t)breg::nconst(d), 0.0);
    {
        double *xi0 = cst.data(), *W0 = xi0 + d, *m0 = W0 + d * d, *im = m0 + d + 1, *iv = im + d;
        for (int i = 0; i < d; ++i) xi0[i] = ds->prior_xi[i];
        for (int i = 0; i < d * d; ++i) { W0[i] = w0[(size_t)i]; iv[i] = vinit[(size_t)i]; }
        for (int i = 0; i < d; ++i) {
            double s = 0.0;
            for (int j = 0; j < d; ++j) s += v0[(size_t)(i * d + j)] * xi0[j];
            m0[i] = s;
        }
        m0[d] = ld_w0;
        for (int i = 0; i < d; ++i) im[i] = ds->init_mean ? ds->init_mean[i] : m0[i];
    }
    const size_t C = (size_t)ds->n_problems, N = (size_t)ds->N, DP = (size_t)breg::dpad(d);
    e->br.nchunk = breg::chunks(ds->N, d);
    e->br.nchunk_xi = (int)std::min<long long>((ds->N + BREG_XI_ROWS - 1) / BREG_XI_ROWS, 256);
    HIPCHK(e, hipMalloc(&e->br.d_cst, sizeof(double) * cst.size()));
    HIPCHK(e, hipMemcpy(e->br.d_cst, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&e->br.d_X, sizeof(double) * C * N * (size_t)d));
    HIPCHK(e, hipMalloc(&e->br.d_neff, sizeof(double) * C * N));
    HIPCHK(e, hipMalloc(&e->br.d_kappa, sizeof(double) * C * N));
    HIPCHK(e, hipMalloc(&e->br.d_xi, sizeof(double) * C * (size_t)d));
    HIPCHK(e, hipMalloc(&e->br.d_lc, sizeof(double) * C));
    HIPCHK(e, hipMalloc(&e->br.d_S, sizeof(double) * C * DP * DP));
    HIPCHK(e, hipMalloc(&e->br.d_part, sizeof(double) * C * (size_t)e->br.nchunk * (size_t)breg::npart(d)));
    HIPCHK(e, hipMalloc(&e->br.d_xi_part, sizeof(double) * C * (size_t)e->br.nchunk_xi * 32));
    return finish_create(e, C, 32);
}

rxhip_status rxhip_binreg_get_parameters(rxhip_engine* e, double* mean, double* cov, double* free_energy) {
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, e && e->kind == EngineKind::Binreg, "binreg_get_parameters", free_energy != nullptr)) return st;
    const size_t C = (size_t)e->n_chains, d = (size_t)e->br.d, rows = (size_t)e->last_iterations * C;
    const BregParams p = breg_params(e);
    if (mean) HIPCHK(e, hipMemcpy(mean, p.hist_m, sizeof(double) * rows * d, hipMemcpyDeviceToHost));
    if (cov) HIPCHK(e, hipMemcpy(cov, p.hist_v, sizeof(double) * rows * d * d, hipMemcpyDeviceToHost));
    if (free_energy) HIPCHK(e, hipMemcpy(free_energy, p.fe_prob, sizeof(double) * rows, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

}  // extern "C"

// X, y and n_trials of a binomial regression engine, checked on the host before anything reaches the device: ±Inf anywhere (NaN too, except in y,
// where it means missing), n_i < 0, an observed y_i outside 0 … n_i.  A refused array counts as not set.
static rxhip_status binreg_set_data(rxhip_engine* e, int32_t var_id, const double* host, size_t n) {
    const size_t C = (size_t)e->n_chains, N = (size_t)e->T, d = (size_t)e->br.d;
    auto& b = e->br;
    if (var_id != RXHIP_VAR_Y && var_id != RXHIP_VAR_REGRESSORS && var_id != RXHIP_VAR_TRIALS)
        return fail(e, RXHIP_ERR_BADARG, "set_data: variable %d is not a data variable of the binomial regression engine", var_id);
    const size_t need = var_id == RXHIP_VAR_REGRESSORS ? C * N * d : C * N;
    if (!host || n != need) return fail(e, RXHIP_ERR_BADARG, "set_data: expected %zu doubles, got %zu", need, n);
    b.ready = false;
    if (var_id == RXHIP_VAR_REGRESSORS) {
        b.have_X = false;
        for (size_t i = 0; i < need; ++i)
            if (!std::isfinite(host[i])) return fail(e, RXHIP_ERR_BADARG, "set_data: regressor %zu is not finite (%g)", i, host[i]);
        SET_DEVICE(e);
        HIPCHK(e, hipMemcpyAsync(b.d_X, host, sizeof(double) * need, hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        b.have_X = true;
        return RXHIP_OK;
    }
    bool& have = var_id == RXHIP_VAR_Y ? b.have_y : b.have_n;
    std::vector<double>& keep = var_id == RXHIP_VAR_Y ? b.h_y : b.h_n;
    have = false;
    for (size_t i = 0; i < need; ++i) {
        const double v = host[i];
        if (var_id == RXHIP_VAR_Y ? std::isinf(v) : !std::isfinite(v)) return fail(e, RXHIP_ERR_BADARG, "set_data: %s %zu is not finite (%g)", var_id == RXHIP_VAR_Y ? "observation" : "n_trials", i, v);
        if (var_id == RXHIP_VAR_TRIALS && v < 0.0) return fail(e, RXHIP_ERR_BADARG, "set_data: n_trials %zu is negative (%g)", i, v);
    }
    keep.assign(host, host + need);
    have = true;
    if (b.have_y && b.have_n)
        for (size_t i = 0; i < need; ++i) {
            const double y = b.h_y[i];
            if (y == y && !(y >= 0.0 && y <= b.h_n[i])) {
                have = false;
                return fail(e, RXHIP_ERR_BADARG, "set_data: observation %zu = %g lies outside 0 … n_trials = %g", i, y, b.h_n[i]);
            }
        }
    return RXHIP_OK;
}

// once per data set: n_eff, κ, lc from the host copies of y and n_trials; ξ on the device
static rxhip_status breg_prepare(rxhip_engine* e) {
    const size_t C = (size_t)e->n_chains, N = (size_t)e->T;
    auto& b = e->br;
    std::vector<double> neff(C * N), kappa(C * N), lc(C);
    for (size_t c = 0; c < C; ++c) {
        double s = 0.0;
        for (size_t i = 0; i < N; ++i) {
            const double y = b.h_y[c * N + i], n = b.h_n[c * N + i];
            const bool seen = y == y;
            neff[c * N + i] = seen ? n : 0.0;
            kappa[c * N + i] = seen ? y - 0.5 * n : 0.0;
            if (seen) s += std::lgamma(n + 1.0) - std::lgamma(y + 1.0) - std::lgamma(n - y + 1.0);
        }
        lc[c] = s;
    }
    HIPCHK(e, hipMemcpyAsync(b.d_neff, neff.data(), sizeof(double) * C * N, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(b.d_kappa, kappa.data(), sizeof(double) * C * N, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(b.d_lc, lc.data(), sizeof(double) * C, hipMemcpyHostToDevice, e->stream));
    const BregParams p = breg_params(e);
    hipLaunchKernelGGL(k_breg_xi, dim3((unsigned)p.nchunk_xi, (unsigned)C), dim3(256), 0, e->stream, p);
    hipLaunchKernelGGL(k_breg_xi_total, dim3((unsigned)((C * (size_t)p.d + 255) / 256)), dim3(256), 0, e->stream, p);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));   // the host images go out of scope
    b.ready = true;
    return RXHIP_OK;
}

static rxhip_status binreg_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations, false)) return st;   // (its three arrays, not have_data: below)
    auto& b = e->br;
    if (!b.have_X || !b.have_y || !b.have_n)
        return fail(e, RXHIP_ERR_STATE, "run: the binomial regression engine needs RXHIP_VAR_REGRESSORS, RXHIP_VAR_Y and RXHIP_VAR_TRIALS (missing:%s%s%s)",
                    b.have_X ? "" : " regressors", b.have_y ? "" : " y", b.have_n ? "" : " n_trials");
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains, d = (size_t)b.d;
    if (C > 65535) return fail(e, RXHIP_ERR_BADARG, "binreg: at most 65535 problems per engine (got %zu)", C);
    if (!b.ready)
        if (rxhip_status st = breg_prepare(e)) return st;
    rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}});
    // the parameter history and the per-problem free energies: every iteration of the run
    if (!rs) rs = reserve(e, &b.hist_cap, iterations, {{&b.d_hist, C * (d + d * d)}, {&b.d_fe_prob, C}});
    if (rs) return rs;
    BregParams p = breg_params(e);
    p.want_fe = want_fe ? 1 : 0;
    const dim3 pgrid((unsigned)p.nchunk, (unsigned)C);
    hipLaunchKernelGGL(k_breg_init, dim3((unsigned)C), dim3(64), 0, e->stream, p);   // every run starts from the initial q(β)
    for (int i = 0; i < iterations; ++i) {
        switch (p.d) {
            case 1: hipLaunchKernelGGL(k_breg_pass_small<1>, pgrid, dim3(256), 0, e->stream, p); break;
            case 2: hipLaunchKernelGGL(k_breg_pass_small<2>, pgrid, dim3(256), 0, e->stream, p); break;
            case 3: hipLaunchKernelGGL(k_breg_pass_small<3>, pgrid, dim3(256), 0, e->stream, p); break;
            case 4: hipLaunchKernelGGL(k_breg_pass_small<4>, pgrid, dim3(256), 0, e->stream, p); break;
            default:
                if (p.d <= 16) hipLaunchKernelGGL(k_breg_pass<1>, pgrid, dim3(256), 0, e->stream, p);
                else hipLaunchKernelGGL(k_breg_pass<2>, pgrid, dim3(256), 0, e->stream, p);
        }
        hipLaunchKernelGGL(k_breg_update, dim3((unsigned)C), dim3(64), 0, e->stream, p, i);
        if (want_fe) hipLaunchKernelGGL(k_breg_fe_total, dim3(1), dim3(256), 0, e->stream, p, i, e->d_fe_total);
    }
    if (want_fe)
        HIPCHK(e, hipMemcpyAsync(e->d_fe_chain, b.d_fe_prob + (size_t)(iterations - 1) * C, sizeof(double) * C, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per problem and iteration: per point the BinomialPolya node's message toward β and its ω marginal; the prior's
    // message; products of the N + 1 messages at β
    const uint64_t Cs = (uint64_t)C, N = (uint64_t)e->T, I = (uint64_t)iterations;
    e->rule_calls = I * Cs * (N + 1);
    e->products = I * Cs * N;
    e->marginals = I * Cs * (N + 1);
    return RXHIP_OK;
}

// ---- regression / autoregression with unknown coefficients and noise precision (arreg_kernels.hpp) ----
static bool is_arreg(const rxhip_engine* e) { return e->kind == EngineKind::Arreg || e->kind == EngineKind::ArregLagged; }

static ArregParams arreg_params(const rxhip_engine* e) {
    const auto& a = e->ar;
    ArregParams p;
    p.N = a.rows; p.T = e->T; p.C = e->n_chains;
    p.d = a.d; p.nchunk = a.nchunk; p.shared = a.shared; p.want_fe = 0; p.iterations = 0;
    p.X = a.d_X; p.y = a.lagged ? e->d_y : a.d_yreg;
    p.cst = a.d_cst; p.part = a.d_part; p.hist = a.d_hist; p.fe = a.d_fe; p.fe_total = e->d_fe_total; p.fe_chain = e->d_fe_chain;
    p.status = e->d_status;
    return p;
}

extern "C" {

void rxhip_arreg_schedule(int64_t n_rows, int32_t d, int32_t* tile_rows, int32_t* chunks) {
    const bool ok = n_rows >= 0 && d >= 1 && d <= arreg::kMaxD;
    if (tile_rows) *tile_rows = ok ? arreg::tile_rows(d) : 0;
    if (chunks) *chunks = ok ? arreg::chunks(n_rows, d) : 0;
}

rxhip_status rxhip_arreg_create(const rxhip_arreg_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds != nullptr, out, EngineKind::Arreg)) return st;
    rxhip_engine* e = *out;
    if (ds->lagged) e->kind = EngineKind::ArregLagged;
    if (ds->d < 1 || ds->d > arreg::kMaxD) return fail(e, RXHIP_ERR_BADARG, "arreg: d must be 1 … %d (got %d)", arreg::kMaxD, ds->d);
    if (ds->N < 1) return fail(e, RXHIP_ERR_BADARG, "arreg: N must be at least 1 (got %lld)", (long long)ds->N);
    if (ds->n_series < 1) return fail(e, RXHIP_ERR_BADARG, "arreg: n_series must be at least 1 (got %lld)", (long long)ds->n_series);
    if (ds->n_series > 65535) return fail(e, RXHIP_ERR_BADARG, "arreg: at most 65535 series per engine (got %lld)", (long long)ds->n_series);
    auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!positive(ds->prior_gamma_shape) || !positive(ds->prior_gamma_rate))
        return fail(e, RXHIP_ERR_BADARG, "arreg: prior_gamma shape and rate must be positive and finite (got %g, %g)", ds->prior_gamma_shape, ds->prior_gamma_rate);
    const double ia = ds->init_gamma_shape ? *ds->init_gamma_shape : ds->prior_gamma_shape, ib = ds->init_gamma_rate ? *ds->init_gamma_rate : ds->prior_gamma_rate;
    if (!positive(ia) || !positive(ib)) return fail(e, RXHIP_ERR_BADARG, "arreg: init_gamma shape and rate must be positive and finite (got %g, %g)", ia, ib);
    if (!ds->prior_theta_mean || !ds->prior_theta_precision) return fail(e, RXHIP_ERR_BADARG, "arreg: prior_theta_mean and prior_theta_precision are required");
    const int d = ds->d;
    for (int i = 0; i < d; ++i)
        if (!std::isfinite(ds->prior_theta_mean[i])) return fail(e, RXHIP_ERR_BADARG, "arreg: prior_theta_mean must be finite");
    std::vector<double> l0, v0;
    double ld_l0 = 0.0;
    if (!spd_inverse(d, ds->prior_theta_precision, l0, v0, &ld_l0)) return fail(e, RXHIP_ERR_BADARG, "arreg: prior_theta_precision is not symmetric positive definite");
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    auto& a = e->ar;
    a.d = d; a.lagged = ds->lagged ? 1 : 0; a.shared = ds->share_parameters ? 1 : 0;
    a.rows = a.lagged ? arreg::lag_rows(ds->N, d) : ds->N;
    a.nchunk = arreg::chunks(a.rows, d);
    e->T = ds->N;
    e->n_chains = ds->n_series;
    e->d = e->dy = e->dpad = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    // constants: Λ0 | m0 | Λ0 m0 | a0, b0, initial a, initial b, ln det Λ0, lnΓ(a0), ln b0
    std::vector<double> cst((size_t)arreg::nconst(d), 0.0);
    {
        double *L0 = cst.data(), *m0 = L0 + d * d, *wm0 = m0 + d, *sc = wm0 + d;
        for (int i = 0; i < d * d; ++i) L0[i] = l0[(size_t)i];
        for (int i = 0; i < d; ++i) m0[i] = ds->prior_theta_mean[i];
        for (int i = 0; i < d; ++i) {
            double s = 0.0;
            for (int j = 0; j < d; ++j) s += L0[i * d + j] * m0[j];
            wm0[i] = s;
        }
        sc[0] = ds->prior_gamma_shape; sc[1] = ds->prior_gamma_rate; sc[2] = ia; sc[3] = ib; sc[4] = ld_l0;
        sc[5] = std::lgamma(ds->prior_gamma_shape); sc[6] = std::log(ds->prior_gamma_rate);
    }
    const size_t C = (size_t)ds->n_series, N = (size_t)ds->N;
    HIPCHK(e, hipMalloc(&a.d_cst, sizeof(double) * cst.size()));
    HIPCHK(e, hipMemcpy(a.d_cst, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice));
    if (!a.lagged) {
        HIPCHK(e, hipMalloc(&a.d_X, sizeof(double) * C * N * (size_t)d));
        HIPCHK(e, hipMalloc(&a.d_yreg, sizeof(double) * C * N));
    }
    HIPCHK(e, hipMalloc(&a.d_part, sizeof(double) * C * (size_t)a.nchunk * (size_t)arreg::nstat(d)));
    return finish_create(e, C, 32);
}

}  // extern "C"

// regressor mode: X and y, checked on the host before anything reaches the device (NaN or ±Inf in X, ±Inf in y); a refused array counts as not set
static rxhip_status arreg_set_data(rxhip_engine* e, int32_t var_id, const double* host, size_t n) {
    const size_t C = (size_t)e->n_chains, N = (size_t)e->T, d = (size_t)e->ar.d;
    auto& a = e->ar;
    if (var_id != RXHIP_VAR_Y && var_id != RXHIP_VAR_REGRESSORS)
        return fail(e, RXHIP_ERR_BADARG, "set_data: variable %d is not a data variable of the regression engine", var_id);
    const bool isX = var_id == RXHIP_VAR_REGRESSORS;
    const size_t need = isX ? C * N * d : C * N;
    if (!host || n != need) return fail(e, RXHIP_ERR_BADARG, "set_data: expected %zu doubles, got %zu", need, n);
    a.stats_ready = false;
    bool& have = isX ? a.have_X : a.have_y;
    have = false;
    for (size_t i = 0; i < need; ++i) {
        const double v = host[i];
        if (isX ? !std::isfinite(v) : std::isinf(v))
            return fail(e, RXHIP_ERR_BADARG, isX ? "set_data: regressor %zu is not finite (%g)" : "set_data: observation %zu is infinite (%g; finite values and NaN = a dropped row are accepted)", i, v);
    }
    SET_DEVICE(e);
    HIPCHK(e, hipMemcpyAsync(isX ? a.d_X : a.d_yreg, host, sizeof(double) * need, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    have = true;
    return RXHIP_OK;
}

// lagged mode: the series arrived through the common ingest (host or device): finite or NaN, checked on the device copy; new data, new statistics
static rxhip_status arreg_check_data(rxhip_engine* e) {
    e->ar.stats_ready = false;
    return check_observations(e, [](rxhip_engine* e, long long n, unsigned nb) {
        hipLaunchKernelGGL(k_lar_check_y, dim3(nb), dim3(256), 0, e->stream, (const double*)e->d_y, n, e->d_status);
    }, ST_LAR_BAD_Y, "set_data: an observation is infinite (finite values and NaN = missing are accepted)");
}

template <bool LAG>
static void arreg_launch_pass(const ArregParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.nchunk, (unsigned)p.C);
    switch (p.d) {
        case 1: hipLaunchKernelGGL((k_arreg_pass_small<1, LAG>), grid, dim3(256), 0, stream, p); break;
        case 2: hipLaunchKernelGGL((k_arreg_pass_small<2, LAG>), grid, dim3(256), 0, stream, p); break;
        case 3: hipLaunchKernelGGL((k_arreg_pass_small<3, LAG>), grid, dim3(256), 0, stream, p); break;
        case 4: hipLaunchKernelGGL((k_arreg_pass_small<4, LAG>), grid, dim3(256), 0, stream, p); break;
        default:
            if (p.d <= 16) hipLaunchKernelGGL((k_arreg_pass<1, LAG>), grid, dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((k_arreg_pass<2, LAG>), grid, dim3(256), 0, stream, p);
    }
}

// "run: …" refusals of an engine without its data; then the statistics pass, once per data set
static rxhip_status arreg_statistics(rxhip_engine* e, const char* who) {
    auto& a = e->ar;
    if (a.lagged ? !e->have_data : !(a.have_X && a.have_y)) {
        if (a.lagged) return fail(e, RXHIP_ERR_STATE, "%s: no observations (call rxhip_set_data first)", who);
        return fail(e, RXHIP_ERR_STATE, "%s: the regression engine needs RXHIP_VAR_REGRESSORS and RXHIP_VAR_Y (missing:%s%s)", who, a.have_X ? "" : " regressors",
                    a.have_y ? "" : " y");
    }
    if (a.stats_ready) return RXHIP_OK;
    const ArregParams p = arreg_params(e);
    if (a.lagged) arreg_launch_pass<true>(p, e->stream);
    else arreg_launch_pass<false>(p, e->stream);
    HIPCHK(e, hipGetLastError());
    a.stats_ready = true;
    return RXHIP_OK;
}

static rxhip_status arreg_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations, false)) return st;   // (its own data flags: arreg_statistics)
    SET_DEVICE(e);
    auto& a = e->ar;
    if (rxhip_status st = arreg_statistics(e, "run")) return st;
    const size_t C = (size_t)e->n_chains, G = a.shared ? 1 : C;
    rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}});
    // the parameter history and the per-group free energies: every iteration of the run
    if (!rs) rs = reserve(e, &a.hist_cap, iterations, {{&a.d_hist, G * (size_t)arreg::nhist(a.d)}, {&a.d_fe, G}});
    if (rs) return rs;
    ArregParams p = arreg_params(e);
    p.want_fe = want_fe ? 1 : 0;
    p.iterations = iterations;
    hipLaunchKernelGGL(k_arreg_iterate, dim3((unsigned)G), dim3(64), 0, e->stream, p);   // every run starts from the initial q(γ); ONE launch for all iterations
    if (want_fe && G > 1) hipLaunchKernelGGL(k_arreg_fe_total, dim3((unsigned)iterations), dim3(256), 0, e->stream, p);
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per series and iteration: per row the Normal node's messages toward θ and γ; the two priors' messages; products of
    // the N + 1 messages at θ and at γ; the two marginals
    const uint64_t Cs = (uint64_t)C, N = (uint64_t)a.rows, I = (uint64_t)iterations;
    e->rule_calls = I * Cs * (2 * N + 2);
    e->products = I * Cs * 2 * N;
    e->marginals = I * Cs * 2;
    return RXHIP_OK;
}

extern "C" {

rxhip_status rxhip_arreg_get_parameters(rxhip_engine* e, double* theta_mean, double* theta_cov, double* gamma_shape, double* gamma_rate, double* free_energy) {
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, e && is_arreg(e), "arreg_get_parameters", free_energy != nullptr)) return st;
    const size_t C = (size_t)e->n_chains, d = (size_t)e->ar.d, G = e->ar.shared ? 1 : C, NH = (size_t)arreg::nhist((int)d), rows = (size_t)e->last_iterations * G;
    std::vector<double> tmp(rows * NH);
    HIPCHK(e, hipMemcpy(tmp.data(), e->ar.d_hist, sizeof(double) * tmp.size(), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
        const double* q = &tmp[r * NH];
        if (theta_mean) std::memcpy(theta_mean + r * d, q, sizeof(double) * d);
        if (theta_cov) std::memcpy(theta_cov + r * d * d, q + d, sizeof(double) * d * d);
        if (gamma_shape) gamma_shape[r] = q[d + d * d];
        if (gamma_rate) gamma_rate[r] = q[d + d * d + 1];
    }
    if (free_energy) HIPCHK(e, hipMemcpy(free_energy, e->ar.d_fe, sizeof(double) * rows, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

rxhip_status rxhip_arreg_get_statistics(rxhip_engine* e, double* Gout, double* hout, double* sout, double* nout) {
    if (!e || !is_arreg(e)) return RXHIP_ERR_BADARG;
    SET_DEVICE(e);
    if (rxhip_status st = arreg_statistics(e, "arreg_get_statistics")) return st;
    const size_t C = (size_t)e->n_chains, d = (size_t)e->ar.d, NS = (size_t)arreg::nstat((int)d), NG = (size_t)arreg::ngram((int)d), nchunk = (size_t)e->ar.nchunk;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    std::vector<double> part(C * nchunk * NS), tot(NS);
    HIPCHK(e, hipMemcpy(part.data(), e->ar.d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < C; ++s) {
        sum_chunk_partials(&part[s * nchunk * NS], nchunk, NS, tot.data());   // as k_arreg_iterate adds them
        for (size_t i = 0; i < d; ++i) {
            if (Gout)
                for (size_t j = 0; j < d; ++j) {
                    const size_t lo = std::max(i, j), hi = std::min(i, j);
                    Gout[(s * d + i) * d + j] = tot[lo * (lo + 1) / 2 + hi];
                }
            if (hout) hout[s * d + i] = tot[NG + i];
        }
        if (sout) sout[s] = tot[NG + d];
        if (nout) nout[s] = tot[NG + d + 1];
    }
    return RXHIP_OK;
}

}  // extern "C"

// ---- multinomial regression, stick-breaking Pólya-Gamma VMP from the column sums (mnreg_kernels.hpp): two rows, offline and online ----
static bool is_mnreg(const rxhip_engine* e) { return e->kind == EngineKind::Mnreg || e->kind == EngineKind::MnregOnline; }

static MnregParams mnreg_params(const rxhip_engine* e) {
    const auto& m = e->mn;
    const size_t C = (size_t)e->n_chains, T = (size_t)e->T, d = (size_t)m.d;
    MnregParams p;
    p.N = e->T; p.C = e->n_chains; p.K = m.K; p.d = m.d; p.nchunk = m.nchunk; p.want_fe = 0; p.iterations = 0; p.keep_cov = m.keep_cov;
    p.data = m.d_data; p.cst = m.d_cst; p.part = m.d_part;
    if (m.online) {
        p.hist_m = m.d_on; p.hist_v = m.d_on + T * C * d; p.fe = m.d_on + 2 * T * C * d; p.last = m.d_on + 2 * T * C * d + T * C;
    } else {
        p.hist_m = m.d_hist; p.hist_v = m.d_hist + (size_t)m.hist_cap * C * d; p.fe = m.d_fe; p.last = nullptr;
    }
    p.hist_cov = m.d_oncov; p.fe_it = m.d_feit;
    p.fe_total = e->d_fe_total; p.fe_chain = e->d_fe_chain; p.status = e->d_status;
    return p;
}

extern "C" {

void rxhip_mnreg_schedule(int64_t N, int32_t K, int32_t* tile_rows, int32_t* chunks) {
    const bool ok = N >= 1 && K >= mnreg::kMinK && K <= mnreg::kMaxK;
    if (tile_rows) *tile_rows = ok ? mnreg::tile_rows(K) : 0;
    if (chunks) *chunks = ok ? mnreg::chunks(N, K) : 0;
}

rxhip_status rxhip_mnreg_create(const rxhip_mnreg_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds != nullptr, out, EngineKind::Mnreg)) return st;
    rxhip_engine* e = *out;
    if (ds->mode == RXHIP_MNREG_ONLINE) e->kind = EngineKind::MnregOnline;
    if (ds->mode != RXHIP_MNREG_BATCH && ds->mode != RXHIP_MNREG_ONLINE) return fail(e, RXHIP_ERR_BADARG, "mnreg: mode must be RXHIP_MNREG_BATCH or RXHIP_MNREG_ONLINE (got %d)", ds->mode);
    if (ds->K < mnreg::kMinK || ds->K > mnreg::kMaxK) return fail(e, RXHIP_ERR_BADARG, "mnreg: K must be %d … %d (got %d)", mnreg::kMinK, mnreg::kMaxK, ds->K);
    if (ds->N < 1) return fail(e, RXHIP_ERR_BADARG, "mnreg: N must be at least 1 (got %lld)", (long long)ds->N);
    if (ds->n_problems < 1 || ds->n_problems > 65535) return fail(e, RXHIP_ERR_BADARG, "mnreg: n_problems must be 1 … 65535 (got %lld)", (long long)ds->n_problems);
    if (ds->n_trials < 0 || ds->n_trials > (1LL << 31)) return fail(e, RXHIP_ERR_BADARG, "mnreg: n_trials must be 0 (not checked) … 2^31 (got %lld)", (long long)ds->n_trials);
    if (!ds->prior_xi || !ds->prior_precision) return fail(e, RXHIP_ERR_BADARG, "mnreg: prior_xi and prior_precision are required");
    const int K = ds->K, d = K - 1;
    for (int i = 0; i < d; ++i) {
        if (!std::isfinite(ds->prior_xi[i])) return fail(e, RXHIP_ERR_BADARG, "mnreg: prior_xi must be finite");
        if (ds->init_mean && !std::isfinite(ds->init_mean[i])) return fail(e, RXHIP_ERR_BADARG, "mnreg: init_mean must be finite");
    }
    std::vector<double> w0, v0, vinit, winit;
    double ld_w0 = 0.0, ld = 0.0;
    if (!spd_inverse(d, ds->prior_precision, w0, v0, &ld_w0)) return fail(e, RXHIP_ERR_BADARG, "mnreg: prior_precision is not symmetric positive definite");
    if (ds->init_cov) {
        if (!spd_inverse(d, ds->init_cov, vinit, winit, &ld)) return fail(e, RXHIP_ERR_BADARG, "mnreg: init_cov is not symmetric positive definite");
    } else
        vinit = v0;   // the prior's own covariance
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    auto& m = e->mn;
    m.K = K; m.d = d; m.online = ds->mode == RXHIP_MNREG_ONLINE; m.keep_cov = m.online && ds->keep_cov_history ? 1 : 0; m.n_trials = ds->n_trials;
    m.nchunk = mnreg::chunks(ds->N, K);
    e->T = ds->N;
    e->n_chains = ds->n_problems;
    e->d = e->dy = e->dpad = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    // constants: ξ0 | W0 | m0 = W0⁻¹ξ0 | ln det W0 | initial m | initial V
    std::vector<double> cst((size_t)mnreg::nconst(d), 0.0);
    {
        double *xi0 = cst.data(), *W0 = xi0 + d, *m0 = W0 + d * d, *im = m0 + d + 1, *iv = im + d;
        for (int i = 0; i < d; ++i) xi0[i] = ds->prior_xi[i];
        for (int i = 0; i < d * d; ++i) { W0[i] = w0[(size_t)i]; iv[i] = vinit[(size_t)i]; }
        for (int i = 0; i < d; ++i) {
            double s = 0.0;
            for (int j = 0; j < d; ++j) s += v0[(size_t)(i * d + j)] * xi0[j];
            m0[i] = s;
        }
        m0[d] = ld_w0;
        for (int i = 0; i < d; ++i) im[i] = ds->init_mean ? ds->init_mean[i] : m0[i];
    }
    const size_t C = (size_t)ds->n_problems, N = (size_t)ds->N, D = (size_t)d;
    HIPCHK(e, hipMalloc(&m.d_cst, sizeof(double) * cst.size()));
    HIPCHK(e, hipMemcpy(m.d_cst, cst.data(), sizeof(double) * cst.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&m.d_data, sizeof(double) * C * N * (size_t)K));
    if (m.online) {
        HIPCHK(e, hipMalloc(&m.d_on, sizeof(double) * (2 * N * C * D + N * C + C * (D + D * D))));
        if (m.keep_cov) HIPCHK(e, hipMalloc(&m.d_oncov, sizeof(double) * N * C * D * D));
    } else
        HIPCHK(e, hipMalloc(&m.d_part, sizeof(double) * C * (size_t)m.nchunk * (size_t)mnreg::npart(K)));
    return finish_create(e, C, 32);
}

}  // extern "C"

// the counts, checked on the host before anything reaches the device: ±Inf, a negative or non-integer count, a row sum above 2³¹ or different from the
// descriptor's n_trials; a row with any NaN is missing.  A refused array counts as not set.
static rxhip_status mnreg_set_data(rxhip_engine* e, int32_t var_id, const double* host, size_t n) {
    auto& m = e->mn;
    const size_t C = (size_t)e->n_chains, N = (size_t)e->T, K = (size_t)m.K, need = C * N * K;
    if (var_id != RXHIP_VAR_Y) return fail(e, RXHIP_ERR_BADARG, "set_data: variable %d is not a data variable of the multinomial regression engine (mnreg)", var_id);
    if (!host || n != need) return fail(e, RXHIP_ERR_BADARG, "set_data: mnreg expected %zu doubles, got %zu", need, n);
    m.have = false;
    m.stats_ready = false;
    for (size_t r = 0; r < C * N; ++r) {
        const double* y = host + r * K;
        bool missing = false;
        double sum = 0.0;
        for (size_t k = 0; k < K; ++k) {
            const double v = y[k];
            if (v != v) { missing = true; continue; }
            if (std::isinf(v)) return fail(e, RXHIP_ERR_BADARG, "set_data: mnreg count %zu of row %zu is infinite", k, r);
            if (v < 0.0 || v != std::floor(v)) return fail(e, RXHIP_ERR_BADARG, "set_data: mnreg count %zu of row %zu is not a non-negative integer (%g)", k, r, v);
            sum += v;
        }
        if (missing) continue;
        if (sum > 2147483648.0) return fail(e, RXHIP_ERR_BADARG, "set_data: mnreg row %zu sums to %g, above 2^31", r, sum);
        if (m.n_trials > 0 && sum != (double)m.n_trials)
            return fail(e, RXHIP_ERR_BADARG, "set_data: mnreg row %zu sums to %g, the descriptor's n_trials is %lld", r, sum, (long long)m.n_trials);
    }
    SET_DEVICE(e);
    HIPCHK(e, hipMemcpyAsync(m.d_data, host, sizeof(double) * need, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    m.have = true;
    return RXHIP_OK;
}

// the refusal of an engine without its data; then (offline) the statistics pass, once per data set
static rxhip_status mnreg_statistics(rxhip_engine* e, const char* who) {
    auto& m = e->mn;
    if (!m.have) return fail(e, RXHIP_ERR_STATE, "%s: no observations (the multinomial regression engine, mnreg, takes its counts through rxhip_set_data with RXHIP_VAR_Y)", who);
    if (m.online || m.stats_ready) return RXHIP_OK;
    const MnregParams p = mnreg_params(e);
    rxhip_status st;
    if ((st = prof_begin(e, RXHIP_K_GMM_PASS))) return st;
    hipLaunchKernelGGL(k_mnreg_stats, dim3((unsigned)p.nchunk, (unsigned)p.C), dim3(256), 0, e->stream, p);
    if ((st = prof_end(e))) return st;
    HIPCHK(e, hipGetLastError());
    m.stats_ready = true;
    ++m.stats_launches;
    return RXHIP_OK;
}

static rxhip_status mnreg_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations, false)) return st;   // (its own data flag: mnreg_statistics)
    SET_DEVICE(e);
    auto& m = e->mn;
    if (rxhip_status st = mnreg_statistics(e, "run")) return st;
    const size_t C = (size_t)e->n_chains, d = (size_t)m.d;
    rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}});
    if (!rs) {
        if (m.online) rs = reserve(e, &m.hist_cap, iterations, {{&m.d_feit, C}});
        else rs = reserve(e, &m.hist_cap, iterations, {{&m.d_hist, C * (d + d * d)}, {&m.d_fe, C}});
    }
    if (rs) return rs;
    MnregParams p = mnreg_params(e);
    p.want_fe = want_fe ? 1 : 0;
    p.iterations = iterations;
    const bool big = m.d > mnreg::kSmallMaxD;
    rxhip_status st;
    if ((st = prof_begin(e, RXHIP_K_GMM_UPDATE))) return st;
    if (m.online) {   // ONE launch for all T steps of every series
        if (big) hipLaunchKernelGGL(k_mnreg_online<true>, dim3((unsigned)C), dim3(64), 0, e->stream, p);
        else hipLaunchKernelGGL(k_mnreg_online<false>, dim3((unsigned)C), dim3(64), 0, e->stream, p);
    } else {          // every run starts from the initial q(ψ); ONE launch for all iterations
        if (big) hipLaunchKernelGGL(k_mnreg_iterate<true>, dim3((unsigned)C), dim3(64), 0, e->stream, p);
        else hipLaunchKernelGGL(k_mnreg_iterate<false>, dim3((unsigned)C), dim3(64), 0, e->stream, p);
    }
    if ((st = prof_end(e))) return st;
    if (want_fe && C > 1) hipLaunchKernelGGL(k_mnreg_fe_total, dim3((unsigned)iterations), dim3(256), 0, e->stream, p, (const double*)(m.online ? p.fe_it : p.fe));
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per problem and iteration (per step online): per row the MultinomialPolya node's message toward ψ and its ω marginals;
    // the prior's message; the products at ψ
    const uint64_t Cs = (uint64_t)C, N = (uint64_t)e->T, I = (uint64_t)iterations;
    e->rule_calls = I * Cs * (m.online ? 2 * N : N + 1);
    e->products = I * Cs * N;
    e->marginals = I * Cs * (m.online ? 2 * N : N + 1);
    return RXHIP_OK;
}

extern "C" {

rxhip_status rxhip_mnreg_get_parameters(rxhip_engine* e, double* mean, double* cov, double* free_energy) {
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, e && is_mnreg(e), "mnreg_get_parameters", free_energy != nullptr)) return st;
    const size_t C = (size_t)e->n_chains, d = (size_t)e->mn.d, T = (size_t)e->T;
    const MnregParams p = mnreg_params(e);
    if (e->mn.online) {   // the last step: mean [series][d], cov [series][d][d], F_T [series]
        std::vector<double> last(C * (d + d * d));
        HIPCHK(e, hipMemcpy(last.data(), p.last, sizeof(double) * last.size(), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < C; ++s) {
            if (mean) std::memcpy(mean + s * d, &last[s * (d + d * d)], sizeof(double) * d);
            if (cov) std::memcpy(cov + s * d * d, &last[s * (d + d * d) + d], sizeof(double) * d * d);
        }
        if (free_energy) HIPCHK(e, hipMemcpy(free_energy, p.fe + (T - 1) * C, sizeof(double) * C, hipMemcpyDeviceToHost));
        return RXHIP_OK;
    }
    const size_t rows = (size_t)e->last_iterations * C;
    if (mean) HIPCHK(e, hipMemcpy(mean, p.hist_m, sizeof(double) * rows * d, hipMemcpyDeviceToHost));
    if (cov) HIPCHK(e, hipMemcpy(cov, p.hist_v, sizeof(double) * rows * d * d, hipMemcpyDeviceToHost));
    if (free_energy) HIPCHK(e, hipMemcpy(free_energy, p.fe, sizeof(double) * rows, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

rxhip_status rxhip_mnreg_get_history(rxhip_engine* e, double* mean, double* var, double* cov, double* free_energy) {
    if (!e || !is_mnreg(e)) return RXHIP_ERR_BADARG;
    if (!e->mn.online) return fail(e, RXHIP_ERR_STATE, "mnreg_get_history: the engine was not created with RXHIP_MNREG_ONLINE");
    if (rxhip_status st = results_ready(e, "mnreg_get_history", false)) return st;
    if (cov && !e->mn.keep_cov) return fail(e, RXHIP_ERR_STATE, "mnreg_get_history: the covariance history was not kept (keep_cov_history)");
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, true, "mnreg_get_history", free_energy != nullptr)) return st;
    const size_t rows = (size_t)e->T * (size_t)e->n_chains, d = (size_t)e->mn.d;
    const MnregParams p = mnreg_params(e);
    if (mean) HIPCHK(e, hipMemcpy(mean, p.hist_m, sizeof(double) * rows * d, hipMemcpyDeviceToHost));
    if (var) HIPCHK(e, hipMemcpy(var, p.hist_v, sizeof(double) * rows * d, hipMemcpyDeviceToHost));
    if (cov) HIPCHK(e, hipMemcpy(cov, p.hist_cov, sizeof(double) * rows * d * d, hipMemcpyDeviceToHost));
    if (free_energy) HIPCHK(e, hipMemcpy(free_energy, p.fe, sizeof(double) * rows, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

rxhip_status rxhip_mnreg_get_statistics(rxhip_engine* e, double* Yout, double* Sout, double* lcout, double* nout) {
    if (!e || !is_mnreg(e)) return RXHIP_ERR_BADARG;
    if (e->mn.online) return fail(e, RXHIP_ERR_STATE, "mnreg_get_statistics: an online engine keeps no statistics of the whole data set");
    SET_DEVICE(e);
    if (rxhip_status st = mnreg_statistics(e, "mnreg_get_statistics")) return st;
    const size_t C = (size_t)e->n_chains, K = (size_t)e->mn.K, NP = (size_t)mnreg::npart((int)K), nchunk = (size_t)e->mn.nchunk;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    std::vector<double> part(C * nchunk * NP), tot(NP), S(K), kap(K);
    HIPCHK(e, hipMemcpy(part.data(), e->mn.d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < C; ++s) {
        sum_chunk_partials(&part[s * nchunk * NP], nchunk, NP, tot.data());   // as k_mnreg_iterate adds them
        mnreg::suffix((int)K, tot.data(), S.data(), kap.data());
        S[K - 1] = tot[K - 1];
        if (Yout) std::memcpy(Yout + s * K, tot.data(), sizeof(double) * K);
        if (Sout) std::memcpy(Sout + s * K, S.data(), sizeof(double) * K);
        if (nout) nout[s] = tot[K];
        if (lcout) lcout[s] = tot[K + 1];
    }
    return RXHIP_OK;
}

}  // extern "C"

// every observation of a hidden Markov model engine is an integer code 0 … M−1 or NaN
static rxhip_status hmm_check_data(rxhip_engine* e) {
    char msg[128];
    snprintf(msg, sizeof msg, "set_data: an observation is neither an integer symbol code 0 … %d nor NaN (missing)", e->hm.M - 1);
    return check_observations(e, [](rxhip_engine* e, long long n, unsigned nb) {
        hipLaunchKernelGGL(k_hmm_check_x, dim3(nb), dim3(256), 0, e->stream, (const double*)e->d_y, n, e->hm.M, e->d_status);
    }, ST_HMM_BAD_X, msg);
}

template <int R>
static void hmm_launch_sweep(const HmmParams& p, bool out, hipStream_t stream) {
    const unsigned spw = 64 / R, grid = (unsigned)((p.n_series + spw - 1) / spw);
    const size_t lds = sizeof(double) * 64 * (size_t)p.M;   // [series in wave][M][R]
    if (out) hipLaunchKernelGGL((k_hmm_sweep<R, true>), dim3(grid), dim3(64), lds, stream, p);
    else hipLaunchKernelGGL((k_hmm_sweep<R, false>), dim3(grid), dim3(64), lds, stream, p);
}

static rxhip_status hmm_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains;
    rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}});
    if (!rs && want_fe) rs = reserve(e, &e->hm.fe_cap, iterations, {{&e->hm.d_fe_series, C}});
    if (rs) return rs;
    const HmmParams p = hmm_params(e);
    const int K = p.K, KM = (K + p.M) * K;
    const long long G = p.shared ? 1 : p.n_series;
    const unsigned cgrid = (unsigned)((G * 2 * K + 255) / 256), sgrid = (unsigned)((C + 255) / 256);
    // every run starts from init_A, init_B: their tables go to half 0 of the log tables; iteration i reads half i % 2 and writes the other
    hipLaunchKernelGGL(k_hmm_tables, dim3(cgrid), dim3(256), 0, e->stream, p, 0);
    for (int i = 0; i < iterations; ++i) {
        const bool last = i == iterations - 1;
        const int cur = (i + 1) & 1;
        if (K <= 2) hmm_launch_sweep<2>(p, last, e->stream);
        else if (K <= 4) hmm_launch_sweep<4>(p, last, e->stream);
        else if (K <= 8) hmm_launch_sweep<8>(p, last, e->stream);
        else hmm_launch_sweep<16>(p, last, e->stream);
        if (p.shared) hipLaunchKernelGGL(k_hmm_reduce, dim3((unsigned)((KM + 255) / 256)), dim3(256), 0, e->stream, p);
        hipLaunchKernelGGL(k_hmm_update, dim3(cgrid), dim3(256), 0, e->stream, p, cur);
        if (want_fe) {
            hipLaunchKernelGGL(k_hmm_fe, dim3(sgrid), dim3(256), 0, e->stream, p, i, cur);
            hipLaunchKernelGGL(k_hmm_fe_total, dim3(1), dim3(256), 0, e->stream, p, i, e->d_fe_total);
        }
    }
    if (want_fe)
        HIPCHK(e, hipMemcpyAsync(e->d_fe_chain, e->hm.d_fe_series + (size_t)(iterations - 1) * C, sizeof(double) * C, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per series and iteration: a forward and a backward transition message and an observation message per step, the
    // messages toward A and B; products and marginals at the T + 1 states and the two matrices
    const uint64_t Cs = (uint64_t)C, T = (uint64_t)e->T, I = (uint64_t)iterations;
    e->rule_calls = I * Cs * (3 * T + 2);
    e->products = I * Cs * 2 * (T + 1);
    e->marginals = I * Cs * (T + 3);
    return RXHIP_OK;
}

// every observation of a probit engine is 0, 1 or NaN
static rxhip_status probit_check_data(rxhip_engine* e) {
    return check_observations(e, [](rxhip_engine* e, long long n, unsigned nb) {
        hipLaunchKernelGGL(k_probit_check_y, dim3(nb), dim3(256), 0, e->stream, (const double*)e->d_y, n, e->d_status);
    }, ST_PROBIT_BAD_Y, "set_data: a Probit observation is neither 0, 1 nor NaN (missing)");
}

static rxhip_status probit_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains, R = (size_t)e->T + 1;
    rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}});
    if (!rs && want_fe) rs = reserve(e, &e->pb.fe_cap, iterations, {{&e->pb.d_fe_series, C}});
    if (rs) return rs;
    const rxhip_probit_desc& d = e->pb.ds;
    ProbitParams p;
    p.T = e->T; p.n_series = e->n_chains; p.y = e->d_y;
    p.xi = e->pb.d_block; p.w = p.xi + R * C; p.pm = p.w + R * C; p.pv = p.pm + R * C;
    p.fe_gauss = p.pv + R * C; p.fe_part = p.fe_gauss + C;
    p.mean = e->d_mean; p.var = e->d_cov; p.fe_series = e->pb.d_fe_series; p.gh = e->pb.d_gh;
    p.a = d.a; p.c = d.c; p.q = d.q; p.m0 = d.m0; p.v0 = d.v0; p.n_gh = d.n_gh; p.status = e->d_status;
    p.echunk = probit_echunk(e->T);
    const long long chunks = (e->T + p.echunk - 1) / p.echunk;
    HIPCHK(e, hipMemsetAsync(p.xi, 0, sizeof(double) * 2 * R * C, e->stream));   // every run starts from empty sites
    const dim3 grid((unsigned)((C + 63) / 64)), egrid((unsigned)((C + 255) / 256), (unsigned)chunks);
    rxhip_status st;
    // sweep i = 0 … iterations − 1 performs update i + 1 and (i ≥ 1) sees the marginals of iteration i; the last sweep only reads
    for (int i = 0; i <= iterations; ++i) {
        const bool update = i < iterations, fe = want_fe && i >= 1;
        if ((st = prof_begin(e, RXHIP_K_PROBIT_SWEEP))) return st;
        if (update && !fe) hipLaunchKernelGGL((k_probit_sweep<true, false, false>), grid, dim3(64), 0, e->stream, p);
        else if (update) hipLaunchKernelGGL((k_probit_sweep<true, true, true>), grid, dim3(64), 0, e->stream, p);
        else if (fe) hipLaunchKernelGGL((k_probit_sweep<false, true, true>), grid, dim3(64), 0, e->stream, p);
        else hipLaunchKernelGGL((k_probit_sweep<false, true, false>), grid, dim3(64), 0, e->stream, p);
        if ((st = prof_end(e))) return st;
        if (fe) {
            hipLaunchKernelGGL(k_probit_energy, egrid, dim3(256), 0, e->stream, p);
            hipLaunchKernelGGL(k_probit_fe, dim3(1), dim3(256), 0, e->stream, p, i - 1, chunks, e->d_fe_total);
        }
    }
    if (want_fe)
        HIPCHK(e, hipMemcpyAsync(e->d_fe_chain, e->pb.d_fe_series + (size_t)(iterations - 1) * C, sizeof(double) * C, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per series and iteration: a forward and a backward transition message per step, a Probit(:in) message per
    // observed step (counted as every step: the mask lives on the device); products and marginals at the T + 1 states
    const uint64_t Cs = (uint64_t)C, T = (uint64_t)e->T, I = (uint64_t)iterations;
    e->rule_calls = I * Cs * (3 * T + 1);
    e->products = I * Cs * 2 * (T + 1);
    e->marginals = I * Cs * (T + 1);
    return RXHIP_OK;
}

static rxhip_status hgf_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    const size_t C = (size_t)e->n_chains, T = (size_t)e->T;
    if (rxhip_status st = reserve(e, &e->h.fe_cap, iterations, {{&e->h.d_fe_series, C}, {&e->h.d_fe_total, 1}})) return st;
    HIPCHK(e, hipMemsetAsync(e->h.d_fe_series, 0, sizeof(double) * (size_t)iterations * C, e->stream));
    HgfParams p;
    p.T = e->T; p.n_series = e->n_chains; p.y = e->d_y;
    p.zm = e->h.d_out; p.zv = e->h.d_out + T * C; p.xm = e->h.d_out + 2 * T * C; p.xv = e->h.d_out + 3 * T * C;
    p.fe_series = e->h.d_fe_series; p.gh = e->h.d_gh;
    const rxhip_hgf_desc& d = e->h.ds;
    p.kappa = d.kappa; p.omega = d.omega; p.z_variance = d.z_variance; p.y_variance = d.y_variance;
    p.z0m = d.z0_mean; p.z0v = d.z0_var; p.x0m = d.x0_mean; p.x0v = d.x0_var;
    p.iters = iterations; p.n_gh = d.n_gh; p.status = e->d_status;
    rxhip_status st;
    if ((st = prof_begin(e, RXHIP_K_HGF_FILTER))) return st;
    const unsigned nb = (unsigned)((C + HGF_SERIES_PER_WAVE - 1) / HGF_SERIES_PER_WAVE);
    if (want_fe) hipLaunchKernelGGL((k_hgf_filter<true>), dim3(nb), dim3(64), 0, e->stream, p);
    else hipLaunchKernelGGL((k_hgf_filter<false>), dim3(nb), dim3(64), 0, e->stream, p);
    if ((st = prof_end(e))) return st;
    if (want_fe) {
        hipLaunchKernelGGL(k_hgf_fe, dim3(iterations), dim3(256), 0, e->stream, p, e->h.d_fe_total);
        HIPCHK(e, hipMemcpyAsync(e->d_fe_chain, e->h.d_fe_series + (size_t)(iterations - 1) * C, sizeof(double) * C,
                                 hipMemcpyDeviceToDevice, e->stream));
    }
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    e->rule_calls = (uint64_t)C * T * (4 + 2 * (uint64_t)iterations);
    e->products = (uint64_t)C * T * 2 * (uint64_t)iterations;
    e->marginals = (uint64_t)C * T * 3 * (uint64_t)iterations;
    return RXHIP_OK;
}

// ---- Gamma mixture with a point-mass shape (gammamix_kernels.hpp): one row ----
static GammaMixParams gammamix_params(const rxhip_engine* e) {
    const auto& g = e->gx;
    GammaMixParams p;
    p.N = e->T; p.C = e->n_chains;
    p.K = g.K; p.nchunk = g.nchunk; p.want_fe = 0; p.iterations = 0; p.iteration = 0; p.write_resp = 0;
    p.y = e->n_chains > 1 ? g.d_yt : e->d_y; p.ly = g.d_ly;
    p.prior = g.d_prior; p.init = g.d_init; p.state = g.d_state; p.part = g.d_part; p.hist = g.d_hist; p.fe = g.d_fe;
    p.fe_total = e->d_fe_total; p.fe_chain = e->d_fe_chain; p.resp = g.d_resp; p.status = e->d_status;
    return p;
}

// what the kernels read beside the ingested array: the problem-major copy of a batch, and ln y for the streamed pass on stored logarithms
static rxhip_status gammamix_prepare(rxhip_engine* e) {
    auto& g = e->gx;
    const size_t n = (size_t)e->T * (size_t)e->n_chains;
    const bool want_yt = e->n_chains > 1, want_ly = g.stored_log != 0;
    if (!want_yt && !want_ly) return RXHIP_OK;
    SET_DEVICE(e);
    if (want_yt && !g.d_yt) HIPCHK(e, hipMalloc(&g.d_yt, sizeof(double) * n));
    if (want_ly && !g.d_ly) HIPCHK(e, hipMalloc(&g.d_ly, sizeof(double) * n));
    hipLaunchKernelGGL(k_gammamix_prepare, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, e->stream, (const double*)e->d_y, (long long)e->T,
                       (long long)e->n_chains, want_yt ? g.d_yt : nullptr, want_ly ? g.d_ly : nullptr);
    HIPCHK(e, hipGetLastError());
    return RXHIP_OK;
}

// the observations arrived through the common ingest (host or device): positive and finite, or NaN = missing; checked on the device copy
static rxhip_status gammamix_check_data(rxhip_engine* e) {
    rxhip_status st = check_observations(e, [](rxhip_engine* e, long long n, unsigned nb) {
        hipLaunchKernelGGL(k_gammamix_check_y, dim3(nb), dim3(256), 0, e->stream, (const double*)e->d_y, n, e->d_status);
    }, ST_GAMMAMIX_BAD_Y, "set_data: gammamix: an observation is zero, negative or infinite (positive finite values and NaN = missing are accepted)");
    return st ? st : gammamix_prepare(e);
}

template <int KT>
static void gammamix_launch_pass(const GammaMixParams& p, bool stored_log, hipStream_t s) {
    const dim3 grid((unsigned)p.nchunk, (unsigned)p.C);
    if (stored_log) hipLaunchKernelGGL((k_gammamix_pass<KT, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_gammamix_pass<KT, false>), grid, dim3(256), 0, s, p);
}
#define GAMMAMIX_BY_KT(KT, CALL)            \
    switch (KT) {                           \
        case 1: CALL(1); break;             \
        case 2: CALL(2); break;             \
        case 4: CALL(4); break;             \
        case 8: CALL(8); break;             \
        default: CALL(16);                  \
    }

static rxhip_status gammamix_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    auto& g = e->gx;
    const size_t C = (size_t)e->n_chains;
    rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}});
    if (!rs) rs = reserve(e, &g.hist_cap, iterations, {{&g.d_hist, C * 4 * (size_t)g.K}, {&g.d_fe, C}});
    if (rs) return rs;
    GammaMixParams p = gammamix_params(e);
    p.want_fe = want_fe ? 1 : 0;
    p.iterations = iterations;
    rxhip_status st;
    {   // every run starts from the initial state (the kernels of iteration 0 read d_init)
        const bool stored = g.stored_log != 0;
        for (int it = 0; it < iterations; ++it) {
            p.iteration = it;
            p.write_resp = g.materialize && it == iterations - 1;
            if ((st = prof_begin(e, RXHIP_K_GMM_PASS))) return st;
#define GX_CALL(KT) gammamix_launch_pass<KT>(p, stored, e->stream)
            GAMMAMIX_BY_KT(g.KT, GX_CALL)
#undef GX_CALL
            if ((st = prof_end(e))) return st;
            if ((st = prof_begin(e, RXHIP_K_GMM_UPDATE))) return st;
            hipLaunchKernelGGL(k_gammamix_update, dim3((unsigned)C), dim3(64), 0, e->stream, p);
            if ((st = prof_end(e))) return st;
        }
    }
    if (want_fe && C > 1) hipLaunchKernelGGL(k_gammamix_fe_total, dim3((unsigned)iterations), dim3(256), 0, e->stream, p);
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0);
    // reference-equivalent events per problem and iteration: per point the GammaMixture node's messages toward z, and toward a[k], b[k] per component;
    // the Categorical's message; per component and for s the product of the N + 1 messages and the marginal; the point's q(z)
    const uint64_t N = (uint64_t)e->T, K = (uint64_t)g.K, I = (uint64_t)iterations;
    e->rule_calls = I * C * (N * (2 + 2 * K) + 2 * K + 1);
    e->products = I * C * (N * (2 * K + 2));
    e->marginals = I * C * (N + 2 * K + 1);
    return RXHIP_OK;
}

extern "C" {

int32_t rxhip_gammamix_schedule(int64_t N, int32_t K) { return gammamix::schedule(N, K); }

rxhip_status rxhip_gammamix_create(const rxhip_gammamix_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds != nullptr, out, EngineKind::GammaMix)) return st;
    rxhip_engine* e = *out;
    constexpr int KS = gammamix::kMaxK;
    if (ds->K < 1 || ds->K > KS) return fail(e, RXHIP_ERR_BADARG, "gammamix: K must be 1 … %d (got %d)", KS, ds->K);
    if (ds->N < 1) return fail(e, RXHIP_ERR_BADARG, "gammamix: N must be at least 1 (got %lld)", (long long)ds->N);
    if (ds->n_problems < 1 || ds->n_problems > 65535)
        return fail(e, RXHIP_ERR_BADARG, "gammamix: n_problems must be 1 … 65535 (got %lld)", (long long)ds->n_problems);
    if (ds->schedule < 0 || ds->schedule > 2) return fail(e, RXHIP_ERR_BADARG, "gammamix: schedule must be 0 (auto) or 1 (streamed) (got %d)", ds->schedule);
    if (ds->schedule == gammamix::SCHED_RESIDENT)
        return fail(e, RXHIP_ERR_BADARG, "gammamix: schedule 2 (resident: a run in one launch) is not part of this build; 0 and 1 run the streamed schedule");
    if (!ds->prior_a_shape || !ds->prior_a_rate || !ds->prior_b_shape || !ds->prior_b_rate || !ds->prior_alpha)
        return fail(e, RXHIP_ERR_BADARG, "gammamix: prior_a_shape, prior_a_rate, prior_b_shape, prior_b_rate and prior_alpha are required ([n_problems][K] each)");
    const int K = ds->K;
    const size_t C = (size_t)ds->n_problems, PK = C * (size_t)K;
    auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
    const struct { const double* p; const char* name; } arrays[] = {
        {ds->prior_a_shape, "prior_a_shape"}, {ds->prior_a_rate, "prior_a_rate"}, {ds->prior_b_shape, "prior_b_shape"}, {ds->prior_b_rate, "prior_b_rate"},
        {ds->prior_alpha, "prior_alpha"}, {ds->init_a, "init_a"}, {ds->init_b_shape, "init_b_shape"}, {ds->init_b_rate, "init_b_rate"}, {ds->init_s_alpha, "init_s_alpha"}};
    for (const auto& a : arrays)
        for (size_t q = 0; a.p && q < PK; ++q)
            if (!positive(a.p[q])) return fail(e, RXHIP_ERR_BADARG, "gammamix: %s must be positive and finite (entry %zu is %g)", a.name, q, a.p[q]);
    for (size_t q = 0; q < PK; ++q)
        if (ds->prior_a_shape[q] < 1.0)
            return fail(e, RXHIP_ERR_BADARG, "gammamix: prior_a_shape must be at least 1 (entry %zu is %g): below it the shape's objective is not concave", q, ds->prior_a_shape[q]);
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    auto& g = e->gx;
    g.K = K; g.KT = gammamix::padded_k(K);
    g.sched = ds->schedule ? ds->schedule : gammamix::schedule(ds->N, K);
    g.nchunk = gammamix::chunks(ds->N);
    g.materialize = ds->materialize_responsibilities ? 1 : 0;
    g.stored_log = 1;   // the measured choice: the streamed pass reads ln y stored at ingest
    e->T = ds->N;
    e->n_chains = ds->n_problems;
    e->d = e->dy = e->dpad = 1;
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    // the prior blocks and the state every run starts from (with the constants of its first pass), rows of kMaxK
    std::vector<double> prior(C * gammamix::kPriorRows * KS, 1.0), init(C * gammamix::kStateRows * KS, 1.0);
    for (size_t c = 0; c < C; ++c) {
        double *pr = &prior[c * gammamix::kPriorRows * KS], *st = &init[c * gammamix::kStateRows * KS];
        double asum = 0.0;
        for (int k = 0; k < K; ++k) {
            const size_t q = c * (size_t)K + (size_t)k;
            pr[k] = ds->prior_a_shape[q]; pr[KS + k] = ds->prior_a_rate[q]; pr[2 * KS + k] = ds->prior_b_shape[q]; pr[3 * KS + k] = ds->prior_b_rate[q];
            pr[4 * KS + k] = ds->prior_alpha[q];
            st[k] = ds->init_a ? ds->init_a[q] : 1.0;
            st[KS + k] = ds->init_b_shape ? ds->init_b_shape[q] : 1.0;
            st[2 * KS + k] = ds->init_b_rate ? ds->init_b_rate[q] : 1.0;
            st[3 * KS + k] = ds->init_s_alpha ? ds->init_s_alpha[q] : ds->prior_alpha[q];
            asum += st[3 * KS + k];
        }
        for (int k = 0; k < KS; ++k) {
            double c0 = -1e300, c1 = 0.0, c2 = 0.0;   // padding components never receive responsibility
            if (k < K) gammamix::pass_constants(st[k], st[KS + k], st[2 * KS + k], digamma_dev(st[3 * KS + k]) - digamma_dev(asum), std::lgamma(st[k]), c0, c1, c2);
            st[4 * KS + k] = c0; st[5 * KS + k] = c1; st[6 * KS + k] = c2;
        }
    }
    const size_t NQ = 3 * (size_t)g.KT + 1;
    HIPCHK(e, hipMalloc(&g.d_prior, sizeof(double) * prior.size()));
    HIPCHK(e, hipMemcpy(g.d_prior, prior.data(), sizeof(double) * prior.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&g.d_init, sizeof(double) * init.size()));
    HIPCHK(e, hipMemcpy(g.d_init, init.data(), sizeof(double) * init.size(), hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&g.d_state, sizeof(double) * init.size()));
    HIPCHK(e, hipMalloc(&g.d_part, sizeof(double) * C * (size_t)g.nchunk * NQ));
    if (g.materialize) HIPCHK(e, hipMalloc(&g.d_resp, sizeof(double) * C * (size_t)ds->N * (size_t)K));
    return finish_create(e, C, 32);
}

rxhip_status rxhip_gammamix_set_stored_log(rxhip_engine* e, int32_t stored) {
    if (!e || e->kind != EngineKind::GammaMix) return RXHIP_ERR_BADARG;
    if (stored != 0 && stored != 1) return fail(e, RXHIP_ERR_BADARG, "gammamix_set_stored_log: 0 (recompute ln y in the pass) or 1 (read it from memory, the default)");
    const bool fill = stored && !e->gx.stored_log && e->have_data;   // switched on with the data in place: ln y is computed now
    e->gx.stored_log = stored;
    return fill ? gammamix_prepare(e) : RXHIP_OK;
}

rxhip_status rxhip_gammamix_get_history(rxhip_engine* e, double* hist, double* free_energy) {
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, e && e->kind == EngineKind::GammaMix, "gammamix_get_history", free_energy != nullptr)) return st;
    const size_t rows = (size_t)e->last_iterations * (size_t)e->n_chains;
    if (hist) HIPCHK(e, hipMemcpy(hist, e->gx.d_hist, sizeof(double) * rows * 4 * (size_t)e->gx.K, hipMemcpyDeviceToHost));
    if (free_energy) HIPCHK(e, hipMemcpy(free_energy, e->gx.d_fe, sizeof(double) * rows, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

rxhip_status rxhip_gammamix_get_responsibilities(rxhip_engine* e, double* resp) {
    if (!e || e->kind != EngineKind::GammaMix || !resp) return RXHIP_ERR_BADARG;
    if (!e->gx.materialize) return fail(e, RXHIP_ERR_STATE, "gammamix_get_responsibilities: the engine was created without materialize_responsibilities");
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, true, "gammamix_get_responsibilities", false)) return st;
    HIPCHK(e, hipMemcpy(resp, e->gx.d_resp, sizeof(double) * (size_t)e->n_chains * (size_t)e->T * (size_t)e->gx.K, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Nonlinear state-space engine (nlssm_kernels.hpp) and the expression programs it runs (expr.hpp)
// the C descriptor of a program as the device's fixed-size block; 0 or a text
static int expr_pack(const rxhip_expr_program* f, int d, expr::Program& out, char* msg, size_t n) {
    if (!f || !f->code || (f->n_consts > 0 && !f->consts)) { snprintf(msg, n, "expr: the program or one of its arrays is null"); return 1; }
    if (f->n_code < 1 || f->n_code > expr::EXPR_MAX_CODE) { snprintf(msg, n, "expr: a program has 1 … %d instructions (got %d)", expr::EXPR_MAX_CODE, f->n_code); return 1; }
    if (f->n_consts < 0 || f->n_consts > expr::EXPR_MAX_CONSTS) { snprintf(msg, n, "expr: a program has at most %d constants (got %d)", expr::EXPR_MAX_CONSTS, f->n_consts); return 1; }
    std::memset(&out, 0, sizeof out);
    out.n_code = f->n_code; out.n_consts = f->n_consts; out.d = f->d; out.n_slots = f->n_slots;
    std::memcpy(out.code, f->code, sizeof(int32_t) * 4 * (size_t)f->n_code);
    if (f->n_consts > 0) std::memcpy(out.consts, f->consts, sizeof(double) * (size_t)f->n_consts);
    return expr::expr_validate(out, d, msg, n);
}
// LDS of a workgroup that runs program p at dimension d with up to `comps` components per pass
static size_t expr_lds_bytes(const expr::Program& p, int d, int comps) {
    const int nc = std::min(comps, expr::expr_max_comps(p.n_slots, d));
    return (size_t)expr::rows_of(p.n_slots, d) * (size_t)nc * expr::EXPR_LANES * sizeof(double);
}
template <int D>
static void expr_eval_launch(const expr::Program* dp, const double* dx, double* dv, double* dj, long long n, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL((k_expr_eval<D>), dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, dp, dx, dv, dj, n);
}
extern "C++" rxhip_status rxhip::expr_eval(const rxhip_expr_program* f, const double* x, int64_t n, double* value, double* jac, int device, std::string& err) {
    char msg[256];
    if (!f || !x || !value || !jac || n < 1) { err = "expr_eval: null argument or no points"; return RXHIP_ERR_BADARG; }
    expr::Program prog;
    if (expr_pack(f, f->d, prog, msg, sizeof msg)) { err = msg; return RXHIP_ERR_BADARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { err = "expr_eval: no HIP device visible"; return RXHIP_ERR_NO_DEVICE; }
    if (device >= ndev) { err = "expr_eval: device ordinal out of range"; return RXHIP_ERR_BADARG; }
    DevGuard guard;
    hipError_t he = hipSuccess;
    if (device >= 0) he = guard.set(device);
    const size_t d = (size_t)prog.d, N = (size_t)n;
    DevTmp blk;
    if (he == hipSuccess) he = hipMalloc(&blk.p, sizeof prog + sizeof(double) * N * (2 * d + d * d));
    if (he == hipSuccess) {
        double* dx = (double*)((char*)blk.p + sizeof prog);
        double *dv = dx + N * d, *dj = dv + N * d;
        he = hipMemcpy(blk.p, &prog, sizeof prog, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(dx, x, sizeof(double) * N * d, hipMemcpyHostToDevice);
        if (he == hipSuccess) {
            const size_t lds = expr_lds_bytes(prog, prog.d, prog.d + 1);
            const expr::Program* dp = (const expr::Program*)blk.p;
            switch (prog.d) {
                case 1: expr_eval_launch<1>(dp, dx, dv, dj, n, lds, nullptr); break;
                case 2: expr_eval_launch<2>(dp, dx, dv, dj, n, lds, nullptr); break;
                case 3: expr_eval_launch<3>(dp, dx, dv, dj, n, lds, nullptr); break;
                default: expr_eval_launch<4>(dp, dx, dv, dj, n, lds, nullptr); break;
            }
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipDeviceSynchronize();
        if (he == hipSuccess) he = hipMemcpy(value, dv, sizeof(double) * N * d, hipMemcpyDeviceToHost);
        if (he == hipSuccess) he = hipMemcpy(jac, dj, sizeof(double) * N * d * d, hipMemcpyDeviceToHost);
    }
    if (he != hipSuccess) { err = std::string("expr_eval: ") + hipGetErrorString(he); return RXHIP_ERR_HIP; }
    return RXHIP_OK;
}

// symmetric positive SEMI-definite (n ≤ 4): symmetric to 1e-12 of its scale, and a Cholesky in which a pivot below 1e-12 of the scale is a zero
// pivot whose column must vanish with it
static bool host_sym_psd(int n, const double* A) {
    double scale = 0.0, L[16] = {0};
    for (int i = 0; i < n * n; ++i) { if (!std::isfinite(A[i])) return false; scale = std::max(scale, std::fabs(A[i])); }
    if (scale == 0.0) return true;
    const double tol = 1e-12 * scale;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (std::fabs(A[i * n + j] - A[j * n + i]) > tol) return false;
    for (int j = 0; j < n; ++j) {
        double sum = A[j * n + j];
        for (int k = 0; k < j; ++k) sum -= L[j * n + k] * L[j * n + k];
        if (sum < -tol) return false;
        const bool zero = sum <= tol;
        L[j * n + j] = zero ? 0.0 : std::sqrt(sum);
        for (int i = j + 1; i < n; ++i) {
            double v = A[i * n + j];
            for (int k = 0; k < j; ++k) v -= L[i * n + k] * L[j * n + k];
            if (zero) { if (std::fabs(v) > 1e-6 * scale) return false; L[i * n + j] = 0.0; }
            else L[i * n + j] = v / L[j * n + j];
        }
    }
    return true;
}
static bool host_sym_spd(int n, const double* A) {
    double tmp[16];
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (std::fabs(A[i * n + j] - A[j * n + i]) > 1e-12 * (std::fabs(A[i * n + i]) + std::fabs(A[j * n + j]))) return false;
    for (int i = 0; i < n * n; ++i) if (!std::isfinite(A[i])) return false;
    return host_chol_inv(n, A, tmp, nullptr);
}

rxhip_status rxhip_nlssm_create(const rxhip_nlssm_desc* ds, rxhip_engine** out) {
    if (rxhip_status st = new_handle(ds && ds->T > 0 && ds->n_series > 0, out, EngineKind::Nlssm)) return st;
    rxhip_engine* e = *out;
    const int d = ds->d, dy = ds->dy;
    if (d < 1 || d > 4) return fail(e, RXHIP_ERR_UNSUPPORTED, "nlssm: the state dimension d must be 1 … 4 (got %d)", d);
    if (dy < 1 || dy > d) return fail(e, RXHIP_ERR_BADARG, "nlssm: the observation dimension d_y must be 1 … d = %d (got %d)", d, dy);
    if (!ds->m0 || !ds->V0 || !ds->H) return fail(e, RXHIP_ERR_BADARG, "nlssm: m0, V0 and H are required");
    if (ds->method != RXHIP_NLSSM_LINEARIZATION && ds->method != RXHIP_NLSSM_UNSCENTED) return fail(e, RXHIP_ERR_BADARG, "nlssm: unknown method %d", ds->method);
    if (ds->mode != RXHIP_NLSSM_FILTER && ds->mode != RXHIP_NLSSM_SMOOTH) return fail(e, RXHIP_ERR_BADARG, "nlssm: unknown mode %d", ds->mode);
    const bool unknown = ds->noise_shape != 0.0;
    if (unknown) {
        if (dy != 1) return fail(e, RXHIP_ERR_UNSUPPORTED, "nlssm: unknown observation noise needs d_y = 1 (got %d)", dy);
        if (!(ds->noise_shape > 0) || !(ds->noise_rate > 0) || !std::isfinite(ds->noise_shape) || !std::isfinite(ds->noise_rate))
            return fail(e, RXHIP_ERR_BADARG, "nlssm: the Gamma prior of the observation precision needs a positive finite shape and rate (got %g, %g)", ds->noise_shape, ds->noise_rate);
        if (ds->mode == RXHIP_NLSSM_SMOOTH) return fail(e, RXHIP_ERR_UNSUPPORTED, "nlssm: smoothing with unknown observation noise is not supported (filter mode runs it)");
    } else {
        if (!ds->R) return fail(e, RXHIP_ERR_BADARG, "nlssm: known observation noise needs R");
        if (!host_sym_spd(dy, ds->R)) return fail(e, RXHIP_ERR_NOT_POSDEF, "nlssm: the observation covariance R is not symmetric positive definite");
    }
    const size_t npri = ds->per_series ? (size_t)ds->n_series : 1, dd = (size_t)d * d;
    for (size_t s = 0; s < npri; ++s) {
        for (int i = 0; i < d; ++i)
            if (!std::isfinite(ds->m0[s * d + i])) return fail(e, RXHIP_ERR_BADARG, "nlssm: the prior mean m0 of series %zu is not finite", s);
        if (!host_sym_spd(d, ds->V0 + s * dd)) return fail(e, RXHIP_ERR_NOT_POSDEF, "nlssm: the prior covariance V0 of series %zu is not symmetric positive definite", s);
    }
    if (ds->Q && !host_sym_psd(d, ds->Q)) return fail(e, RXHIP_ERR_NOT_POSDEF, "nlssm: the process covariance Q is not symmetric positive semi-definite");
    for (int i = 0; i < dy * d; ++i)
        if (!std::isfinite(ds->H[i])) return fail(e, RXHIP_ERR_BADARG, "nlssm: the observation matrix H is not finite");
    rxhip_engine::Nlssm& nl = e->nl;
    if (ds->method == RXHIP_NLSSM_UNSCENTED) {
        if (!(ds->alpha > 0) || !std::isfinite(ds->alpha) || !std::isfinite(ds->beta) || !std::isfinite(ds->kappa))
            return fail(e, RXHIP_ERR_BADARG, "nlssm: the unscented alpha must be positive and alpha, beta, kappa finite (got alpha = %g; this engine's defaults are "
                                             "1e-3, 2, 0)", ds->alpha);
        const double alpha = ds->alpha, beta = ds->beta, kappa = ds->kappa;
        const double sc = alpha * alpha * (d + kappa);   // d + λ
        if (!(sc > 0)) return fail(e, RXHIP_ERR_BADARG, "nlssm: the unscented parameters give d + lambda = %g, which must be positive", sc);
        nl.sc = sc; nl.wm0 = (sc - d) / sc; nl.wc0 = nl.wm0 + 1.0 - alpha * alpha + beta; nl.wi = 0.5 / sc;
    }
    expr::Program prog;
    char msg[256];
    if (expr_pack(ds->f, d, prog, msg, sizeof msg)) return fail(e, RXHIP_ERR_BADARG, "nlssm: %s", msg);
    int ndev = 0;
    if (rxhip_status st = count_devices(e, &ndev)) return st;
    e->T = ds->T; e->n_chains = ds->n_series; e->d = e->dpad = d; e->dy = dy;
    nl.method = ds->method; nl.unknown = unknown ? 1 : 0; nl.per_series = ds->per_series ? 1 : 0; nl.smooth = ds->mode == RXHIP_NLSSM_SMOOTH;
    nl.a0 = unknown ? ds->noise_shape : 1.0; nl.b0 = unknown ? ds->noise_rate : 1.0;
    for (size_t i = 0; i < dd; ++i) nl.Q[i] = ds->Q ? ds->Q[i] : 0.0;
    for (int i = 0; i < dy * d; ++i) nl.Hm[i] = ds->H[i];
    for (int i = 0; i < dy * dy; ++i) nl.R[i] = unknown ? 0.0 : ds->R[i];
    nl.lds_bytes = expr_lds_bytes(prog, d, ds->method == RXHIP_NLSSM_UNSCENTED ? 2 * d + 1 : d + 1);
    DevGuard guard;
    if (rxhip_status st = open_device(e, guard, ds->device, ds->stream, ndev)) return st;
    const size_t C = (size_t)ds->n_series, T = (size_t)ds->T;
    HIPCHK(e, hipMalloc(&nl.d_prog, sizeof prog));
    HIPCHK(e, hipMemcpy(nl.d_prog, &prog, sizeof prog, hipMemcpyHostToDevice));
    HIPCHK(e, hipMalloc(&nl.d_prior, sizeof(double) * npri * (d + dd)));
    {
        std::vector<double> pri(npri * (d + dd));
        for (size_t s = 0; s < npri; ++s) {
            std::memcpy(&pri[s * (d + dd)], ds->m0 + s * d, sizeof(double) * d);
            std::memcpy(&pri[s * (d + dd) + d], ds->V0 + s * dd, sizeof(double) * dd);
        }
        HIPCHK(e, hipMemcpy(nl.d_prior, pri.data(), sizeof(double) * pri.size(), hipMemcpyHostToDevice));
    }
    if (unknown) HIPCHK(e, hipMalloc(&nl.d_noise, sizeof(double) * 2 * T * C));
    if (nl.smooth) HIPCHK(e, hipMalloc(&nl.d_rec, sizeof(double) * T * (size_t)nlssm::n_records(d) * C));
    HIPCHK(e, hipMalloc(&nl.d_fe_series, sizeof(double) * C));
    HIPCHK(e, hipMalloc(&nl.d_where, sizeof(unsigned long long)));
    HIPCHK(e, hipMalloc(&e->d_mean, sizeof(double) * T * C * d));
    HIPCHK(e, hipMalloc(&e->d_cov, sizeof(double) * T * C * dd));
    return finish_create(e, C, 16);
}

rxhip_status rxhip_nlssm_get_noise(rxhip_engine* e, double* shape, double* rate) {
    if (!e || e->kind != EngineKind::Nlssm) return RXHIP_ERR_BADARG;
    if (!e->nl.unknown) return fail(e, RXHIP_ERR_BADARG, "nlssm_get_noise: the observation noise of this engine is known");
    DevGuard guard;
    if (rxhip_status st = open_results(e, guard, true, "nlssm_get_noise", false)) return st;
    const size_t n = (size_t)e->T * e->n_chains;
    if (shape) HIPCHK(e, hipMemcpy(shape, e->nl.d_noise, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (rate) HIPCHK(e, hipMemcpy(rate, e->nl.d_noise + n, sizeof(double) * n, hipMemcpyDeviceToHost));
    return RXHIP_OK;
}

template <int D>
static void nlssm_launch(const NlssmParams& p, size_t lds, bool backward, hipStream_t s) {
    const dim3 grid((unsigned)((p.n_series + 63) / 64));
    if (backward) hipLaunchKernelGGL((k_nlssm_backward<D>), grid, dim3(64), 0, s, p);
    else hipLaunchKernelGGL((k_nlssm_forward<D>), grid, dim3(64), lds, s, p);
}
static rxhip_status nlssm_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    if (rxhip_status st = run_preamble(e, iterations)) return st;
    SET_DEVICE(e);
    if (rxhip_status rs = reserve(e, &e->fe_total_cap, iterations, {{&e->d_fe_total, 1}})) return rs;
    const rxhip_engine::Nlssm& nl = e->nl;
    const size_t C = (size_t)e->n_chains, T = (size_t)e->T;
    NlssmParams p{};
    p.T = e->T; p.n_series = e->n_chains; p.dy = e->dy; p.method = nl.method; p.unknown = nl.unknown; p.per_series = nl.per_series;
    p.iterations = iterations; p.smooth = nl.smooth;
    p.prog = (const expr::Program*)nl.d_prog; p.y = e->d_y; p.prior = nl.d_prior;
    std::memcpy(p.Q, nl.Q, sizeof p.Q); std::memcpy(p.H, nl.Hm, sizeof p.H); std::memcpy(p.R, nl.R, sizeof p.R);
    p.a0 = nl.a0; p.b0 = nl.b0; p.u = {nl.sc, nl.wm0, nl.wc0, nl.wi};
    p.mean = e->d_mean; p.cov = e->d_cov; p.shape = nl.d_noise; p.rate = nl.d_noise ? nl.d_noise + T * C : nullptr;
    p.rec = nl.d_rec; p.fe_series = nl.d_fe_series; p.status = e->d_status; p.where = (unsigned long long*)nl.d_where;
    HIPCHK(e, hipMemsetAsync(nl.d_where, 0xff, sizeof(unsigned long long), e->stream));
    HIPCHK(e, hipMemsetAsync(nl.d_fe_series, 0, sizeof(double) * C, e->stream));
    rxhip_status st;
    for (int backward = 0; backward <= (nl.smooth ? 1 : 0); ++backward) {
        if ((st = prof_begin(e, backward ? RXHIP_K_BACKWARD : RXHIP_K_FORWARD))) return st;
        switch (e->d) {
            case 1: nlssm_launch<1>(p, nl.lds_bytes, backward, e->stream); break;
            case 2: nlssm_launch<2>(p, nl.lds_bytes, backward, e->stream); break;
            case 3: nlssm_launch<3>(p, nl.lds_bytes, backward, e->stream); break;
            default: nlssm_launch<4>(p, nl.lds_bytes, backward, e->stream); break;
        }
        if ((st = prof_end(e))) return st;
    }
    if (want_fe) {
        hipLaunchKernelGGL(k_nlssm_fe, dim3(1), dim3(256), 0, e->stream, (const double*)nl.d_fe_series, e->n_chains, e->d_fe_total, (int)iterations, e->d_status);
        HIPCHK(e, hipMemcpyAsync(e->d_fe_chain, nl.d_fe_series, sizeof(double) * C, hipMemcpyDeviceToDevice, e->stream));
    }
    HIPCHK(e, hipGetLastError());
    finish_run(e, iterations, want_fe != 0, !nl.smooth);
    // reference-equivalent events per series: a delta-node rule forward (and backward when smoothing) and an observation rule per step, the
    // q(τ) and q(x) updates per VMP iteration with unknown noise; a product and a marginal per state
    const uint64_t Cs = (uint64_t)C, Ts = (uint64_t)T, I = nl.unknown ? (uint64_t)iterations : 1;
    e->rule_calls = Cs * Ts * ((nl.smooth ? 2 : 1) + (nl.unknown ? 2 * I : 1));
    e->products = Cs * Ts * (nl.smooth ? 2 : 1) * I;
    e->marginals = Cs * Ts * I;
    return RXHIP_OK;
}

// the mixture engines' run: the split-phase entry points (several GPUs all-reduce the statistics between accumulate and update) back to back
static rxhip_status mixture_run_async(rxhip_engine* e, int32_t iterations, int32_t want_fe) {
    rxhip_status st = rxhip_gmm_begin_run(e, iterations);
    for (int it = 0; !st && it < iterations; ++it) {
        st = rxhip_gmm_accumulate(e);
        if (!st) st = rxhip_gmm_update(e, want_fe);
    }
    return st;
}

// The rows of the family table (engine.hpp EngineFamily; rxhip.hip's family_of looks here for the kinds it does not own).
const EngineFamily* rxhip::vmp_family(EngineKind kind) {
    using E = rxhip_engine;
    const char* const host_only = "set_data_device: the binomial regression engine checks its data on the host (rxhip_set_data)";
    //                            run                filter check              set_data         no_device_data  fe_total, has_x, release
    static const EngineFamily mixture = {mixture_run_async, false, nullptr, nullptr, nullptr, [](const E* e) { return e->g.d_fe; }, false, [](E* e) {
        free_buffers(e, {&e->g.d_resp, &e->g.d_par, &e->g.d_drv, &e->g.d_prior, &e->g.d_init, &e->g.d_partial, &e->g.d_totals, &e->g.d_hist, &e->g.d_fe});
    }};
    static const EngineFamily hgf = {hgf_run_async, false, nullptr, nullptr, nullptr, [](const E* e) { return e->h.d_fe_total; }, false, [](E* e) {
        free_buffers(e, {&e->h.d_out, &e->h.d_fe_series, &e->h.d_gh, &e->h.d_fe_total});
    }};
    static const EngineFamily probit = {probit_run_async, false, probit_check_data, nullptr, nullptr, nullptr, true, [](E* e) {
        free_buffers(e, {&e->pb.d_block, &e->pb.d_gh, &e->pb.d_fe_series});
    }};
    static const EngineFamily hmm = {hmm_run_async, false, hmm_check_data, nullptr, nullptr, nullptr, false, [](E* e) {
        free_buffers(e, {&e->hm.d_par, &e->hm.d_alpha, &e->hm.d_gamma, &e->hm.d_fe_series});
    }};
    static const EngineFamily lar = {lar_run_async, false, lar_check_data, nullptr, nullptr, nullptr, false, [](E* e) {
        free_buffers(e, {&e->la.d_cst, &e->la.d_par, &e->la.d_hist, &e->la.d_rec, &e->la.d_out, &e->la.d_fe_series});
    }};
    static const EngineFamily binreg = {binreg_run_async, false, nullptr, binreg_set_data, host_only, nullptr, false, [](E* e) {
        free_buffers(e, {&e->br.d_X, &e->br.d_neff, &e->br.d_kappa, &e->br.d_cst, &e->br.d_xi, &e->br.d_lc, &e->br.d_S, &e->br.d_part, &e->br.d_xi_part,
                         &e->br.d_hist, &e->br.d_fe_prob});
    }};
    // regression / autoregression: two rows that differ in how the data arrive — X and y through the family's own host-side set_data, or the raw
    // series through the common ingest (host or device) with the check of the latent autoregressive engine
    const char* const arreg_host_only = "set_data_device: the regression engine checks X and y on the host (rxhip_set_data); the lagged mode takes device data";
    const auto arreg_release = [](E* e) { free_buffers(e, {&e->ar.d_X, &e->ar.d_yreg, &e->ar.d_cst, &e->ar.d_part, &e->ar.d_hist, &e->ar.d_fe}); };
    static const EngineFamily arreg = {arreg_run_async, false, nullptr, arreg_set_data, arreg_host_only, nullptr, false, arreg_release};
    static const EngineFamily arreg_lagged = {arreg_run_async, false, arreg_check_data, nullptr, nullptr, nullptr, false, arreg_release};
    // multinomial regression: two rows that share everything (the kind tells the run which resident kernel to launch)
    const char* const mnreg_host_only = "set_data_device: the multinomial regression engine (mnreg) checks its counts on the host (rxhip_set_data)";
    const auto mnreg_release = [](E* e) {
        free_buffers(e, {&e->mn.d_data, &e->mn.d_cst, &e->mn.d_part, &e->mn.d_hist, &e->mn.d_fe, &e->mn.d_on, &e->mn.d_oncov, &e->mn.d_feit});
    };
    static const EngineFamily mnreg_row = {mnreg_run_async, false, nullptr, mnreg_set_data, mnreg_host_only, nullptr, false, mnreg_release};
    static const EngineFamily mnreg_online = {mnreg_run_async, false, nullptr, mnreg_set_data, mnreg_host_only, nullptr, false, mnreg_release};
    // Gamma mixture: the common ingest (host or device) with its own check of the observations
    static const EngineFamily gammamix_row = {gammamix_run_async, false, gammamix_check_data, nullptr, nullptr, nullptr, false, [](E* e) {
        free_buffers(e, {&e->gx.d_prior, &e->gx.d_init, &e->gx.d_state, &e->gx.d_part, &e->gx.d_hist, &e->gx.d_fe, &e->gx.d_resp, &e->gx.d_yt, &e->gx.d_ly});
    }};
    // nonlinear state-space model: the common ingest (any double is data, NaN = missing); the mode is the descriptor's, so no streaming twin
    static const EngineFamily nlssm_row = {nlssm_run_async, false, nullptr, nullptr, nullptr, nullptr, true, [](E* e) {
        free_buffers(e, {&e->nl.d_prog, &e->nl.d_prior, &e->nl.d_noise, &e->nl.d_rec, &e->nl.d_fe_series, &e->nl.d_where});
    }};
    switch (kind) {
        case EngineKind::Nlssm: return &nlssm_row;
        case EngineKind::GammaMix: return &gammamix_row;
        case EngineKind::Mnreg: return &mnreg_row;
        case EngineKind::MnregOnline: return &mnreg_online;
        case EngineKind::Arreg: return &arreg;
        case EngineKind::ArregLagged: return &arreg_lagged;
        case EngineKind::Mixture: return &mixture;
        case EngineKind::Hgf: return &hgf;
        case EngineKind::Probit: return &probit;
        case EngineKind::Hmm: return &hmm;
        case EngineKind::Lar: return &lar;
        case EngineKind::Binreg: return &binreg;
        default: return nullptr;
    }
}

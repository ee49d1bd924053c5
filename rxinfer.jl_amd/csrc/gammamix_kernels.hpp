// gammamix_kernels.hpp — batched variational message passing for the Gamma mixture with a point-mass shape, on gfx950.
//
// Reference model (test/models/mixtures/gamma_mixture_tests.jl:7-40), for each of n_problems independent mixtures of N points and K = 1 … 16 components:
//     s ~ Dirichlet(α⁰);  a[k] ~ Gamma(shape = c⁰_k, rate = d⁰_k);  b[k] ~ Gamma(shape = e⁰_k, rate = f⁰_k)
//     z[i] ~ Categorical(s);  y[i] ~ GammaMixture(switch = z[i], a = a, b = b),   p(y | z = k) = Gamma(y | shape a_k, rate b_k)
//     q = q(s) Π q(z_i) Π q(b_k) Π δ(a_k − â_k)
// The shape has no conjugate posterior; q(a_k) is a point mass at the maximiser of a 1-D concave objective, found by safeguarded Newton in ln a.
//
// One ITERATION is a defined semantic (include/rxhip.h).  With E ln b_k = ψ(e_k) − ln f_k, E b_k = e_k/f_k, E ln s_k = ψ(α_k) − ψ(Σα):
//   1. q(z_i) = softmax_k(E ln s_k + â_k E ln b_k − lnΓ(â_k) + (â_k − 1) ln y_i − E b_k y_i);  S0_k = Σ r_ik, S1_k = Σ r_ik y_i, SL_k = Σ r_ik ln y_i, H = −Σ r ln r;
//   2. α_k = α⁰_k + S0_k;
//   3. â_k: the root of g'(a) = (c⁰_k − 1)/a − d⁰_k + S0_k E ln b_k + SL_k − S0_k ψ(a) with the OLD q(b) (S0_k == 0: â_k is kept, ST_GAMMAMIX_EMPTY);
//   4. e_k = e⁰_k + S0_k â_k (new â), f_k = f⁰_k + S1_k;
//   5. F = −Σ_k[S0_k(E ln s_k + â_k E ln b_k − lnΓ(â_k)) + (â_k − 1) SL_k − E b_k S1_k] − H + KL(Dir(α)‖Dir(α⁰)) + Σ_k KL(Gamma(e_k, f_k)‖Gamma(e⁰_k, f⁰_k))
//          − Σ_k ln Gamma(â_k; c⁰_k, d⁰_k)   at the new q(s), â, q(b) and this iteration's q(z).
// The reference's own rule bodies and its point-mass optimiser were not at hand: the values per iteration belong to this engine.
//
// One schedule, streamed: per iteration
//   k_gammamix_pass<KT, LOGY> on a grid (chunks, problems), a lane per point, the per-component constants (c0, c1, c2) = (E ln s + â E ln b − lnΓ â,
//             â − 1, E b) read as wave-uniform values, 3·KT + 1 statistics in registers, fixed-shape wave/block reduction, per-block partials;
//   k_gammamix_update, one wavefront per problem: a lane per statistic adds the partials in ascending chunk order, then a lane per component
//             runs steps 2 – 5 (gammamix::update_component), the next pass's constants and the history entry;
//   k_gammamix_fe_total when F is wanted and problems > 1.
//   LOGY = true (shipped: measured faster) reads ln y stored at ingest (16 B/point), false recomputes it (8 B/point and an fp64 log): the
//   same function, the same bits.
// A resident schedule (every iteration of a run in one launch, the data in LDS) is NOT part of this file: its kernel faulted on the MI355X for a cause
// that was not found, and it was taken out whole.  gammamix::schedule therefore answers streamed for every (N, K) of the engine's range.
// No floating-point atomics anywhere; the bits of a problem do not depend on the batch, on F being asked for, or on the run.
//
// The point function and the helpers of the update (Newton step and solve, the whole per-component update, free-energy terms) are `__host__ __device__`, floating-point contraction off: the same
// functions compile for the host (tests/host_emul/gammamix_main.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "digamma.hpp"
#if defined(__HIPCC__)
#include "gmm_kernels.hpp"   // wave_sum, exp_nonpos
#endif

#if defined(__clang__)
#define GMIX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GMIX_NO_CONTRACT
#endif
#define GMIX_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace gammamix {

constexpr int kMaxK = 16;          // components; also the row stride of the per-problem blocks
constexpr int kTile = 256;         // points a workgroup takes per step
constexpr int kChunkCap = 1024;    // largest number of workgroups per problem of the streamed pass
constexpr int kNewtonCap = 40;     // Newton steps per shape at most
constexpr int kStateRows = 7;      // per-problem block: â | e | f | α | c0 | c1 | c2, rows of kMaxK
constexpr int kPriorRows = 5;      // per-problem prior block: c⁰ | d⁰ | e⁰ | f⁰ | α⁰
constexpr int SCHED_STREAMED = 1, SCHED_RESIDENT = 2;   // (2 is a value of the descriptor that this build refuses)

GMIX_HD int padded_k(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }
GMIX_HD int chunks(long long N) {
    const long long tiles = (N + kTile - 1) / kTile;
    return (int)(tiles < 1 ? 1 : tiles < kChunkCap ? tiles : kChunkCap);
}
// the schedule of (N, K): 0 outside the engine's range
GMIX_HD int schedule(long long N, int K) {
    if (N < 1 || K < 1 || K > kMaxK) return 0;
    return SCHED_STREAMED;
}

// g'(a) of step 3 and a·g''(a): B = S0·E ln b + SL
GMIX_HD double shape_grad(double a, double c0m1, double d0, double S0, double B, double psi_a) {
    GMIX_NO_CONTRACT
    return c0m1 / a - d0 + B - S0 * psi_a;
}
GMIX_HD double shape_curv_a(double a, double c0m1, double S0, double tri_a) {   // a·g''(a) < 0
    GMIX_NO_CONTRACT
    return -(c0m1 / a) - S0 * a * tri_a;
}
// One safeguarded Newton step in t = ln a: [lo, hi] brackets the root once both signs of g' have been seen (lo > hi: that side is open).  A step
// that leaves the bracket is replaced by its midpoint; with an open side the step is limited to ±2 (a factor e² in a).  Returns the new t.
GMIX_HD double newton_step(double t, double g, double ga, double& lo, double& hi, bool& have_lo, bool& have_hi) {
    GMIX_NO_CONTRACT
    if (g > 0.0) { lo = t; have_lo = true; }
    else { hi = t; have_hi = true; }
    double dt = -g / ga;
    if (!(dt == dt)) dt = g > 0.0 ? 2.0 : -2.0;
    if (dt > 2.0) dt = 2.0;
    if (dt < -2.0) dt = -2.0;
    double tn = t + dt;
    if (have_lo && have_hi && !(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
    return tn;
}
// â of step 3 from the previous â: stops when the step in ln a is within 8 ulp of 1 (|Δ ln a| ≤ 8·2⁻⁵²: a relative step in a) or after kNewtonCap steps
GMIX_HD double solve_shape(double a_prev, double c0, double d0, double S0, double B) {
    GMIX_NO_CONTRACT
    const double c0m1 = c0 - 1.0;
    double t = log(a_prev), lo = 0.0, hi = 0.0, a = a_prev;
    bool have_lo = false, have_hi = false;
    for (int it = 0; it < kNewtonCap; ++it) {
        const double g = shape_grad(a, c0m1, d0, S0, B, digamma_dev(a));
        if (g == 0.0) break;
        const double tn = newton_step(t, g, shape_curv_a(a, c0m1, S0, trigamma_dev(a)), lo, hi, have_lo, have_hi);
        const double step = tn - t;
        t = tn;
        a = exp(t);
        if (fabs(step) <= 8.0 * 2.220446049250313e-16) break;
    }
    return a;
}
// the constants of the responsibility rule: logit_k(y) = c0 + c1 ln y − c2 y
GMIX_HD void pass_constants(double a, double e, double f, double Elns, double lgamma_a, double& c0, double& c1, double& c2) {
    GMIX_NO_CONTRACT
    const double Elnb = digamma_dev(e) - log(f);
    c0 = Elns + a * Elnb - lgamma_a;
    c1 = a - 1.0;
    c2 = e / f;
}
// KL(Gamma(a, b) ‖ Gamma(a0, b0)), shape–rate; exactly 0 at a = a0, b = b0
GMIX_HD double gamma_kl(double a, double b, double a0, double b0) {
    GMIX_NO_CONTRACT
    return (a - a0) * digamma_dev(a) - lgamma(a) + lgamma(a0) + a0 * (log(b) - log(b0)) + a * (b0 - b) / b;
}
// component k's part of F: −[S0 c0 + c1 SL − c2 S1] + KL(q(b_k)‖prior) − ln Gamma(â; c⁰, d⁰) + its terms of KL(Dir(α)‖Dir(α⁰)):
// −lnΓ(α_k) + lnΓ(α⁰_k) + (α_k − α⁰_k) E ln s_k
GMIX_HD double fe_component(double S0, double S1, double SL, double c0, double c1, double c2, double a, double e, double f, double pc, double pd, double pe, double pf,
                            double al, double al0, double Elns) {
    GMIX_NO_CONTRACT
    const double lik = S0 * c0 + c1 * SL - c2 * S1;
    const double lp = pc * log(pd) - lgamma(pc) + (pc - 1.0) * log(a) - pd * a;
    const double dir = -lgamma(al) + lgamma(al0) + (al - al0) * Elns;
    return -lik + gamma_kl(e, f, pe, pf) - lp + dir;
}
// F from the components' parts (added in ascending k by the caller), the entropy and the Dirichlet normalisers
GMIX_HD double fe_total(double sum_components, double H, double asum, double a0sum) {
    GMIX_NO_CONTRACT
    return sum_components - H + (lgamma(asum) - lgamma(a0sum));
}

// Steps 3 – 5 for ONE component from its statistics, its prior, its α (step 2, with Σα) and the state before the iteration: â (kept, `empty` set, when
// S0 == 0), e, f, the next pass's constants, and the component's part of F.  What a lane of k_gammamix_update runs, and what the host build runs.
struct ComponentUpdate { double a, e, f, c0, c1, c2, fk; bool empty; };
GMIX_HD ComponentUpdate update_component(double S0, double S1, double SL, double pc, double pd, double pe, double pf, double al, double al0, double asum, double a_old,
                                         double e_old, double f_old) {
    GMIX_NO_CONTRACT
    ComponentUpdate u;
    u.empty = !(S0 > 0.0);
    u.a = u.empty ? a_old : solve_shape(a_old, pc, pd, S0, S0 * (digamma_dev(e_old) - log(f_old)) + SL);
    u.e = pe + S0 * u.a;
    u.f = pf + S1;
    const double Elns = digamma_dev(al) - digamma_dev(asum);
    pass_constants(u.a, u.e, u.f, Elns, lgamma(u.a), u.c0, u.c1, u.c2);
    u.fk = fe_component(S0, S1, SL, u.c0, u.c1, u.c2, u.a, u.e, u.f, pc, pd, pe, pf, al, al0, Elns);
    return u;
}

// one point: logits, softmax, statistics.  sc: [3][KT] constants (LDS on the device), w: 1 or 0 (missing: y = 1, ln y = 0 are passed)
template <int KT>
GMIX_HD void point(double y, double ly, double w, const double* sc, double (&S0)[KT], double (&S1)[KT], double (&SL)[KT], double& Hz,
              double (&r)[KT]) {
    GMIX_NO_CONTRACT
    double lg[KT], mx = -1e308;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        lg[k] = (sc[k] + sc[KT + k] * ly) - sc[2 * KT + k] * y;
        mx = fmax(mx, lg[k]);
    }
    double Z = 0.0, sl = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
        r[k] = exp_nonpos(lg[k] - mx);   // the range-check-free exp of the Gaussian mixture pass
#else
        r[k] = exp(lg[k] - mx);
#endif
        Z += r[k];
    }
    const double zi = w / Z;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const double pi = r[k] * zi;
        sl += pi * (lg[k] - mx);
        S0[k] += pi;
        S1[k] += pi * y;
        SL[k] += pi * ly;
        r[k] = pi;
    }
    Hz += w * log(Z) - sl;
}

}  // namespace gammamix
}  // namespace rxhip

#if defined(__HIPCC__)

namespace rxhip {

constexpr int ST_GAMMAMIX_BAD_Y = 64;    // status bit of k_gammamix_check_y (next to ST_NOT_POSDEF = 1, ST_NONFINITE = 2, …, ST_LAR_BAD_Y = 16, ST_HMM_UNDERFLOW = 32)
constexpr int ST_GAMMAMIX_EMPTY = 128;   // a component received no responsibility at all (S0_k == 0): its â was kept; outside the contract

struct GammaMixParams {
    long long N, C;                  // points per problem, problems
    int K, nchunk, want_fe, iterations, iteration, write_resp;
    const double* y;                 // [C][N] (C == 1: the ingested array itself)
    const double* ly;                // [C][N] ln y (the pass on stored logarithms), else unused
    const double* prior;             // [C][kPriorRows][kMaxK]
    const double* init;              // [C][kStateRows][kMaxK]: the state every run starts from
    double* state;                   // [C][kStateRows][kMaxK]: the current state
    double* part;                    // [C][nchunk][3·KT + 1]
    double* hist;                    // [iterations][C][4][K]
    double* fe;                      // [iterations][C]
    double* fe_total;                // [iterations]
    double* fe_chain;                // [C]: F of the last iteration
    double* resp;                    // [C][N][K] or nullptr
    int* status;
};

// y ≤ 0 or ±Inf is refused; NaN is a missing point
static __global__ void __launch_bounds__(256) k_gammamix_check_y(const double* y, long long n, int* status) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = y[i];
        bad = bad || (v == v && !(v > 0.0 && v - v == 0.0));
    }
    if (bad) atomicOr(status, ST_GAMMAMIX_BAD_Y);
}
// the ingested [N][C] array -> [C][N] (batches), and ln y [C][N] when the pass reads stored logarithms
static __global__ void __launch_bounds__(256) k_gammamix_prepare(const double* src, long long N, long long C, double* yt, double* ly) {
    const long long n = N * C;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
        const long long c = q / N, i = q - c * N;
        const double v = src[i * C + c];
        if (yt) yt[q] = v;
        if (ly) ly[q] = log(v);
    }
}

// the block's statistics: wave shuffles, then the four wavefronts in wave order.  sh: [4][3·KT + 1]; out[q], q < 3·KT + 1, by the first threads
template <int KT>
__device__ __forceinline__ void gammamix_block_sum(const double (&S0)[KT], const double (&S1)[KT], const double (&SL)[KT], double Hz, double* sh, double* out) {
    constexpr int NQ = 3 * KT + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        const double a = wave_sum(S0[k]), b = wave_sum(S1[k]), c = wave_sum(SL[k]);
        if (lane == 0) {
            sh[w * NQ + k] = a;
            sh[w * NQ + KT + k] = b;
            sh[w * NQ + 2 * KT + k] = c;
        }
    }
    {
        const double a = wave_sum(Hz);
        if (lane == 0) sh[w * NQ + 3 * KT] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < NQ) out[threadIdx.x] = ((sh[threadIdx.x] + sh[NQ + threadIdx.x]) + sh[2 * NQ + threadIdx.x]) + sh[3 * NQ + threadIdx.x];
}

// Steps 2 – 5 for one problem on a wavefront, a lane per component (lanes ≥ K idle but take part in the shuffles).  tot: the statistics [3·KT + 1] with
// row stride KT; old: the state before the iteration; the new state goes to `st` (may be `old`'s block: a lane touches its own column only).  Nothing
// but the free-energy stores depends on want_fe (F's component parts are computed either way).
__device__ __forceinline__ void gammamix_update_lane(const GammaMixParams& p, long long prob, int it, int KT, const double* tot, const double* pr, const double* old,
                                                     double* st) {
    GMIX_NO_CONTRACT
    constexpr int KS = gammamix::kMaxK;
    const int k = threadIdx.x & 63, K = p.K;
    const bool on = k < K;
    double S0 = 0.0, S1 = 0.0, SL = 0.0, pc = 1.0, pd = 1.0, pe = 1.0, pf = 1.0, al0 = 0.0, a = 1.0, e_old = 1.0, f_old = 1.0;
    if (on) {
        S0 = tot[k]; S1 = tot[KT + k]; SL = tot[2 * KT + k];
        pc = pr[k]; pd = pr[KS + k]; pe = pr[2 * KS + k]; pf = pr[3 * KS + k]; al0 = pr[4 * KS + k];
        a = old[k]; e_old = old[KS + k]; f_old = old[2 * KS + k];
    }
    const double al = al0 + S0;
    double asum = 0.0, a0sum = 0.0;
    for (int j = 0; j < K; ++j) {
        asum += __shfl(al, j);
        a0sum += __shfl(al0, j);
    }
    double c0 = -1e300, c1 = 0.0, c2 = 0.0, fk = 0.0;   // padding components never receive responsibility
    if (on) {
        const gammamix::ComponentUpdate u = gammamix::update_component(S0, S1, SL, pc, pd, pe, pf, al, al0, asum, a, e_old, f_old);
        if (u.empty) atomicOr(p.status, ST_GAMMAMIX_EMPTY);
        c0 = u.c0; c1 = u.c1; c2 = u.c2; fk = u.fk;
        st[k] = u.a; st[KS + k] = u.e; st[2 * KS + k] = u.f; st[3 * KS + k] = al;
        double* h = p.hist + ((size_t)it * p.C + prob) * 4 * K;
        h[k] = u.a; h[K + k] = u.e; h[2 * K + k] = u.f; h[3 * K + k] = al;
    }
    if (k < KS) { st[4 * KS + k] = c0; st[5 * KS + k] = c1; st[6 * KS + k] = c2; }
    if (p.want_fe) {
        double sum = 0.0;
        for (int j = 0; j < K; ++j) sum += __shfl(fk, j);
        if (k == 0) {
            const double F = gammamix::fe_total(sum, tot[3 * KT], asum, a0sum);
            p.fe[(size_t)it * p.C + prob] = F;
            if (p.C == 1) p.fe_total[it] = F;
            if (it == p.iterations - 1) p.fe_chain[prob] = F;
            if (!(F - F == 0.0)) atomicOr(p.status, ST_NONFINITE);
        }
    }
}

template <int KT, bool LOGY>
__global__ void __launch_bounds__(256) k_gammamix_pass(GammaMixParams p) {
    GMIX_NO_CONTRACT
    constexpr int NQ = 3 * KT + 1, KS = gammamix::kMaxK;
    __shared__ double sh[4 * NQ];
    __shared__ double sc[3 * KT];
    const long long prob = blockIdx.y, N = p.N;
    const double* blk = (p.iteration == 0 ? p.init : p.state) + (size_t)prob * gammamix::kStateRows * KS;
    if ((int)threadIdx.x < 3 * KT) sc[threadIdx.x] = blk[(4 + threadIdx.x / KT) * KS + threadIdx.x % KT];
    __syncthreads();
    const double* Y = p.y + prob * N;
    const double* LY = LOGY ? p.ly + prob * N : nullptr;
    double S0[KT], S1[KT], SL[KT], Hz = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) S0[k] = S1[k] = SL[k] = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        double y = Y[i], ly;
        if constexpr (LOGY) ly = LY[i];
        const bool ok = y == y;
        if (!ok) y = 1.0;
        if constexpr (!LOGY) ly = log(y);
        if (!ok) ly = 0.0;
        double r[KT];
        gammamix::point<KT>(y, ly, ok ? 1.0 : 0.0, sc, S0, S1, SL, Hz, r);
        if (p.write_resp) {
            double* q = p.resp + ((size_t)prob * N + i) * p.K;
#pragma unroll
            for (int k = 0; k < KT; ++k)
                if (k < p.K) q[k] = r[k];
        }
    }
    gammamix_block_sum<KT>(S0, S1, SL, Hz, sh, p.part + ((size_t)prob * p.nchunk + blockIdx.x) * NQ);
}

// one wavefront per problem: the partials in ascending chunk order (a lane per statistic, 16 loads in flight ahead of the adds), then the update
static __global__ void __launch_bounds__(64) k_gammamix_update(GammaMixParams p) {
    GMIX_NO_CONTRACT
    constexpr int KS = gammamix::kMaxK;
    __shared__ double tot[3 * KS + 1];
    const int t = threadIdx.x, KT = gammamix::padded_k(p.K), NQ = 3 * KT + 1;
    const long long prob = blockIdx.x;
    if (t < NQ) {
        const double* part = p.part + (size_t)prob * p.nchunk * NQ;
        double acc = part[t];
        int c = 1;
        for (; c + 16 <= p.nchunk; c += 16) {
            double v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = part[(size_t)(c + k) * NQ + t];
#pragma unroll
            for (int k = 0; k < 16; ++k) acc += v[k];
        }
        for (; c < p.nchunk; ++c) acc += part[(size_t)c * NQ + t];
        tot[t] = acc;
    }
    __syncthreads();
    double* st = p.state + (size_t)prob * gammamix::kStateRows * KS;
    const double* old = p.iteration == 0 ? p.init + (size_t)prob * gammamix::kStateRows * KS : st;
    gammamix_update_lane(p, prob, p.iteration, KT, tot, p.prior + (size_t)prob * gammamix::kPriorRows * KS, old, st);
}

// the totals of a batch, one workgroup per iteration: the problems in a fixed tree
static __global__ void __launch_bounds__(256) k_gammamix_fe_total(GammaMixParams p) {
    GMIX_NO_CONTRACT
    __shared__ double sh[256];
    const int it = blockIdx.x;
    double acc = 0.0;
    for (long long s = threadIdx.x; s < p.C; s += 256) acc += p.fe[(size_t)it * p.C + s];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int wd = 128; wd > 0; wd >>= 1) {
        if ((int)threadIdx.x < wd) sh[threadIdx.x] += sh[threadIdx.x + wd];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.fe_total[it] = sh[0];
}

}  // namespace rxhip
#endif

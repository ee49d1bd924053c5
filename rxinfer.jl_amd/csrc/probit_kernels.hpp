// probit_kernels.hpp — batched expectation propagation for a scalar Gaussian chain observed through Probit, on gfx950.
//
// Reference model (test/models/statespace/probit_tests.jl:11-18), for each of n_series independent series:
//     x[0] ~ Normal(m0, v0);   x[k] ~ Normal(a·x[k-1] + c, q);   y[k-1] ~ Probit(x[k])      k = 1 … T,  y ∈ {0, 1}, NaN = missing
// Reference rules replaced (bodies in the un-vendored ReactiveMP.jl): the Probit node's :in rule under
// RequireMessageFunctionalDependencies (moment matching of N(x; m, v)·Φ(s·x), s = 2y − 1), its average energy (Gauss–Hermite), the
// NormalMeanPrecision transition / prior rules and the Bethe free energy of a Gaussian q.
//
// One ITERATION of this engine is a parallel EP update — a defined semantic, not the reactive engine's update order:
//   1. the chain is smoothed with the current Gaussian sites (ξ_k, w_k) (weighted mean, precision; all empty at the start) as
//      pseudo-observations: forward predictive message and backward message at every x[k]; their product is the cavity N(m, v) of step k;
//   2. the new site of EVERY observed step is computed from its cavity of that one pass:
//         z = s·m/√(1+v),  r = φ(z)/Φ(z),  m̃ = m + s·v·r/√(1+v),  ṽ = v − v²·r·(z+r)/(1+v),
//         w' = max(1/ṽ − 1/v, 1e-12),  ξ' = m̃/ṽ − m/v                        (missing steps keep the empty site);
//      at step k the backward message toward k−1 is built from the OLD site k and the new one is stored afterwards;
//   3. the posteriors and the free energy OF ITERATION i are those of the Gaussian q given the sites after i updates.
// The reference's per-iteration values depend on its reactive order and need not equal these; the fixed point does (the reference test
// asserts one free energy for three different initial messages, probit_tests.jl:65-78: 15.646236967225065, reproduced to 1e-13).
//
// Schedule.  A series is sequential in time, series are independent: k_probit_sweep gives a lane to a series, arrays are [step][series]
// (a wavefront's loads coalesce), everything fp64.  A sweep is a forward loop (reads the sites, writes the predictive messages) and a
// backward loop (reads them, y and the sites; writes the new sites and — when asked — the marginals and the Gaussian part of the
// free energy, accumulated in the lane in time order).  The free energy of iteration i is folded into the sweep of iteration i + 1
// (its marginals are the cavities times the old sites, which that sweep forms anyway); a last sweep without an update gives the
// posteriors and the last free energy: iterations + 1 sweeps per run.  The Probit average energies need n_gh ≤ 32 log Φ each and
// nothing but the marginals, so they are NOT in the sequential lane: k_probit_energy evaluates them over (step-chunk, series) with
// the whole device, one fixed-order partial sum per chunk of PROBIT_ECHUNK steps, and k_probit_fe adds a series' partials in chunk
// order and the series in a fixed tree.  Like the HGF kernel (hgf_kernels.hpp) the loop is bound by fp64 transcendentals and
// dependent-issue latency, not by HBM: 88 B per (series, step, iteration) without the free energy, 128 B with it.
//
// The per-step math is `__host__ __device__` and self-contained (no other header of the library), floating-point contraction off: the
// same functions compile for the host (tests/host_emul/probit_main.cpp) and give the same bits in every kernel instance, so a run
// with and without the free energy returns bit-identical posteriors.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#if defined(__clang__)
#define PROBIT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PROBIT_NO_CONTRACT
#endif
#define PROBIT_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace probit {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;
constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr double kSqrt2OverPi = 0.79788456080286535588;   // √(2/π)
constexpr double kInvSqrtPi = 0.56418958354775628695;
constexpr double kSiteFloor = 1e-12;

// erfcx(t) = exp(t²)·erfc(t) for t ≥ 0.  Below 4: the product itself, t² split into a rounded square and its residual so that the
// exponential carries no amplified rounding error.  From 4 on (erfc heads for underflow; Φ(−40) IS zero in fp64): the continued
// fraction  erfcx(t) = (1/√π) / (t + (1/2)/(t + 1/(t + (3/2)/(t + 2/(t + …))))), 24 levels evaluated backward — at t = 4 the
// truncation error is below 1e-18 and it falls with t.  Beyond 1e8 the first level is exact in fp64.
PROBIT_HD double erfcx_nonneg(double t) {
    PROBIT_NO_CONTRACT
    if (t < 4.0) {
        const double hi = t * t, lo = fma(t, t, -hi);
        return exp(hi) * erfc(t) * (1.0 + lo);
    }
    if (t > 1e8) return kInvSqrtPi / t;
    double f = t;
    for (int n = 24; n >= 1; --n) f = t + (0.5 * n) / f;
    return kInvSqrtPi / f;
}

// r(z) = φ(z)/Φ(z), finite and accurate over the whole line: through erfcx for z < 0 (r(−40) = 40.02496…), through erfc otherwise
PROBIT_HD double mills_ratio(double z) {
    PROBIT_NO_CONTRACT
    if (z < 0.0) return kSqrt2OverPi / erfcx_nonneg(-z * kInvSqrt2);
    return kSqrt2OverPi * exp(-0.5 * z * z) / erfc(-z * kInvSqrt2);
}

// log Φ(x): log1p(−½ erfc(x/√2)) above zero, log(½ erfc(−x/√2)) down to the point where erfc leaves the comfortable range, and
// log(½ erfcx(t)) − t² with t = −x/√2 in the lower tail
PROBIT_HD double log_ndtr(double x) {
    PROBIT_NO_CONTRACT
    if (x > 0.0) return log1p(-0.5 * erfc(x * kInvSqrt2));
    const double t = -x * kInvSqrt2;
    if (t < 4.0) return log(0.5 * erfc(t));
    return log(0.5 * erfcx_nonneg(t)) - t * t;
}

// ---- message algebra of the chain.  Messages toward a state are (ξ, w): weighted mean and precision; (0, 0) is the empty message.
// forward: the belief of x[k-1] (predictive message N(pm, pv) times its site) pushed through x[k] ~ N(a·x[k-1] + c, q)
PROBIT_HD void predict(double pm, double pv, double xi, double w, double a, double c, double q, double& pm_next, double& pv_next) {
    PROBIT_NO_CONTRACT
    const double fp = 1.0 / pv + w;
    const double fm = (pm / pv + xi) / fp;
    pm_next = a * fm + c;
    pv_next = a * a / fp + q;
}
// backward: what x[k] hears from its observation and the future, (lξ, lw), pulled through the transition toward x[k-1]
PROBIT_HD void pull_back(double lxi, double lw, double a, double c, double q, double& bxi, double& bw) {
    PROBIT_NO_CONTRACT
    const double den = 1.0 + q * lw;
    bxi = a * (lxi - c * lw) / den;
    bw = a * a * lw / den;
}
// cavity of step k: predictive message times backward message
PROBIT_HD void cavity(double pm, double pv, double bxi, double bw, double& m, double& v) {
    PROBIT_NO_CONTRACT
    const double cp = 1.0 / pv + bw;
    v = 1.0 / cp;
    m = (pm / pv + bxi) * v;
}
// marginal of x[k]: cavity times site
PROBIT_HD void marginal(double pm, double pv, double bxi, double bw, double xi, double w, double& mean, double& var) {
    PROBIT_NO_CONTRACT
    var = 1.0 / (1.0 / pv + bw + w);
    mean = (pm / pv + bxi + xi) * var;
}

// New site of an observed step from its cavity N(m, v), s = ±1.  With g = r·(z + r) the header's formulas are, term for term,
//     ṽ = v·((1+v) − v·g)/(1+v),   1/ṽ − 1/v = g/((1+v) − v·g),   m̃/ṽ − m/v = (s·r·√(1+v) + m·g)/((1+v) − v·g):
// the same numbers without the difference of two nearly equal reciprocals.
PROBIT_HD void site_update(double m, double v, double s, double& xi_new, double& w_new) {
    PROBIT_NO_CONTRACT
    const double sq = sqrt(1.0 + v);
    const double z = s * m / sq;
    const double r = mills_ratio(z);
    const double g = r * (z + r);
    const double den = (1.0 + v) - v * g;
    const double w = g / den;
    xi_new = (s * r * sq + m * g) / den;
    w_new = w > kSiteFloor ? w : kSiteFloor;
}
// tilted moments themselves (the host check compares them with quadrature)
PROBIT_HD void tilted_moments(double m, double v, double s, double& mt, double& vt) {
    PROBIT_NO_CONTRACT
    const double sq = sqrt(1.0 + v);
    const double z = s * m / sq;
    const double r = mills_ratio(z);
    mt = m + s * v * r / sq;
    vt = v * ((1.0 + v) - v * (r * (z + r))) / (1.0 + v);
}

// ---- Bethe free energy of the Gaussian q.  Per factor U − H[q_f], per variable (deg − 1)·H[q_v]:
PROBIT_HD double entropy(double var) {
    PROBIT_NO_CONTRACT
    return 0.5 * (kLog2Pi + 1.0 + log(var));
}
// prior node: E_q[−log N(x0; m0, v0)] − H[q(x0)]
PROBIT_HD double prior_term(double mean, double var, double m0, double v0) {
    PROBIT_NO_CONTRACT
    const double dm = mean - m0;
    return 0.5 * (kLog2Pi + log(v0)) + 0.5 * (dm * dm + var) / v0 - entropy(var);
}
// transition (k-1, k): E_q[−log N(x_k; a·x_{k-1} + c, q)] − H[q(x_{k-1}, x_k)].  The pair marginal is the filtered belief of x[k-1]
// (precision fp, weighted mean fxi) times the transition times (lξ, lw) on x[k]; its precision is [[fp + a²/q, −a/q], [−a/q, 1/q + lw]].
// With D = q·det = fp·(1 + q·lw) + a²·lw the residual mean and variance of x_k − a·x_{k-1} − c are closed forms without cancellation:
//     E[res] = q·(fp·(lξ − c·lw) − a·lw·fξ)/D,   var[res] = q·(fp + a²·lw)/D,   H = log 2πe − ½ log(D/q).
PROBIT_HD double transition_term(double fp, double fxi, double lxi, double lw, double a, double c, double q) {
    PROBIT_NO_CONTRACT
    const double D = fp * (1.0 + q * lw) + a * a * lw;
    const double res = q * (fp * (lxi - c * lw) - a * lw * fxi) / D;
    const double e2 = res * res + q * (fp + a * a * lw) / D;
    const double lq = log(q);
    return 0.5 * (kLog2Pi + lq) + 0.5 * e2 / q - (kLog2Pi + 1.0 - 0.5 * (log(D) - lq));
}
// observed Probit node: E_{q(x_k)}[−log Φ(s·x_k)] by the n_gh-point Gauss–Hermite rule (gh: [2][32] nodes | weights/√π); its −H[q(x_k)]
// is taken with the variable terms below (variable_term)
PROBIT_HD double probit_energy(double mean, double var, double s, const double* gh, int n_gh) {
    PROBIT_NO_CONTRACT
    const double sc = sqrt(2.0 * var);
    double e = 0.0;
    for (int i = 0; i < n_gh; ++i) e -= gh[32 + i] * log_ndtr(s * (mean + sc * gh[i]));
    return e;
}
// variables: (deg − 1)·H[q(x_k)], deg = (prior | incoming transition) + [k < T: outgoing transition] + [observed].  Together with the −H of an observed
// Probit node (whose energy k_probit_energy adds) the observation cancels: what the sweep adds per state is [k < T]·H[q(x_k)].
PROBIT_HD double variable_term(bool has_next, double var) {
    PROBIT_NO_CONTRACT
    return has_next ? entropy(var) : 0.0;
}

}  // namespace probit
}  // namespace rxhip

#if defined(__HIPCC__) || defined(RXHIP_HOST_EMUL)   // (the host build of tests/host_emul/probit_main.cpp runs these one thread at a time)
namespace rxhip {

constexpr int PROBIT_ECHUNK = 16;    // steps per partial sum of k_probit_energy (more when T/16 would not fit a grid dimension: ProbitParams::echunk)
constexpr int ST_PROBIT_BAD_Y = 4;   // status bit of k_probit_check_y (next to ST_NOT_POSDEF = 1, ST_NONFINITE = 2)

struct ProbitParams {
    long long T, n_series;
    const double* y;        // [T][series]
    double *xi, *w;         // [T+1][series] sites (row 0 stays empty: x[0] has no observation)
    double *pm, *pv;        // [T+1][series] forward predictive messages of the running sweep
    double *mean, *var;     // [T+1][series] marginals
    double* fe_gauss;       // [series] Gaussian part of the free energy of the sweep
    double* fe_part;        // [chunks][series] Probit average energies, echunk steps each
    double* fe_series;      // [iterations][series]
    const double* gh;       // [2][32]
    double a, c, q, m0, v0;
    int n_gh;
    long long echunk;       // steps per partial sum, chunks = ⌈T/echunk⌉
    int* status;
};

// One sweep of a series per lane.  UPDATE: store the new sites.  OUT: store the marginals.  FE: accumulate prior, transition and entropy terms.
template <bool UPDATE, bool OUT, bool FE>
__global__ void __launch_bounds__(64) k_probit_sweep(ProbitParams p) {
    PROBIT_NO_CONTRACT
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= p.n_series) return;
    const long long C = p.n_series, T = p.T;
    const double a = p.a, c = p.c, q = p.q;
    // forward: predictive message at every x[k]; the site of the next step is loaded while this one is computed
    double pm = p.m0, pv = p.v0;
    p.pm[s] = pm; p.pv[s] = pv;
    double xi = 0.0, w = 0.0;                       // site of x[k-1] (x[0]: none)
    double xin = T >= 1 ? p.xi[C + s] : 0.0, wn = T >= 1 ? p.w[C + s] : 0.0;
    for (long long k = 1; k <= T; ++k) {
        double pmn, pvn;
        probit::predict(pm, pv, xi, w, a, c, q, pmn, pvn);
        pm = pmn; pv = pvn;
        xi = xin; w = wn;
        if (k < T) { xin = p.xi[(k + 1) * C + s]; wn = p.w[(k + 1) * C + s]; }
        p.pm[k * C + s] = pm; p.pv[k * C + s] = pv;
    }
    // backward: now (pm, pv) is the predictive message and (xi, w) the old site of x[T]
    double bxi = 0.0, bw = 0.0, fe = 0.0;
    bool bad = false;
    double yk = T >= 1 ? p.y[(T - 1) * C + s] : 0.0;
    for (long long k = T; k >= 0; --k) {
        // the step below, loaded ahead: its predictive message, its old site, its observation
        double pm1 = 0.0, pv1 = 1.0, xi1 = 0.0, w1 = 0.0, y1 = 0.0;
        if (k >= 1) {
            pm1 = p.pm[(k - 1) * C + s]; pv1 = p.pv[(k - 1) * C + s];
            if (k >= 2) { xi1 = p.xi[(k - 1) * C + s]; w1 = p.w[(k - 1) * C + s]; y1 = p.y[(k - 2) * C + s]; }
        }
        if (OUT || FE) {
            double mean, var;
            probit::marginal(pm, pv, bxi, bw, xi, w, mean, var);
            bad = bad || !(var > 0.0) || !(mean - mean == 0.0);
            if (OUT) { p.mean[k * C + s] = mean; p.var[k * C + s] = var; }
            if (FE) {
                fe += probit::variable_term(k < T, var);
                if (k == 0) fe += probit::prior_term(mean, var, p.m0, p.v0);
            }
        }
        if (k >= 1) {
            if (UPDATE && yk == yk) {               // observed: new site from the cavity of this pass
                double m, v, nxi, nw;
                probit::cavity(pm, pv, bxi, bw, m, v);
                probit::site_update(m, v, yk > 0.5 ? 1.0 : -1.0, nxi, nw);
                bad = bad || !(v > 0.0) || !(nxi - nxi == 0.0) || !(nw - nw == 0.0);
                p.xi[k * C + s] = nxi; p.w[k * C + s] = nw;
            }
            const double lxi = bxi + xi, lw = bw + w;   // the OLD site: every new site of this iteration sees the same pass
            if (FE) fe += probit::transition_term(1.0 / pv1 + w1, pm1 / pv1 + xi1, lxi, lw, a, c, q);
            probit::pull_back(lxi, lw, a, c, q, bxi, bw);
        }
        pm = pm1; pv = pv1; xi = xi1; w = w1; yk = y1;
    }
    if (FE) p.fe_gauss[s] = fe;
    if (bad) atomicOr(p.status, 2);   // ST_NONFINITE
}

// Probit average energies of one sweep's marginals: thread = (series, chunk of echunk steps), steps of a chunk added in time order
__global__ void __launch_bounds__(256) k_probit_energy(ProbitParams p) {
    PROBIT_NO_CONTRACT
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long ch = blockIdx.y;
    if (s >= p.n_series) return;
    const long long k0 = 1 + ch * p.echunk;
    const long long k1 = k0 + p.echunk <= p.T + 1 ? k0 + p.echunk : p.T + 1;
    double e = 0.0;
    for (long long k = k0; k < k1; ++k) {
        const double y = p.y[(k - 1) * p.n_series + s];
        if (y == y) e += probit::probit_energy(p.mean[k * p.n_series + s], p.var[k * p.n_series + s], y > 0.5 ? 1.0 : -1.0, p.gh, p.n_gh);
    }
    p.fe_part[ch * p.n_series + s] = e;
}

// free energy of iteration n per series (Gaussian part + the chunks in order) and summed over the series (fixed tree)
__global__ void __launch_bounds__(256) k_probit_fe(ProbitParams p, int n, long long chunks, double* fe_total) {
    PROBIT_NO_CONTRACT
    __shared__ double sh[256];
    double acc = 0.0;
    for (long long s = threadIdx.x; s < p.n_series; s += 256) {
        double f = p.fe_gauss[s];
        for (long long ch = 0; ch < chunks; ++ch) f += p.fe_part[ch * p.n_series + s];
        p.fe_series[(long long)n * p.n_series + s] = f;
        acc += f;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int wd = 128; wd > 0; wd >>= 1) {
        if ((int)threadIdx.x < wd) sh[threadIdx.x] += sh[threadIdx.x + wd];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        fe_total[n] = sh[0];
        if (!(sh[0] - sh[0] == 0.0)) atomicOr(p.status, 2);   // ST_NONFINITE
    }
}

// every observation is 0, 1 or NaN (missing)
__global__ void __launch_bounds__(256) k_probit_check_y(const double* y, long long n, int* status) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = y[i];
        bad = bad || !(v == 0.0 || v == 1.0 || v != v);
    }
    if (bad) atomicOr(status, ST_PROBIT_BAD_Y);
}

}  // namespace rxhip
#endif

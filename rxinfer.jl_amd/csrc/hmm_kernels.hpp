// hmm_kernels.hpp — batched variational message passing for the hidden Markov model with unknown transition and observation matrices, on gfx950.
//
// Reference model (test/models/statespace/hmm_tests.jl:8-24), for each of n_series independent series:
//     A ~ DirichletCollection(prior_A)     K×K, A[i,j] = p(s_t = i | s_{t-1} = j): each COLUMN j is one Dirichlet
//     B ~ DirichletCollection(prior_B)     M×K, B[m,i] = p(x_t = m | s_t = i):     each column one Dirichlet
//     s_0 ~ Categorical(prior_s0);   s_t ~ DiscreteTransition(s_{t-1}, A);   x_t ~ DiscreteTransition(s_t, B)       t = 1 … T
//     q(s_0 … s_T, A, B) = q(s_0 … s_T) q(A) q(B)
// x_t is a symbol code 0 … M−1 stored as a double, NaN = missing.  2 ≤ K ≤ 16, 2 ≤ M ≤ 64.  Reference rules replaced (bodies in the un-vendored
// ReactiveMP.jl): DiscreteTransition(:out | :in | :a) under the structured factorisation above, the Categorical prior, the DirichletCollection
// prior / product, their average energies and the Bethe free energy.
//
// One ITERATION of this engine is a defined semantic, not the reactive engine's update order:
//   1. expected-log tables from the current counts: lA[i,j] = ψ(a[i,j]) − ψ(Σ_i a[i,j]), lB likewise; Ã = exp lA, B̃ = exp lB;
//   2. scaled forward–backward over s_0 … s_T with the weights π, Ã and B̃[x_t, ·] (a missing step has factor 1):
//         α̂_0 = π;   v = B̃[x_t,·] ∘ (Ã α̂_{t-1}),  c_t = Σ v,  α̂_t = v / c_t;   log Z̃ = Σ_t log c_t          (added in time order)
//         β̂_T = 1;   w = B̃[x_t,·] ∘ β̂_t,  b = Ãᵀ w,  d = α̂_{t-1}·b,  ξ_t[i,j] = w[i] Ã[i,j] α̂_{t-1}[j] / d,  β̂_{t-1} = b / d;   γ_t = α̂_t ∘ β̂_t
//      and from them the statistics N[i,j] = Σ_t ξ_t[i,j] and Mstat[m,i] = Σ_{t: x_t = m} γ_t[i];
//   3. a ← prior_A + N, b ← prior_B + Mstat  (with shared parameters N and Mstat are first summed over the series in ascending order).
// The posteriors OF ITERATION i are (γ, a, b) after step 3; its free energy is the Bethe free energy at exactly that point,
//     F = −log Z̃ + Σ N∘(lA_old − lA_new) + Σ Mstat∘(lB_old − lB_new) + KL(q_new(A)‖p(A)) + KL(q_new(B)‖p(B))       (KL summed over columns)
// — q(s) is the exact posterior under the old tables, so −log Z̃ is its energy minus entropy there, and the two sums move the tables to the new
// counts; nothing per step is needed beyond what step 2 reduces (tests/hmm_ref.py holds this against U − H term by term).  With shared
// parameters the per-series part is −log Z̃ + the two sums and the KL terms enter the total once.  Per-iteration values depend on this order;
// the fixed point is the reference's (60.6144 on its data, asserted there as 60.614480654 ± 0.01).
//
// Schedule.  A series is sequential in time, series are independent.  k_hmm_sweep<R> gives a series a ROW of R lanes, R the power of two ≥ K:
// lane i holds row i and column i of Ã (2R doubles) and α̂[i] or β̂[i]; a wavefront carries 64/R series.  The mat-vec of a step broadcasts the
// K values of the row by shuffles inside the row, the normaliser is a butterfly over the row (every lane of a row ends with the same bits).
// The forward loop stores α̂ as [step][series][K]; the backward loop reads it back, forms γ and the lane's row of ξ, accumulates N[i,·] in
// registers and Mstat[·,i] in an LDS array indexed by the symbol (the lane's own cells: no other lane touches them).  Every (series, state) has
// one owner that adds in time order: results are bit-identical run to run and do not depend on which other series are in the batch.  γ goes
// to global memory only on the sweep whose posteriors are read (the last).  The observation and its B̃ row are loaded one and two steps ahead.
// k_hmm_tables / k_hmm_update give a thread one Dirichlet column (its digammas, log-gammas, exp); k_hmm_fe a thread per series.
// Range: the sweep is in the linear domain with one normaliser per step, so it refuses (status bit, RXHIP_ERR_NONFINITE_FE) a run in which a
// normaliser falls to hmm::kMinNormaliser or below, where entries of Ã, B̃ have underflowed; the update forms the KL terms from the statistics
// themselves (hmm::lgamma_diff), so the free energy keeps its digits at counts of 1e9 (tests/test_hmm_contract_*.py).
// Bytes per (series, step, iteration): x read twice (16), α̂ written and read (16·K); γ (8·K) on the last sweep only.
//
// The per-column and per-state arithmetic is `__host__ __device__` and self-contained (only digamma.hpp), floating-point contraction off: the
// same functions compile for the host (tests/host_emul/hmm_main.cpp), and a run with and without the free energy gives bit-identical posteriors.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "digamma.hpp"

#if defined(__clang__)
#define HMM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HMM_NO_CONTRACT
#endif
#define HMM_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace hmm {

constexpr int kMaxK = 16, kMaxM = 64;

// A sweep whose normaliser c_t or d_t is at or below this is refused (k_hmm_sweep).  Ã = exp(ψ(c) − ψ(Σc)) is about exp(−1/c) at small counts and
// reaches the denormal range when 1/c nears 700: a denormal entry has lost digits but is still positive, and the sums it enters come out finite
// and wrong.  The smallest normal double is 2.2e-308, so with a normaliser above 1e-200 a term lost to underflow is below 1e-108 of the sum it
// belongs to.  Measured: every silently wrong run found had a normaliser of 2.8e-234 or less.
constexpr double kMinNormaliser = 1e-200;

// lnΓ(p + n) − lnΓ(p), n ≥ 0, without forming either: from p = 64 on by Stirling's series,
//     (p − ½)·log1p(n/p) + n·(ln(p + n) − 1) + S(p + n) − S(p),   S(x) = 1/(12x) − 1/(360x³) + 1/(1260x⁵) − 1/(1680x⁷)
// (the next term of S is below 1/(1188·64⁹) = 5e-20); below 64 the two log-gammas are O(100) and their plain difference keeps its digits.
constexpr double kLgammaDiffFrom = 64.0;
HMM_HD double stirling_tail(double x) {
    HMM_NO_CONTRACT
    const double r = 1.0 / x, r2 = r * r;
    return r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
}
HMM_HD double lgamma_diff(double p, double n) {
    HMM_NO_CONTRACT
    const double c = p + n;
    if (p < kLgammaDiffFrom) return lgamma(c) - lgamma(p);
    return (p - 0.5) * log1p(n / p) + n * (log(c) - 1.0) + (stirling_tail(c) - stirling_tail(p));
}

// One Dirichlet column (n counts, `stride` doubles apart): expected logs l[i] = ψ(c_i) − ψ(Σc) and their exponentials t[i]; returns
// KL(Dir(c) ‖ Dir(p)) = lnΓ(Σc) − lnΓ(Σp) − Σ(lnΓ(c_i) − lnΓ(p_i)) + Σ(c_i − p_i)·l[i].
// `st`: the statistics the counts were updated with (c_i = p_i + st_i bit for bit), or nullptr (the initial counts of a run, whose KL enters no
// free energy).  With them the KL term takes c_i − p_i and the log-gamma differences from st_i itself: at counts of 1e12, c_i − p_i has lost
// the digits of a statistic of 10, and lnΓ(c_i) − lnΓ(p_i) is a difference of numbers near 1e13 whose sum over the column is O(1).
HMM_HD double column_table(const double* cnt, const double* pri, const double* st, int n, int stride, double* l, double* t) {
    HMM_NO_CONTRACT
    double sc = 0.0, sp = 0.0, ss = 0.0;
    for (int i = 0; i < n; ++i) {
        sc += cnt[i * stride];
        sp += pri[i * stride];
        if (st) ss += st[i * stride];
    }
    const double dsum = digamma_dev(sc);
    double kl = st ? lgamma_diff(sp, ss) : lgamma(sc) - lgamma(sp);
    for (int i = 0; i < n; ++i) {
        const double c = cnt[i * stride], p = pri[i * stride];
        const double li = digamma_dev(c) - dsum;
        l[i * stride] = li;
        t[i * stride] = exp(li);
        if (st) kl += st[i * stride] * li - lgamma_diff(p, st[i * stride]);
        else kl += (c - p) * li - (lgamma(c) - lgamma(p));
    }
    return kl;
}

// Σ_j a[j]·b[j] in ascending j over a padded row (entries beyond K are zero)
template <int R>
HMM_HD double dot(const double* a, const double* b) {
    HMM_NO_CONTRACT
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) s += a[j] * b[j];
    return s;
}
// forward, state i: v[i] = B̃[x_t,i]·Σ_j Ã[i,j] α̂_{t-1}[j]   (arow: row i of Ã, al: the row's α̂_{t-1}); the row then divides by c_t = Σ_i v[i]
template <int R>
HMM_HD double forward_state(const double* arow, const double* al, double f) {
    HMM_NO_CONTRACT
    return f * dot<R>(arow, al);
}
// backward, state i: β̃_{t-1}[i] = Σ_j Ã[j,i]·w[j], w = B̃[x_t,·] ∘ β̂_t   (acol: column i of Ã, wl: the row's w); the row then divides by d = α̂_{t-1}·β̃_{t-1}
template <int R>
HMM_HD double backward_state(const double* acol, const double* wl) {
    HMM_NO_CONTRACT
    return dot<R>(acol, wl);
}
// … and row i of ξ_t added to row i of N:  N[i,j] += Ã[i,j]·α̂_{t-1}[j]·(w[i]/d)
template <int R>
HMM_HD void accumulate_xi(double* nrow, const double* arow, const double* al, double w_over_d) {
    HMM_NO_CONTRACT
#pragma unroll
    for (int j = 0; j < R; ++j) nrow[j] += arow[j] * al[j] * w_over_d;
}
// the symbol of an observed step as a table row; the data were checked (k_hmm_check_x), the clamp keeps a stray value inside the table anyway
HMM_HD int symbol(double x, int M) {
    return x >= (double)M ? M - 1 : x > 0.0 ? (int)x : 0;
}

}  // namespace hmm
}  // namespace rxhip

#if defined(__HIPCC__)
namespace rxhip {

constexpr int ST_HMM_BAD_X = 8;   // status bit of k_hmm_check_x (next to ST_NOT_POSDEF = 1, ST_NONFINITE = 2, ST_PROBIT_BAD_Y = 4)

struct HmmParams {
    long long T, n_series;
    int K, M, shared;
    const double* x;        // [T][series]
    const double* pi;       // [K]
    // per parameter set g (one per series, or one when shared), KM = (K + M)·K doubles each: the K×K block of A, then the M×K block of B, row-major
    const double *prior, *init;
    double* counts;
    double* ltab;           // [2][G][KM] expected logs, ping-pong: the iteration's old and new tables
    double* ttab;           // [G][KM] Ã | B̃
    double* kl;             // [G][2K] KL of every column (A's K columns, then B's)
    double* alpha;          // [T+1][series][K]
    double* gamma;          // [T+1][series][K]
    double* stat;           // [series][KM] N | Mstat of the running sweep
    double* stat_sum;       // [KM] their sum over series (shared parameters)
    double* logz;           // [series]
    double* fe_series;      // [iterations][series]
    int* status;
};

template <int R>
__device__ __forceinline__ double hmm_row_sum(double v) {
    HMM_NO_CONTRACT
#pragma unroll
    for (int off = R / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, R);
    return v;   // the same bits in every lane of the row
}

// Tables (and KL terms) of every Dirichlet column from the initial counts (FROM_STATS = false: the start of a run) or from prior + statistics
// (true: step 3 of an iteration).  Thread = (parameter set, column); `cur` selects the half of ltab that is written.
template <bool FROM_STATS>
__device__ __forceinline__ void hmm_column_thread(const HmmParams& p, int cur) {
    HMM_NO_CONTRACT
    const long long G = p.shared ? 1 : p.n_series, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int K = p.K, M = p.M, KM = (K + M) * K;
    if (idx >= G * 2 * K) return;
    const long long g = idx / (2 * K);
    const int c = (int)(idx % (2 * K));
    const bool isB = c >= K;
    const int n = isB ? M : K;
    const long long in_set = (isB ? K * K : 0) + (isB ? c - K : c), off = g * KM + in_set;
    double* cnt = p.counts + off;
    const double* st = FROM_STATS ? (p.shared ? p.stat_sum : p.stat + g * KM) + in_set : nullptr;
    if (FROM_STATS) {
        for (int i = 0; i < n; ++i) cnt[i * K] = p.prior[off + i * K] + st[i * K];
    } else {
        for (int i = 0; i < n; ++i) cnt[i * K] = p.init[off + i * K];
    }
    const double kl = hmm::column_table(cnt, p.prior + off, st, n, K, p.ltab + (long long)cur * G * KM + off, p.ttab + off);
    p.kl[idx] = kl;
    if (!(kl - kl == 0.0)) atomicOr(p.status, 2);   // ST_NONFINITE
}
__global__ void __launch_bounds__(256) k_hmm_tables(HmmParams p, int cur) { hmm_column_thread<false>(p, cur); }
__global__ void __launch_bounds__(256) k_hmm_update(HmmParams p, int cur) { hmm_column_thread<true>(p, cur); }

// shared parameters: N | Mstat summed over the series in ascending order, a thread per entry
__global__ void __launch_bounds__(256) k_hmm_reduce(HmmParams p) {
    HMM_NO_CONTRACT
    const int KM = (p.K + p.M) * p.K, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= KM) return;
    double acc = p.stat[e];
    for (long long s = 1; s < p.n_series; ++s) acc += p.stat[s * KM + e];
    p.stat_sum[e] = acc;
}

// One forward–backward sweep: a row of R lanes per series, 64/R series per wavefront (one wavefront per block).  OUT: store γ.
// Dynamic LDS: 64·M doubles, the rows' Mstat tables [series in wave][M][R].
template <int R, bool OUT>
__global__ void __launch_bounds__(64) k_hmm_sweep(HmmParams p) {
    HMM_NO_CONTRACT
    extern __shared__ double hmm_lds[];
    constexpr int SPW = 64 / R;
    const int lane = threadIdx.x, i = lane & (R - 1), r = lane / R;
    const long long C = p.n_series, T = p.T;
    const int K = p.K, M = p.M, KM = (K + M) * K;
    // a row beyond the batch repeats the last series (the shuffles stay uniform, every load stays in bounds) and stores nothing; so does a lane beyond K
    const long long s_raw = (long long)blockIdx.x * SPW + r;
    const bool live = s_raw < C, act = i < K, mine = live && act;
    const long long s = live ? s_raw : C - 1;
    const int ic = act ? i : K - 1;
    const double* At = p.ttab + (p.shared ? 0 : s * KM);
    const double* Bt = At + K * K;
    double arow[R], acol[R], nrow[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int jc = j < K ? j : K - 1;
        const double ar = At[ic * K + jc], ac = At[jc * K + ic];
        arow[j] = act && j < K ? ar : 0.0;
        acol[j] = act && j < K ? ac : 0.0;
        nrow[j] = 0.0;
    }
    double* ms = hmm_lds + (long long)r * M * R + i;   // Mstat[m][i] of this row at ms[m·R]
    for (int m = 0; m < M; ++m) ms[m * R] = 0.0;
    auto factor = [&](double xv) { return act ? (xv == xv ? Bt[hmm::symbol(xv, M) * K + ic] : 1.0) : 0.0; };
    const double* xs = p.x + s;                         // x_t at xs[(t − 1)·C]
    double* al_s = p.alpha + s * K + ic;                // α̂_t[i] at al_s[t·C·K]
    const long long CK = C * K;
    bool bad = false;

    // forward: a = α̂_t[i]
    double a = act ? p.pi[ic] : 0.0;
    if (mine) al_s[0] = a;
    double logz = 0.0;
    double f1 = factor(xs[0]);                          // factor of step t + 1, the observation of step t + 2
    double x2 = T >= 2 ? xs[C] : 0.0;
    for (long long t = 1; t <= T; ++t) {
        const double f = f1;
        if (t < T) f1 = factor(x2);
        if (t + 1 < T) x2 = xs[(t + 1) * C];
        double al[R];
#pragma unroll
        for (int j = 0; j < R; ++j) al[j] = __shfl(a, j, R);
        const double v = hmm::forward_state<R>(arow, al, f);
        const double c = hmm_row_sum<R>(v);
        bad = bad || !(c > hmm::kMinNormaliser) || !(c - c == 0.0);
        a = v / c;
        logz += log(c);
        if (mine) al_s[t * CK] = a;
    }

    // backward: b = β̂_t[i]; the factor of step t − 1 and α̂_{t-1} are loaded a step ahead
    double b = 1.0;
    double xt = xs[(T - 1) * C];
    double f = factor(xt);
    double ap = al_s[(T - 1) * CK];                     // α̂_{t-1}[i]: the lane's own store of the forward loop
    double xp = T >= 2 ? xs[(T - 2) * C] : 0.0;
    for (long long t = T; t >= 1; --t) {
        double fp = 0.0, app = 0.0, xpp = 0.0;
        if (t >= 2) {
            fp = factor(xp);
            app = al_s[(t - 2) * CK];
            if (t >= 3) xpp = xs[(t - 3) * C];
        }
        const double gam = a * b;
        if (OUT && mine) p.gamma[t * CK + s * K + i] = gam;
        if (xt == xt) ms[hmm::symbol(xt, M) * R] += gam;
        const double w = f * b;
        const double am = act ? ap : 0.0;               // (a lane beyond K read a valid address, not a value of its own)
        double wl[R], al[R];
#pragma unroll
        for (int j = 0; j < R; ++j) { wl[j] = __shfl(w, j, R); al[j] = __shfl(am, j, R); }
        const double bt = hmm::backward_state<R>(acol, wl);
        const double d = hmm_row_sum<R>(am * bt);
        bad = bad || !(d > hmm::kMinNormaliser) || !(d - d == 0.0);
        hmm::accumulate_xi<R>(nrow, arow, al, w / d);
        b = bt / d;
        a = am; f = fp; xt = xp; ap = app; xp = xpp;
    }
    if (mine) {
        if (OUT) p.gamma[s * K + i] = a * b;
        double* st = p.stat + s * KM;
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (j < K) st[i * K + j] = nrow[j];
        for (int m = 0; m < M; ++m) st[K * K + m * K + i] = ms[m * R];
        if (i == 0) p.logz[s] = logz;
        if (bad) atomicOr(p.status, 32);   // ST_HMM_UNDERFLOW (engine.hpp): a normaliser at or below hmm::kMinNormaliser, or not finite
    }
}

// per-series part of the free energy of iteration `it`: −log Z̃ + Σ N∘(lA_old − lA_new) + Σ Mstat∘(lB_old − lB_new), + the KL terms of the
// series' own columns unless the parameters are shared.  `cur` is the half of ltab with the NEW tables.
__global__ void __launch_bounds__(256) k_hmm_fe(HmmParams p, int it, int cur) {
    HMM_NO_CONTRACT
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n_series) return;
    const long long G = p.shared ? 1 : p.n_series, g = p.shared ? 0 : s;
    const int KM = (p.K + p.M) * p.K;
    const double *ln = p.ltab + ((long long)cur * G + g) * KM, *lo = p.ltab + ((long long)(1 - cur) * G + g) * KM, *st = p.stat + s * KM;
    double f = -p.logz[s];
    for (int e = 0; e < KM; ++e) f += st[e] * (lo[e] - ln[e]);
    if (!p.shared)
        for (int c = 0; c < 2 * p.K; ++c) f += p.kl[s * 2 * p.K + c];
    p.fe_series[(long long)it * p.n_series + s] = f;
}
// … and the total: the series in a fixed tree, + the KL terms once when the parameters are shared
__global__ void __launch_bounds__(256) k_hmm_fe_total(HmmParams p, int it, double* fe_total) {
    HMM_NO_CONTRACT
    __shared__ double sh[256];
    double acc = 0.0;
    for (long long s = threadIdx.x; s < p.n_series; s += 256) acc += p.fe_series[(long long)it * p.n_series + s];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int wd = 128; wd > 0; wd >>= 1) {
        if ((int)threadIdx.x < wd) sh[threadIdx.x] += sh[threadIdx.x + wd];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double f = sh[0];
        if (p.shared)
            for (int c = 0; c < 2 * p.K; ++c) f += p.kl[c];
        fe_total[it] = f;
        if (!(f - f == 0.0)) atomicOr(p.status, 2);   // ST_NONFINITE
    }
}

// every observation is an integer code 0 … M−1 or NaN (missing)
__global__ void __launch_bounds__(256) k_hmm_check_x(const double* x, long long n, int M, int* status) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = x[i];
        bad = bad || !(v != v || (v >= 0.0 && v < (double)M && v == floor(v)));
    }
    if (bad) atomicOr(status, ST_HMM_BAD_X);
}

}  // namespace rxhip
#endif

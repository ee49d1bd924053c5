// arreg_kernels.hpp — batched Normal-Gamma variational message passing for Bayesian linear regression with unknown coefficients and noise precision,
// and for the autoregression it is when the regressors are the lags of the series itself, on gfx950.
//
// Reference model (test/models/autoregressive/ar_tests.jl:17-46, benchmarked there as "models" "ar"), for each of n_series independent problems (or one
// θ, γ for all of them) with N rows and d = 1 … 32 regressors:
//     γ ~ Gamma(a0, b0);   θ ~ MvNormal(mean = m0, precision = Λ0);   y[i] ~ Normal(mean = dot(x[i], θ), precision = γ);      q(γ, θ) = q(γ) q(θ)
// The data enter through G = Σ x xᵀ, h = Σ y x, s = Σ y², n alone: ONE streaming pass per data set, then d × d work per iteration.
//
// One ITERATION is a defined semantic (include/rxhip.h), from q(γ) = Gamma(a, b), ḡ = a/b:
//   1. Λ = Λ0 + ḡ G,  V = Λ⁻¹,  m = V(Λ0 m0 + ḡ h);
//   2. a = a0 + n/2,  b = b0 + R/2,  R = s − 2 mᵀh + tr((V + m mᵀ) G) with the new θ.
// F = −[n/2 (ψ(a) − ln b − ln 2π) − ½ (a/b) R] + KL(N(m, V) ‖ N(m0, Λ0⁻¹)) + KL(Gamma(a, b) ‖ Gamma(a0, b0)) after step 2.
//
// Schedule.  The pass runs on a grid (chunks, series); `chunks` depends on the number of rows and d only (arreg::chunks), so a series' bits do not
// depend on the batch.  Each workgroup strides over tiles of rows and leaves ONE partial: packed lower triangle of G | h | s | n.  No floating-point
// atomics, fixed summation order.  A row whose y is NaN (regressor mode) or whose window y, x holds a NaN (lagged mode) contributes exact zeros.
//   k_arreg_pass_small<D, LAG>, D = 1 … 4: a lane per row, D(D+1)/2 + D + 2 accumulators, wave_sum, the four wavefronts added in wave order.
//   k_arreg_pass<NT, LAG>, d = 5 … 32, D = 16·NT: G on v_mfma_f64_16x16x4_f64, lower tiles only, A = B = the rows (k = the row inside a group of
//     four, operand lane map A[l&15][k = l>>4], result row (l>>4) + 4r, column l&15); each wavefront contracts its own quarter of the tile into its own
//     accumulators; h, s and n are in-lane sums; the four wavefronts are added in wave order through LDS.
//   LAG = false: X [series][N][d] and y [series][N]; the MFMA kernel stages a tile of X in LDS (leading dimension D + 1).
//   LAG = true: only the series z [T][series]; row i is y = z[i + p], x = (z[i + p − 1], …, z[i]).  A tile's rows plus the halo of p values are staged
//     ONCE in LDS and every operand is read from there at unit-stride offsets (the Hankel structure): no X exists anywhere.
//   k_arreg_iterate: one wavefront per series (one in all when the parameters are shared), ONE launch for the whole run: partials in ascending chunk
//     (and series) order with 32 loads in flight ahead of the adds, then every iteration — Λ, the Cholesky inverse with log-determinant
//     (mvd_chol_inv), m, R, a, b, F and the iteration's entry of the history.
// Bytes: 8·T per series in lagged mode, 8·N·(d + 1) in regressor mode; flops on the matrix path 2·N·D² nominal.
//
// Numerical envelope: R is formed from s, h and G, so its relative error is about ε·s/R; data whose residual is below 1e-8 of their energy are
// outside the contract.
//
// The schedule constants and the assembly of R, the two KL terms and F are `__host__ __device__`, floating-point contraction off: the same functions
// compile for the host (tests/host_emul/arreg_main.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#if defined(__clang__)
#define ARREG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define ARREG_NO_CONTRACT
#endif
#define ARREG_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace arreg {

constexpr int kMaxD = 32;          // largest number of regressors / largest order (two column tiles)
constexpr int kSmallMaxD = 4;      // … of the lane-per-row path
constexpr int kSmallTile = 256;    // rows a workgroup of the lane path takes per step
constexpr int kSmallCap = 2048;    // its largest number of chunks
constexpr int kMfmaTile = 128;     // rows per tile of the matrix-core path: 4 wavefronts × 8 groups of 4
constexpr int kMfmaCap = 512;      // its largest number of chunks

ARREG_HD int tile_rows(int d) { return d <= kSmallMaxD ? kSmallTile : kMfmaTile; }
// workgroups per series: one per tile up to the cap, at least one (a series without rows still gets its zero partial); a function of rows and d ONLY
ARREG_HD int chunks(long long rows, int d) {
    const long long tp = tile_rows(d), tiles = (rows + tp - 1) / tp, cap = d <= kSmallMaxD ? kSmallCap : kMfmaCap;
    return (int)(tiles < 1 ? 1 : tiles < cap ? tiles : cap);
}
// rows of a lagged series of length T at order p
ARREG_HD long long lag_rows(long long T, int p) { return T > p ? T - p : 0; }
ARREG_HD int ngram(int d) { return d * (d + 1) / 2; }
ARREG_HD int nstat(int d) { return ngram(d) + d + 2; }         // the statistics: packed lower triangle of G | h [d] | s | n
ARREG_HD int nhist(int d) { return d + d * d + 2; }            // an entry of the history: m [d] | V [d][d] | a | b
// the engine's constants: Λ0 [d][d] | m0 [d] | Λ0 m0 [d] | a0, b0, initial a, initial b, ln det Λ0, lnΓ(a0), ln b0
ARREG_HD int nconst(int d) { return d * d + 2 * d + 7; }

// R = Σ (y − xᵀθ)² under q(θ) from the statistics: s − 2 mᵀh + tr((V + m mᵀ) G)
ARREG_HD double residual(double s, double mh, double tr_sg) {
    ARREG_NO_CONTRACT
    return s - 2.0 * mh + tr_sg;
}
// KL(N(m, V) ‖ N(m0, Λ0⁻¹)) from tr(Λ0 V), (m − m0)ᵀΛ0(m − m0), ln det Λ0, ln det V
ARREG_HD double normal_kl(double tr_l0v, double quad0, int d, double logdet_l0, double logdet_v) {
    ARREG_NO_CONTRACT
    return 0.5 * (tr_l0v + quad0 - (double)d - logdet_l0 - logdet_v);
}
// KL(Gamma(a, b) ‖ Gamma(a0, b0)), shape–rate (the expression of the latent autoregressive engine); exactly 0 at a = a0, b = b0
ARREG_HD double gamma_kl(double a, double b, double a0, double b0, double psi_a, double lgamma_a, double lgamma_a0, double log_b, double log_b0) {
    ARREG_NO_CONTRACT
    return (a - a0) * psi_a - lgamma_a + lgamma_a0 + a0 * (log_b - log_b0) + a * (b0 - b) / b;
}
ARREG_HD double free_energy(double n, double a, double b, double R, double psi_a, double log_b, double kl_theta, double kl_gamma) {
    ARREG_NO_CONTRACT
    const double log_2pi = 1.8378770664093454836;
    return -(0.5 * n * (psi_a - log_b - log_2pi) - 0.5 * (a / b) * R) + kl_theta + kl_gamma;
}

}  // namespace arreg
}  // namespace rxhip

#if defined(__HIPCC__)
#include "digamma.hpp"
#include "mvgmm_dense_kernels.hpp"

namespace rxhip {

struct ArregParams {
    long long N;                     // rows per series as the pass counts them: N (regressor mode), max(T − p, 0) (lagged mode)
    long long T, C;                  // lagged mode: length of a series; series
    int d, nchunk, shared, want_fe, iterations;
    const double* X;                 // regressor mode: [C][N][d]
    const double* y;                 // regressor mode: [C][N]; lagged mode: the series z [T][C]
    const double* cst;               // arreg::nconst(d)
    double* part;                    // [C][nchunk][nstat]
    double* hist;                    // [iterations][G][nhist], G = C or 1 (shared)
    double* fe;                      // [iterations][G]
    double* fe_total;                // [iterations]
    double* fe_chain;                // [C]: F of the last iteration per group (shared: entry 0)
    int* status;
};

template <int D, bool LAG>
__global__ void __launch_bounds__(256) k_arreg_pass_small(ArregParams p) {
    ARREG_NO_CONTRACT
    constexpr int NG = D * (D + 1) / 2, NS = NG + D + 2, TP = arreg::kSmallTile;
    __shared__ double red[4][NS];
    __shared__ double zs[LAG ? TP + D : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long ser = blockIdx.y, N = p.N;
    const double* X = LAG ? nullptr : p.X + ser * N * D;
    const double* Y = LAG ? p.y + ser : p.y + ser * N;
    double acc[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) acc[q] = 0.0;
    for (long long base = (long long)blockIdx.x * TP; base < N; base += (long long)gridDim.x * TP) {
        const long long i = base + tid;
        double x[D], yv = 0.0;
        bool ok = i < N;
        if constexpr (LAG) {
            __syncthreads();   // the previous tile has been read
            for (int j = tid; j < TP + D; j += 256) {
                const long long t = base + j;
                zs[j] = t < p.T ? Y[t * p.C] : __builtin_nan("");
            }
            __syncthreads();
            yv = zs[tid + D];
            ok = ok && yv == yv;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                x[a] = zs[tid + D - 1 - a];
                ok = ok && x[a] == x[a];
            }
        } else {
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = ok ? X[i * D + a] : 0.0;
            if (ok) yv = Y[i];
            ok = ok && yv == yv;
        }
        if (!ok) {
            yv = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) x[a] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < D; ++a) {
#pragma unroll
            for (int b = 0; b <= a; ++b) acc[a * (a + 1) / 2 + b] += x[a] * x[b];
            acc[NG + a] += yv * x[a];
        }
        acc[NG + D] += yv * yv;
        acc[NG + D + 1] += ok ? 1.0 : 0.0;
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) red[w][q] = s;
    }
    __syncthreads();
    if (tid < NS) p.part[((size_t)ser * p.nchunk + blockIdx.x) * NS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

template <int NT, bool LAG>
__global__ void __launch_bounds__(256) k_arreg_pass(ArregParams p) {
    ARREG_NO_CONTRACT
    constexpr int D = 16 * NT, LD = D + 1, NTRI = NT * (NT + 1) / 2, TP = arreg::kMfmaTile, NRED = 4 * NTRI * 256;
    constexpr int NBUF = LAG ? NRED : (TP * LD > NRED ? TP * LD : NRED);
    constexpr int HG = 64 / D, HR = (TP / 4) / HG;   // h: groups of D lanes per wavefront, rows each takes of the wavefront's quarter
    __shared__ double buf[NBUF];            // LAG: the series tile z[base … base + TP + p) (NaN stored as 0); else the tile of X; at the end the reduction
    __shared__ int bad[LAG ? TP + D : 1];   // LAG: the value is NaN or past the end of the series
    __shared__ double yrow[TP], wrow[TP];   // y of the row (0 when the row is dropped), 1 / 0 = the row counts
    __shared__ double hred[4][D], sred[4][2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int d = p.d;
    const long long ser = blockIdx.y, N = p.N;
    const double* X = LAG ? nullptr : p.X + ser * N * d;
    const double* Y = LAG ? p.y + ser : p.y + ser * N;
    // the operand X[row pt of the tile][column c]: zero past column d
    auto xval = [&](int pt, int c) -> double {
        if constexpr (LAG) return c < d ? buf[pt + d - 1 - c] : 0.0;
        else return buf[pt * LD + c];
    };

    mvd_d4 G[NTRI];
#pragma unroll
    for (int q = 0; q < NTRI; ++q) G[q] = (mvd_d4){0.0, 0.0, 0.0, 0.0};
    double hacc = 0.0, sacc = 0.0, nacc = 0.0;
    if constexpr (!LAG) {
        for (int q = tid; q < TP * LD; q += 256) buf[q] = 0.0;
        __syncthreads();
    }

    for (long long base = (long long)blockIdx.x * TP; base < N; base += (long long)gridDim.x * TP) {
        // ---- stage the tile
        const long long left = N - base;
        const int npts = left < TP ? (int)left : TP;
        if constexpr (LAG) {
            for (int j = tid; j < TP + d; j += 256) {
                const long long t = base + j;
                const double v = t < p.T ? Y[t * p.C] : __builtin_nan("");
                const bool isnan_v = !(v == v);
                buf[j] = isnan_v ? 0.0 : v;
                bad[j] = isnan_v ? 1 : 0;
            }
            __syncthreads();
            if (tid < TP) {
                int nb = tid < npts ? 0 : 1;
                for (int c = 0; c <= d; ++c) nb += bad[tid + c];
                const bool ok = nb == 0;
                yrow[tid] = ok ? buf[tid + d] : 0.0;
                wrow[tid] = ok ? 1.0 : 0.0;
            }
        } else {
            const double* xt = X + base * d;
            for (int q = tid; q < TP * d; q += 256) {
                const int pt = q / d, c = q - pt * d;
                buf[pt * LD + c] = q < npts * d ? xt[q] : 0.0;
            }
            if (tid < TP) {
                const double v = tid < npts ? Y[base + tid] : __builtin_nan("");
                const bool ok = v == v;
                yrow[tid] = ok ? v : 0.0;
                wrow[tid] = ok ? 1.0 : 0.0;
            }
        }
        __syncthreads();

        // ---- s, n: a lane per row;  h: a lane per (column, group of rows) of the wavefront's quarter
        if (tid < TP) {
            const double v = yrow[tid];
            sacc += v * v;
            nacc += wrow[tid];
        }
        {
            const int c = lane & (D - 1), g = lane / D;
#pragma unroll 4
            for (int r = 0; r < HR; ++r) {
                const int pt = (TP / 4) * w + g + HG * r;
                hacc += yrow[pt] * xval(pt, c);   // yrow is 0 for a dropped row
            }
        }
        // ---- G += Xᵀ X over the quarter of the tile this wavefront owns; a dropped row enters with weight 0 on the A side
#pragma unroll 2
        for (int kk = 0; kk < TP / 16; ++kk) {
            const int pt = (TP / 4) * w + 4 * kk + lq;
            const double wv = wrow[pt];
            double xv[NT], a[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                xv[t] = xval(pt, 16 * t + lr);
                a[t] = wv * xv[t];
            }
#pragma unroll
            for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                for (int tb = 0; tb <= ta; ++tb) G[ta * (ta + 1) / 2 + tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], xv[tb], G[ta * (ta + 1) / 2 + tb], 0, 0, 0);
        }
        __syncthreads();   // the next tile overwrites buf / yrow / wrow
    }

    // ---- the four wavefronts' accumulators, added in wave order through LDS
    double* red = buf;
#pragma unroll
    for (int q = 0; q < NTRI; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((w * NTRI + q) * 4 + r) * 64 + lane] = G[q][r];
#pragma unroll
    for (int off = D; off < 64; off <<= 1) hacc += __shfl_xor(hacc, off);   // the groups of rows, fixed order
    if (lane < D) hred[w][lane] = hacc;
    {
        const double a = wave_sum(sacc), b = wave_sum(nacc);
        if (lane == 0) { sred[w][0] = a; sred[w][1] = b; }
    }
    __syncthreads();
    const int NGR = arreg::ngram(d), NS = arreg::nstat(d);
    double* part = p.part + ((size_t)ser * p.nchunk + blockIdx.x) * NS;
    for (int e = tid; e < NTRI * 256; e += 256) {
        const int q = e >> 8, r = (e >> 6) & 3, ln = e & 63;
        const double s = ((red[e] + red[NTRI * 256 + e]) + red[2 * NTRI * 256 + e]) + red[3 * NTRI * 256 + e];
        const int ta = q == 0 ? 0 : 1, tb = q == 2 ? 1 : 0;
        const int a = 16 * ta + (ln >> 4) + 4 * r, b = 16 * tb + (ln & 15);
        if (a < d && b <= a) part[a * (a + 1) / 2 + b] = s;
    }
    if (tid < d) part[NGR + tid] = ((hred[0][tid] + hred[1][tid]) + hred[2][tid]) + hred[3][tid];
    if (tid < 2) part[NGR + d + tid] = ((sred[0][tid] + sred[1][tid]) + sred[2][tid]) + sred[3][tid];
}

// The whole run of one group (a series, or all of them when the parameters are shared) on one wavefront: the statistics from the partials, then every
// iteration.  Nothing depends on want_fe but the free-energy stores.
static __global__ void __launch_bounds__(64) k_arreg_iterate(ArregParams p) {
    ARREG_NO_CONTRACT
    __shared__ double A[MVD_DMAX * MVD_LDM], Wk[MVD_DMAX * MVD_LDM], Gm[MVD_DMAX * MVD_LDM];
    __shared__ double tot[MVD_DMAX * (MVD_DMAX + 1) / 2 + MVD_DMAX + 2], m[MVD_DMAX], m0[MVD_DMAX], wm0[MVD_DMAX];
    const int t = threadIdx.x, d = p.d, dd = d * d, NGR = arreg::ngram(d), NS = arreg::nstat(d), NH = arreg::nhist(d);
    const long long grp = blockIdx.x, ngrp = p.shared ? 1 : p.C;
    const long long first = p.shared ? 0 : grp, count = p.shared ? p.C : 1;
    // ---- the statistics: chunks in ascending order, 32 loads in flight ahead of the adds; then the series in ascending order
    for (int q = t; q < NS; q += 64) {
        double total = 0.0;
        for (long long s = first; s < first + count; ++s) {
            const double* part = p.part + (size_t)s * p.nchunk * NS;
            double acc = part[q];
            int c = 1;
            for (; c + 32 <= p.nchunk; c += 32) {
                double v[32];
#pragma unroll
                for (int k = 0; k < 32; ++k) v[k] = part[(size_t)(c + k) * NS + q];
#pragma unroll
                for (int k = 0; k < 32; ++k) acc += v[k];
            }
            for (; c < p.nchunk; ++c) acc += part[(size_t)c * NS + q];
            total = s == first ? acc : total + acc;
        }
        tot[q] = total;
    }
    const double *L0 = p.cst, *pm0 = L0 + dd, *pwm0 = pm0 + d, *sc = pwm0 + d;
    const double a0 = sc[0], b0 = sc[1], logdet_l0 = sc[4], lgamma_a0 = sc[5], log_b0 = sc[6];
    if (t < d) {
        m0[t] = pm0[t];
        wm0[t] = pwm0[t];
    }
    __syncthreads();
    for (int q = t; q < dd; q += 64) {
        const int a = q / d, b = q - a * d, lo = a > b ? a : b, hi = a > b ? b : a;
        Gm[a * MVD_LDM + b] = tot[lo * (lo + 1) / 2 + hi];
    }
    const double* h = tot + NGR;
    const double ssq = tot[NGR + d], n = tot[NGR + d + 1];
    const double a = a0 + 0.5 * n;   // the same in every iteration
    double psi_a = 0.0, lgamma_a = 0.0;
    if (p.want_fe) {
        psi_a = digamma_dev(a);
        lgamma_a = lgamma(a);
    }
    double gbar = sc[2] / sc[3];
    __syncthreads();
    for (int it = 0; it < p.iterations; ++it) {
        // ---- 1. q(θ)
        for (int q = t; q < dd; q += 64) {
            const int i = q / d, j = q - i * d;
            A[i * MVD_LDM + j] = L0[q] + gbar * Gm[i * MVD_LDM + j];
        }
        __syncthreads();
        double logdet_l;
        const bool ok = mvd_chol_inv(d, A, Wk, logdet_l);   // A = V
        if (t < d) {
            double s = 0.0;
            for (int j = 0; j < d; ++j) s += A[t * MVD_LDM + j] * (wm0[j] + gbar * h[j]);
            m[t] = s;
        }
        __syncthreads();
        // ---- 2. q(γ) with the new θ
        double tr_sg = 0.0, mh = 0.0, tr_l0v = 0.0, quad0 = 0.0;
        for (int q = t; q < dd; q += 64) {
            const int i = q / d, j = q - i * d;
            const double v = A[i * MVD_LDM + j];
            tr_sg += (v + m[i] * m[j]) * Gm[i * MVD_LDM + j];
            tr_l0v += L0[q] * v;
            quad0 += L0[q] * ((m[i] - m0[i]) * (m[j] - m0[j]));
        }
        if (t < d) mh = m[t] * h[t];
        tr_sg = __shfl(wave_sum(tr_sg), 0);
        mh = __shfl(wave_sum(mh), 0);
        const double R = arreg::residual(ssq, mh, tr_sg);
        const double b = b0 + 0.5 * R;
        double* hs = p.hist + ((size_t)it * ngrp + grp) * NH;
        if (t < d) hs[t] = m[t];
        for (int q = t; q < dd; q += 64) hs[d + q] = A[(q / d) * MVD_LDM + (q - (q / d) * d)];
        if (t == 0) {
            hs[d + dd] = a;
            hs[d + dd + 1] = b;
        }
        if (p.want_fe) {
            tr_l0v = wave_sum(tr_l0v);
            quad0 = wave_sum(quad0);
            if (t == 0) {
                const double log_b = log(b);
                const double F = arreg::free_energy(n, a, b, R, psi_a, log_b, arreg::normal_kl(tr_l0v, quad0, d, logdet_l0, -logdet_l),
                                                    arreg::gamma_kl(a, b, a0, b0, psi_a, lgamma_a, lgamma_a0, log_b, log_b0));
                p.fe[(size_t)it * ngrp + grp] = F;
                if (ngrp == 1) p.fe_total[it] = F;
                if (it == p.iterations - 1) p.fe_chain[grp] = F;
                if (ok && !(F - F == 0.0)) atomicOr(p.status, ST_NONFINITE);
            }
        }
        if (!ok && t == 0) atomicOr(p.status, ST_NOT_POSDEF);
        gbar = a / b;
        __syncthreads();   // A, m are rewritten by the next iteration
    }
}

// the totals of a batch, one workgroup per iteration: the groups in a fixed tree
static __global__ void __launch_bounds__(256) k_arreg_fe_total(ArregParams p) {
    ARREG_NO_CONTRACT
    __shared__ double sh[256];
    const long long ngrp = p.shared ? 1 : p.C;
    const int it = blockIdx.x;
    double acc = 0.0;
    for (long long s = threadIdx.x; s < ngrp; s += 256) acc += p.fe[(size_t)it * ngrp + s];
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

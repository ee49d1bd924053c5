// binreg_kernels.hpp — batched variational message passing for Bayesian binomial (logistic) regression under Pólya-Gamma augmentation, on gfx950.
//
// Reference model (test/models/regression/binomialreg_tests.jl), for each of n_problems independent regressions with N points and d features:
//     β ~ MvNormalWeightedMeanPrecision(ξ0, W0);   y[i] ~ BinomialPolya(x[i], n[i], β):  y_i | β ~ Binomial(n_i, σ(x_iᵀβ))          i = 1 … N
//     q(β, ω) = q(β) Π_i q(ω_i)      (Polson–Scott–Windle augmentation; the mean-field family of Durante–Rigon)
// A NaN y_i is missing and contributes no factor.  κ_i = y_i − n_i/2;  ξ = ξ0 + Σ_obs κ_i x_i and lc = Σ_obs ln C(n_i, y_i) are formed once per data set.
//
// One ITERATION of this engine is a defined semantic (include/rxhip.h), two exact coordinate updates from the current q(β) = N(m, V):
//   1. S = V + m mᵀ,  c_i² = x_iᵀ S x_i,  q(ω_i) = PG(n_i, c_i),  ω̄_i = n_i tanh(c_i/2)/(2 c_i) (→ n_i/4 as c_i → 0),
//      G = Σ_obs ω̄_i x_i x_iᵀ,   P = Σ_obs (−n_i ln(2 cosh(c_i/2)) + ½ c_i² ω̄_i);
//   2. W = W0 + G,  V = W⁻¹,  m = V ξ.
// The posterior OF ITERATION i is q(β) after step 2; the free energy at exactly that point is
//     F = −[lc + mᵀ(ξ − ξ0) − ½ tr((V + m mᵀ) G) + P] + KL(N(m, V) ‖ N(W0⁻¹ξ0, W0⁻¹)),
// exact for q(ω) of step 1 and the new q(β) (Σ ω̄_i x_iᵀ S_new x_i = tr(S_new G): no second pass over X); it cannot rise between iterations.
//
// Schedule.  The pass reads X and n_eff (n_i, 0 where y_i is missing: a point with n_eff = 0 adds exact zeros) on a grid (chunks, problem);
// `chunks` depends on N and d only (breg::chunks), so a problem's bits do not depend on what else is in the batch.  Each workgroup strides over
// tiles of points and leaves ONE partial (packed lower triangle of G, then P).  No floating-point atomics: two runs give the same bits.
//   k_breg_pass_small<D>, D = 1 … 4: a lane per point, S in scalar registers, D(D+1)/2 + 1 accumulators per lane, wave_sum, the four wavefronts
//     added in wave order through LDS.
//   k_breg_pass<NT>, d = 5 … 32, D = 16·NT: on v_mfma_f64_16x16x4_f64, laid out like k_mvgd_pass with one component.  A tile of 128 points is
//     staged in LDS (leading dimension D + 1, zero padded).  C = S·Xᵀ: A operand S[16t + (l&15)][4kk + (l>>4)] loaded ONCE and kept in registers
//     (4 doubles per lane at NT = 1, 16 at NT = 2), B operand x[point = l&15][4kk + (l>>4)]; the lane then holds rows (l>>4) + 4r of its point's
//     column and exactly those entries of x, so c² is an in-lane product and two cross-lane adds.  ω̄ and the P term a lane per point; the Gram update
//     G += (ω̄ ∘ X)ᵀ X with A = ω̄_i x_i, B = x_i on lower tiles only.  Each wavefront contracts its own quarter of the tile's points (the
//     quarter whose ω̄ it has just computed) into its own accumulators; the four are added in wave order through LDS at the end.
//   k_breg_update: one wavefront per problem: partials added in ascending chunk order, W, Cholesky inverse with log-determinant (mvd_chol_inv),
//     m, the next S, F, and the iteration's entry of the parameter history.  k_breg_fe_total adds the problems in a fixed tree.
// Bytes per (point, iteration): 8(d + 1); flops on the matrix path: 4·D² per point.
//
// The arithmetic where this model can go wrong numerically (ω̄ near c = 0, ln 2cosh at large c, the per-point term, the free-energy assembly) and
// the schedule constants are `__host__ __device__` and self-contained, floating-point contraction off: the same functions compile for the host
// (tests/host_emul/binreg_main.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#if defined(__clang__)
#define BREG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BREG_NO_CONTRACT
#endif
#define BREG_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace breg {

constexpr int kMaxD = 32;          // largest number of features (two column tiles)
constexpr int kSmallMaxD = 4;      // … of the lane-per-point path
constexpr int kSmallTile = 256;    // points a workgroup of the lane path takes per step
constexpr int kSmallCap = 2048;    // its largest number of chunks (eight workgroups per CU)
constexpr int kMfmaTile = 128;     // points per tile of the matrix-core path: 4 wavefronts × 2 groups of 16
constexpr int kMfmaCap = 512;      // its largest number of chunks (two workgroups per CU)
// below this c² the series of tanh(c/2)/(2c) replaces the quotient: ¼(1 − u/12 + u²/120 − 17u³/20160 + 31u⁴/362880 − …), u = c²; cut after u³ the
// first omitted term is 8.6e-5·u⁴ ≤ 8.6e-17 relative at u = 1e-3, under half an ulp.  (The quotient itself is accurate for every c > 0; the
// series is there for c = 0 — a zero row of X — and for a c² that rounding left a hair below 0.)
constexpr double kSeriesBelow = 1e-3;

BREG_HD int tile_points(int d) { return d <= kSmallMaxD ? kSmallTile : kMfmaTile; }
// workgroups per problem: one per tile up to the cap; a function of N and d ONLY
BREG_HD int chunks(long long N, int d) {
    const long long tp = tile_points(d), tiles = (N + tp - 1) / tp, cap = d <= kSmallMaxD ? kSmallCap : kMfmaCap;
    return (int)(tiles < cap ? tiles : cap);
}
BREG_HD int dpad(int d) { return d <= kSmallMaxD ? d : (d > 16 ? 32 : 16); }   // leading dimension of S as the pass reads it
BREG_HD int npart(int d) { return d * (d + 1) / 2 + 1; }                        // a partial: packed lower triangle of G | P
// the engine's constants: ξ0[d] | W0[d][d] | m0 = W0⁻¹ξ0 [d] | ln det W0 | initial m [d] | initial V [d][d]
BREG_HD int nconst(int d) { return 2 * d * d + 3 * d + 1; }

// ω̄ = E[ω], ω ~ PG(n, c), from c²: n·tanh(c/2)/(2c); exactly n/4 at c² = 0, no 0/0; NaN propagates
BREG_HD double pg_mean(double n, double c2) {
    BREG_NO_CONTRACT
    const double u = c2 < 0.0 ? 0.0 : c2;
    if (u < kSeriesBelow) return 0.25 * n * (1.0 + u * (-1.0 / 12.0 + u * (1.0 / 120.0 - u * (17.0 / 20160.0))));
    const double c = sqrt(u);
    return n * tanh(0.5 * c) / (2.0 * c);
}
// ln(2 cosh(c/2)), c ≥ 0, as c/2 + log1p(exp(−c)): finite for every finite c
BREG_HD double log_2cosh_half(double c) {
    BREG_NO_CONTRACT
    return 0.5 * c + log1p(exp(-c));
}
// a point's ω̄ (returned through w) and its term of P: −n ln(2 cosh(c/2)) + ½ c² ω̄; both are exact zeros at n = 0.  The two functions above in
// one, sharing their transcendentals: with h = expm1(−c) ∈ (−1, 0], tanh(c/2) = −h/(2 + h) (no cancellation as c → 0, which 1 − exp(−c) would
// have) and ln(2 cosh(c/2)) = c/2 + ln(2 + h) (the argument lies in (1, 2]; at c = 1500 h = −1 and the logarithm is 0): one square root, one
// expm1, one logarithm and one division per point instead of a tanh, an exp, a log1p and two divisions.
BREG_HD double point_term(double n, double c2, double& w) {
    BREG_NO_CONTRACT
    const double u = c2 < 0.0 ? 0.0 : c2;
    const double c = sqrt(u), h = expm1(-c), q = 2.0 + h;
    const double series = 0.25 * n * (1.0 + u * (-1.0 / 12.0 + u * (1.0 / 120.0 - u * (17.0 / 20160.0))));
    const bool small = u < kSeriesBelow;
    const double quot = n * -h / (small ? 1.0 : 2.0 * c * q);        // (no 0/0 at c = 0: the series is taken there, and the divisor is 1)
    w = small ? series : quot;
    return -n * (0.5 * c + log(q)) + 0.5 * u * w;
}
// F from its sums: lc, mᵀ(ξ − ξ0), tr((V + m mᵀ) G), P, tr(W0 V), (m − m0)ᵀW0(m − m0), ln det W0, ln det V
BREG_HD double free_energy(double lc, double m_dxi, double tr_sg, double P, double tr_w0v, double quad0, int d, double logdet_w0, double logdet_v) {
    BREG_NO_CONTRACT
    const double kl = 0.5 * (tr_w0v + quad0 - (double)d - logdet_w0 - logdet_v);
    return -(lc + m_dxi - 0.5 * tr_sg + P) + kl;
}

}  // namespace breg
}  // namespace rxhip

#if defined(__HIPCC__)
#include "mvgmm_dense_kernels.hpp"

namespace rxhip {

struct BregParams {
    long long N, C;                  // points per problem, problems
    int d, nchunk, nchunk_xi, want_fe;
    const double* X;                 // [C][N][d]
    const double* neff;              // [C][N]: n_i, 0 where y_i is missing
    const double* kappa;             // [C][N]: y_i − n_i/2, 0 where y_i is missing
    const double* cst;               // breg::nconst(d)
    double* xi;                      // [C][d]
    const double* lc;                // [C]
    double* S;                       // [C][dpad][dpad]: V + m mᵀ of the current q(β), zero padded
    double* part;                    // [C][nchunk][npart]
    double* xi_part;                 // [C][nchunk_xi][32]
    double *hist_m, *hist_v;         // [iterations][C][d], [iterations][C][d][d]
    double* fe_prob;                 // [iterations][C]
    int* status;
};

constexpr int BREG_XI_ROWS = 8;      // k_breg_xi: 8 rows of 32 feature columns per workgroup step

// ξ = ξ0 + Σ κ_i x_i, once per data set: per-chunk partials over 8 rows × 32 columns, rows added in ascending order …
static __global__ void __launch_bounds__(256) k_breg_xi(BregParams p) {
    BREG_NO_CONTRACT
    __shared__ double red[BREG_XI_ROWS][32];
    const int c = threadIdx.x & 31, r = threadIdx.x >> 5, d = p.d;
    const long long prob = blockIdx.y, N = p.N;
    const double* X = p.X + prob * N * d;
    const double* kp = p.kappa + prob * N;
    double acc = 0.0;
    if (c < d)
        for (long long i = (long long)blockIdx.x * BREG_XI_ROWS + r; i < N; i += (long long)gridDim.x * BREG_XI_ROWS) acc += kp[i] * X[i * d + c];
    red[r][c] = acc;
    __syncthreads();
    if (r == 0) {
        double s = red[0][c];
        for (int q = 1; q < BREG_XI_ROWS; ++q) s += red[q][c];
        p.xi_part[((size_t)prob * p.nchunk_xi + blockIdx.x) * 32 + c] = s;
    }
}
// … and the chunks in ascending order, a thread per (problem, feature)
static __global__ void __launch_bounds__(256) k_breg_xi_total(BregParams p) {
    BREG_NO_CONTRACT
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= p.C * p.d) return;
    const long long prob = e / p.d;
    const int c = (int)(e - prob * p.d);
    const double* part = p.xi_part + (size_t)prob * p.nchunk_xi * 32 + c;
    double s = p.cst[c];
    for (int q = 0; q < p.nchunk_xi; ++q) s += part[(size_t)q * 32];
    p.xi[e] = s;
}

// every run starts from the initial q(β): S = V + m mᵀ, zero padded to the pass's leading dimension
static __global__ void __launch_bounds__(64) k_breg_init(BregParams p) {
    BREG_NO_CONTRACT
    const int d = p.d, DP = breg::dpad(d);
    const double *m = p.cst + 2 * d + d * d + 1, *V = m + d;
    double* S = p.S + (size_t)blockIdx.x * DP * DP;
    for (int q = threadIdx.x; q < DP * DP; q += 64) {
        const int i = q / DP, j = q - i * DP;
        S[q] = (i < d && j < d) ? V[i * d + j] + m[i] * m[j] : 0.0;
    }
}

template <int D>
__global__ void __launch_bounds__(256) k_breg_pass_small(BregParams p) {
    BREG_NO_CONTRACT
    constexpr int NG = D * (D + 1) / 2, NP = NG + 1;
    __shared__ double red[4][NP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long prob = blockIdx.y, N = p.N;
    const double* Sp = p.S + (size_t)prob * D * D;
    double S[D][D];   // uniform in the workgroup
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) S[a][b] = Sp[a * D + b];
    const double* X = p.X + prob * N * D;
    const double* ne = p.neff + prob * N;
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) acc[q] = 0.0;
    for (long long i = (long long)blockIdx.x * breg::kSmallTile + tid; i < N; i += (long long)gridDim.x * breg::kSmallTile) {
        double x[D];
#pragma unroll
        for (int a = 0; a < D; ++a) x[a] = X[i * D + a];
        const double n = ne[i];
        double c2 = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < D; ++b) s += S[a][b] * x[b];
            c2 += x[a] * s;
        }
        double wv;
        acc[NG] += breg::point_term(n, c2, wv);
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double wa = wv * x[a];
#pragma unroll
            for (int b = 0; b <= a; ++b) acc[a * (a + 1) / 2 + b] += wa * x[b];
        }
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) red[w][q] = s;
    }
    __syncthreads();
    if (tid < NP) p.part[((size_t)prob * p.nchunk + blockIdx.x) * NP + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

template <int NT>
__global__ void __launch_bounds__(256) k_breg_pass(BregParams p) {
    BREG_NO_CONTRACT
    constexpr int D = 16 * NT, LD = D + 1, NK = D / 4, NTRI = NT * (NT + 1) / 2, TP = breg::kMfmaTile, PG = TP / 64;
    static_assert(TP * LD >= 4 * NTRI * 256, "the final reduction reuses the point tile");
    __shared__ double ys[TP * LD];   // the tile of points; columns d … D−1 and rows past N are zero
    __shared__ double ws[TP];        // ω̄ per point
    __shared__ double hred[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int d = p.d;
    const long long prob = blockIdx.y, N = p.N;
    const double* Sp = p.S + (size_t)prob * D * D;
    const double* X = p.X + prob * N * d;
    const double* ne = p.neff + prob * N;

    double sreg[NK][NT];   // the A operand of S·Xᵀ: S is symmetric, S[16t + lr][4kk + lq] is read as S[4kk + lq][16t + lr]
#pragma unroll
    for (int kk = 0; kk < NK; ++kk)
#pragma unroll
        for (int t = 0; t < NT; ++t) sreg[kk][t] = Sp[(4 * kk + lq) * D + 16 * t + lr];
    mvd_d4 G[NTRI];
#pragma unroll
    for (int q = 0; q < NTRI; ++q) G[q] = (mvd_d4){0.0, 0.0, 0.0, 0.0};
    double Pacc = 0.0;
    for (int q = tid; q < TP * LD; q += 256) ys[q] = 0.0;
    __syncthreads();

    for (long long base = (long long)blockIdx.x * TP; base < N; base += (long long)gridDim.x * TP) {
        // ---- stage the tile: its points are contiguous in X [N][d]
        const long long left = N - base;
        const int npts = left < TP ? (int)left : TP;
        const double* xt = X + base * d;
        for (int q = tid; q < TP * d; q += 256) {
            const int pt = q / d, c = q - pt * d;
            ys[pt * LD + c] = q < npts * d ? xt[q] : 0.0;
        }
        __syncthreads();

        // ---- c² = xᵀ S x of the wavefront's 16·PG points; then ω̄ and the P term, a lane per point (the row of lanes lq takes group lq)
        static_assert(PG <= 4, "a row of 16 lanes per group of points");
        double c2mine = 0.0;
#pragma unroll
        for (int g = 0; g < PG; ++g) {
            const int pt = 16 * (w * PG + g) + lr;
            double dv[NK];
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) dv[kk] = ys[pt * LD + 4 * kk + lq];
            mvd_d4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = (mvd_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(sreg[kk][t], dv[kk], acc[t], 0, 0, 0);
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += acc[t][r] * dv[4 * t + r];   // row 16t + lq + 4r of the product, this lane's point
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (lq == g) c2mine = s;
        }
        if (lq < PG) {
            const int pt = 16 * (w * PG + lq) + lr;
            const long long i = base + pt;
            const double n = i < N ? ne[i] : 0.0;
            double wv;
            Pacc += breg::point_term(n, c2mine, wv);
            ws[pt] = wv;
        }
        __syncthreads();

        // ---- G += (ω̄ ∘ X)ᵀ X over the quarter of the tile this wavefront owns (the points whose ω̄ it has just written)
#pragma unroll 2
        for (int kk = 0; kk < TP / 16; ++kk) {
            const int pt = (TP / 4) * w + 4 * kk + lq;
            const double wv = ws[pt];
            double yv[NT], a[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                yv[t] = ys[pt * LD + 16 * t + lr];
                a[t] = wv * yv[t];
            }
#pragma unroll
            for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                for (int tb = 0; tb <= ta; ++tb) G[ta * (ta + 1) / 2 + tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], yv[tb], G[ta * (ta + 1) / 2 + tb], 0, 0, 0);
        }
        __syncthreads();   // the next tile overwrites ys / ws
    }

    // ---- the four wavefronts' accumulators, added in wave order through LDS
    double* red = ys;
#pragma unroll
    for (int q = 0; q < NTRI; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((w * NTRI + q) * 4 + r) * 64 + lane] = G[q][r];
    {
        const double a = wave_sum(Pacc);
        if (lane == 0) hred[w] = a;
    }
    __syncthreads();
    const int NP = breg::npart(d);
    double* part = p.part + ((size_t)prob * p.nchunk + blockIdx.x) * NP;
    for (int e = tid; e < NTRI * 256; e += 256) {
        const int q = e >> 8, r = (e >> 6) & 3, ln = e & 63;
        const double s = ((red[e] + red[NTRI * 256 + e]) + red[2 * NTRI * 256 + e]) + red[3 * NTRI * 256 + e];
        const int ta = q == 0 ? 0 : 1, tb = q == 2 ? 1 : 0;
        const int a = 16 * ta + (ln >> 4) + 4 * r, b = 16 * tb + (ln & 15);
        if (a < d && b <= a) part[a * (a + 1) / 2 + b] = s;
    }
    if (tid == 0) part[NP - 1] = ((hred[0] + hred[1]) + hred[2]) + hred[3];
}

// step 2 of iteration `it` for one problem per wavefront, F of the iteration, its entry of the history, the S of the next pass
static __global__ void __launch_bounds__(64) k_breg_update(BregParams p, int it) {
    BREG_NO_CONTRACT
    __shared__ double A[MVD_DMAX * MVD_LDM], Wk[MVD_DMAX * MVD_LDM], Gm[MVD_DMAX * MVD_LDM];
    __shared__ double tot[MVD_DMAX * (MVD_DMAX + 1) / 2 + 1], xi[MVD_DMAX], m[MVD_DMAX], m0[MVD_DMAX];
    const int t = threadIdx.x, d = p.d, dd = d * d, NP = breg::npart(d), DP = breg::dpad(d);
    const long long prob = blockIdx.x;
    const double *xi0 = p.cst, *W0 = p.cst + d, *pm0 = W0 + dd;
    const double logdet_w0 = pm0[d];
    const double* part = p.part + (size_t)prob * p.nchunk * NP;
    for (int q = t; q < NP; q += 64) {   // ascending chunk order; 32 loads in flight ahead of the adds (up to 2048 chunks hang off this one chain)
        double s = part[q];
        int c = 1;
        for (; c + 32 <= p.nchunk; c += 32) {
            double v[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) v[k] = part[(size_t)(c + k) * NP + q];
#pragma unroll
            for (int k = 0; k < 32; ++k) s += v[k];
        }
        for (; c < p.nchunk; ++c) s += part[(size_t)c * NP + q];
        tot[q] = s;
    }
    if (t < d) {
        xi[t] = p.xi[prob * d + t];
        m0[t] = pm0[t];
    }
    __syncthreads();
    for (int q = t; q < dd; q += 64) {
        const int a = q / d, b = q - a * d, lo = a > b ? a : b, hi = a > b ? b : a;
        const double g = tot[lo * (lo + 1) / 2 + hi];
        Gm[a * MVD_LDM + b] = g;
        A[a * MVD_LDM + b] = W0[q] + g;
    }
    __syncthreads();
    double logdet_w;
    const bool ok = mvd_chol_inv(d, A, Wk, logdet_w);   // A = V
    if (t < d) {
        double s = 0.0;
        for (int b = 0; b < d; ++b) s += A[t * MVD_LDM + b] * xi[b];
        m[t] = s;
    }
    __syncthreads();
    double* S = p.S + (size_t)prob * DP * DP;
    double* hv = p.hist_v + ((size_t)it * p.C + prob) * dd;
    for (int q = t; q < dd; q += 64) {
        const int a = q / d, b = q - a * d;
        const double v = A[a * MVD_LDM + b];
        S[a * DP + b] = v + m[a] * m[b];
        hv[q] = v;
    }
    if (t < d) p.hist_m[((size_t)it * p.C + prob) * d + t] = m[t];
    if (p.want_fe) {
        double tr_sg = 0.0, tr_w0v = 0.0, quad0 = 0.0, m_dxi = 0.0;
        for (int q = t; q < dd; q += 64) {
            const int a = q / d, b = q - a * d;
            const double v = A[a * MVD_LDM + b];
            tr_sg += (v + m[a] * m[b]) * Gm[a * MVD_LDM + b];
            tr_w0v += W0[q] * v;
            quad0 += W0[q] * ((m[a] - m0[a]) * (m[b] - m0[b]));
        }
        if (t < d) m_dxi = m[t] * (xi[t] - xi0[t]);
        tr_sg = wave_sum(tr_sg);
        tr_w0v = wave_sum(tr_w0v);
        quad0 = wave_sum(quad0);
        m_dxi = wave_sum(m_dxi);
        if (t == 0) {
            const double F = breg::free_energy(p.lc[prob], m_dxi, tr_sg, tot[NP - 1], tr_w0v, quad0, d, logdet_w0, -logdet_w);
            p.fe_prob[(size_t)it * p.C + prob] = F;
            if (ok && !(F - F == 0.0)) atomicOr(p.status, ST_NONFINITE);
        }
    }
    if (!ok && t == 0) atomicOr(p.status, ST_NOT_POSDEF);
}

// the total of iteration `it`: the problems in a fixed tree
static __global__ void __launch_bounds__(256) k_breg_fe_total(BregParams p, int it, double* fe_total) {
    BREG_NO_CONTRACT
    __shared__ double sh[256];
    double acc = 0.0;
    for (long long s = threadIdx.x; s < p.C; s += 256) acc += p.fe_prob[(size_t)it * p.C + s];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int wd = 128; wd > 0; wd >>= 1) {
        if ((int)threadIdx.x < wd) sh[threadIdx.x] += sh[threadIdx.x + wd];
        __syncthreads();
    }
    if (threadIdx.x == 0) fe_total[it] = sh[0];
}

}  // namespace rxhip
#endif

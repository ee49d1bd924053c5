// mnreg_kernels.hpp — batched variational message passing for Bayesian multinomial regression under stick-breaking Pólya-Gamma augmentation, on gfx950.
//
// Reference model (test/models/regression/multinomialreg_tests.jl), for each of n_problems independent problems with N count vectors of K categories,
// d = K − 1:
//     ψ ~ MvNormalWeightedMeanPrecision(ξ0, W0);   y[i] ~ MultinomialPolya(N_i, ψ):  p(y_i | ψ) = Π_{k<K} Binomial(y_ik | N_ik, σ(ψ_k)),
//     N_ik = Σ_{j≥k} y_ij (the stick remainders),   κ_ik = y_ik − N_ik/2,   q(ψ, ω) = q(ψ) Π q(ω_ik).
// A row with any NaN is missing.  Once per data set (k_mnreg_stats), over the observed rows:
//     Y_k = Σ_i y_ik,  n = rows,  lc = Σ_i [lnΓ(N_i + 1) − Σ_k lnΓ(y_ik + 1)];   then S_k = Σ_{j≥k} Y_j = Σ_i N_ik,  κ_k = Y_k − S_k/2,  ξ = ξ0 + κ.
// Y, S, κ and n are sums of integers below 2⁵³: exact in fp64 in any order.  Only lc depends on the order, which is fixed.
//
// One ITERATION is a defined semantic (include/rxhip.h), from the current q(ψ) = N(m, V):
//   1. c_k² = m_k² + V_kk,  ω̄_k = S_k tanh(c_k/2)/(2 c_k)  (every observation shares c_k and the PG mean is linear in its first parameter),
//      P = Σ_k (−S_k ln(2 cosh(c_k/2)) + ½ c_k² ω̄_k);
//   2. W = W0 + diag(ω̄),  V = W⁻¹,  m = V ξ.
//     F = −[lc + mᵀκ − ½ Σ_k (V_kk + m_k²) ω̄_k + P] + KL(N(m, V) ‖ N(W0⁻¹ξ0, W0⁻¹)).
// It is the binomial engine's iteration (binreg_kernels.hpp) on the expanded problem with rows x = e_k, n = N_ik, y = y_ik; the point arithmetic
// (breg::point_term) and the free-energy assembly (breg::free_energy) are that engine's, unchanged.
//
// ONLINE mode streams T rows per series: step t takes the current (ξ, W) as its prior, starts from q(ψ) = N(W⁻¹ξ, W⁻¹), runs `iterations` offline
// iterations on the single row t, and leaves ξ += κ_t, W += diag(ω̄_t) (the ω̄ of the last iteration), which is its posterior in weighted-mean /
// precision form.  F_t is the one-row free energy of the last iteration against the step's prior.  A missing row changes nothing, repeats the
// history entry and gives F_t = 0.  Only the diagonal of W ever changes, so the resident state is ξ and diag(W) in LDS over the constant W0.
//
// Schedule.
//   k_mnreg_stats: grid (chunks, problem), 256 threads; `chunks` depends on N and K only (mnreg::chunks).  A tile of tile_rows(K) rows is staged in LDS
//     by flat, coalesced loads; a thread per row forms N_i and the missing flag; then threads stride over the tile by a multiple of K, so a thread
//     always meets the same column.  ONE partial per workgroup: Y[K] | n | lc.  No atomics.
//   k_mnreg_iterate<BIG>: one wavefront per problem, ONE launch per run: partials in ascending chunk order (32 loads in flight ahead of the adds),
//     suffix sums, then every iteration.  d ≤ 32 (BIG = false) inverts with mvd_chol_inv on [d][33] matrices; d = 33 … 64 with the same algorithm
//     on leading dimension 65 and the lower-triangular L⁻¹ packed (mn_chol_inv), 50 KB of LDS that the small class does not pay.
//   k_mnreg_fe_total: the problems of a batch in a fixed tree, a workgroup per iteration.
//   k_mnreg_online<BIG>: one wavefront per series, ONE launch per run; row t + 1 is loaded into registers before step t's factorisation.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "binreg_kernels.hpp"

namespace rxhip {
namespace mnreg {

constexpr int kMinK = 2, kMaxK = 65;   // categories; d = K − 1 = 1 … 64
constexpr int kSmallMaxD = 32;         // … of the class that uses mvd_chol_inv
constexpr int kLdBig = 65;             // leading dimension of the second class
constexpr int kTileDoubles = 4160;     // LDS doubles of the statistics pass's tile (64 rows of 65)
constexpr int kChunksCap = 1024;       // largest number of workgroups per problem (four per CU)

// rows per tile of the statistics pass: a power of two with tile_rows·K ≤ kTileDoubles
BREG_HD int tile_rows(int K) { return K <= 8 ? 512 : K <= 16 ? 256 : K <= 32 ? 128 : 64; }
// workgroups per problem: one per tile up to the cap; a function of N and K ONLY
BREG_HD int chunks(long long N, int K) {
    const long long tr = tile_rows(K), tiles = (N + tr - 1) / tr;
    return (int)(tiles < kChunksCap ? tiles : kChunksCap);
}
BREG_HD int npart(int K) { return K + 2; }   // a partial: Y[K] | n | lc
// the engine's constants, laid out as the binomial engine's: ξ0[d] | W0[d][d] | m0 = W0⁻¹ξ0 [d] | ln det W0 | initial m [d] | initial V [d][d]
BREG_HD int nconst(int d) { return breg::nconst(d); }
// S_k = Σ_{j≥k} Y_j, κ_k = Y_k − S_k/2 for k < K − 1, from the column sums (exact for integer counts)
BREG_HD void suffix(int K, const double* Y, double* S, double* kappa) {
    BREG_NO_CONTRACT
    double s = Y[K - 1];
    for (int k = K - 2; k >= 0; --k) {
        s += Y[k];
        S[k] = s;
        kappa[k] = Y[k] - 0.5 * s;
    }
}

}  // namespace mnreg
}  // namespace rxhip

#if defined(__HIPCC__)
namespace rxhip {

struct MnregParams {
    long long N, C;                  // rows per problem (T online), problems (series online)
    int K, d, nchunk, want_fe, iterations, keep_cov;
    const double* data;              // [C][N][K]
    const double* cst;               // mnreg::nconst(d)
    double* part;                    // [C][nchunk][K + 2]
    double *hist_m, *hist_v;         // offline [iterations][C][d], [iterations][C][d][d]; online [T][C][d] both (variances)
    double* hist_cov;                // online, keep_cov: [T][C][d][d]
    double* last;                    // online: [C][d + d·d], mean | covariance of the last step
    double* fe;                      // offline [iterations][C]; online F_t [T][C]
    double* fe_it;                   // online [iterations][C]: Σ_t of the step's F after that many iterations
    double *fe_total, *fe_chain;
    int* status;
};

static __global__ void __launch_bounds__(256) k_mnreg_stats(MnregParams p) {
    BREG_NO_CONTRACT
    __shared__ double ys[mnreg::kTileDoubles];
    __shared__ double rowobs[512];
    __shared__ double red[256];
    const int tid = threadIdx.x, K = p.K, TR = mnreg::tile_rows(K);
    const int per = 256 / K, S = per * K;            // threads tid < S stride by S: column tid % K for all their elements
    const long long prob = blockIdx.y, N = p.N;
    const double* D = p.data + (size_t)prob * N * K;
    double ycol = 0.0, lc = 0.0, cnt = 0.0;
    for (long long base = (long long)blockIdx.x * TR; base < N; base += (long long)gridDim.x * TR) {
        const long long left = N - base;
        const int nrows = left < TR ? (int)left : TR, nel = nrows * K;
        const double* src = D + base * K;
        for (int q = tid; q < nel; q += 256) ys[q] = src[q];
        __syncthreads();
        for (int r = tid; r < nrows; r += 256) {
            double s = 0.0;
            for (int k = 0; k < K; ++k) s += ys[r * K + k];   // NaN if any entry is
            const bool seen = s == s;
            rowobs[r] = seen ? 1.0 : 0.0;
            if (seen) {
                lc += lgamma(s + 1.0);
                cnt += 1.0;
            }
        }
        __syncthreads();
        if (tid < S) {
            int r = tid / K;
            for (int q = tid; q < nel; q += S, r += per)
                if (rowobs[r] != 0.0) {
                    const double v = ys[q];
                    ycol += v;
                    lc -= lgamma(v + 1.0);
                }
        }
        __syncthreads();   // the next tile overwrites ys / rowobs
    }
    double* part = p.part + ((size_t)prob * p.nchunk + blockIdx.x) * (size_t)mnreg::npart(K);
    red[tid] = tid < S ? ycol : 0.0;
    __syncthreads();
    if (tid < K) {
        double s = red[tid];
        for (int j = 1; j < per; ++j) s += red[tid + j * K];
        part[tid] = s;
    }
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {   // n (exact), then lc in a fixed tree
        red[tid] = pass == 0 ? cnt : lc;
        __syncthreads();
        for (int wd = 128; wd > 0; wd >>= 1) {
            if (tid < wd) red[tid] += red[tid + wd];
            __syncthreads();
        }
        if (tid == 0) part[K + pass] = red[0];
        __syncthreads();
    }
}

// mvd_chol_inv's algorithm on leading dimension 65 for n ≤ 64 and one wavefront: A (both triangles) <- A⁻¹ through A = LLᵀ, L⁻¹ column by column
// into Wp (lower triangle, packed by rows: entry (i, c) at i(i + 1)/2 + c), A⁻¹ = L⁻ᵀL⁻¹.  Returns false when a pivot is not positive.
__device__ __forceinline__ bool mn_chol_inv_big(int n, double* A, double* Wp, double& logdet) {
    constexpr int LD = mnreg::kLdBig;
    const int t = threadIdx.x;
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        const double pv = A[j * LD + j];
        if (!(pv > 0.0)) ok = false;
        const double s = sqrt(pv), is = 1.0 / s;
        __syncthreads();
        for (int i = j + t; i < n; i += 64) A[i * LD + j] = (i == j) ? s : A[i * LD + j] * is;
        __syncthreads();
        const int m = n - j - 1;
        for (int q = t; q < m * m; q += 64) {
            const int i = j + 1 + q / m, c = j + 1 + q % m;
            if (c <= i) A[i * LD + c] -= A[i * LD + j] * A[c * LD + j];
        }
        __syncthreads();
    }
    double ld = 0.0;
    for (int j = 0; j < n; ++j) ld += log(A[j * LD + j]);
    logdet = 2.0 * ld;
    if (t < n) {   // column t of L⁻¹
        for (int i = t; i < n; ++i) {
            double s = (i == t) ? 1.0 : 0.0;
            for (int m = t; m < i; ++m) s -= A[i * LD + m] * Wp[m * (m + 1) / 2 + t];
            Wp[i * (i + 1) / 2 + t] = s / A[i * LD + i];
        }
    }
    __syncthreads();
    for (int q = t; q < n * n; q += 64) {
        const int a = q / n, b = q % n;
        if (b <= a) {
            double s = 0.0;
            for (int i = a; i < n; ++i) s += Wp[i * (i + 1) / 2 + a] * Wp[i * (i + 1) / 2 + b];
            A[a * LD + b] = s;
            A[b * LD + a] = s;
        }
    }
    __syncthreads();
    return ok;
}

template <bool BIG>
struct MnShape {
    static constexpr int DMAX = BIG ? mnreg::kMaxK - 1 : mnreg::kSmallMaxD;
    static constexpr int LD = BIG ? mnreg::kLdBig : MVD_LDM;
    static constexpr int NW = BIG ? DMAX * (DMAX + 1) / 2 : MVD_DMAX * MVD_LDM;   // doubles of the work matrix
};
template <bool BIG>
__device__ __forceinline__ bool mn_chol_inv(int n, double* A, double* W, double& logdet) {
    if constexpr (BIG) return mn_chol_inv_big(n, A, W, logdet);
    else return mvd_chol_inv(n, A, W, logdet);
}

// The vectors every step of the iteration shares, in LDS
template <bool BIG>
struct MnVec {
    double xi[MnShape<BIG>::DMAX], kap[MnShape<BIG>::DMAX], Srem[MnShape<BIG>::DMAX], w[MnShape<BIG>::DMAX], m[MnShape<BIG>::DMAX], mp[MnShape<BIG>::DMAX],
        vd[MnShape<BIG>::DMAX], wdiag[MnShape<BIG>::DMAX];
};

// One iteration on the wavefront: step 1 from (m, vd), W = Wbase + diag(w) with Wbase = W0 off the diagonal and wdiag on it, V into A, the new m and vd.
// Returns P (in every lane) and the log-determinant of W; `ok` is cleared by a pivot that is not positive.
template <bool BIG>
__device__ __forceinline__ double mn_iteration(int d, const double* W0, MnVec<BIG>& v, double* A, double* Wk, double& logdet_w, bool& ok) {
    BREG_NO_CONTRACT
    constexpr int LD = MnShape<BIG>::LD;
    const int t = threadIdx.x;
    double pk = 0.0;
    if (t < d) {
        double wv;
        pk = breg::point_term(v.Srem[t], v.m[t] * v.m[t] + v.vd[t], wv);
        v.w[t] = wv;
    }
    const double P = __shfl(wave_sum(pk), 0);
    __syncthreads();
    for (int q = t; q < d * d; q += 64) {
        const int i = q / d, j = q - i * d;
        A[i * LD + j] = i == j ? v.wdiag[i] + v.w[i] : W0[q];
    }
    __syncthreads();
    ok = mn_chol_inv<BIG>(d, A, Wk, logdet_w) && ok;
    double s = 0.0;
    if (t < d)
        for (int b = 0; b < d; ++b) s += A[t * LD + b] * (v.xi[b] + v.kap[b]);
    __syncthreads();
    if (t < d) {
        v.m[t] = s;
        v.vd[t] = A[t * LD + t];
    }
    __syncthreads();
    return P;
}

// F of the iteration just made, against the prior N(mp, Wbase⁻¹) with ln det Wbase = logdet_base (value in lane 0)
template <bool BIG>
__device__ __forceinline__ double mn_free_energy(int d, const double* W0, const MnVec<BIG>& v, const double* A, double lc, double P, double logdet_base, double logdet_w) {
    BREG_NO_CONTRACT
    constexpr int LD = MnShape<BIG>::LD;
    const int t = threadIdx.x;
    double tr_sg = 0.0, tr_w0v = 0.0, quad0 = 0.0, m_dxi = 0.0;
    for (int q = t; q < d * d; q += 64) {
        const int a = q / d, b = q - a * d;
        const double wb = a == b ? v.wdiag[a] : W0[q];
        tr_w0v += wb * A[a * LD + b];
        quad0 += wb * ((v.m[a] - v.mp[a]) * (v.m[b] - v.mp[b]));
    }
    if (t < d) {
        m_dxi = v.m[t] * v.kap[t];
        tr_sg = (v.vd[t] + v.m[t] * v.m[t]) * v.w[t];
    }
    tr_sg = wave_sum(tr_sg);
    tr_w0v = wave_sum(tr_w0v);
    quad0 = wave_sum(quad0);
    m_dxi = wave_sum(m_dxi);
    return breg::free_energy(lc, m_dxi, tr_sg, P, tr_w0v, quad0, d, logdet_base, -logdet_w);
}

// The whole run of one problem on one wavefront.  Nothing depends on want_fe but the free-energy stores.
template <bool BIG>
__global__ void __launch_bounds__(64) k_mnreg_iterate(MnregParams p) {
    BREG_NO_CONTRACT
    constexpr int LD = MnShape<BIG>::LD;
    __shared__ double A[MnShape<BIG>::DMAX * LD], Wk[MnShape<BIG>::NW];
    __shared__ double tot[mnreg::kMaxK + 2];
    __shared__ MnVec<BIG> v;
    const int t = threadIdx.x, K = p.K, d = p.d, dd = d * d, NP = mnreg::npart(K);
    const long long prob = blockIdx.x;
    const double* part = p.part + (size_t)prob * p.nchunk * NP;
    for (int q = t; q < NP; q += 64) {   // ascending chunk order; 32 loads in flight ahead of the adds
        double s = part[q];
        int c = 1;
        for (; c + 32 <= p.nchunk; c += 32) {
            double u[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) u[k] = part[(size_t)(c + k) * NP + q];
#pragma unroll
            for (int k = 0; k < 32; ++k) s += u[k];
        }
        for (; c < p.nchunk; ++c) s += part[(size_t)c * NP + q];
        tot[q] = s;
    }
    const double *xi0 = p.cst, *W0 = p.cst + d, *pm0 = W0 + dd, *im = pm0 + d + 1, *iv = im + d;
    const double logdet_w0 = pm0[d];
    __syncthreads();
    if (t == 0) mnreg::suffix(K, tot, v.Srem, v.kap);
    __syncthreads();
    if (t < d) {
        v.xi[t] = xi0[t];
        v.mp[t] = pm0[t];
        v.m[t] = im[t];
        v.vd[t] = iv[t * d + t];
        v.wdiag[t] = W0[t * d + t];
    }
    const double lc = tot[K + 1];
    __syncthreads();
    bool ok = true;
    for (int it = 0; it < p.iterations; ++it) {
        double logdet_w;
        const double P = mn_iteration<BIG>(d, W0, v, A, Wk, logdet_w, ok);
        double* hv = p.hist_v + ((size_t)it * p.C + prob) * dd;
        for (int q = t; q < dd; q += 64) hv[q] = A[(q / d) * LD + (q - (q / d) * d)];
        if (t < d) p.hist_m[((size_t)it * p.C + prob) * d + t] = v.m[t];
        if (p.want_fe) {
            const double F = mn_free_energy<BIG>(d, W0, v, A, lc, P, logdet_w0, logdet_w);
            if (t == 0) {
                p.fe[(size_t)it * p.C + prob] = F;
                if (p.C == 1) p.fe_total[it] = F;
                if (it == p.iterations - 1) p.fe_chain[prob] = F;
                if (ok && !(F - F == 0.0)) atomicOr(p.status, ST_NONFINITE);
            }
        }
        __syncthreads();   // A, v are rewritten by the next iteration
    }
    if (!ok && t == 0) atomicOr(p.status, ST_NOT_POSDEF);
}

// the totals of a batch, one workgroup per iteration: the problems (offline: p.fe; online: p.fe_it) in a fixed tree
static __global__ void __launch_bounds__(256) k_mnreg_fe_total(MnregParams p, const double* src) {
    BREG_NO_CONTRACT
    __shared__ double sh[256];
    const int it = blockIdx.x;
    double acc = 0.0;
    for (long long s = threadIdx.x; s < p.C; s += 256) acc += src[(size_t)it * p.C + s];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int wd = 128; wd > 0; wd >>= 1) {
        if ((int)threadIdx.x < wd) sh[threadIdx.x] += sh[threadIdx.x + wd];
        __syncthreads();
    }
    if (threadIdx.x == 0) p.fe_total[it] = sh[0];
}

// The T steps of one series on one wavefront; ξ and diag(W) stay in LDS, W0 is read from the constants.
template <bool BIG>
__global__ void __launch_bounds__(64) k_mnreg_online(MnregParams p) {
    BREG_NO_CONTRACT
    constexpr int LD = MnShape<BIG>::LD;
    __shared__ double A[MnShape<BIG>::DMAX * LD], Wk[MnShape<BIG>::NW];
    __shared__ double row[mnreg::kMaxK + 1];
    __shared__ MnVec<BIG> v;
    const int t = threadIdx.x, K = p.K, d = p.d, dd = d * d;
    const long long ser = blockIdx.x, T = p.N, C = p.C;
    const double* D = p.data + (size_t)ser * T * K;
    const double *xi0 = p.cst, *W0 = p.cst + d;
    // before step 1 (ξ, W) is the prior: q(ψ) = N(W0⁻¹ξ0, W0⁻¹)
    for (int q = t; q < dd; q += 64) A[(q / d) * LD + (q - (q / d) * d)] = W0[q];
    if (t < d) {
        v.xi[t] = xi0[t];
        v.kap[t] = 0.0;
        v.wdiag[t] = W0[t * d + t];
    }
    __syncthreads();
    double logdet_base;
    bool ok = mn_chol_inv<BIG>(d, A, Wk, logdet_base);
    {
        double s = 0.0;
        if (t < d)
            for (int b = 0; b < d; ++b) s += A[t * LD + b] * v.xi[b];
        if (t < d) {
            v.m[t] = s;
            v.vd[t] = A[t * LD + t];
        }
    }
    if (p.want_fe && t == 0)
        for (int i = 0; i < p.iterations; ++i) p.fe_it[(size_t)i * C + ser] = 0.0;
    double fsum = 0.0;
    __syncthreads();
    // row 0 in registers: lane k holds y_k, lane 0 also y_64
    double r0 = t < K ? D[t] : 0.0, r1 = (t == 0 && K > 64) ? D[64] : 0.0;
    for (long long step = 0; step < T; ++step) {
        const double c0 = r0, c1 = r1;
        if (step + 1 < T) {   // the next row's loads are in flight during this step's factorisations
            const double* nx = D + (step + 1) * K;
            r0 = t < K ? nx[t] : 0.0;
            r1 = (t == 0 && K > 64) ? nx[64] : 0.0;
        }
        const bool missing = __any((c0 != c0) || (c1 != c1));
        double F = 0.0;
        if (!missing) {
            if (t < K) row[t] = c0;
            if (t == 0 && K > 64) row[64] = c1;
            __syncthreads();
            double lg = t < K ? lgamma(c0 + 1.0) : 0.0;
            if (t == 0 && K > 64) lg += lgamma(c1 + 1.0);
            lg = __shfl(wave_sum(lg), 0);
            if (t == 0) mnreg::suffix(K, row, v.Srem, v.kap);
            if (t < d) v.mp[t] = v.m[t];
            __syncthreads();
            const double lc = lgamma(v.Srem[0] + 1.0) - lg;
            double logdet_w = logdet_base;
            for (int it = 0; it < p.iterations; ++it) {
                const double P = mn_iteration<BIG>(d, W0, v, A, Wk, logdet_w, ok);
                if (p.want_fe) {
                    F = mn_free_energy<BIG>(d, W0, v, A, lc, P, logdet_base, logdet_w);
                    if (t == 0) p.fe_it[(size_t)it * C + ser] += F;
                }
            }
            // the step's posterior in weighted-mean / precision form is the next step's prior
            if (t < d) {
                v.xi[t] += v.kap[t];
                v.wdiag[t] += v.w[t];
                v.kap[t] = 0.0;
            }
            logdet_base = logdet_w;
            __syncthreads();
        }
        if (t < d) {
            p.hist_m[((size_t)step * C + ser) * d + t] = v.m[t];
            p.hist_v[((size_t)step * C + ser) * d + t] = v.vd[t];
        }
        if (p.keep_cov) {
            double* hc = p.hist_cov + ((size_t)step * C + ser) * dd;
            for (int q = t; q < dd; q += 64) hc[q] = A[(q / d) * LD + (q - (q / d) * d)];
        }
        if (p.want_fe && t == 0) {
            p.fe[(size_t)step * C + ser] = F;
            fsum += F;
            if (ok && !(F - F == 0.0)) atomicOr(p.status, ST_NONFINITE);
        }
    }
    double* last = p.last + (size_t)ser * (d + dd);
    if (t < d) last[t] = v.m[t];
    for (int q = t; q < dd; q += 64) last[d + q] = A[(q / d) * LD + (q - (q / d) * d)];
    if (p.want_fe && t == 0) {
        p.fe_chain[ser] = fsum;
        if (C == 1)
            for (int i = 0; i < p.iterations; ++i) p.fe_total[i] = p.fe_it[(size_t)i * C + ser];
    }
    if (!ok && t == 0) atomicOr(p.status, ST_NOT_POSDEF);
}

}  // namespace rxhip
#endif

// mvgmm_dense_kernels.hpp — the multivariate Gaussian-mixture engine at d = 5…32, K = 1…16 on v_mfma_f64_16x16x4_f64.
//
// Model, schedule and algebra are those of mvgmm_kernels.hpp (q(z) from the previous marginals; q(s), q(m[k]) with the previous E[W];
// q(w[k]) with the new q(m[k]); free energy from the same closed forms).  That file keeps every statistic of a lane in registers and
// evaluates the quadratic form in scalar code, which stops at d = 4.  Here the pass is a pair of small GEMMs per tile of points:
//
//   logits      for component k and 16 points:  C = H_k · (Y − m̄_k)ᵀ  (H_k = ½E[W_k], D×D, D = 16·NT columns, zero padded),
//               A operand H_k[i = l&15][c = l>>4] (read through L2/L1: K·D² doubles do not fit next to the point tile in LDS),
//               B operand (Y − m̄_k)[point = l&15][c = l>>4];  C holds row i = (l>>4) + 4r of column `point = l&15`, and the lane already
//               holds (y − m̄)[point][i] for exactly those rows (its B operand of k-step 4t + r), so the quadratic form is an in-lane
//               product and two cross-lane adds.  The difference is formed BEFORE the product: nothing cancels when |m̄| is large
//               against the spread.
//   softmax     one thread per point over the logits in LDS: max, exp_nonpos, normalisation, H[q(z_i)]; NaN propagates as in k_mvg_pass
//   statistics  S2_k += (π_k ∘ Y)ᵀ Y contracted over the points of the tile: A operand π_k[pt]·y[pt][a], B operand y[pt][b]; wavefront w owns the
//               components k ≡ w (mod 4), whose accumulators (lower tiles only) stay in registers over all tiles of the workgroup;
//               Σπ and Σπy are the running sums of the A operands.
//
// Per-workgroup partials in the layout of mvgmm_kernels.hpp (K·(1 + d + d(d+1)/2) + 1, packed lower triangle, no component padding),
// reduced by k_mvg_reduce; no floating-point atomics anywhere: two runs give the same bits.
// The update runs one wavefront per component with the d×d matrices in LDS (Cholesky inverse with log-determinant), leaves the
// component's free-energy term behind the statistics, and k_mvgd_fe adds them up in component order.
#pragma once
#include <hip/hip_runtime.h>

#include "mvgmm_kernels.hpp"

namespace rxhip {

typedef double mvd_d4 __attribute__((ext_vector_type(4)));

constexpr int MVD_DMAX = 32;                 // largest dimension (two column tiles)
constexpr int MVD_KMAX = 16;                 // largest number of components
constexpr int MVD_PG = 2;                    // groups of 16 points per wavefront in the logit step (one H_k operand load serves both)
constexpr int MVD_TP = 4 * 16 * MVD_PG;      // points per tile
constexpr int MVD_KO = MVD_KMAX / 4;         // components a wavefront owns at most
constexpr int MVD_GRID_CAP = 512;            // workgroups of the pass: two per CU, grid-stride over the tiles
constexpr int MVD_LDM = MVD_DMAX + 1;        // leading dimension of the update kernel's matrices in LDS

// constants of the responsibility rule per component: H_k [D][D] | m̄_k [D] | c_k (+ padding to a 64-byte multiple)
__host__ __device__ inline int mvd_tiles(int d) { return d > 16 ? 2 : 1; }
__host__ __device__ inline int mvd_drv_stride(int d) {
    const int D = 16 * mvd_tiles(d);
    return D * D + D + 8;
}

template <int NT>
__global__ void __launch_bounds__(256) k_mvgd_pass(MvgParams p, int d) {
    constexpr int D = 16 * NT, LD = D + 1, NK = D / 4, NTRI = NT * (NT + 1) / 2, DRV = D * D + D + 8;
    __shared__ double ys[MVD_TP * LD];           // the tile of points, columns d…D−1 and rows past N are zero
    __shared__ double pis[MVD_KMAX * MVD_TP];    // [k][point]: logits, then responsibilities
    __shared__ double hred[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int K = p.K;
    const long long N = p.N;
    const int STAT = 1 + d + d * (d + 1) / 2, nq = K * STAT + 1;

    mvd_d4 S2[MVD_KO][NTRI];
    double S1[MVD_KO][NT], S0[MVD_KO], Hz = 0.0;
#pragma unroll
    for (int o = 0; o < MVD_KO; ++o) {
        S0[o] = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) S1[o][t] = 0.0;
#pragma unroll
        for (int q = 0; q < NTRI; ++q) S2[o][q] = (mvd_d4){0.0, 0.0, 0.0, 0.0};
    }
    for (int q = tid; q < MVD_TP * LD; q += 256) ys[q] = 0.0;
    __syncthreads();

    for (long long base = (long long)blockIdx.x * MVD_TP; base < N; base += (long long)gridDim.x * MVD_TP) {
        // ---- stage the tile: the points of a tile are contiguous in y [N][d]
        const long long left = N - base;
        const int npts = left < MVD_TP ? (int)left : MVD_TP;
        const double* yt = p.y + base * d;
        for (int q = tid; q < MVD_TP * d; q += 256) {
            const int pt = q / d, c = q - pt * d;
            ys[pt * LD + c] = q < npts * d ? yt[q] : 0.0;
        }
        __syncthreads();

        // ---- logits of the wavefront's 16·PG points, component by component
        for (int k = 0; k < K; ++k) {
            const double* dr = p.drv + (size_t)k * DRV;
            double dv[MVD_PG][NK];
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
                const double mb = dr[D * D + 4 * kk + lq];
#pragma unroll
                for (int g = 0; g < MVD_PG; ++g) dv[g][kk] = ys[(16 * (w * MVD_PG + g) + lr) * LD + 4 * kk + lq] - mb;
            }
            const double ck = dr[D * D + D];
            mvd_d4 acc[MVD_PG][NT];
#pragma unroll
            for (int g = 0; g < MVD_PG; ++g)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[g][t] = (mvd_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < NK; ++kk)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const double a = dr[(4 * kk + lq) * D + 16 * t + lr];   // H_k[16t + lr][4kk + lq]: H_k is stored symmetric
#pragma unroll
                    for (int g = 0; g < MVD_PG; ++g) acc[g][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, dv[g][kk], acc[g][t], 0, 0, 0);
                }
#pragma unroll
            for (int g = 0; g < MVD_PG; ++g) {
                double s = 0.0;
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s += acc[g][t][r] * dv[g][4 * t + r];   // row 16t + lq + 4r of the product, this lane's point
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                if (lq == 0) pis[k * MVD_TP + 16 * (w * MVD_PG + g) + lr] = ck - s;
            }
        }
        __syncthreads();

        // ---- softmax, one thread per point
        if (tid < MVD_TP) {
            const long long i = base + tid;
            if (i < N) {
                double mx = -1e308;
                for (int k = 0; k < K; ++k) mx = fmax(mx, pis[k * MVD_TP + tid]);
                double Z = 0.0, se = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double t = pis[k * MVD_TP + tid] - mx, e = exp_nonpos(t);
                    Z += e;
                    se += e * t;
                    pis[k * MVD_TP + tid] = e;
                }
                const double zi = 1.0 / Z;
                for (int k = 0; k < K; ++k) {
                    const double pi = pis[k * MVD_TP + tid] * zi;
                    pis[k * MVD_TP + tid] = pi;
                    if (p.write_resp) p.resp[i * K + k] = pi;
                }
                double ysum = 0.0;
                for (int c = 0; c < D; ++c) ysum += ys[tid * LD + c];
                Hz += (log(Z) - se * zi) + (ysum - ysum);   // H[q(z_i)] = −Σ π log π;  NaN for a non-finite observation (exp_nonpos hides it)
            } else
                for (int k = 0; k < K; ++k) pis[k * MVD_TP + tid] = 0.0;
        }
        __syncthreads();

        // ---- statistics of the components this wavefront owns, contracted over the points of the tile
#pragma unroll 2
        for (int kk = 0; kk < MVD_TP / 4; ++kk) {
            const int pt = 4 * kk + lq;
            double yv[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) yv[t] = ys[pt * LD + 16 * t + lr];
#pragma unroll
            for (int o = 0; o < MVD_KO; ++o) {
                const int k = w + 4 * o;
                if (k < K) {
                    const double pi = pis[k * MVD_TP + pt];
                    S0[o] += pi;
                    double a[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        a[t] = pi * yv[t];
                        S1[o][t] += a[t];
                    }
#pragma unroll
                    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                        for (int tb = 0; tb <= ta; ++tb)
                            S2[o][ta * (ta + 1) / 2 + tb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ta], yv[tb], S2[o][ta * (ta + 1) / 2 + tb], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // the next tile overwrites ys / pis
    }

    // ---- partials of this workgroup: Σπ | Σπy | Σπyy' (packed lower) per component, then Σ_i H[q(z_i)]
    double* part = p.partial + (size_t)blockIdx.x * nq;
#pragma unroll
    for (int o = 0; o < MVD_KO; ++o) {
        const int k = w + 4 * o;
        if (k < K) {
            double* P = part + (size_t)k * STAT;
            double s0 = S0[o];   // the 16 lanes of a group hold the same sum over the points ≡ lq (mod 4)
            s0 += __shfl_xor(s0, 16);
            s0 += __shfl_xor(s0, 32);
            if (lane == 0) P[0] = s0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                double s1 = S1[o][t];
                s1 += __shfl_xor(s1, 16);
                s1 += __shfl_xor(s1, 32);
                if (lq == 0 && 16 * t + lr < d) P[1 + 16 * t + lr] = s1;
            }
#pragma unroll
            for (int ta = 0; ta < NT; ++ta)
#pragma unroll
                for (int tb = 0; tb <= ta; ++tb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int a = 16 * ta + lq + 4 * r, b = 16 * tb + lr;
                        if (a < d && b <= a) P[1 + d + a * (a + 1) / 2 + b] = S2[o][ta * (ta + 1) / 2 + tb][r];
                    }
        }
    }
    {
        const double a = wave_sum(Hz);
        if (lane == 0) hred[w] = a;
    }
    __syncthreads();
    if (tid == 0) part[nq - 1] = ((hred[0] + hred[1]) + hred[2]) + hred[3];
}

// ------------------------------------------------------------------------------------------
// update / derive: one wavefront per component, matrices [n][MVD_LDM] in LDS

// A (n×n, symmetric positive definite, both triangles) <- A⁻¹ through A = LL', L⁻¹ column by column, A⁻¹ = L⁻ᵀL⁻¹; W: work matrix.
// Returns false when a pivot is not positive (NaN included); the arithmetic then runs on to the end with non-finite values.
__device__ __forceinline__ bool mvd_chol_inv(int n, double* A, double* W, double& logdet) {
    const int t = threadIdx.x;
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        const double pv = A[j * MVD_LDM + j];
        if (!(pv > 0.0)) ok = false;
        const double s = sqrt(pv), is = 1.0 / s;
        __syncthreads();
        for (int i = j + t; i < n; i += 64) A[i * MVD_LDM + j] = (i == j) ? s : A[i * MVD_LDM + j] * is;
        __syncthreads();
        const int m = n - j - 1;
        for (int q = t; q < m * m; q += 64) {
            const int i = j + 1 + q / m, c = j + 1 + q % m;
            if (c <= i) A[i * MVD_LDM + c] -= A[i * MVD_LDM + j] * A[c * MVD_LDM + j];
        }
        __syncthreads();
    }
    double ld = 0.0;
    for (int j = 0; j < n; ++j) ld += log(A[j * MVD_LDM + j]);
    logdet = 2.0 * ld;
    if (t < n) {   // column t of L⁻¹
        for (int i = 0; i < n; ++i) {
            double s = (i == t) ? 1.0 : 0.0;
            for (int m = t; m < i; ++m) s -= A[i * MVD_LDM + m] * W[m * MVD_LDM + t];
            W[i * MVD_LDM + t] = (i < t) ? 0.0 : s / A[i * MVD_LDM + i];
        }
    }
    __syncthreads();
    for (int q = t; q < n * n; q += 64) {
        const int a = q / n, b = q % n;
        if (b <= a) {
            double s = 0.0;
            for (int i = a; i < n; ++i) s += W[i * MVD_LDM + a] * W[i * MVD_LDM + b];
            A[a * MVD_LDM + b] = s;
            A[b * MVD_LDM + a] = s;
        }
    }
    __syncthreads();
    return ok;
}

// constants of the next pass from q(m[k]) = N(mean, Cm), q(w[k]) = Wishart(nu, V) (ldV = log|V|), q(s): see mvg_derive
__device__ __forceinline__ void mvd_derive(const MvgParams& p, int d, int k, double nu, double al, double asum, double ldV, const double* V,
                                           const double* Cm, const double* mean) {
    const int t = threadIdx.x, D = 16 * mvd_tiles(d);
    double* dr = p.drv + (size_t)k * mvd_drv_stride(d);
    double tr = 0.0;
    for (int q = t; q < d * d; q += 64) {
        const int i = q / d, j = q % d;
        tr += nu * V[i * MVD_LDM + j] * Cm[j * MVD_LDM + i];
    }
    tr = wave_sum(tr);
    for (int q = t; q < D * D; q += 64) {
        const int i = q / D, j = q % D;
        dr[q] = (i < d && j < d) ? 0.5 * nu * V[i * MVD_LDM + j] : 0.0;
    }
    for (int j = t; j < D + 8; j += 64) dr[D * D + j] = j < d ? mean[j] : 0.0;
    __syncthreads();
    if (t == 0) {
        const double Elw = mvdigamma_dev(0.5 * nu, d) + d * 0.69314718055994530942 + ldV;
        const double Els = digamma_dev(al) - digamma_dev(asum);
        dr[D * D + D] = Els + 0.5 * Elw - 0.5 * tr;
    }
}

static __global__ void __launch_bounds__(64) k_mvgd_init(MvgParams p, int d) {
    __shared__ double Vm[MVD_DMAX * MVD_LDM], Cm[MVD_DMAX * MVD_LDM], T[MVD_DMAX * MVD_LDM], W[MVD_DMAX * MVD_LDM], mean[MVD_DMAX];
    const int k = blockIdx.x, t = threadIdx.x, dd = d * d, SZ = 2 + d + 2 * dd;
    const double* st = p.state + (size_t)k * SZ;
    for (int q = t; q < dd; q += 64) {
        const int a = q / d, b = q % d;
        const double v = 0.5 * (st[d + dd + 1 + a * d + b] + st[d + dd + 1 + b * d + a]);
        Vm[a * MVD_LDM + b] = v;
        T[a * MVD_LDM + b] = v;
        Cm[a * MVD_LDM + b] = 0.5 * (st[d + a * d + b] + st[d + b * d + a]);
    }
    if (t < d) mean[t] = st[t];
    __syncthreads();
    double ldV;
    const bool ok = mvd_chol_inv(d, T, W, ldV);
    double asum = 0.0;
    for (int j = 0; j < p.K; ++j) asum += p.state[(size_t)j * SZ + SZ - 1];
    mvd_derive(p, d, k, st[d + dd], st[SZ - 1], asum, ldV, Vm, Cm, mean);
    if (!ok && t == 0) atomicOr(p.status, ST_NOT_POSDEF);
}

// the component's term of the free energy goes to totals[nq + k] (behind the statistics; k_mvgd_fe adds the terms up)
template <bool FE>
__global__ void __launch_bounds__(64) k_mvgd_update(MvgParams p, int d) {
    __shared__ double A[MVD_DMAX * MVD_LDM], B[MVD_DMAX * MVD_LDM], W[MVD_DMAX * MVD_LDM], Sc[MVD_DMAX * MVD_LDM], EW[MVD_DMAX * MVD_LDM];
    __shared__ double S1[MVD_DMAX], xi[MVD_DMAX], mb[MVD_DMAX], mu0[MVD_DMAX];
    const int k = blockIdx.x, t = threadIdx.x, K = p.K, dd = d * d;
    const int STAT = 1 + d + d * (d + 1) / 2, SZ = 2 + d + 2 * dd, PRI = d + 2 * dd + 4, nq = K * STAT + 1;
    const double* tot = p.totals + (size_t)k * STAT;
    const double* pr = p.prior + (size_t)k * PRI;
    double* st = p.state + (size_t)k * SZ;
    const double* S0i = pr + d;
    const double* V0i = pr + d + dd + 1;
    const double S0 = tot[0], nu_old = st[d + dd], nu0 = pr[d + dd], al0 = pr[d + 2 * dd + 1], ldS0 = pr[d + 2 * dd + 2], ldV0 = pr[d + 2 * dd + 3];
    if (t < d) {
        S1[t] = tot[1 + t];
        mu0[t] = pr[t];
    }
    // q(m[k]) = N(μ0, S0) × Π_i N(y_i, (π_ik E[W])⁻¹):  Λ = S0⁻¹ + Σπ E[W],  ξ = S0⁻¹μ0 + E[W] Σπy   (E[W] = νV of the previous q(w[k]))
    for (int q = t; q < dd; q += 64) {
        const int a = q / d, b = q % d, lo = a > b ? a : b, hi = a > b ? b : a;
        const double ew = nu_old * (0.5 * (st[d + dd + 1 + a * d + b] + st[d + dd + 1 + b * d + a]));
        EW[a * MVD_LDM + b] = ew;
        A[a * MVD_LDM + b] = 0.5 * (S0i[a * d + b] + S0i[b * d + a]) + S0 * ew;
        Sc[a * MVD_LDM + b] = tot[1 + d + lo * (lo + 1) / 2 + hi];
    }
    __syncthreads();
    if (t < d) {
        double s = 0.0;
        for (int b = 0; b < d; ++b) s += 0.5 * (S0i[t * d + b] + S0i[b * d + t]) * mu0[b] + EW[t * MVD_LDM + b] * S1[b];
        xi[t] = s;
    }
    double ldL, ldVin;
    bool ok = mvd_chol_inv(d, A, W, ldL);   // A = cov of q(m[k])
    if (t < d) {
        double s = 0.0;
        for (int b = 0; b < d; ++b) s += A[t * MVD_LDM + b] * xi[b];
        mb[t] = s;
    }
    __syncthreads();
    // q(w[k]) = Wishart(ν0, V0) × Π_i (…):  ν = ν0 + Σπ,  V⁻¹ = V0⁻¹ + Σ_i π E[(y_i − m)(y_i − m)'] with the NEW q(m[k])
    for (int q = t; q < dd; q += 64) {
        const int a = q / d, b = q % d;
        const double sc = Sc[a * MVD_LDM + b] - mb[a] * S1[b] - S1[a] * mb[b] + S0 * (mb[a] * mb[b] + A[a * MVD_LDM + b]);
        Sc[a * MVD_LDM + b] = sc;
        B[a * MVD_LDM + b] = 0.5 * (V0i[a * d + b] + V0i[b * d + a]) + sc;
    }
    __syncthreads();
    ok = mvd_chol_inv(d, B, W, ldVin) && ok;   // B = V of q(w[k])
    const double nu = nu0 + S0, al = al0 + S0, ldV = -ldVin, ldC = -ldL;
    double asum = 0.0;
    for (int j = 0; j < K; ++j) asum += p.prior[(size_t)j * PRI + d + 2 * dd + 1] + p.totals[(size_t)j * STAT];
    if (FE) {
        double trWS = 0.0, trV0W = 0.0, trS0 = 0.0;
        for (int q = t; q < dd; q += 64) {
            const int a = q / d, b = q % d;
            trWS += nu * B[a * MVD_LDM + b] * Sc[b * MVD_LDM + a];
            trV0W += 0.5 * (V0i[a * d + b] + V0i[b * d + a]) * nu * B[b * MVD_LDM + a];
            trS0 += 0.5 * (S0i[a * d + b] + S0i[b * d + a]) * (A[b * MVD_LDM + a] + (mb[b] - mu0[b]) * (mb[a] - mu0[a]));
        }
        trWS = wave_sum(trWS);
        trV0W = wave_sum(trV0W);
        trS0 = wave_sum(trS0);
        if (t == 0) {
            const double LOG2 = 0.69314718055994530942;
            const double Elw = mvdigamma_dev(0.5 * nu, d) + d * LOG2 + ldV;
            double fk = 0.5 * (S0 * (d * kLog2Pi - Elw) + trWS);                                                   // Σ_i π_ik U_k(i)
            fk += 0.5 * (d * kLog2Pi + ldS0 + trS0) - 0.5 * (d * (kLog2Pi + 1.0) + ldC);                           // U_m − H[m]
            fk += -(0.5 * (nu0 - d - 1.0) * Elw - 0.5 * trV0W - 0.5 * nu0 * d * LOG2 - 0.5 * nu0 * ldV0 - mvlgamma_dev(0.5 * nu0, d));   // U_w
            fk -= 0.5 * (d + 1.0) * ldV + 0.5 * d * (d + 1.0) * LOG2 + mvlgamma_dev(0.5 * nu, d) - 0.5 * (nu - d - 1.0) * mvdigamma_dev(0.5 * nu, d) +
                  0.5 * nu * d;                                                                                    // − H[w]
            const double dga = digamma_dev(al), Els = dga - digamma_dev(asum);
            fk += -S0 * Els;                                                                                       // Categorical
            if (K > 1) fk += (lgamma(al0) - (al0 - 1.0) * Els) - (lgamma(al) - (al - 1.0) * dga);                  // Dirichlet parts
            p.totals[nq + k] = fk;
        }
    }
    // the new marginals (+ history)
    double* h = p.hist + ((size_t)p.iteration * K + k) * SZ;
    for (int q = t; q < SZ; q += 64) {
        double v;
        if (q < d) v = mb[q];
        else if (q < d + dd) v = A[((q - d) / d) * MVD_LDM + (q - d) % d];
        else if (q == d + dd) v = nu;
        else if (q < SZ - 1) v = B[((q - d - dd - 1) / d) * MVD_LDM + (q - d - dd - 1) % d];
        else v = al;
        st[q] = v;
        h[q] = v;
    }
    if (!ok && t == 0) atomicOr(p.status, ST_NOT_POSDEF);
    mvd_derive(p, d, k, nu, al, asum, ldV, B, A, mb);
}

// F = −Σ_i H[q(z_i)] + Σ_k (component terms, in component order) + the Dirichlet normalisers
static __global__ void __launch_bounds__(64) k_mvgd_fe(MvgParams p, int d) {
    if (threadIdx.x != 0) return;
    const int K = p.K, dd = d * d, STAT = 1 + d + d * (d + 1) / 2, PRI = d + 2 * dd + 4, nq = K * STAT + 1;
    double F = -p.totals[nq - 1], asum = 0.0, a0sum = 0.0;
    for (int j = 0; j < K; ++j) {
        const double al0 = p.prior[(size_t)j * PRI + d + 2 * dd + 1];
        a0sum += al0;
        asum += al0 + p.totals[(size_t)j * STAT];
        F += p.totals[nq + j];
    }
    if (K > 1) F += -lgamma(a0sum) - (-lgamma(asum) + (asum - K) * digamma_dev(asum));
    p.fe[p.iteration] = F;
    if (!is_finite(F)) atomicOr(p.status, ST_NONFINITE);
}

}  // namespace rxhip

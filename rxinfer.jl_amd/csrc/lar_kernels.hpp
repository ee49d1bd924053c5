// lar_kernels.hpp — batched structured variational message passing for the latent autoregressive model with unknown coefficients and
// driving-noise precision, on gfx950.
//
// Reference model (test/models/autoregressive/lar_tests.jl:51-76), for each of n_series independent series, written in scalars: order p
// (1 … 8), latent z_{-p+1} … z_T, n = T + p scalars, z_t at index t + p − 1;  x_t = (z_t … z_{t-p+1}),  x0 = (z_0 … z_{-p+1}):
//     γ ~ Gamma(a0, b0);  θ ~ N(mθ0, Wθ0⁻¹);  x0 ~ N(m0, W0⁻¹);  z_t | x_{t-1} ~ N(θᵀx_{t-1}, 1/γ);  y_t | z_t ~ N(z_t, 1/τ)       t = 1 … T
//     q(z, θ, γ) = q(z) q(θ) q(γ)
// The shift rows of the AR node are exact identities (the reference's ARsafe ε is not modelled); a NaN y_t is missing and contributes no factor.
//
// One ITERATION of this engine is a defined semantic (include/rxhip.h), three exact coordinate updates in the order x, θ, γ:
//   1. q(z) = N(m, Λ⁻¹) under the current q(θ) = N(mθ, Vθ), q(γ) = Gamma(a, b), mγ = a/b:  Λ = W0 on the first p scalars + Σ_t mγ·G on
//      w_t = (z_t, z_{t-1} … z_{t-p}), G = [[1, −mθᵀ], [−mθ, mθmθᵀ + Vθ]], + τ on the diagonal of every observed z_t;  h = W0 m0 on x0 + τ y_t.
//      Λ is SPD and banded with bandwidth p:  Λ = L D Lᵀ (unit lower L),  m = Λ⁻¹h,  ln det Λ = Σ ln d_i, and the band of Σ = Λ⁻¹ up to lag p by
//      the backward selected-inverse recursion  Σ_ij = δ_ij/d_i − Σ_{i<k≤i+p} L_ki Σ_kj.  Statistics: S = Σ_t E[w_t w_tᵀ] ((p+1)×(p+1):
//      Szz = S_00, Szx = S_0,1:, Sxx = S_1:,1:), E_y = Σ_obs((y_t − m_t)² + Σ_tt), N_obs, E_0 = (m_x0 − m0)ᵀW0(m_x0 − m0) + tr(W0 Σ_x0).
//   2. q(θ):  Wθ = Wθ0 + mγ Sxx (the old mγ),  Vθ = Wθ⁻¹,  mθ = Vθ(Wθ0 mθ0 + mγ Szx).
//   3. q(γ):  a = a0 + T/2,  b = b0 + R/2,  R = Szz − 2 mθᵀSzx + tr((mθmθᵀ + Vθ) Sxx) with the NEW θ.
// The posteriors OF ITERATION i are q(z) of step 1 and q(θ), q(γ) after steps 2 and 3; its free energy is the exact variational free energy there,
//     F = −½(n ln 2πe − ln det Λ) + ½(p ln 2π − ln det W0 + E_0) + ½(T ln 2π − T(ψ(a) − ln b) + (a/b) R) + ½(N_obs ln 2π − N_obs ln τ + τ E_y)
//         + KL(q(θ)‖p(θ)) + KL(q(γ)‖p(γ)),
// which cannot rise from one iteration to the next.  Shared parameters: one q(θ), q(γ) for all series; S is summed over the series in ascending
// order before steps 2 and 3, a = a0 + C·T/2, F = Σ_series(the first four terms) + the two KL terms once.
//
// Schedule.  A series is sequential in its rows, series are independent: k_lar_sweep<P> gives a series a LANE, arrays are [row][series].
//   forward, rows i = 0 … n−1: row i of Λ's band is formed on the fly — interior rows (p ≤ i < T) from the P + 1 diagonal sums of mγ·G the lane
//     keeps, the first and last p rows from lam_entry(), which sums only the factors that exist; the LDLᵀ row and the forward solve run against a
//     register window of the previous P rows; the record (l_i[P], 1/d_i, u_i = (L⁻¹h)_i/d_i) goes to memory.  (The reciprocal is stored in place
//     of d_i: the row step multiplies by it, the backward loop needs it for Σ_ii, and ln d_i = −ln(1/d_i).)
//   backward, rows i = n−1 … 0: the records are read a row ahead; the windows of L's columns, of m and of the Σ band stay in registers;
//     m_i = u_i − Σ_a L(i+a, i) m_{i+a};  Σ_{i,i+b} by the recursion above;  S, E_y, N_obs, E_0, ln det Λ are added row by row in this (descending)
//     order by the one lane that owns the series.  m_i and Σ_{i,i…i+p} go to memory only on the sweep whose posteriors are read (the last).
// One owner per series and a fixed order: results are bit-identical run to run, independent of the batch and of whether the free energy is asked
// for.  A lane beyond the batch repeats the last series and stores nothing.  Bytes per (series, row, iteration): y read in both loops (16) and the
// record written and read (16·(p + 2)).
// k_lar_update: a thread per parameter set (one per series, or one when shared): steps 2 and 3 with a P×P Cholesky, the next G, the KL terms, and
// the iteration's entry of the parameter history.  k_lar_fe: a thread per series, the first four terms of F with the series' own R under the new
// θ.  k_lar_reduce / k_lar_fe_total: fixed-order sums over the series.
//
// The arithmetic (band entry, row step, back-substitution and selected-inverse step, statistics, the θ/γ update, the energy of a series) is
// `__host__ __device__` and self-contained (only digamma.hpp), floating-point contraction off: the same functions compile for the host
// (tests/host_emul/lar_main.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "digamma.hpp"

#if defined(__clang__)
#define LAR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LAR_NO_CONTRACT
#endif
#define LAR_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace lar {

constexpr int kMaxP = 8;
constexpr double kLn2Pi = 1.8378770664093454835606594728112;

// sizes of the per-set blocks for order p: q = (mθ[p] | Vθ[p][p] | a | b);  g = (G[(p+1)][(p+1)] | mγ);  per-series statistics (S[(p+1)²] | E_y | N_obs | E_0 | ln det Λ)
LAR_HD int nq(int p) { return p + p * p + 2; }
LAR_HD int ng(int p) { return (p + 1) * (p + 1) + 1; }
LAR_HD int ns(int p) { return (p + 1) * (p + 1) + 4; }
// the engine's constants: W0[p][p] | m0[p] | W0 m0 [p] | Wθ0[p][p] | mθ0[p] | Wθ0 mθ0 [p] | a0 | b0 | ln det W0 | ln det Wθ0 | τ | lnΓ(a0) | ln b0 | ln τ
struct Consts {
    const double *w0, *m0, *h0, *wth0, *mth0, *wm0;
    double a0, b0, logdet_w0, logdet_wth0, tau, lgamma_a0, log_b0, log_tau;
};
LAR_HD int nconst(int p) { return 2 * p * p + 4 * p + 8; }
LAR_HD Consts consts(const double* c, int p) {
    Consts k;
    k.w0 = c; k.m0 = c + p * p; k.h0 = k.m0 + p; k.wth0 = k.h0 + p; k.mth0 = k.wth0 + p * p; k.wm0 = k.mth0 + p;
    const double* s = k.wm0 + p;
    k.a0 = s[0]; k.b0 = s[1]; k.logdet_w0 = s[2]; k.logdet_wth0 = s[3]; k.tau = s[4]; k.lgamma_a0 = s[5]; k.log_b0 = s[6]; k.log_tau = s[7];
    return k;
}

// Λ(i, i − k), 0 ≤ k ≤ P: the AR factors that hold both scalars (factor t covers the indices t − 1 … t + P − 1; scalar i sits at position
// ki = t + P − 1 − i of w_t, so ki runs over max(0, P − i) … min(P − k, n − 1 − i)), the x0 prior on the first P scalars, τ on the diagonal of an
// observed step (tau_i: τ or 0).  g: G row-major; an entry left of column 0 is 0.
template <int P>
LAR_HD double lam_entry(long long i, int k, long long n, const double* g, double mg, const double* w0, double tau_i) {
    LAR_NO_CONTRACT
    const long long j = i - k;
    if (j < 0) return 0.0;
    const long long lo = i < P ? P - i : 0, hi = n - 1 - i < P - k ? n - 1 - i : P - k;
    double s = 0.0;
    for (long long ki = lo; ki <= hi; ++ki) s += g[ki * (P + 1) + ki + k];
    double v = mg * s;
    if (i < P) v += w0[(P - 1 - i) * P + (P - 1 - j)];
    if (k == 0) v += tau_i;
    return v;
}

// the forward window: of the previous rows r = 1 … P (row i − r) the entries L(i − r, i − r − k) that a later row still needs (k ≤ P − r),
// 1/d and the forward-solve value v = (L⁻¹h); rows before row 0 are zeros
template <int P>
struct FwdWindow {
    double L[P][P], inv[P], v[P];
};
template <int P>
LAR_HD void fwd_clear(FwdWindow<P>& w) {
#pragma unroll
    for (int r = 0; r < P; ++r) {
        w.inv[r] = 0.0;
        w.v[r] = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) w.L[r][k] = 0.0;
    }
}
// row i of the factorisation from row i of the band a[k] = Λ(i, i − k) and h_i:  s_k = a_k − Σ_{m>k} s_m L(i − k, i − m) (ascending column),
// l_k = s_k/d_{i-k},  d_i = a_0 − Σ s_k l_k,  v_i = h_i − Σ l_k v_{i-k};  returns l[k − 1], 1/d_i, u_i = v_i/d_i and moves the window on
template <int P>
LAR_HD void row_step(FwdWindow<P>& w, const double (&a)[P + 1], double h, double (&l)[P], double& invd, double& u) {
    LAR_NO_CONTRACT
    double s[P + 1];
#pragma unroll
    for (int k = P; k >= 1; --k) {
        double acc = a[k];
#pragma unroll
        for (int m = P; m > k; --m) acc -= s[m] * w.L[k - 1][m - k - 1];
        s[k] = acc;
        l[k - 1] = acc * w.inv[k - 1];
    }
    double d = a[0], v = h;
#pragma unroll
    for (int k = P; k >= 1; --k) {
        d -= s[k] * l[k - 1];
        v -= l[k - 1] * w.v[k - 1];
    }
    invd = 1.0 / d;
    u = v * invd;
#pragma unroll
    for (int r = P - 1; r >= 1; --r) {
        w.inv[r] = w.inv[r - 1];
        w.v[r] = w.v[r - 1];
#pragma unroll
        for (int k = 0; k < P - 1 - r; ++k) w.L[r][k] = w.L[r - 1][k];
    }
    w.inv[0] = invd;
    w.v[0] = v;
#pragma unroll
    for (int k = 0; k < P - 1; ++k) w.L[0][k] = l[k];
}

// the backward window: of the rows i + r, r = 1 … P, the entries L(i + r, i + r − k) still to come as column entries (k ≥ r), m_{i+r}, and
// the band Σ(i + a, i + b), 1 ≤ a ≤ b ≤ P; rows beyond n − 1 are zeros
template <int P>
struct BwdWindow {
    double L[P][P], m[P], S[P][P];
};
template <int P>
LAR_HD void bwd_clear(BwdWindow<P>& w) {
#pragma unroll
    for (int r = 0; r < P; ++r) {
        w.m[r] = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) { w.L[r][k] = 0.0; w.S[r][k] = 0.0; }
    }
}
// row i of the back substitution and of the selected inverse: c_a = L(i + a, i);  m_i = u_i − Σ_a c_a m_{i+a};  Σ_{i,i+b} = −Σ_a c_a Σ_{i+a,i+b}
// (b = 1 … P),  Σ_ii = 1/d_i − Σ_a c_a Σ_{i,i+a};  row[b] = Σ_{i,i+b}
template <int P>
LAR_HD void back_step(const BwdWindow<P>& w, double invd, double u, double& mi, double (&row)[P + 1]) {
    LAR_NO_CONTRACT
    double m = u;
#pragma unroll
    for (int a = 1; a <= P; ++a) m -= w.L[a - 1][a - 1] * w.m[a - 1];
    mi = m;
#pragma unroll
    for (int b = 1; b <= P; ++b) {
        double acc = 0.0;
#pragma unroll
        for (int a = 1; a <= P; ++a) acc -= w.L[a - 1][a - 1] * (a <= b ? w.S[a - 1][b - 1] : w.S[b - 1][a - 1]);
        row[b] = acc;
    }
    double acc = invd;
#pragma unroll
    for (int a = 1; a <= P; ++a) acc -= w.L[a - 1][a - 1] * row[a];
    row[0] = acc;
}
// S += E[w_t w_tᵀ] of the factor t = i + 1, whose scalars are the window i … i + P (position k of w_t is index i + P − k); upper triangle only
template <int P>
LAR_HD void accumulate_s(double (&S)[P + 1][P + 1], const BwdWindow<P>& w, double mi, const double (&row)[P + 1]) {
    LAR_NO_CONTRACT
#pragma unroll
    for (int ka = 0; ka <= P; ++ka)
#pragma unroll
        for (int kb = ka; kb <= P; ++kb) {
            const int lo = P - kb, hi = P - ka;   // window offsets, lo ≤ hi
            const double cov = lo == 0 ? row[hi] : w.S[lo - 1][hi - 1];
            const double mlo = lo == 0 ? mi : w.m[lo - 1], mhi = hi == 0 ? mi : w.m[hi - 1];
            S[ka][kb] += cov + mlo * mhi;
        }
}
// row i < P of E_0: the terms of (m_x0 − m0)ᵀW0(m_x0 − m0) + tr(W0 Σ_x0) that pair scalar i with the scalars i … P − 1 (x0 component P − 1 − i)
template <int P>
LAR_HD double e0_terms(long long i, const BwdWindow<P>& w, double mi, const double (&row)[P + 1], const double* w0, const double* m0) {
    LAR_NO_CONTRACT
    double e = 0.0;
    const double dmi = mi - m0[P - 1 - i];
#pragma unroll
    for (int b = 0; b < P; ++b)
        if (i + b < P) {
            const double wt = w0[(P - 1 - i) * P + (P - 1 - i - b)];
            const double dmb = (b == 0 ? mi : w.m[b == 0 ? 0 : b - 1]) - m0[P - 1 - i - b];
            e += ((b == 0 ? 1.0 : 2.0) * wt) * (dmi * dmb + row[b]);
        }
    return e;
}
// … and the window moves on: l = the record of row i
template <int P>
LAR_HD void back_shift(BwdWindow<P>& w, const double (&l)[P], double mi, const double (&row)[P + 1]) {
#pragma unroll
    for (int r = P - 1; r >= 1; --r) {
        w.m[r] = w.m[r - 1];
#pragma unroll
        for (int k = r; k < P; ++k) w.L[r][k] = w.L[r - 1][k];
#pragma unroll
        for (int b = r; b < P; ++b) w.S[r][b] = w.S[r - 1][b - 1];
    }
    w.m[0] = mi;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        w.L[0][k] = l[k];
        w.S[0][k] = row[k];
    }
}

// In-place inverse of an SPD matrix (row-major n×n) by Cholesky: returns false when a pivot is not positive; *logdet = ln det A
LAR_HD bool spd_inverse(double* A, int n, double* logdet) {
    LAR_NO_CONTRACT
    double ld = 0.0;
    for (int j = 0; j < n; ++j) {
        double d = A[j * n + j];
        for (int k = 0; k < j; ++k) d -= A[j * n + k] * A[j * n + k];
        if (!(d > 0.0) || !(d - d == 0.0)) return false;
        const double r = sqrt(d);
        ld += log(d);
        A[j * n + j] = r;
        for (int i = j + 1; i < n; ++i) {
            double s = A[i * n + j];
            for (int k = 0; k < j; ++k) s -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = s / r;
        }
    }
    for (int j = 0; j < n; ++j) {          // X = L⁻¹, column by column (the columns right of j still hold L)
        A[j * n + j] = 1.0 / A[j * n + j];
        for (int i = j + 1; i < n; ++i) {
            double s = A[i * n + j] * A[j * n + j];
            for (int k = j + 1; k < i; ++k) s += A[i * n + k] * A[k * n + j];
            A[i * n + j] = -s / A[i * n + i];
        }
    }
    for (int i = 0; i < n; ++i)            // A⁻¹ = XᵀX, lower triangle row by row (row i needs the rows ≥ i of X only)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int k = i; k < n; ++k) s += A[k * n + i] * A[k * n + j];
            A[i * n + j] = s;
        }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) A[i * n + j] = A[j * n + i];
    *logdet = ld;
    return true;
}

// R = Szz − 2 mθᵀSzx + tr((mθmθᵀ + Vθ) Sxx);  S at S[e·ss], e = row·(p + 1) + column
LAR_HD double residual(const double* S, long long ss, const double* mth, const double* vth, int p) {
    LAR_NO_CONTRACT
    double cross = 0.0, quad = 0.0;
    for (int i = 0; i < p; ++i) {
        cross += mth[i] * S[(i + 1) * ss];
        for (int j = 0; j < p; ++j) quad += (mth[i] * mth[j] + vth[i * p + j]) * S[((i + 1) * (p + 1) + j + 1) * ss];
    }
    return S[0] - 2.0 * cross + quad;
}

// G = [[1, −mθᵀ], [−mθ, mθmθᵀ + Vθ]] and mγ = a/b of a q = (mθ | Vθ | a | b)
LAR_HD void make_g(const double* q, int p, double* g) {
    LAR_NO_CONTRACT
    const double *mth = q, *vth = q + p;
    g[0] = 1.0;
    for (int i = 0; i < p; ++i) {
        g[i + 1] = g[(i + 1) * (p + 1)] = -mth[i];
        for (int j = 0; j < p; ++j) g[(i + 1) * (p + 1) + j + 1] = mth[i] * mth[j] + vth[i * p + j];
    }
    g[(p + 1) * (p + 1)] = q[p + p * p] / q[p + p * p + 1];
}

// Steps 2 and 3 for one parameter set: q_new and its G from the statistics S (stride ss), the old mγ and the number of factors (T, or C·T when
// shared); g doubles as the work space of the right-hand side.  Returns KL(q(θ)‖p(θ)) + KL(q(γ)‖p(γ)); *ok = false: Wθ lost positive definiteness.
LAR_HD double update_theta_gamma(const double* S, long long ss, double mg_old, double n_factors, const Consts& c, int p, double* q, double* g, bool* ok) {
    LAR_NO_CONTRACT
    double *mth = q, *vth = q + p, *rhs = g;
    for (int i = 0; i < p; ++i) {
        rhs[i] = c.wm0[i] + mg_old * S[(i + 1) * ss];
        for (int j = 0; j < p; ++j) vth[i * p + j] = c.wth0[i * p + j] + mg_old * S[((i + 1) * (p + 1) + j + 1) * ss];
    }
    double logdet_w = 0.0;
    *ok = spd_inverse(vth, p, &logdet_w);
    for (int i = 0; i < p; ++i) {
        double s = 0.0;
        for (int j = 0; j < p; ++j) s += vth[i * p + j] * rhs[j];
        mth[i] = s;
    }
    const double a = c.a0 + 0.5 * n_factors, b = c.b0 + 0.5 * residual(S, ss, mth, vth, p);
    q[p + p * p] = a;
    q[p + p * p + 1] = b;
    make_g(q, p, g);
    double tr = 0.0, quad = 0.0;
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) {
            tr += c.wth0[i * p + j] * vth[i * p + j];
            quad += (mth[i] - c.mth0[i]) * c.wth0[i * p + j] * (mth[j] - c.mth0[j]);
        }
    const double kl_theta = 0.5 * (tr + quad - (double)p + logdet_w - c.logdet_wth0);
    const double kl_gamma = (a - c.a0) * digamma_dev(a) - lgamma(a) + c.lgamma_a0 + c.a0 * (log(b) - c.log_b0) + a * (c.b0 - b) / b;
    return kl_theta + kl_gamma;
}

// the first four terms of F for one series (statistics st, stride ss) at the new q
LAR_HD double series_energy(const double* st, long long ss, const double* q, const Consts& c, int p, long long T) {
    LAR_NO_CONTRACT
    const int e = (p + 1) * (p + 1);
    const double ey = st[e * ss], nobs = st[(e + 1) * ss], e0 = st[(e + 2) * ss], logdet = st[(e + 3) * ss];
    const double a = q[p + p * p], b = q[p + p * p + 1], Td = (double)T;
    double f = -0.5 * ((double)(T + p) * (kLn2Pi + 1.0) - logdet);
    f += 0.5 * ((double)p * kLn2Pi - c.logdet_w0 + e0);
    f += 0.5 * (Td * kLn2Pi - Td * (digamma_dev(a) - log(b)) + (a / b) * residual(st, ss, q, q + p, p));
    f += 0.5 * (nobs * kLn2Pi - nobs * c.log_tau + c.tau * ey);
    return f;
}

}  // namespace lar
}  // namespace rxhip

#if defined(__HIPCC__)
namespace rxhip {

constexpr int ST_LAR_BAD_Y = 16;   // status bit of k_lar_check_y (next to ST_NOT_POSDEF = 1, ST_NONFINITE = 2, ST_PROBIT_BAD_Y = 4, ST_HMM_BAD_X = 8)

struct LarParams {
    long long T, n_series;
    int P, shared, want_fe;
    const double* y;        // [T][series]
    const double* cst;      // lar::Consts image
    const double* init;     // [nq] the initial q(θ), q(γ)
    double* hist;           // [iterations][G][nq] q after every iteration (G = series, or 1 when shared)
    double* gm;             // [G][ng] G | mγ of the current q
    double* kl;             // [G]
    double* rec;            // [n][P + 2][series] l_i | 1/d_i | u_i
    double* zmean;          // [n][series]
    double* band;           // [n][P + 1][series] Σ(i, i … i + P)
    double* stat;           // [ns][series] statistics of the running sweep
    double* stat_sum;       // [ns] S summed over the series (shared parameters)
    double* fe_series;      // [iterations][series]
    int* status;
};

// G | mγ of the initial q for every parameter set: the start of a run
__global__ void __launch_bounds__(256) k_lar_init(LarParams p) {
    const long long G = p.shared ? 1 : p.n_series, g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    lar::make_g(p.init, p.P, p.gm + g * lar::ng(p.P));
}

// One sweep: a lane per series.  OUT: store m and the band of Σ.
template <int P, bool OUT>
__global__ void __launch_bounds__(64) k_lar_sweep(LarParams p) {
    LAR_NO_CONTRACT
    const long long C = p.n_series, T = p.T, n = T + P;
    const long long s_raw = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool live = s_raw < C;
    const long long s = live ? s_raw : C - 1;   // a lane beyond the batch repeats the last series (every load stays in bounds) and stores nothing
    const lar::Consts c = lar::consts(p.cst, P);
    const double* gm = p.gm + (p.shared ? 0 : s) * lar::ng(P);
    const double mg = gm[(P + 1) * (P + 1)], tau = c.tau;
    double cb[P + 1];                           // an interior row of the band: the diagonal sums of mγ·G (lam_entry far from both ends)
#pragma unroll
    for (int k = 0; k <= P; ++k) cb[k] = lar::lam_entry<P>(P, k, (long long)1 << 40, gm, mg, c.w0, 0.0);
    const double* ys = p.y + s;                 // y_t at ys[(t − 1)·C]; row i ≥ P is z_t with t = i − P + 1
    double* rec = p.rec + s;                    // entry e of row i at rec[(i·(P + 2) + e)·C]
    bool bad = false;

    {
        lar::FwdWindow<P> fw;
        lar::fwd_clear<P>(fw);
        double ynext = ys[0];
        for (long long i = 0; i < n; ++i) {
            double yv = 0.0;
            bool seen = false;
            if (i >= P) {
                yv = ynext;
                if (i + 1 < n) ynext = ys[(i + 1 - P) * C];
                seen = yv == yv;
            }
            const double tau_i = seen ? tau : 0.0;
            double a[P + 1], h;
            if (i >= P && i < T) {
#pragma unroll
                for (int k = 1; k <= P; ++k) a[k] = cb[k];
                a[0] = cb[0] + tau_i;
                h = 0.0 + (seen ? tau * yv : 0.0);
            } else {
#pragma unroll
                for (int k = 0; k <= P; ++k) a[k] = lar::lam_entry<P>(i, k, n, gm, mg, c.w0, tau_i);
                h = (i < P ? c.h0[P - 1 - i] : 0.0) + (seen ? tau * yv : 0.0);
            }
            double l[P], invd, u;
            lar::row_step<P>(fw, a, h, l, invd, u);
            bad = bad || !(invd > 0.0) || !(invd - invd == 0.0);
            if (live) {
                double* r = rec + i * (P + 2) * C;
#pragma unroll
                for (int k = 0; k < P; ++k) r[k * C] = l[k];
                r[P * C] = invd;
                r[(P + 1) * C] = u;
            }
        }
    }

    lar::BwdWindow<P> bw;
    lar::bwd_clear<P>(bw);
    double S[P + 1][P + 1];
#pragma unroll
    for (int ka = 0; ka <= P; ++ka)
#pragma unroll
        for (int kb = 0; kb <= P; ++kb) S[ka][kb] = 0.0;
    double ey = 0.0, nobs = 0.0, e0 = 0.0, logdet = 0.0;
    // the record of row i − 1 and its observation are loaded while row i is worked on; the loads of this lane's own stores above
    double l[P], invd, u, yv;
    {
        const double* r = rec + (n - 1) * (P + 2) * C;
#pragma unroll
        for (int k = 0; k < P; ++k) l[k] = r[k * C];
        invd = r[P * C];
        u = r[(P + 1) * C];
        yv = ys[(T - 1) * C];
    }
    for (long long i = n - 1; i >= 0; --i) {
        double ln[P], invdn = 0.0, un = 0.0, yn = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) ln[k] = 0.0;
        if (i >= 1) {
            const double* r = rec + (i - 1) * (P + 2) * C;
#pragma unroll
            for (int k = 0; k < P; ++k) ln[k] = r[k * C];
            invdn = r[P * C];
            un = r[(P + 1) * C];
            if (i - 1 >= P) yn = ys[(i - 1 - P) * C];
        }
        double mi, row[P + 1];
        lar::back_step<P>(bw, invd, u, mi, row);
        if (i < T) lar::accumulate_s<P>(S, bw, mi, row);
        if (i >= P && yv == yv) {
            const double r = yv - mi;
            ey += r * r + row[0];
            nobs += 1.0;
        }
        if (i < P) e0 += lar::e0_terms<P>(i, bw, mi, row, c.w0, c.m0);
        if (p.want_fe) logdet -= log(invd);
        if (OUT && live) {
            p.zmean[i * C + s] = mi;
            double* b = p.band + i * (P + 1) * C + s;
#pragma unroll
            for (int k = 0; k <= P; ++k) b[k * C] = row[k];
        }
        lar::back_shift<P>(bw, l, mi, row);
#pragma unroll
        for (int k = 0; k < P; ++k) l[k] = ln[k];
        invd = invdn; u = un; yv = yn;
    }
    if (live) {
        double* st = p.stat + s;
#pragma unroll
        for (int ka = 0; ka <= P; ++ka)
#pragma unroll
            for (int kb = 0; kb <= P; ++kb) st[(ka * (P + 1) + kb) * C] = ka <= kb ? S[ka][kb] : S[kb][ka];
        constexpr int e = (P + 1) * (P + 1);
        st[e * C] = ey;
        st[(e + 1) * C] = nobs;
        st[(e + 2) * C] = e0;
        st[(e + 3) * C] = logdet;
        if (bad) atomicOr(p.status, 1);   // ST_NOT_POSDEF
    }
}

// shared parameters: the statistics summed over the series in ascending order, a thread per entry
__global__ void __launch_bounds__(256) k_lar_reduce(LarParams p) {
    LAR_NO_CONTRACT
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= lar::ns(p.P)) return;
    const double* st = p.stat + (long long)e * p.n_series;
    double acc = st[0];
    for (long long s = 1; s < p.n_series; ++s) acc += st[s];
    p.stat_sum[e] = acc;
}

// steps 2 and 3 of iteration `it` for every parameter set; writes the set's entry of the history, its G and its KL terms
__global__ void __launch_bounds__(256) k_lar_update(LarParams p, int it) {
    LAR_NO_CONTRACT
    const long long G = p.shared ? 1 : p.n_series, g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int P = p.P, NQ = lar::nq(P);
    const double* old = it == 0 ? p.init : p.hist + ((long long)(it - 1) * G + g) * NQ;
    double* q = p.hist + ((long long)it * G + g) * NQ;
    const double mg_old = old[P + P * P] / old[P + P * P + 1];
    const lar::Consts c = lar::consts(p.cst, P);
    bool ok = true;
    const double kl = p.shared ? lar::update_theta_gamma(p.stat_sum, 1, mg_old, (double)p.n_series * (double)p.T, c, P, q, p.gm, &ok)
                               : lar::update_theta_gamma(p.stat + g, p.n_series, mg_old, (double)p.T, c, P, q, p.gm + g * lar::ng(P), &ok);
    p.kl[g] = kl;
    if (!ok) atomicOr(p.status, 1);                                   // ST_NOT_POSDEF
    else if (p.want_fe && !(kl - kl == 0.0)) atomicOr(p.status, 2);   // ST_NONFINITE
}

// per-series part of the free energy of iteration `it`: the first four terms, + the KL terms of the series' own q unless the parameters are shared
__global__ void __launch_bounds__(256) k_lar_fe(LarParams p, int it) {
    LAR_NO_CONTRACT
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= p.n_series) return;
    const long long G = p.shared ? 1 : p.n_series, g = p.shared ? 0 : s;
    const double* q = p.hist + ((long long)it * G + g) * lar::nq(p.P);
    double f = lar::series_energy(p.stat + s, p.n_series, q, lar::consts(p.cst, p.P), p.P, p.T);
    if (!p.shared) f += p.kl[s];
    p.fe_series[(long long)it * p.n_series + s] = f;
}
// … and the total: the series in a fixed tree, + the KL terms once when the parameters are shared
__global__ void __launch_bounds__(256) k_lar_fe_total(LarParams p, int it, double* fe_total) {
    LAR_NO_CONTRACT
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
        if (p.shared) f += p.kl[0];
        fe_total[it] = f;
        if (!(f - f == 0.0)) atomicOr(p.status, 2);   // ST_NONFINITE
    }
}

// every observation is finite or NaN (missing)
__global__ void __launch_bounds__(256) k_lar_check_y(const double* y, long long n, int* status) {
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = y[i];
        bad = bad || (v == v && !(v - v == 0.0));
    }
    if (bad) atomicOr(status, ST_LAR_BAD_Y);
}

}  // namespace rxhip
#endif

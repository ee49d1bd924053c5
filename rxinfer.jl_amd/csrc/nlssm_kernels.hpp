// nlssm_kernels.hpp — batched extended / unscented Kalman filtering and smoothing of a nonlinear state-space model, on gfx950.
//
// Model (the reference's delta node under Linearization() / Unscented(), paper/example.jl and test/models/nonlinear), for each of n_series
// independent series, d = 1 … 4:
//     x[0] ~ N(m0, V0);   x[t] ~ N(f(x[t-1]), Q)   (Q PSD, may be 0)   t = 1 … T
//     known noise:    y[t] ~ N(H x[t], R)           d_y = 1 … d, R SPD
//     unknown noise:  τ ~ Gamma(a0, b0);  y[t] ~ N(cᵀx[t], 1/τ)   d_y = 1,  q(x, τ) = q(x) q(τ)
// A step of y with a NaN in any component is missing.  f is an expression program (expr.hpp), the same for every series.
//
// Delta node: a prior N(m, V) becomes a predicted mean m̃, a covariance Ṽ and a cross-covariance C̃ = cov(x, f(x)):
//     Linearization   m̃ = f(m), J = ∂f/∂x(m) (forward-mode duals), C̃ = V Jᵀ, Ṽ = J C̃;
//     Unscented       λ = α²(d+κ) − d, L = chol((d+λ)V), points m, m ± L e_i, weights Wm₀ = λ/(d+λ), Wc₀ = Wm₀ + 1 − α² + β, W_i = 1/(2(d+λ)),
//                     m̃, Ṽ, C̃ the weighted moments (V must be SPD here: a singular V raises the non-SPD status);
// Ṽ is symmetrised, P = Ṽ + Q.
//
// Schedule.  A lane is a series, its state lives in registers, the time loop runs inside the lane: k_nlssm_forward is ONE launch for the whole
// filter (Kalman update with known noise; `iterations` VMP iterations per observation with the feedback of q(τ) in the lane with unknown noise).
// In SMOOTH mode it stores per step the filtered (m, V), (m̃, P) and C̃ as [step][record][series] — a wavefront's stores coalesce — and
// k_nlssm_backward is ONE more launch: the extended / unscented RTS pass G = C̃ P⁻¹, mˢ = m + G(mˢ₊₁ − m̃), Vˢ = V + G(Vˢ₊₁ − P)Gᵀ.  No resident
// or persistent scheme: a workgroup is one wavefront, it needs no barrier (the expression slots of a lane are its own LDS column).
//
// A value of f, of its Jacobian or of the moments that is not finite raises ST_NLSSM_NONFINITE and leaves (step, series) of the FIRST such
// event — smallest step, then smallest series — in `where` (one 64-bit atomic minimum); the lane stops there.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "digamma.hpp"
#include "expr.hpp"

#define NLSSM_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace nlssm {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;
constexpr int METHOD_LINEARIZATION = 0, METHOD_UNSCENTED = 1;

// lower Cholesky factor of the leading n×n block of A (n ≤ D, the rest of L is zero); false: a pivot was not positive
template <int D>
NLSSM_HD bool chol(const double (&A)[D][D], double (&L)[D][D], int n) {
    EXPR_NO_CONTRACT
    bool ok = true;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) L[i][j] = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        if (j < n) {
            double sum = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) sum -= L[j][k] * L[j][k];
            ok = ok && sum > 0.0;
            const double ljj = sqrt(sum);
            L[j][j] = ljj;
#pragma unroll
            for (int i = j + 1; i < D; ++i) {
                if (i < n) {
                    double v = A[i][j];
#pragma unroll
                    for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
                    L[i][j] = v / ljj;
                }
            }
        }
    }
    return ok;
}
// z = L⁻¹ b and x = L⁻ᵀ z on the leading n entries
template <int D>
NLSSM_HD void solve_lower(const double (&L)[D][D], const double (&b)[D], double (&z)[D], int n) {
    EXPR_NO_CONTRACT
#pragma unroll
    for (int i = 0; i < D; ++i) {
        z[i] = 0.0;
        if (i < n) {
            double v = b[i];
#pragma unroll
            for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
            z[i] = v / L[i][i];
        }
    }
}
template <int D>
NLSSM_HD void solve_upper(const double (&L)[D][D], const double (&z)[D], double (&x)[D], int n) {
    EXPR_NO_CONTRACT
#pragma unroll
    for (int i = D - 1; i >= 0; --i) {
        x[i] = 0.0;
        if (i < n) {
            double v = z[i];
#pragma unroll
            for (int k = i + 1; k < D; ++k) v -= L[k][i] * x[k];   // (rows ≥ n of L are zero)
            x[i] = v / L[i][i];
        }
    }
}
template <int D>
NLSSM_HD void symmetrise(double (&A)[D][D]) {
    EXPR_NO_CONTRACT
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i + 1; j < D; ++j) { const double v = 0.5 * (A[i][j] + A[j][i]); A[i][j] = v; A[j][i] = v; }
}
template <int D>
NLSSM_HD bool all_finite(const double (&m)[D], const double (&A)[D][D], const double (&B)[D][D]) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        acc += m[i] - m[i];
#pragma unroll
        for (int j = 0; j < D; ++j) acc += (A[i][j] - A[i][j]) + (B[i][j] - B[i][j]);
    }
    return acc == 0.0;
}

struct Unscented { double sc, wm0, wc0, wi; };   // d + λ and the weights

// the delta node: 0 ok, 1 V not SPD (unscented), 2 a value that is not finite
template <int D>
NLSSM_HD int delta(const expr::Program* __restrict__ prog, double* lds, int lane, int method, const Unscented& u, const double (&m)[D],
                   const double (&V)[D][D], double (&mt)[D], double (&Vt)[D][D], double (&Ct)[D][D]) {
    EXPR_NO_CONTRACT
    if (method == METHOD_LINEARIZATION) {
        double J[D][D];
        expr::eval_jacobian<D>(prog, lds, lane, m, mt, J);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) v += V[i][k] * J[j][k];
                Ct[i][j] = v;
            }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) v += J[i][k] * Ct[k][j];
                Vt[i][j] = v;
            }
    } else {
        double A[D][D], L[D][D], X[2 * D + 1][D], Y[2 * D + 1][D];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) A[i][j] = u.sc * V[i][j];
        if (!chol<D>(A, L, D)) return 1;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            X[0][i] = m[i];
#pragma unroll
            for (int k = 0; k < D; ++k) { X[1 + k][i] = m[i] + L[i][k]; X[1 + D + k][i] = m[i] - L[i][k]; }
        }
        expr::eval_points<D, 2 * D + 1>(prog, lds, lane, X, Y);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double v = u.wm0 * Y[0][i];
#pragma unroll
            for (int p = 1; p <= 2 * D; ++p) v += u.wi * Y[p][i];
            mt[i] = v;
        }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double v = u.wc0 * ((Y[0][i] - mt[i]) * (Y[0][j] - mt[j]));
#pragma unroll
                for (int p = 1; p <= 2 * D; ++p) v += u.wi * ((Y[p][i] - mt[i]) * (Y[p][j] - mt[j]));
                Vt[i][j] = v;
                double c = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) c += u.wi * (L[i][k] * (Y[1 + k][j] - Y[1 + D + k][j]));   // Σ_p W_p (X_p − m)(Y_p − m̃)ᵀ: the m̃ terms of ±L e_k cancel
                Ct[i][j] = c;
            }
    }
    symmetrise<D>(Vt);
    return all_finite<D>(mt, Vt, Ct) ? 0 : 2;
}

// Kalman update of (m, P) with y ~ N(H x, R), dy ≤ D rows: S = H P Hᵀ + R = L Lᵀ, W = L⁻¹ H P, z = L⁻¹(y − H m): m ← m + Wᵀz, V = P − WᵀW,
// and −ln N(y; H m, S) = ½(dy ln 2π + 2 Σ ln L_ii + zᵀz).  false: S was not SPD
template <int D>
NLSSM_HD bool kalman_update(const double (&H)[D][D], const double (&R)[D][D], int dy, const double (&y)[D], double (&m)[D], double (&P)[D][D], double& nll) {
    EXPR_NO_CONTRACT
    double HP[D][D], S[D][D], L[D][D], r[D], z[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double hm = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) hm += H[a][k] * m[k];
        r[a] = y[a] - hm;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) v += H[a][k] * P[k][j];
            HP[a][j] = v;
        }
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
            double v = R[a][b];
#pragma unroll
            for (int k = 0; k < D; ++k) v += HP[a][k] * H[b][k];
            S[a][b] = v;
        }
    symmetrise<D>(S);
    if (!chol<D>(S, L, dy)) return false;
    solve_lower<D>(L, r, z, dy);
    double W[D][D];   // W[a][j] = (L⁻¹ HP)[a][j]
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double col[D], w[D];
#pragma unroll
        for (int a = 0; a < D; ++a) col[a] = HP[a][j];
        solve_lower<D>(L, col, w, dy);
#pragma unroll
        for (int a = 0; a < D; ++a) W[a][j] = w[a];
    }
    double q = 0.0, ld = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a)
        if (a < dy) { q += z[a] * z[a]; ld += log(L[a][a]); }
    nll = 0.5 * (dy * kLog2Pi + q) + ld;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < D; ++a) v += W[a][i] * z[a];
        m[i] += v;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) s += W[a][i] * W[a][j];
            P[i][j] -= s;
        }
    }
    symmetrise<D>(P);
    return true;
}

// Unknown observation precision: `iterations` VMP iterations on one observation y ~ N(cᵀx, 1/τ) from the prediction (m, P) and q(τ) = Gamma(a, b)
// (shape, rate).  On return (m, P) is q(x_t), (a, b) the new q(τ) and fe the step's free energy after the last iteration:
//     KL(q(x)‖N(m̃, P)) + KL(Gamma(a′, b′)‖Gamma(a, b)) + ½(ln 2π − (ψ(a′) − ln b′) + (a′/b′)((y − cᵀm′)² + cᵀV′c)),
// the Gaussian KL in the closed form of a rank-one update: ½(g²r²s − g s + ln(1 + E[τ] s)), r = y − cᵀm̃ — no inverse of P, so Q = 0 is fine.
template <int D>
NLSSM_HD void noise_update(const double (&c)[D], double y, int iterations, double (&m)[D], double (&P)[D][D], double& a, double& b, double& fe) {
    EXPR_NO_CONTRACT
    double k[D], s = 0.0, cm = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) v += P[i][j] * c[j];
        k[i] = v;
    }
#pragma unroll
    for (int i = 0; i < D; ++i) { s += c[i] * k[i]; cm += c[i] * m[i]; }
    const double r = y - cm;
    double E = a / b, g = 0.0, Eg = E, an = a, bn = b, e2 = 0.0;
    double mn[D], Vn[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        mn[i] = m[i];
#pragma unroll
        for (int j = 0; j < D; ++j) Vn[i][j] = P[i][j];
    }
    for (int it = 0; it < iterations; ++it) {
        Eg = E;
        g = E / (1.0 + E * s);
        double cmn = 0.0, cvc = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            mn[i] = m[i] + k[i] * (g * r);
#pragma unroll
            for (int j = 0; j < D; ++j) Vn[i][j] = P[i][j] - g * (k[i] * k[j]);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            cmn += c[i] * mn[i];
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) v += Vn[i][j] * c[j];
            cvc += c[i] * v;
        }
        const double rn = y - cmn;
        e2 = rn * rn + cvc;
        an = a + 0.5;
        bn = b + 0.5 * e2;
        E = an / bn;
    }
    const double klx = 0.5 * (g * g * r * r * s - g * s + log1p(Eg * s));
    const double psi = digamma_dev(an);
    const double klg = (an - a) * psi - lgamma(an) + lgamma(a) + a * (log(bn) - log(b)) + an * (b - bn) / bn;
    fe = klx + klg + 0.5 * (kLog2Pi - (psi - log(bn)) + (an / bn) * e2);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        m[i] = mn[i];
#pragma unroll
        for (int j = 0; j < D; ++j) P[i][j] = Vn[i][j];
    }
    symmetrise<D>(P);
    a = an;
    b = bn;
}

// records of a smoothing run per step: m | V (upper triangle) | m̃ | P (upper triangle) | C̃
NLSSM_HD int n_records(int d) { return 2 * d + d * (d + 1) + d * d; }

}  // namespace nlssm
}  // namespace rxhip

#if defined(__HIPCC__) || defined(RXHIP_HOST_EMUL)
namespace rxhip {

struct NlssmParams {
    long long T, n_series;
    int dy, method, unknown, per_series, iterations, smooth;
    const expr::Program* prog;
    const double* y;        // [T][series][dy]
    const double* prior;    // m0 [d] | V0 [d][d], one set or [series] sets
    double Q[16], H[16], R[16];   // row-major d×d, dy×d, dy×dy
    double a0, b0;
    nlssm::Unscented u;
    double *mean, *cov;     // [T][series][d], [T][series][d][d]
    double *shape, *rate;   // [T][series] (unknown noise)
    double* rec;            // smoothing: [T][n_records][series]
    double* fe_series;      // [series]
    int* status;
    unsigned long long* where;   // (step << 32) | series of the first non-finite event
};

// the forward pass: filter of a series per lane (see the header)
template <int D>
__global__ void __launch_bounds__(64) k_nlssm_forward(NlssmParams p) {
    EXPR_NO_CONTRACT
    EXPR_LDS_BLOCK(lds);
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= p.n_series) return;
    const long long C = p.n_series;
    const int lane = (int)threadIdx.x, dy = p.dy;
    constexpr int NS = D * (D + 1) / 2, NR = 2 * D + 2 * NS + D * D;
    double m[D], V[D][D], Q[D][D], H[D][D], R[D][D];
    const double* pr = p.prior + (p.per_series ? s * (D + D * D) : 0);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        m[i] = pr[i];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            V[i][j] = pr[D + i * D + j];
            Q[i][j] = p.Q[i * D + j];
            H[i][j] = i < dy ? p.H[i * D + j] : 0.0;
            R[i][j] = (i < dy && j < dy) ? p.R[i * dy + j] : 0.0;
        }
    }
    double a = p.a0, b = p.b0, fe = 0.0;
    bool notpd = false;
    for (long long t = 0; t < p.T; ++t) {
        double mt[D], P[D][D], Ct[D][D];
        const int flag = nlssm::delta<D>(p.prog, lds, lane, p.method, p.u, m, V, mt, P, Ct);
        if (flag == 2) {
            atomicOr(p.status, 64);   // ST_NLSSM_NONFINITE (engine.hpp)
            atomicMin(p.where, ((unsigned long long)t << 32) | (unsigned long long)s);
            return;
        }
        if (flag == 1) { atomicOr(p.status, 1); return; }   // ST_NOT_POSDEF
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) P[i][j] += Q[i][j];
        if (p.smooth) {
            double* r = p.rec + (t * NR + D + NS) * C + s;
            int q = 0;
#pragma unroll
            for (int i = 0; i < D; ++i) r[(q++) * C] = mt[i];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = i; j < D; ++j) r[(q++) * C] = P[i][j];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) r[(q++) * C] = Ct[i][j];
        }
        double y[D];
        bool missing = false;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            y[i] = i < dy ? p.y[(t * C + s) * dy + i] : 0.0;
            missing = missing || y[i] != y[i];
        }
        if (!missing) {
            if (p.unknown) {
                double c[D], f = 0.0;
#pragma unroll
                for (int i = 0; i < D; ++i) c[i] = H[0][i];
                nlssm::noise_update<D>(c, y[0], p.iterations, mt, P, a, b, f);
                fe += f;
            } else {
                double nll = 0.0;
                const bool spd = nlssm::kalman_update<D>(H, R, dy, y, mt, P, nll);
                notpd = notpd || !spd;
                fe += nll;
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            m[i] = mt[i];
#pragma unroll
            for (int j = 0; j < D; ++j) V[i][j] = P[i][j];
        }
        if (p.smooth) {
            double* r = p.rec + (t * NR) * C + s;
            int q = 0;
#pragma unroll
            for (int i = 0; i < D; ++i) r[(q++) * C] = m[i];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = i; j < D; ++j) r[(q++) * C] = V[i][j];
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                p.mean[(t * C + s) * D + i] = m[i];
#pragma unroll
                for (int j = 0; j < D; ++j) p.cov[((t * C + s) * D + i) * D + j] = V[i][j];
            }
        }
        if (p.unknown) { p.shape[t * C + s] = a; p.rate[t * C + s] = b; }
    }
    p.fe_series[s] = fe;
    if (notpd) atomicOr(p.status, 1);
    if (!(fe - fe == 0.0)) atomicOr(p.status, 2);   // ST_NONFINITE
}

// the backward pass of a smoothing run (see the header): reads the records, writes the smoothed marginals
template <int D>
__global__ void __launch_bounds__(64) k_nlssm_backward(NlssmParams p) {
    EXPR_NO_CONTRACT
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= p.n_series) return;
    // a forward lane that met a value that was not finite, or a V that was not SPD, stopped and left its later records unwritten: the run is refused
    // already (the flag stands, rxhip_sync reports it), and no lane reads records that may not exist.  The forward launch has finished: same stream.
    if (*p.status != 0) return;
    const long long C = p.n_series;
    constexpr int NS = D * (D + 1) / 2, NR = 2 * D + 2 * NS + D * D;
    double ms[D] = {}, Vs[D][D] = {};
    bool notpd = false;
    for (long long t = p.T - 1; t >= 0; --t) {
        double m[D], V[D][D];
        const double* r = p.rec + (t * NR) * C + s;
        int q = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) m[i] = r[(q++) * C];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = i; j < D; ++j) { V[i][j] = r[q * C]; V[j][i] = r[q * C]; ++q; }
        if (t < p.T - 1) {
            double mt[D], P[D][D], Ct[D][D], L[D][D], G[D][D];
            const double* rn = p.rec + ((t + 1) * NR + D + NS) * C + s;
            q = 0;
#pragma unroll
            for (int i = 0; i < D; ++i) mt[i] = rn[(q++) * C];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = i; j < D; ++j) { P[i][j] = rn[q * C]; P[j][i] = rn[q * C]; ++q; }
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) Ct[i][j] = rn[(q++) * C];
            const bool spd = nlssm::chol<D>(P, L, D);
            notpd = notpd || !spd;
#pragma unroll
            for (int i = 0; i < D; ++i) {   // row i of G = C̃ P⁻¹
                double ci[D], z[D], g[D];
#pragma unroll
                for (int j = 0; j < D; ++j) ci[j] = Ct[i][j];
                nlssm::solve_lower<D>(L, ci, z, D);
                nlssm::solve_upper<D>(L, z, g, D);
#pragma unroll
                for (int j = 0; j < D; ++j) G[i][j] = g[j];
            }
            double GD[D][D];   // G (Vˢ₊₁ − P)
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double dm = 0.0;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    dm += G[i][j] * (ms[j] - mt[j]);
                    double v = 0.0;
#pragma unroll
                    for (int k = 0; k < D; ++k) v += G[i][k] * (Vs[k][j] - P[k][j]);
                    GD[i][j] = v;
                }
                m[i] += dm;
            }
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    double v = 0.0;
#pragma unroll
                    for (int k = 0; k < D; ++k) v += GD[i][k] * G[j][k];
                    V[i][j] += v;
                }
            nlssm::symmetrise<D>(V);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            ms[i] = m[i];
            p.mean[(t * C + s) * D + i] = m[i];
#pragma unroll
            for (int j = 0; j < D; ++j) { Vs[i][j] = V[i][j]; p.cov[((t * C + s) * D + i) * D + j] = V[i][j]; }
        }
    }
    if (notpd) atomicOr(p.status, 1);   // ST_NOT_POSDEF
}

// free energy summed over the series (fixed tree), written to every one of the run's `n` per-iteration entries
__global__ void __launch_bounds__(256) k_nlssm_fe(const double* fe_series, long long n_series, double* fe_total, int n, int* status) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (long long s = threadIdx.x; s < n_series; s += 256) acc += fe_series[s];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int wd = 128; wd > 0; wd >>= 1) {
        if ((int)threadIdx.x < wd) sh[threadIdx.x] += sh[threadIdx.x + wd];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int i = 0; i < n; ++i) fe_total[i] = sh[0];
        if (!(sh[0] - sh[0] == 0.0)) atomicOr(status, 2);   // ST_NONFINITE
    }
}

}  // namespace rxhip
#endif

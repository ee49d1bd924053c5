// tests/host_emul/binreg_main.cpp — the `__host__ __device__` helpers of the binomial regression engine (csrc/binreg_kernels.hpp: ω̄ with its series
// near c = 0, ln 2cosh, the per-point term, the free-energy assembly, the schedule constants) compiled for the HOST through the stand-in
// <hip/hip_runtime.h> of this directory, and a SERIAL statement of the device's run around them, in the device's order: ξ and lc once per data set;
// per iteration the pass (tile by tile per chunk as breg::chunks lays them out, one partial per chunk in the packed-lower layout, then P) and the
// update (partials in ascending chunk order, W = W0 + G, the Cholesky inverse in the steps of mvd_chol_inv: L, L⁻¹ column by column, L⁻ᵀL⁻¹, m = Vξ,
// S, F through breg::free_energy).  tests/test_binreg_host.py compares the output with tests/binreg_ref.py.
//
// stdin:  n_cases, then per case   N C d iterations | ξ0 [d] | W0 [d][d] | ln det W0 | init m [d] | init V [d][d] | X [C][N][d] | y [C][N] (nan = missing)
//                                  | n_trials [C][N]
// stdout: first line               tile(d=2) chunk cap(d=2) tile(d=5) chunk cap(d=5) | ω̄(8, 0) | ω̄(1, c²) at c² = 0.999e-3 and 1.001e-3 (both sides of the
//                                  series threshold) | ln 2cosh(1500/2)
//         then per case three lines    mean [iterations][C][d] | cov [iterations][C][d][d] | free energy [iterations][C]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "binreg_kernels.hpp"

using namespace rxhip;

static double read_double() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return std::strtod(tok, nullptr);   // (accepts "nan")
}

// A (d×d SPD, row-major) <- A⁻¹, ln det A: the steps of mvd_chol_inv
static bool chol_inv(int d, std::vector<double>& A, double& logdet) {
    bool ok = true;
    std::vector<double> W((size_t)d * d, 0.0);
    for (int j = 0; j < d; ++j) {
        const double pv = A[j * d + j];
        if (!(pv > 0.0)) ok = false;
        const double s = std::sqrt(pv), is = 1.0 / s;
        for (int i = j; i < d; ++i) A[i * d + j] = i == j ? s : A[i * d + j] * is;
        for (int i = j + 1; i < d; ++i)
            for (int c = j + 1; c <= i; ++c) A[i * d + c] -= A[i * d + j] * A[c * d + j];
    }
    double ld = 0.0;
    for (int j = 0; j < d; ++j) ld += std::log(A[j * d + j]);
    logdet = 2.0 * ld;
    for (int t = 0; t < d; ++t)
        for (int i = 0; i < d; ++i) {
            double s = i == t ? 1.0 : 0.0;
            for (int m = t; m < i; ++m) s -= A[i * d + m] * W[m * d + t];
            W[i * d + t] = i < t ? 0.0 : s / A[i * d + i];
        }
    for (int a = 0; a < d; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int i = a; i < d; ++i) s += W[i * d + a] * W[i * d + b];
            A[a * d + b] = s;
            A[b * d + a] = s;
        }
    return ok;
}

static void print_line(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %.17g" : "%.17g", v[i]);
    std::printf("\n");
}

static void run_case() {
    const long long N = (long long)read_double(), C = (long long)read_double();
    const int d = (int)read_double(), iterations = (int)read_double(), dd = d * d;
    std::vector<double> xi0((size_t)d), W0((size_t)dd), im((size_t)d), iv((size_t)dd);
    for (auto& v : xi0) v = read_double();
    for (auto& v : W0) v = read_double();
    const double logdet_w0 = read_double();
    for (auto& v : im) v = read_double();
    for (auto& v : iv) v = read_double();
    std::vector<double> X((size_t)(C * N * d)), y((size_t)(C * N)), nt((size_t)(C * N));
    for (auto& v : X) v = read_double();
    for (auto& v : y) v = read_double();
    for (auto& v : nt) v = read_double();
    // m0 = W0⁻¹ξ0
    std::vector<double> V0 = W0, m0((size_t)d, 0.0);
    double ld0;
    chol_inv(d, V0, ld0);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) m0[(size_t)i] += V0[(size_t)(i * d + j)] * xi0[(size_t)j];

    const int NP = breg::npart(d), nchunk = breg::chunks(N, d), tile = breg::tile_points(d);
    std::vector<double> means((size_t)(iterations * C * d)), covs((size_t)(iterations * C * dd)), fes((size_t)(iterations * C));
    for (long long prob = 0; prob < C; ++prob) {
        const double *Xp = &X[(size_t)(prob * N * d)], *yp = &y[(size_t)(prob * N)], *np_ = &nt[(size_t)(prob * N)];
        // once per data set: n_eff, ξ, lc
        std::vector<double> neff((size_t)N), xi = xi0;
        double lc = 0.0;
        for (long long i = 0; i < N; ++i) {
            const bool seen = yp[i] == yp[i];
            neff[(size_t)i] = seen ? np_[i] : 0.0;
            if (!seen) continue;
            lc += std::lgamma(np_[i] + 1.0) - std::lgamma(yp[i] + 1.0) - std::lgamma(np_[i] - yp[i] + 1.0);
            for (int c = 0; c < d; ++c) xi[(size_t)c] += (yp[i] - 0.5 * np_[i]) * Xp[i * d + c];
        }
        std::vector<double> S((size_t)dd), m = im, V = iv;
        for (int a = 0; a < d; ++a)
            for (int b = 0; b < d; ++b) S[(size_t)(a * d + b)] = V[(size_t)(a * d + b)] + m[(size_t)a] * m[(size_t)b];
        for (int it = 0; it < iterations; ++it) {
            // the pass: a partial per chunk, each chunk striding over its tiles
            std::vector<double> part((size_t)nchunk * NP, 0.0);
            for (int ch = 0; ch < nchunk; ++ch) {
                double* pt = &part[(size_t)ch * NP];
                for (long long base = (long long)ch * tile; base < N; base += (long long)nchunk * tile)
                    for (long long i = base; i < base + tile && i < N; ++i) {
                        const double* x = Xp + i * d;
                        double c2 = 0.0;
                        for (int a = 0; a < d; ++a) {
                            double s = 0.0;
                            for (int b = 0; b < d; ++b) s += S[(size_t)(a * d + b)] * x[b];
                            c2 += x[a] * s;
                        }
                        double w;
                        pt[NP - 1] += breg::point_term(neff[(size_t)i], c2, w);
                        for (int a = 0; a < d; ++a)
                            for (int b = 0; b <= a; ++b) pt[a * (a + 1) / 2 + b] += (w * x[a]) * x[b];
                    }
            }
            // the update
            std::vector<double> tot((size_t)NP);
            for (int q = 0; q < NP; ++q) {
                double s = part[(size_t)q];
                for (int ch = 1; ch < nchunk; ++ch) s += part[(size_t)ch * NP + q];
                tot[(size_t)q] = s;
            }
            std::vector<double> G((size_t)dd), A((size_t)dd);
            for (int a = 0; a < d; ++a)
                for (int b = 0; b < d; ++b) {
                    const int lo = a > b ? a : b, hi = a > b ? b : a;
                    G[(size_t)(a * d + b)] = tot[(size_t)(lo * (lo + 1) / 2 + hi)];
                    A[(size_t)(a * d + b)] = W0[(size_t)(a * d + b)] + G[(size_t)(a * d + b)];
                }
            double logdet_w;
            if (!chol_inv(d, A, logdet_w)) { std::fprintf(stderr, "not positive definite\n"); std::exit(3); }
            V = A;
            for (int a = 0; a < d; ++a) {
                double s = 0.0;
                for (int b = 0; b < d; ++b) s += V[(size_t)(a * d + b)] * xi[(size_t)b];
                m[(size_t)a] = s;
            }
            double tr_sg = 0.0, tr_w0v = 0.0, quad0 = 0.0, m_dxi = 0.0;
            for (int a = 0; a < d; ++a) {
                for (int b = 0; b < d; ++b) {
                    const double v = V[(size_t)(a * d + b)];
                    S[(size_t)(a * d + b)] = v + m[(size_t)a] * m[(size_t)b];
                    tr_sg += S[(size_t)(a * d + b)] * G[(size_t)(a * d + b)];
                    tr_w0v += W0[(size_t)(a * d + b)] * v;
                    quad0 += W0[(size_t)(a * d + b)] * ((m[(size_t)a] - m0[(size_t)a]) * (m[(size_t)b] - m0[(size_t)b]));
                }
                m_dxi += m[(size_t)a] * (xi[(size_t)a] - xi0[(size_t)a]);
            }
            const size_t row = (size_t)(it * C + prob);
            for (int a = 0; a < d; ++a) means[row * d + a] = m[(size_t)a];
            for (int q = 0; q < dd; ++q) covs[row * dd + q] = V[(size_t)q];
            fes[row] = breg::free_energy(lc, m_dxi, tr_sg, tot[(size_t)(NP - 1)], tr_w0v, quad0, d, logdet_w0, -logdet_w);
        }
    }
    print_line(means);
    print_line(covs);
    print_line(fes);
}

int main() {
    std::printf("%d %d %d %d %.17g %.17g %.17g %.17g\n", breg::tile_points(2), breg::kSmallCap, breg::tile_points(5), breg::kMfmaCap, breg::pg_mean(8.0, 0.0),
                breg::pg_mean(1.0, 0.999e-3), breg::pg_mean(1.0, 1.001e-3), breg::log_2cosh_half(1500.0));
    const int n_cases = (int)read_double();
    for (int i = 0; i < n_cases; ++i) run_case();
    return 0;
}

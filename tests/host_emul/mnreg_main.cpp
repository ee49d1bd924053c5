// tests/host_emul/mnreg_main.cpp — the `__host__ __device__` helpers of the multinomial regression engine (csrc/mnreg_kernels.hpp: the schedule, the
// partial layout, the suffix sums; csrc/binreg_kernels.hpp: the per-point term and the free-energy assembly) compiled for the HOST through the stand-in
// <hip/hip_runtime.h> of this directory, and a SERIAL statement of the device's run around them, in the device's order: the statistics pass (tile by
// tile per chunk as mnreg::chunks lays them out, one partial Y | n | lc per chunk), then the iterations (partials in ascending chunk order, suffix
// sums, W = W0 + diag(ω̄), the Cholesky inverse in the steps of mvd_chol_inv — for d > 32 with L⁻¹ packed as mn_chol_inv_big stores it —, m = Vξ,
// F through breg::free_energy), or the online recursion with ξ and diag(W) carried from step to step.  tests/test_mnreg_host.py compares the output
// with tests/mnreg_ref.py.
//
// stdin:  n_cases, then per case   online N C K iterations | ξ0 [d] | W0 [d][d] | ln det W0 | init m [d] | init V [d][d] | Y [C][N][K] (nan = missing)
// stdout: first line               tile_rows(K) at K = 2, 9, 17, 33, 65 | the chunk cap
//         then per case three lines    offline: mean [iterations][C][d] | cov [iterations][C][d][d] | free energy [iterations][C]
//                                      online:  mean [N][C][d] | cov [N][C][d][d] | F_t [N][C]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mnreg_kernels.hpp"

using namespace rxhip;

static double read_double() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return std::strtod(tok, nullptr);   // (accepts "nan")
}

// A (d×d SPD, row-major) <- A⁻¹, ln det A: the steps of mvd_chol_inv; packed: L⁻¹ stored as mn_chol_inv_big does
static bool chol_inv(int d, std::vector<double>& A, double& logdet, bool packed) {
    bool ok = true;
    std::vector<double> W(packed ? (size_t)d * (d + 1) / 2 : (size_t)d * d, 0.0);
    auto w = [&](int i, int c) -> double& { return packed ? W[(size_t)i * (i + 1) / 2 + c] : W[(size_t)i * d + c]; };
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
        for (int i = t; i < d; ++i) {
            double s = i == t ? 1.0 : 0.0;
            for (int m = t; m < i; ++m) s -= A[i * d + m] * w(m, t);
            w(i, t) = s / A[i * d + i];
        }
    for (int a = 0; a < d; ++a)
        for (int b = 0; b <= a; ++b) {
            double s = 0.0;
            for (int i = a; i < d; ++i) s += w(i, a) * w(i, b);
            A[a * d + b] = s;
            A[b * d + a] = s;
        }
    return ok;
}

static void print_line(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %.17g" : "%.17g", v[i]);
    std::printf("\n");
}

// the statistics pass of one problem in the device's order: Y [K] | n | lc per chunk, the chunks added in ascending order
static std::vector<double> statistics(const double* D, long long N, int K) {
    const int NP = mnreg::npart(K), nchunk = mnreg::chunks(N, K), tile = mnreg::tile_rows(K);
    std::vector<double> part((size_t)nchunk * NP, 0.0), tot((size_t)NP);
    for (int ch = 0; ch < nchunk; ++ch) {
        double* pt = &part[(size_t)ch * NP];
        for (long long base = (long long)ch * tile; base < N; base += (long long)nchunk * tile)
            for (long long i = base; i < base + tile && i < N; ++i) {
                const double* y = D + i * K;
                double s = 0.0;
                for (int k = 0; k < K; ++k) s += y[k];
                if (!(s == s)) continue;   // a row with any NaN is missing
                pt[K] += 1.0;
                pt[K + 1] += std::lgamma(s + 1.0);
                for (int k = 0; k < K; ++k) {
                    pt[k] += y[k];
                    pt[K + 1] -= std::lgamma(y[k] + 1.0);
                }
            }
    }
    for (int q = 0; q < NP; ++q) {
        double s = part[(size_t)q];
        for (int ch = 1; ch < nchunk; ++ch) s += part[(size_t)ch * NP + q];
        tot[(size_t)q] = s;
    }
    return tot;
}

struct State {
    int d;
    std::vector<double> xi, wdiag, m, vd, mp, V;   // ξ and diag(W) of the prior in force, q(ψ), the prior's mean
    double logdet_base;
};

// one iteration (mn_iteration, mn_free_energy): returns F; ω̄ through w
static double iteration(State& s, const std::vector<double>& W0, const std::vector<double>& Srem, const std::vector<double>& kap, double lc, std::vector<double>& w,
                        double& logdet_w) {
    const int d = s.d;
    double P = 0.0;
    for (int k = 0; k < d; ++k) P += breg::point_term(Srem[(size_t)k], s.m[(size_t)k] * s.m[(size_t)k] + s.vd[(size_t)k], w[(size_t)k]);
    std::vector<double> A((size_t)d * d);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) A[(size_t)(i * d + j)] = i == j ? s.wdiag[(size_t)i] + w[(size_t)i] : W0[(size_t)(i * d + j)];
    if (!chol_inv(d, A, logdet_w, d > mnreg::kSmallMaxD)) { std::fprintf(stderr, "not positive definite\n"); std::exit(3); }
    s.V = A;
    for (int a = 0; a < d; ++a) {
        double t = 0.0;
        for (int b = 0; b < d; ++b) t += A[(size_t)(a * d + b)] * (s.xi[(size_t)b] + kap[(size_t)b]);
        s.m[(size_t)a] = t;
    }
    for (int a = 0; a < d; ++a) s.vd[(size_t)a] = A[(size_t)(a * d + a)];
    double tr_sg = 0.0, tr_w0v = 0.0, quad0 = 0.0, m_dxi = 0.0;
    for (int a = 0; a < d; ++a) {
        for (int b = 0; b < d; ++b) {
            const double wb = a == b ? s.wdiag[(size_t)a] : W0[(size_t)(a * d + b)];
            tr_w0v += wb * A[(size_t)(a * d + b)];
            quad0 += wb * ((s.m[(size_t)a] - s.mp[(size_t)a]) * (s.m[(size_t)b] - s.mp[(size_t)b]));
        }
        m_dxi += s.m[(size_t)a] * kap[(size_t)a];
        tr_sg += (s.vd[(size_t)a] + s.m[(size_t)a] * s.m[(size_t)a]) * w[(size_t)a];
    }
    return breg::free_energy(lc, m_dxi, tr_sg, P, tr_w0v, quad0, d, s.logdet_base, -logdet_w);
}

static void run_case() {
    const int online = (int)read_double();
    const long long N = (long long)read_double(), C = (long long)read_double();
    const int K = (int)read_double(), iterations = (int)read_double(), d = K - 1, dd = d * d;
    std::vector<double> xi0((size_t)d), W0((size_t)dd), im((size_t)d), iv((size_t)dd);
    for (auto& v : xi0) v = read_double();
    for (auto& v : W0) v = read_double();
    const double logdet_w0 = read_double();
    for (auto& v : im) v = read_double();
    for (auto& v : iv) v = read_double();
    std::vector<double> Y((size_t)(C * N * K));
    for (auto& v : Y) v = read_double();
    std::vector<double> V0 = W0, m0((size_t)d, 0.0);
    double ld0;
    chol_inv(d, V0, ld0, d > mnreg::kSmallMaxD);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) m0[(size_t)i] += V0[(size_t)(i * d + j)] * xi0[(size_t)j];
    const long long rows = online ? N : iterations;
    std::vector<double> means((size_t)(rows * C * d)), covs((size_t)(rows * C * dd)), fes((size_t)(rows * C));
    std::vector<double> Srem((size_t)K), kap((size_t)K, 0.0), w((size_t)d, 0.0);
    for (long long prob = 0; prob < C; ++prob) {
        const double* D = &Y[(size_t)(prob * N * K)];
        State s;
        s.d = d;
        s.xi = xi0;
        s.wdiag.resize((size_t)d);
        for (int k = 0; k < d; ++k) s.wdiag[(size_t)k] = W0[(size_t)(k * d + k)];
        if (!online) {
            const std::vector<double> tot = statistics(D, N, K);
            mnreg::suffix(K, tot.data(), Srem.data(), kap.data());
            s.m = im; s.V = iv; s.mp = m0; s.logdet_base = logdet_w0;
            s.vd.resize((size_t)d);
            for (int k = 0; k < d; ++k) s.vd[(size_t)k] = iv[(size_t)(k * d + k)];
            for (int it = 0; it < iterations; ++it) {
                double logdet_w;
                const double F = iteration(s, W0, Srem, kap, tot[(size_t)(K + 1)], w, logdet_w);
                const size_t row = (size_t)(it * C + prob);
                for (int a = 0; a < d; ++a) means[row * d + a] = s.m[(size_t)a];
                for (int q = 0; q < dd; ++q) covs[row * dd + q] = s.V[(size_t)q];
                fes[row] = F;
            }
            continue;
        }
        s.V = V0; s.m = m0; s.logdet_base = ld0;
        s.vd.resize((size_t)d);
        for (int k = 0; k < d; ++k) s.vd[(size_t)k] = V0[(size_t)(k * d + k)];
        for (long long t = 0; t < N; ++t) {
            const double* y = D + t * K;
            double sum = 0.0, F = 0.0;
            for (int k = 0; k < K; ++k) sum += y[k];
            if (sum == sum) {
                double lg = 0.0;
                for (int k = 0; k < K; ++k) lg += std::lgamma(y[k] + 1.0);
                mnreg::suffix(K, y, Srem.data(), kap.data());
                const double lc = std::lgamma(Srem[0] + 1.0) - lg;
                s.mp = s.m;
                double logdet_w = s.logdet_base;
                for (int it = 0; it < iterations; ++it) F = iteration(s, W0, Srem, kap, lc, w, logdet_w);
                for (int k = 0; k < d; ++k) {
                    s.xi[(size_t)k] += kap[(size_t)k];
                    s.wdiag[(size_t)k] += w[(size_t)k];
                }
                s.logdet_base = logdet_w;
            }
            const size_t row = (size_t)(t * C + prob);
            for (int a = 0; a < d; ++a) means[row * d + a] = s.m[(size_t)a];
            for (int q = 0; q < dd; ++q) covs[row * dd + q] = s.V[(size_t)q];
            fes[row] = F;
        }
    }
    print_line(means);
    print_line(covs);
    print_line(fes);
}

int main() {
    std::printf("%d %d %d %d %d %d\n", mnreg::tile_rows(2), mnreg::tile_rows(9), mnreg::tile_rows(17), mnreg::tile_rows(33), mnreg::tile_rows(65), mnreg::kChunksCap);
    const int n_cases = (int)read_double();
    for (int i = 0; i < n_cases; ++i) run_case();
    return 0;
}

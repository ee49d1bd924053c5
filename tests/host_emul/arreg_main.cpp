// tests/host_emul/arreg_main.cpp — the `__host__ __device__` helpers of the regression / autoregression engine (csrc/arreg_kernels.hpp: the schedule
// constants, the residual R, the two KL terms and the free-energy assembly; ψ from csrc/digamma.hpp) compiled for the HOST through the stand-in
// <hip/hip_runtime.h> of this directory, and a SERIAL statement of the device's run around them, in the device's order: the pass (tile by tile per
// chunk as arreg::chunks lays them out, one partial per chunk: packed lower G | h | s | n; a dropped row adds exact zeros; in lagged mode every
// operand is read from the series itself at offset i + p − 1 − c, no X is formed), then the iterate kernel's work (partials in ascending chunk and
// series order, Λ = Λ0 + ḡG, the Cholesky inverse in the steps of mvd_chol_inv, m, R, a, b, F).  tests/test_arreg_host.py compares the output
// with tests/arreg_ref.py.
//
// stdin:  n_cases, then per case   lagged N C d iterations shared | Λ0 [d][d] | m0 [d] | a0 b0 ia ib | ln det Λ0
//                                  | lagged = 0: X [C][N][d], y [C][N] (nan = dropped row) | lagged = 1: z [N][C] (N = T; nan = missing)
// stdout: first line               tile(d=4) cap(d=4) tile(d=5) cap(d=5) chunks(0, 5) lag_rows(3, 5) lag_rows(9, 5)
//         then per case six lines  mean [it][G][d] | cov [it][G][d][d] | a [it][G] | b [it][G] | F [it][G] | n [C]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "arreg_kernels.hpp"
#include "digamma.hpp"

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
    const int lagged = (int)read_double();
    const long long N = (long long)read_double(), C = (long long)read_double();
    const int d = (int)read_double(), iterations = (int)read_double(), shared = (int)read_double(), dd = d * d;
    std::vector<double> L0((size_t)dd), m0((size_t)d);
    for (auto& v : L0) v = read_double();
    for (auto& v : m0) v = read_double();
    const double a0 = read_double(), b0 = read_double(), ia = read_double(), ib = read_double(), logdet_l0 = read_double();
    std::vector<double> X, y;
    if (lagged) {
        y.resize((size_t)(N * C));
    } else {
        X.resize((size_t)(C * N * d));
        y.resize((size_t)(C * N));
        for (auto& v : X) v = read_double();
    }
    for (auto& v : y) v = read_double();

    const long long rows = lagged ? arreg::lag_rows(N, d) : N;
    const int NG = arreg::ngram(d), NS = arreg::nstat(d), nchunk = arreg::chunks(rows, d), tile = arreg::tile_rows(d);
    // ---- the pass: a partial per (series, chunk), each chunk striding over its tiles
    std::vector<double> part((size_t)(C * nchunk * NS), 0.0);
    std::vector<double> x((size_t)d);
    for (long long ser = 0; ser < C; ++ser)
        for (int ch = 0; ch < nchunk; ++ch) {
            double* pt = &part[(size_t)((ser * nchunk + ch) * NS)];
            for (long long base = (long long)ch * tile; base < rows; base += (long long)nchunk * tile)
                for (long long i = base; i < base + tile && i < rows; ++i) {
                    double yv;
                    bool ok;
                    if (lagged) {   // z [T][C]: y = z[i + p], x_c = z[i + p − 1 − c]
                        yv = y[(size_t)((i + d) * C + ser)];
                        ok = yv == yv;
                        for (int c = 0; c < d; ++c) {
                            x[(size_t)c] = y[(size_t)((i + d - 1 - c) * C + ser)];
                            ok = ok && x[(size_t)c] == x[(size_t)c];
                        }
                    } else {
                        yv = y[(size_t)(ser * N + i)];
                        ok = yv == yv;
                        for (int c = 0; c < d; ++c) x[(size_t)c] = X[(size_t)((ser * N + i) * d + c)];
                    }
                    if (!ok) {
                        yv = 0.0;
                        for (int c = 0; c < d; ++c) x[(size_t)c] = 0.0;
                    }
                    for (int a = 0; a < d; ++a) {
                        for (int b = 0; b <= a; ++b) pt[a * (a + 1) / 2 + b] += x[(size_t)a] * x[(size_t)b];
                        pt[NG + a] += yv * x[(size_t)a];
                    }
                    pt[NG + d] += yv * yv;
                    pt[NG + d + 1] += ok ? 1.0 : 0.0;
                }
        }
    // ---- the iterate kernel
    const long long G = shared ? 1 : C;
    std::vector<double> wm0((size_t)d, 0.0), nser((size_t)C);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) wm0[(size_t)i] += L0[(size_t)(i * d + j)] * m0[(size_t)j];
    const double lgamma_a0 = std::lgamma(a0), log_b0 = std::log(b0);
    std::vector<double> means((size_t)(iterations * G * d)), covs((size_t)(iterations * G * dd)), as((size_t)(iterations * G)), bs((size_t)(iterations * G)),
        fes((size_t)(iterations * G));
    for (long long grp = 0; grp < G; ++grp) {
        const long long first = shared ? 0 : grp, count = shared ? C : 1;
        std::vector<double> tot((size_t)NS);
        for (int q = 0; q < NS; ++q) {
            double total = 0.0;
            for (long long s = first; s < first + count; ++s) {
                double acc = part[(size_t)(s * nchunk * NS + q)];
                for (int c = 1; c < nchunk; ++c) acc += part[(size_t)((s * nchunk + c) * NS + q)];
                if (q == NS - 1) nser[(size_t)s] = acc;
                total = s == first ? acc : total + acc;
            }
            tot[(size_t)q] = total;
        }
        std::vector<double> Gm((size_t)dd), A((size_t)dd), m((size_t)d);
        for (int a = 0; a < d; ++a)
            for (int b = 0; b < d; ++b) {
                const int lo = a > b ? a : b, hi = a > b ? b : a;
                Gm[(size_t)(a * d + b)] = tot[(size_t)(lo * (lo + 1) / 2 + hi)];
            }
        const double* h = &tot[(size_t)NG];
        const double ssq = tot[(size_t)(NG + d)], n = tot[(size_t)(NG + d + 1)];
        const double a = a0 + 0.5 * n, psi_a = digamma_dev(a), lgamma_a = std::lgamma(a);
        double gbar = ia / ib;
        for (int it = 0; it < iterations; ++it) {
            for (int q = 0; q < dd; ++q) A[(size_t)q] = L0[(size_t)q] + gbar * Gm[(size_t)q];
            double logdet_l;
            if (!chol_inv(d, A, logdet_l)) { std::fprintf(stderr, "not positive definite\n"); std::exit(3); }
            for (int i = 0; i < d; ++i) {
                double s = 0.0;
                for (int j = 0; j < d; ++j) s += A[(size_t)(i * d + j)] * (wm0[(size_t)j] + gbar * h[j]);
                m[(size_t)i] = s;
            }
            double tr_sg = 0.0, mh = 0.0, tr_l0v = 0.0, quad0 = 0.0;
            for (int i = 0; i < d; ++i) {
                for (int j = 0; j < d; ++j) {
                    const double v = A[(size_t)(i * d + j)];
                    tr_sg += (v + m[(size_t)i] * m[(size_t)j]) * Gm[(size_t)(i * d + j)];
                    tr_l0v += L0[(size_t)(i * d + j)] * v;
                    quad0 += L0[(size_t)(i * d + j)] * ((m[(size_t)i] - m0[(size_t)i]) * (m[(size_t)j] - m0[(size_t)j]));
                }
                mh += m[(size_t)i] * h[i];
            }
            const double R = arreg::residual(ssq, mh, tr_sg), b = b0 + 0.5 * R, log_b = std::log(b);
            const size_t row = (size_t)(it * G + grp);
            for (int i = 0; i < d; ++i) means[row * d + i] = m[(size_t)i];
            for (int q = 0; q < dd; ++q) covs[row * dd + q] = A[(size_t)q];
            as[row] = a;
            bs[row] = b;
            fes[row] = arreg::free_energy(n, a, b, R, psi_a, log_b, arreg::normal_kl(tr_l0v, quad0, d, logdet_l0, -logdet_l),
                                          arreg::gamma_kl(a, b, a0, b0, psi_a, lgamma_a, lgamma_a0, log_b, log_b0));
            gbar = a / b;
        }
    }
    print_line(means);
    print_line(covs);
    print_line(as);
    print_line(bs);
    print_line(fes);
    print_line(nser);
}

int main() {
    std::printf("%d %d %d %d %d %lld %lld\n", arreg::tile_rows(4), arreg::kSmallCap, arreg::tile_rows(5), arreg::kMfmaCap, arreg::chunks(0, 5), arreg::lag_rows(3, 5),
                arreg::lag_rows(9, 5));
    const int n_cases = (int)read_double();
    for (int i = 0; i < n_cases; ++i) run_case();
    return 0;
}

// tests/host_emul/gammamix_main.cpp — the `__host__ __device__` helpers of csrc/gammamix_kernels.hpp and csrc/digamma.hpp on the HOST, compiled by g++ through
// the stand-in <hip/hip_runtime.h> of this directory (tests/test_gammamix_host.py).  The Gamma mixture engine's iteration is driven serially in the device's
// order: the points of a workgroup by thread (grid stride), the wavefront's shuffle tree, the four wavefronts in wave order, the chunks in ascending order,
// then per component gammamix::update_component — the function a lane of k_gammamix_update runs — with the sums over the components in ascending order.
//   gammamix_main            stdin: n_cases, then per case  N K iterations  prior[5][K]  init[4][K]  y[N]   (nan = a missing point)
//                            stdout: the constants line, then per case 6 lines: a | e | f | alpha ([iterations][K] each) | F [iterations] | q(z) [N][K]
//   gammamix_main trigamma   stdin: n, then n values x;  stdout: trigamma_dev(x), digamma_dev(x) per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gammamix_kernels.hpp"

using namespace rxhip;

static double wave_tree(double* v) {   // wave_sum: lane l adds lane l + off, off = 32 … 1; lane 0 holds the sum
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] += v[l + off];
    return v[0];
}

template <int KT>
static void run_case(long long N, int K, int iterations, const double* prior, const double* init, const std::vector<double>& y) {
    constexpr int NQ = 3 * KT + 1;
    const int nchunk = gammamix::chunks(N);
    std::vector<double> a(init, init + K), e(init + K, init + 2 * K), f(init + 2 * K, init + 3 * K), al(init + 3 * K, init + 4 * K);
    const double *pc = prior, *pd = prior + K, *pe = prior + 2 * K, *pf = prior + 3 * K, *al0 = prior + 4 * K;
    std::vector<double> ly((size_t)N), sc(3 * KT), resp((size_t)N * K, 0.0);
    std::vector<char> ok((size_t)N);
    for (long long i = 0; i < N; ++i) {
        ok[(size_t)i] = y[(size_t)i] == y[(size_t)i];
        ly[(size_t)i] = ok[(size_t)i] ? log(y[(size_t)i]) : 0.0;
    }
    auto constants = [&]() {
        double asum = 0.0;
        for (int k = 0; k < K; ++k) asum += al[k];
        for (int k = 0; k < KT; ++k) {
            double c0 = -1e300, c1 = 0.0, c2 = 0.0;
            if (k < K) gammamix::pass_constants(a[k], e[k], f[k], digamma_dev(al[k]) - digamma_dev(asum), lgamma(a[k]), c0, c1, c2);
            sc[k] = c0; sc[KT + k] = c1; sc[2 * KT + k] = c2;
        }
    };
    constants();
    std::vector<double> ha, he, hf, hal, hfe;
    for (int it = 0; it < iterations; ++it) {
        double tot[NQ];
        for (int b = 0; b < nchunk; ++b) {
            static double acc[NQ][256];
            for (int q = 0; q < NQ; ++q)
                for (int t = 0; t < 256; ++t) acc[q][t] = 0.0;
            for (int t = 0; t < 256; ++t) {
                double S0[KT], S1[KT], SL[KT], Hz = 0.0;
                for (int k = 0; k < KT; ++k) S0[k] = S1[k] = SL[k] = 0.0;
                for (long long i = (long long)b * 256 + t; i < N; i += (long long)nchunk * 256) {
                    double r[KT];
                    const bool good = ok[(size_t)i];
                    gammamix::point<KT>(good ? y[(size_t)i] : 1.0, ly[(size_t)i], good ? 1.0 : 0.0, sc.data(), S0, S1, SL, Hz, r);
                    if (it == iterations - 1)
                        for (int k = 0; k < K; ++k) resp[(size_t)i * K + k] = r[k];
                }
                for (int k = 0; k < KT; ++k) { acc[k][t] = S0[k]; acc[KT + k][t] = S1[k]; acc[2 * KT + k][t] = SL[k]; }
                acc[3 * KT][t] = Hz;
            }
            for (int q = 0; q < NQ; ++q) {
                double w[4];
                for (int wv = 0; wv < 4; ++wv) w[wv] = wave_tree(&acc[q][64 * wv]);
                const double part = ((w[0] + w[1]) + w[2]) + w[3];
                tot[q] = b == 0 ? part : tot[q] + part;
            }
        }
        // the update, a component at a time, as gammamix_update_lane
        double asum = 0.0, a0sum = 0.0;
        std::vector<double> nal(K);
        for (int k = 0; k < K; ++k) {
            nal[k] = al0[k] + tot[k];
            asum += nal[k];
            a0sum += al0[k];
        }
        double sum = 0.0;
        for (int k = 0; k < K; ++k) {
            const gammamix::ComponentUpdate u = gammamix::update_component(tot[k], tot[KT + k], tot[2 * KT + k], pc[k], pd[k], pe[k], pf[k], nal[k], al0[k], asum, a[k], e[k], f[k]);
            a[k] = u.a; e[k] = u.e; f[k] = u.f; al[k] = nal[k];
            sum += u.fk;
        }
        hfe.push_back(gammamix::fe_total(sum, tot[3 * KT], asum, a0sum));
        ha.insert(ha.end(), a.begin(), a.end());
        he.insert(he.end(), e.begin(), e.end());
        hf.insert(hf.end(), f.begin(), f.end());
        hal.insert(hal.end(), al.begin(), al.end());
        constants();
    }
    for (const std::vector<double>* v : {&ha, &he, &hf, &hal, &hfe, &resp}) {
        for (double x : *v) printf("%.17g ", x);
        printf("\n");
    }
}

static double read_double() {
    char buf[64];
    if (scanf("%63s", buf) != 1) exit(2);
    return strtod(buf, nullptr);   // accepts nan
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "trigamma")) {
        int n = 0;
        if (scanf("%d", &n) != 1) return 2;
        for (int i = 0; i < n; ++i) {
            const double x = read_double();
            printf("%.17g %.17g\n", trigamma_dev(x), digamma_dev(x));
        }
        return 0;
    }
    int ncases = 0;
    if (scanf("%d", &ncases) != 1) return 2;
    printf("%d %d %d %d\n", gammamix::kMaxK, gammamix::kTile, gammamix::kChunkCap, gammamix::kNewtonCap);
    for (int c = 0; c < ncases; ++c) {
        long long N;
        int K, iters;
        if (scanf("%lld %d %d", &N, &K, &iters) != 3 || N < 1 || K < 1 || K > gammamix::kMaxK || iters < 1) return 2;
        std::vector<double> prior(5 * (size_t)K), init(4 * (size_t)K), y((size_t)N);
        for (double& v : prior) v = read_double();
        for (double& v : init) v = read_double();
        for (double& v : y) v = read_double();
        switch (gammamix::padded_k(K)) {
            case 1: run_case<1>(N, K, iters, prior.data(), init.data(), y); break;
            case 2: run_case<2>(N, K, iters, prior.data(), init.data(), y); break;
            case 4: run_case<4>(N, K, iters, prior.data(), init.data(), y); break;
            case 8: run_case<8>(N, K, iters, prior.data(), init.data(), y); break;
            default: run_case<16>(N, K, iters, prior.data(), init.data(), y);
        }
    }
    return 0;
}

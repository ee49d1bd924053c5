// tests/host_emul/lar_main.cpp — the `__host__ __device__` helpers of the latent autoregressive engine (csrc/lar_kernels.hpp: the band entry, the
// LDLᵀ row step, the back-substitution / selected-inverse step, the statistics, the θ/γ update with its Cholesky, digamma and KL terms, the energy
// of a series) compiled for the HOST through the stand-in <hip/hip_runtime.h> of this directory and driven SERIALLY, one series after the other,
// in the order of the device: run_case restates k_lar_sweep's two loops (interior rows from the diagonal sums, boundary rows from lam_entry, the
// record of a row kept in an array where the device keeps it in memory) and the launch sequence of rxhip::lar_run_async (init → per iteration
// sweep → reduce when shared → update → free energy).  tests/test_lar_host.py compares the output with tests/lar_ref.py.
//
// stdin:  n_cases, then per case   T C p iterations shared | τ a0 b0 init_a init_b | mθ0 [p] | Wθ0 [p][p] | m0 [p] | W0 [p][p] | init mθ [p] |
//                                  init Vθ [p][p] | ln det Wθ0 | ln det W0 | y [T][C] (nan = missing)
// stdout: per case six lines       x mean [T][C][p] | x cov [T][C][p][p] | θ mean [iterations][G][p] | θ cov [iterations][G][p][p] |
//                                  γ shape, rate [iterations][G][2] | free energy [iterations]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lar_kernels.hpp"

using namespace rxhip;

static double read_double() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return std::strtod(tok, nullptr);   // (accepts "nan")
}

struct Case {
    int T, C, iterations, shared;
    std::vector<double> cst, init, y;
};

template <int P>
static void sweep(const Case& cs, int s, const double* gm, double* zmean, double* band, double* stat) {
    const long long T = cs.T, C = cs.C, n = T + P;
    const lar::Consts c = lar::consts(cs.cst.data(), P);
    const double mg = gm[(P + 1) * (P + 1)], tau = c.tau;
    double cb[P + 1];
    for (int k = 0; k <= P; ++k) cb[k] = lar::lam_entry<P>(P, k, (long long)1 << 40, gm, mg, c.w0, 0.0);
    std::vector<double> rec((size_t)(n * (P + 2)));
    lar::FwdWindow<P> fw;
    lar::fwd_clear<P>(fw);
    for (long long i = 0; i < n; ++i) {
        const double yv = i >= P ? cs.y[(size_t)((i - P) * C + s)] : 0.0;
        const bool seen = i >= P && yv == yv;
        const double tau_i = seen ? tau : 0.0;
        double a[P + 1], h;
        if (i >= P && i < T) {
            for (int k = 1; k <= P; ++k) a[k] = cb[k];
            a[0] = cb[0] + tau_i;
            h = 0.0 + (seen ? tau * yv : 0.0);
        } else {
            for (int k = 0; k <= P; ++k) a[k] = lar::lam_entry<P>(i, k, n, gm, mg, c.w0, tau_i);
            h = (i < P ? c.h0[P - 1 - i] : 0.0) + (seen ? tau * yv : 0.0);
        }
        double l[P], invd, u;
        lar::row_step<P>(fw, a, h, l, invd, u);
        double* r = &rec[(size_t)(i * (P + 2))];
        for (int k = 0; k < P; ++k) r[k] = l[k];
        r[P] = invd;
        r[P + 1] = u;
    }
    lar::BwdWindow<P> bw;
    lar::bwd_clear<P>(bw);
    double S[P + 1][P + 1] = {};
    double ey = 0.0, nobs = 0.0, e0 = 0.0, logdet = 0.0;
    for (long long i = n - 1; i >= 0; --i) {
        const double* r = &rec[(size_t)(i * (P + 2))];
        double l[P], mi, row[P + 1];
        for (int k = 0; k < P; ++k) l[k] = r[k];
        lar::back_step<P>(bw, r[P], r[P + 1], mi, row);
        if (i < T) lar::accumulate_s<P>(S, bw, mi, row);
        const double yv = i >= P ? cs.y[(size_t)((i - P) * C + s)] : 0.0;
        if (i >= P && yv == yv) {
            const double d = yv - mi;
            ey += d * d + row[0];
            nobs += 1.0;
        }
        if (i < P) e0 += lar::e0_terms<P>(i, bw, mi, row, c.w0, c.m0);
        logdet -= log(r[P]);
        zmean[i] = mi;
        for (int k = 0; k <= P; ++k) band[i * (P + 1) + k] = row[k];
        lar::back_shift<P>(bw, l, mi, row);
    }
    for (int ka = 0; ka <= P; ++ka)
        for (int kb = 0; kb <= P; ++kb) stat[ka * (P + 1) + kb] = ka <= kb ? S[ka][kb] : S[kb][ka];
    const int e = (P + 1) * (P + 1);
    stat[e] = ey; stat[e + 1] = nobs; stat[e + 2] = e0; stat[e + 3] = logdet;
}

template <int P>
static void run_case(const Case& cs) {
    const int T = cs.T, C = cs.C, G = cs.shared ? 1 : C, n = T + P, NQ = lar::nq(P), NG = lar::ng(P), NS = lar::ns(P);
    const lar::Consts c = lar::consts(cs.cst.data(), P);
    std::vector<double> gm((size_t)(G * NG)), hist((size_t)(cs.iterations * G * NQ)), kl((size_t)G), stat((size_t)(C * NS)), sum((size_t)NS), fe;
    std::vector<double> zmean((size_t)(C * n)), band((size_t)(C * n * (P + 1)));
    for (int g = 0; g < G; ++g) lar::make_g(cs.init.data(), P, &gm[(size_t)(g * NG)]);
    for (int it = 0; it < cs.iterations; ++it) {
        for (int s = 0; s < C; ++s)
            sweep<P>(cs, s, &gm[(size_t)((cs.shared ? 0 : s) * NG)], &zmean[(size_t)(s * n)], &band[(size_t)(s * n * (P + 1))], &stat[(size_t)(s * NS)]);
        if (cs.shared)
            for (int e = 0; e < NS; ++e) {
                double acc = stat[(size_t)e];
                for (int s = 1; s < C; ++s) acc += stat[(size_t)(s * NS + e)];
                sum[(size_t)e] = acc;
            }
        for (int g = 0; g < G; ++g) {
            const double* old = it == 0 ? cs.init.data() : &hist[(size_t)(((it - 1) * G + g) * NQ)];
            const double mg_old = old[P + P * P] / old[P + P * P + 1];
            bool ok = true;
            kl[(size_t)g] = lar::update_theta_gamma(cs.shared ? sum.data() : &stat[(size_t)(g * NS)], 1, mg_old, (double)(cs.shared ? C : 1) * (double)T, c, P,
                                                    &hist[(size_t)((it * G + g) * NQ)], &gm[(size_t)(g * NG)], &ok);
            if (!ok) { std::fprintf(stderr, "not positive definite\n"); std::exit(3); }
        }
        double f = 0.0;
        for (int s = 0; s < C; ++s) {
            const int g = cs.shared ? 0 : s;
            double fs = lar::series_energy(&stat[(size_t)(s * NS)], 1, &hist[(size_t)((it * G + g) * NQ)], c, P, T);
            if (!cs.shared) fs += kl[(size_t)s];
            f += fs;   // (the device adds the series in a tree)
        }
        if (cs.shared) f += kl[0];
        fe.push_back(f);
    }
    for (int t = 1; t <= T; ++t)
        for (int s = 0; s < C; ++s)
            for (int a = 0; a < P; ++a) std::printf("%.17g ", zmean[(size_t)(s * n + t + P - 1 - a)]);
    std::printf("\n");
    for (int t = 1; t <= T; ++t)
        for (int s = 0; s < C; ++s)
            for (int a = 0; a < P; ++a)
                for (int b = 0; b < P; ++b) {
                    const int ia = t + P - 1 - a, ib = t + P - 1 - b, lo = ia < ib ? ia : ib, lag = ia < ib ? ib - ia : ia - ib;
                    std::printf("%.17g ", band[(size_t)((s * n + lo) * (P + 1) + lag)]);
                }
    std::printf("\n");
    for (int r = 0; r < cs.iterations * G; ++r)
        for (int a = 0; a < P; ++a) std::printf("%.17g ", hist[(size_t)(r * NQ + a)]);
    std::printf("\n");
    for (int r = 0; r < cs.iterations * G; ++r)
        for (int a = 0; a < P * P; ++a) std::printf("%.17g ", hist[(size_t)(r * NQ + P + a)]);
    std::printf("\n");
    for (int r = 0; r < cs.iterations * G; ++r) std::printf("%.17g %.17g ", hist[(size_t)(r * NQ + P + P * P)], hist[(size_t)(r * NQ + P + P * P + 1)]);
    std::printf("\n");
    for (double f : fe) std::printf("%.17g ", f);
    std::printf("\n");
}

int main() {
    const int n_cases = (int)read_double();
    for (int k = 0; k < n_cases; ++k) {
        Case cs;
        cs.T = (int)read_double(); cs.C = (int)read_double();
        const int p = (int)read_double();
        cs.iterations = (int)read_double(); cs.shared = (int)read_double();
        if (cs.T < 1 || cs.C < 1 || p < 1 || p > lar::kMaxP || cs.iterations < 1) { std::fprintf(stderr, "bad case\n"); return 2; }
        const double tau = read_double(), a0 = read_double(), b0 = read_double(), ia = read_double(), ib = read_double();
        cs.cst.assign((size_t)lar::nconst(p), 0.0);
        cs.init.assign((size_t)lar::nq(p), 0.0);
        double* c = cs.cst.data();
        double *w0 = c, *m0 = c + p * p, *h0 = m0 + p, *wth0 = h0 + p, *mth0 = wth0 + p * p, *wm0 = mth0 + p, *sc = wm0 + p;
        for (int i = 0; i < p; ++i) mth0[i] = read_double();
        for (int i = 0; i < p * p; ++i) wth0[i] = read_double();
        for (int i = 0; i < p; ++i) m0[i] = read_double();
        for (int i = 0; i < p * p; ++i) w0[i] = read_double();
        for (int i = 0; i < p + p * p; ++i) cs.init[(size_t)i] = read_double();
        cs.init[(size_t)(p + p * p)] = ia;
        cs.init[(size_t)(p + p * p + 1)] = ib;
        for (int i = 0; i < p; ++i) {
            double s0 = 0.0, s1 = 0.0;
            for (int j = 0; j < p; ++j) { s0 += w0[i * p + j] * m0[j]; s1 += wth0[i * p + j] * mth0[j]; }
            h0[i] = s0;
            wm0[i] = s1;
        }
        sc[0] = a0; sc[1] = b0;
        sc[3] = read_double();   // ln det Wθ0
        sc[2] = read_double();   // ln det W0
        sc[4] = tau; sc[5] = lgamma(a0); sc[6] = log(b0); sc[7] = log(tau);
        cs.y.resize((size_t)cs.T * (size_t)cs.C);
        for (double& v : cs.y) v = read_double();
        switch (p) {
            case 1: run_case<1>(cs); break;
            case 2: run_case<2>(cs); break;
            case 3: run_case<3>(cs); break;
            case 4: run_case<4>(cs); break;
            case 5: run_case<5>(cs); break;
            case 6: run_case<6>(cs); break;
            case 7: run_case<7>(cs); break;
            default: run_case<8>(cs); break;
        }
    }
    return 0;
}

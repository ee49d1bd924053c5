// tests/host_emul/hmm_main.cpp — the `__host__ __device__` helpers of the hidden Markov model engine (csrc/hmm_kernels.hpp: the table of a Dirichlet
// column with its KL term and the digamma under it, the forward and backward step of one state given the row's values, the row of ξ) compiled for
// the HOST through the stand-in <hip/hip_runtime.h> of this directory and driven SERIALLY over a row: where the device gives state i a lane and
// broadcasts by shuffles, the loops below visit i = 0 … R−1 with the row's values in an array.  Same padded rows (R the power of two ≥ K, zeros
// beyond K), same order of every sum inside a state; the row sums run in ascending i where the device uses a butterfly.  The launch sequence of
// rxhip::hmm_run_async (tables, then per iteration sweep → update → free energy) is restated in run_case.  tests/test_hmm_host.py compares the
// output with tests/hmm_ref.py.
//
// stdin:  n_cases, then per case   T K M iterations | π [K] | prior_A [K][K] | prior_B [M][K] | init_A | init_B | x [T] (nan = missing)
// stdout: first line                hmm::kMinNormaliser
//         per case five lines       γ [T+1][K] | A counts [K][K] | B counts [M][K] | free energy [iterations] | refused (0 / 1), smallest normaliser
//         then, for the rest of stdin, one line ψ(v) per value v
// `refused` is the guard of k_hmm_sweep restated: 1 if a normaliser c_t or d_t of any sweep was at or below hmm::kMinNormaliser or not finite (the
// device then raises its status bit and rxhip_run returns RXHIP_ERR_NONFINITE_FE); the other four lines are printed as computed either way.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hmm_kernels.hpp"

using namespace rxhip;

static double read_double() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return std::strtod(tok, nullptr);   // (accepts "nan")
}

struct Case {
    int T, K, M, iterations;
    std::vector<double> pi, prior, init, x;   // prior / init: the K×K block of A, then the M×K block of B
};

// all columns of a parameter set: what k_hmm_tables / k_hmm_update do with a thread per column
static double tables(const Case& c, const std::vector<double>& counts, const std::vector<double>* stat, std::vector<double>& l, std::vector<double>& t) {
    const int K = c.K, M = c.M;
    double kl = 0.0;
    for (int col = 0; col < 2 * K; ++col) {
        const bool isB = col >= K;
        const int off = (isB ? K * K : 0) + (isB ? col - K : col);
        kl += hmm::column_table(&counts[(size_t)off], &c.prior[(size_t)off], stat ? &(*stat)[(size_t)off] : nullptr, isB ? M : K, K, &l[(size_t)off], &t[(size_t)off]);
    }
    return kl;
}

template <int R>
static void run_case(const Case& c) {
    const int T = c.T, K = c.K, M = c.M, KM = (K + M) * K;
    std::vector<double> counts = c.init, l_old((size_t)KM), l_new((size_t)KM), tt((size_t)KM), stat((size_t)KM), fe;
    std::vector<double> alpha((size_t)(T + 1) * R, 0.0), gamma((size_t)(T + 1) * R, 0.0);
    tables(c, counts, nullptr, l_old, tt);
    bool bad = false;
    double smallest = INFINITY;
    auto guard = [&](double v) {   // k_hmm_sweep's check of c_t and d_t
        bad = bad || !(v > hmm::kMinNormaliser) || !(v - v == 0.0);
        if (!(v >= smallest)) smallest = v;   // (keeps a NaN)
    };
    for (int it = 0; it < c.iterations; ++it) {
        const double *At = tt.data(), *Bt = At + K * K;
        double arow[R][R], acol[R][R], nrow[R][R];
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < R; ++j) {
                const bool in = i < K && j < K;
                arow[i][j] = in ? At[i * K + j] : 0.0;
                acol[i][j] = in ? At[j * K + i] : 0.0;
                nrow[i][j] = 0.0;
            }
        auto factor = [&](double xv, int i) { return i < K ? (xv == xv ? Bt[hmm::symbol(xv, M) * K + i] : 1.0) : 0.0; };
        for (double& v : stat) v = 0.0;
        // forward
        for (int i = 0; i < R; ++i) alpha[(size_t)i] = i < K ? c.pi[(size_t)i] : 0.0;
        double logz = 0.0;
        for (int t = 1; t <= T; ++t) {
            const double* al = &alpha[(size_t)(t - 1) * R];
            double v[R], cs = 0.0;
            for (int i = 0; i < R; ++i) v[i] = hmm::forward_state<R>(arow[i], al, factor(c.x[(size_t)t - 1], i));
            for (int i = 0; i < R; ++i) cs += v[i];
            guard(cs);
            for (int i = 0; i < R; ++i) alpha[(size_t)t * R + i] = v[i] / cs;
            logz += log(cs);
        }
        // backward
        double b[R];
        for (int i = 0; i < R; ++i) b[i] = 1.0;
        for (int t = T; t >= 1; --t) {
            const double xt = c.x[(size_t)t - 1];
            const double *a = &alpha[(size_t)t * R], *am = &alpha[(size_t)(t - 1) * R];
            double w[R], bt[R], d = 0.0;
            for (int i = 0; i < R; ++i) {
                const double gam = a[i] * b[i];
                gamma[(size_t)t * R + i] = gam;
                if (xt == xt && i < K) stat[(size_t)(K * K + hmm::symbol(xt, M) * K + i)] += gam;
                w[i] = factor(xt, i) * b[i];
            }
            for (int i = 0; i < R; ++i) bt[i] = hmm::backward_state<R>(acol[i], w);
            for (int i = 0; i < R; ++i) d += am[i] * bt[i];
            guard(d);
            for (int i = 0; i < R; ++i) {
                hmm::accumulate_xi<R>(nrow[i], arow[i], am, w[i] / d);
                b[i] = bt[i] / d;
            }
        }
        for (int i = 0; i < R; ++i) gamma[(size_t)i] = alpha[(size_t)i] * b[i];
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) stat[(size_t)(i * K + j)] = nrow[i][j];
        // update, tables of the new counts, free energy (k_hmm_update, k_hmm_fe)
        for (int e = 0; e < KM; ++e) counts[(size_t)e] = c.prior[(size_t)e] + stat[(size_t)e];
        const double kl = tables(c, counts, &stat, l_new, tt);
        double f = -logz;
        for (int e = 0; e < KM; ++e) f += stat[(size_t)e] * (l_old[(size_t)e] - l_new[(size_t)e]);
        fe.push_back(f + kl);
        l_old.swap(l_new);
    }
    for (int t = 0; t <= T; ++t)
        for (int i = 0; i < K; ++i) std::printf("%.17g ", gamma[(size_t)t * R + i]);
    std::printf("\n");
    for (int e = 0; e < K * K; ++e) std::printf("%.17g ", counts[(size_t)e]);
    std::printf("\n");
    for (int e = K * K; e < KM; ++e) std::printf("%.17g ", counts[(size_t)e]);
    std::printf("\n");
    for (double f : fe) std::printf("%.17g ", f);
    std::printf("\n");
    std::printf("%d %.17g\n", bad ? 1 : 0, smallest);
}

int main() {
    const int n_cases = (int)read_double();
    std::printf("%.17g\n", hmm::kMinNormaliser);
    for (int cs = 0; cs < n_cases; ++cs) {
        Case c;
        c.T = (int)read_double(); c.K = (int)read_double(); c.M = (int)read_double(); c.iterations = (int)read_double();
        if (c.T < 1 || c.K < 2 || c.K > hmm::kMaxK || c.M < 2 || c.M > hmm::kMaxM || c.iterations < 1) { std::fprintf(stderr, "bad case\n"); return 2; }
        const size_t KM = (size_t)(c.K + c.M) * (size_t)c.K;
        c.pi.resize((size_t)c.K); c.prior.resize(KM); c.init.resize(KM); c.x.resize((size_t)c.T);
        for (double& v : c.pi) v = read_double();
        for (double& v : c.prior) v = read_double();
        for (double& v : c.init) v = read_double();
        for (double& v : c.x) v = read_double();
        if (c.K <= 2) run_case<2>(c);
        else if (c.K <= 4) run_case<4>(c);
        else if (c.K <= 8) run_case<8>(c);
        else run_case<16>(c);
    }
    for (;;) {
        char tok[64];
        if (std::scanf("%63s", tok) != 1) break;
        std::printf("%.17g\n", digamma_dev(std::strtod(tok, nullptr)));
    }
    return 0;
}

// tests/host_emul/probit_main.cpp — the probit engine's kernels (csrc/probit_kernels.hpp) compiled for the HOST through the stand-in <hip/hip_runtime.h> of this
// directory and run one "thread" at a time: the same __host__ __device__ functions, the same loops and the same indexing as on the device, with the launch
// sequence of rxhip::probit_run_async restated below (tests/test_probit_host.py compares the output with tests/probit_ref.py).  Also prints the tilted moments
// and log Φ on request, for the tail checks.
//
// stdin:  n_cases, then per case   T C a c q m0 v0 n_gh iterations   |   T·C observations [T][C] (nan = missing)   |   n_gh nodes   |   n_gh weights/√π
// stdout: per case and series one line each of   mean[0 … T]   var[0 … T]   fe[1 … iterations]
#include <cstdio>
#include <cstdlib>
#include <vector>

#define RXHIP_HOST_EMUL 1
#include "probit_kernels.hpp"

using namespace rxhip;

template <typename F>
static void launch(unsigned gx, unsigned gy, unsigned bx, F&& kernel) {
    gridDim.x = gx; gridDim.y = gy; blockDim.x = bx;
    for (unsigned by = 0; by < gy; ++by)
        for (unsigned b = 0; b < gx; ++b)
            for (unsigned t = 0; t < bx; ++t) {
                blockIdx.x = b; blockIdx.y = by; threadIdx.x = t;
                kernel();
            }
}

static double read_double() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return std::strtod(tok, nullptr);   // (accepts "nan")
}

int main() {
    const int n_cases = (int)read_double();
    for (int cs = 0; cs < n_cases; ++cs) {
        const long long T = (long long)read_double(), C = (long long)read_double();
        ProbitParams p;
        p.T = T; p.n_series = C;
        p.a = read_double(); p.c = read_double(); p.q = read_double(); p.m0 = read_double(); p.v0 = read_double();
        p.n_gh = (int)read_double();
        const int iterations = (int)read_double();
        const size_t R = (size_t)T + 1, n = R * (size_t)C;
        p.echunk = PROBIT_ECHUNK;
        const long long chunks = (T + p.echunk - 1) / p.echunk;
        std::vector<double> y((size_t)(T * C)), gh(64, 0.0), xi(n, 0.0), w(n, 0.0), pm(n), pv(n), mean(n), var(n), feg((size_t)C), fep((size_t)(chunks * C)),
            fes((size_t)iterations * (size_t)C);
        for (double& v : y) v = read_double();
        for (int i = 0; i < p.n_gh; ++i) gh[(size_t)i] = read_double();
        for (int i = 0; i < p.n_gh; ++i) gh[32 + (size_t)i] = read_double();
        int status = 0;
        p.y = y.data(); p.xi = xi.data(); p.w = w.data(); p.pm = pm.data(); p.pv = pv.data(); p.mean = mean.data(); p.var = var.data();
        p.fe_gauss = feg.data(); p.fe_part = fep.data(); p.fe_series = fes.data(); p.gh = gh.data(); p.status = &status;
        launch(1, 1, 256, [&] { k_probit_check_y(p.y, T * C, p.status); });
        if (status) { std::printf("bad_y\n"); continue; }
        const unsigned g = (unsigned)((C + 63) / 64), eg = (unsigned)((C + 255) / 256);
        for (int i = 0; i <= iterations; ++i) {
            const bool update = i < iterations, fe = i >= 1;
            if (update && !fe) launch(g, 1, 64, [&] { k_probit_sweep<true, false, false>(p); });
            else if (update) launch(g, 1, 64, [&] { k_probit_sweep<true, true, true>(p); });
            else launch(g, 1, 64, [&] { k_probit_sweep<false, true, true>(p); });
            if (fe) {
                launch(eg, (unsigned)chunks, 256, [&] { k_probit_energy(p); });
                for (long long s = 0; s < C; ++s) {   // k_probit_fe's per-series sum (its block reduction needs real threads)
                    double f = feg[(size_t)s];
                    for (long long ch = 0; ch < chunks; ++ch) f += fep[(size_t)(ch * C + s)];
                    fes[(size_t)(i - 1) * (size_t)C + (size_t)s] = f;
                }
            }
        }
        if (status) { std::printf("status %d\n", status); continue; }
        for (long long s = 0; s < C; ++s) {
            for (size_t k = 0; k < R; ++k) std::printf("%.17g ", mean[k * (size_t)C + (size_t)s]);
            std::printf("\n");
            for (size_t k = 0; k < R; ++k) std::printf("%.17g ", var[k * (size_t)C + (size_t)s]);
            std::printf("\n");
            for (int i = 0; i < iterations; ++i) std::printf("%.17g ", fes[(size_t)i * (size_t)C + (size_t)s]);
            std::printf("\n");
        }
    }
    // the rest of stdin: triples (m, v, s) -> tilted mean, tilted variance, new site ξ, w, log Φ(m), r(m)
    for (;;) {
        char tok[64];
        if (std::scanf("%63s", tok) != 1) break;
        const double m = std::strtod(tok, nullptr), v = read_double(), s = read_double();
        double mt, vt, nxi, nw;
        probit::tilted_moments(m, v, s, mt, vt);
        probit::site_update(m, v, s, nxi, nw);
        std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", mt, vt, nxi, nw, probit::log_ndtr(m), probit::mills_ratio(m));
    }
    return 0;
}

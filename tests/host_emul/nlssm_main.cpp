// tests/host_emul/nlssm_main.cpp — the nonlinear state-space engine's kernels (csrc/nlssm_kernels.hpp) and the expression interpreter they run
// (csrc/expr.hpp) compiled for the HOST through the stand-in <hip/hip_runtime.h> of this directory and run one "thread" at a time: the same
// __host__ __device__ functions, loops and indexing as on the device, with the launch sequence of nlssm_run_async restated below
// (tests/test_nlssm_host.py compares the output with tests/nlssm_ref.py).  With "expr" as the first token it evaluates a program at points instead,
// as rxhip_expr_eval does.
//
// stdin:  n_cases, then per case   d dy T S method mode unknown per_series iterations a0 b0 sc wm0 wc0 wi | n_code n_consts n_slots | code | consts |
//         Q [d][d] | H [dy][d] | R [dy][dy] | priors | y [T][S][dy] (nan = missing)
//         or   expr | d n_code n_consts n_slots | code | consts | n | x [n][d]
// stdout: per case a line `status <flags> <step> <series>`, then (status 0) mean, cov, shape, rate, fe as one line each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
static inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) { const unsigned long long o = *p; if (v < o) *p = v; return o; }

#define RXHIP_HOST_EMUL 1
#include "nlssm_kernels.hpp"

using namespace rxhip;

template <typename F>
static void launch(unsigned gx, unsigned bx, F&& kernel) {
    gridDim.x = gx; blockDim.x = bx;
    for (unsigned b = 0; b < gx; ++b)
        for (unsigned t = 0; t < bx; ++t) {
            blockIdx.x = b; threadIdx.x = t;
            kernel();
        }
}

static bool next_token(char* tok) { return std::scanf("%63s", tok) == 1; }
static double read_double() {
    char tok[64];
    if (!next_token(tok)) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return std::strtod(tok, nullptr);   // (accepts "nan")
}
static void read_program(expr::Program& pr, int d) {
    std::memset(&pr, 0, sizeof pr);
    pr.d = d;
    pr.n_code = (int)read_double(); pr.n_consts = (int)read_double(); pr.n_slots = (int)read_double();
    if (pr.n_code < 0 || pr.n_code > expr::EXPR_MAX_CODE || pr.n_consts < 0 || pr.n_consts > expr::EXPR_MAX_CONSTS) { std::fprintf(stderr, "program too long\n"); std::exit(2); }
    for (int i = 0; i < 4 * pr.n_code; ++i) pr.code[i] = (int)read_double();
    for (int i = 0; i < pr.n_consts; ++i) pr.consts[i] = read_double();
    char msg[256];
    if (expr::expr_validate(pr, d, msg, sizeof msg)) { std::printf("refused %s\n", msg); std::exit(3); }
}
static void print_line(const std::vector<double>& v) {
    for (double x : v) std::printf("%.17g ", x);
    std::printf("\n");
}
template <int D>
static void eval_points(const expr::Program& pr, const std::vector<double>& x, long long n) {
    std::vector<double> value((size_t)n * D), jac((size_t)n * D * D);
    launch((unsigned)((n + 63) / 64), 64, [&] { k_expr_eval<D>(&pr, x.data(), value.data(), jac.data(), n); });
    print_line(value);
    print_line(jac);
}
template <int D>
static void run_case(NlssmParams& p) {
    const unsigned g = (unsigned)((p.n_series + 63) / 64);
    launch(g, 64, [&] { k_nlssm_forward<D>(p); });
    if (p.smooth) launch(g, 64, [&] { k_nlssm_backward<D>(p); });   // unconditionally, as nlssm_run_async does
}

int main() {
    char tok[64];
    if (!next_token(tok)) return 2;
    if (!std::strcmp(tok, "expr")) {
        const int d = (int)read_double();
        expr::Program pr;
        read_program(pr, d);
        const long long n = (long long)read_double();
        std::vector<double> x((size_t)n * (size_t)d);
        for (double& v : x) v = read_double();
        switch (d) { case 1: eval_points<1>(pr, x, n); break; case 2: eval_points<2>(pr, x, n); break; case 3: eval_points<3>(pr, x, n); break; default: eval_points<4>(pr, x, n); }
        return 0;
    }
    const int n_cases = (int)std::strtod(tok, nullptr);
    for (int cs = 0; cs < n_cases; ++cs) {
        NlssmParams p{};
        const int d = (int)read_double();
        p.dy = (int)read_double(); p.T = (long long)read_double(); p.n_series = (long long)read_double();
        p.method = (int)read_double(); p.smooth = (int)read_double(); p.unknown = (int)read_double(); p.per_series = (int)read_double();
        p.iterations = (int)read_double(); p.a0 = read_double(); p.b0 = read_double();
        p.u.sc = read_double(); p.u.wm0 = read_double(); p.u.wc0 = read_double(); p.u.wi = read_double();
        expr::Program pr;
        read_program(pr, d);
        const size_t T = (size_t)p.T, C = (size_t)p.n_series, dd = (size_t)d * d, npri = p.per_series ? C : 1;
        for (size_t i = 0; i < dd; ++i) p.Q[i] = read_double();
        for (int i = 0; i < p.dy * d; ++i) p.H[i] = read_double();
        for (int i = 0; i < p.dy * p.dy; ++i) p.R[i] = read_double();
        std::vector<double> prior(npri * (d + dd)), y(T * C * (size_t)p.dy), mean(T * C * d), cov(T * C * dd), shape(T * C), rate(T * C),
            rec(T * (size_t)nlssm::n_records(d) * C), fe(C, 0.0);
        for (double& v : prior) v = read_double();
        for (double& v : y) v = read_double();
        int status = 0;
        unsigned long long where = ~0ull;
        p.prog = &pr; p.y = y.data(); p.prior = prior.data(); p.mean = mean.data(); p.cov = cov.data(); p.shape = shape.data(); p.rate = rate.data();
        p.rec = rec.data(); p.fe_series = fe.data(); p.status = &status; p.where = &where;
        switch (d) { case 1: run_case<1>(p); break; case 2: run_case<2>(p); break; case 3: run_case<3>(p); break; default: run_case<4>(p); }
        std::printf("status %d %lld %lld\n", status, status & 64 ? (long long)(where >> 32) : -1, status & 64 ? (long long)(where & 0xffffffffull) : -1);
        if (status) continue;
        print_line(mean); print_line(cov); print_line(shape); print_line(rate); print_line(fe);
    }
    return 0;
}

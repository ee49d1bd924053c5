// expr.hpp — a user's function f : ℝᵈ → ℝᵈ on the device: a straight-line three-address program over numbered value slots, and the one
// interpreter that evaluates it (the delta node of nlssm_kernels.hpp; rxhip_expr_eval evaluates a program on its own).
//
// Program.  An instruction is four int32 (op, dst, a, b):
//     CONST dst ← consts[a]      VAR dst ← x[a]      ADD SUB MUL DIV dst ← slot a ∘ slot b      NEG SQRT EXP LOG SIN COS TANH dst ← op(slot a)
//     OUT   f[dst] ← slot a
// At most EXPR_MAX_CODE instructions, EXPR_MAX_SLOTS live slots and EXPR_MAX_CONSTS constants (expr_validate refuses the rest with a text, and a
// read of a slot that no earlier instruction wrote, and a program whose OUTs do not cover 0 … d−1).  The program is the same for every lane of a
// wavefront: the opcode dispatch is uniform and the program itself is read through scalar loads.
//
// Two modes of the same interpreter over `nc` COMPONENTS per slot:
//   dual   component 0 is the value, components 1 … nc−1 are tangents (forward mode): with the seeds e_k on the inputs the outputs carry
//          f(x) and the columns k of the Jacobian ∂f/∂x;
//   plain  every component is a value of its own (the sigma points of the unscented transform).
// Where the slots live: NOT in a dynamically indexed per-lane array (that is scratch memory on this target) but in LDS, as
// [row][component][lane] doubles, rows = n_slots slots | d outputs | d inputs: a lane touches its own column only, so no barrier is needed and a
// wavefront's accesses are conflict-free.  expr_max_comps gives the components that fit EXPR_LDS_BYTES for a program; a caller with more tangents
// or points than that makes several passes (expr_eval_jacobian below, the delta node of nlssm_kernels.hpp).
//
// Everything here is `__host__ __device__` and self-contained, floating-point contraction off: the host build of tests/host_emul/ runs the same
// functions and gives the same bits wherever the libm calls agree.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#if defined(__clang__)
#define EXPR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EXPR_NO_CONTRACT
#endif
#define EXPR_HD __host__ __device__ __forceinline__

namespace rxhip {
namespace expr {

enum Op : int32_t { OP_CONST = 0, OP_VAR = 1, OP_ADD = 2, OP_SUB = 3, OP_MUL = 4, OP_DIV = 5, OP_NEG = 6, OP_SQRT = 7, OP_EXP = 8, OP_LOG = 9, OP_SIN = 10,
                    OP_COS = 11, OP_TANH = 12, OP_OUT = 13, OP_COUNT = 14 };

constexpr int EXPR_MAX_CODE = 128, EXPR_MAX_SLOTS = 16, EXPR_MAX_CONSTS = 32, EXPR_MAX_D = 4;
constexpr int EXPR_LANES = 64;               // lanes of a workgroup that evaluates programs: one wavefront
constexpr int EXPR_LDS_BYTES = 48 * 1024;    // budget of a workgroup

struct Program {
    int32_t n_code, n_consts, d, n_slots;
    int32_t code[EXPR_MAX_CODE * 4];
    double consts[EXPR_MAX_CONSTS];
};

// rows of a program's LDS block and the components per pass that fit the budget (≥ 4: 24 rows at the caps)
EXPR_HD int rows_of(int n_slots, int d) { return n_slots + 2 * d; }
EXPR_HD int expr_max_comps(int n_slots, int d) { return EXPR_LDS_BYTES / (rows_of(n_slots, d) * EXPR_LANES * (int)sizeof(double)); }

// 0: the program is well formed for dimension d; else a text in msg
inline int expr_validate(const Program& p, int d, char* msg, size_t n) {
    if (d < 1 || d > EXPR_MAX_D) { snprintf(msg, n, "expr: the dimension must be 1 … %d (got %d)", EXPR_MAX_D, d); return 1; }
    if (p.d != d) { snprintf(msg, n, "expr: the program was traced for dimension %d, the model has %d", p.d, d); return 1; }
    if (p.n_code < 1 || p.n_code > EXPR_MAX_CODE) { snprintf(msg, n, "expr: a program has 1 … %d instructions (got %d)", EXPR_MAX_CODE, p.n_code); return 1; }
    if (p.n_slots < 1 || p.n_slots > EXPR_MAX_SLOTS) { snprintf(msg, n, "expr: a program has 1 … %d live slots (got %d)", EXPR_MAX_SLOTS, p.n_slots); return 1; }
    if (p.n_consts < 0 || p.n_consts > EXPR_MAX_CONSTS) { snprintf(msg, n, "expr: a program has at most %d constants (got %d)", EXPR_MAX_CONSTS, p.n_consts); return 1; }
    unsigned written = 0, outs = 0;
    for (int i = 0; i < p.n_code; ++i) {
        const int32_t op = p.code[4 * i], dst = p.code[4 * i + 1], a = p.code[4 * i + 2], b = p.code[4 * i + 3];
        if (op < 0 || op >= OP_COUNT) { snprintf(msg, n, "expr: instruction %d has an unknown opcode %d", i, op); return 1; }
        const bool binary = op >= OP_ADD && op <= OP_DIV, unary = (op >= OP_NEG && op <= OP_TANH) || op == OP_OUT;
        if (op == OP_CONST && (a < 0 || a >= p.n_consts)) { snprintf(msg, n, "expr: instruction %d names constant %d of %d", i, a, p.n_consts); return 1; }
        if (op == OP_VAR && (a < 0 || a >= d)) { snprintf(msg, n, "expr: instruction %d names input %d of %d", i, a, d); return 1; }
        if ((binary || unary) && (a < 0 || a >= p.n_slots || !(written >> a & 1u))) { snprintf(msg, n, "expr: instruction %d reads slot %d before it is written", i, a); return 1; }
        if (binary && (b < 0 || b >= p.n_slots || !(written >> b & 1u))) { snprintf(msg, n, "expr: instruction %d reads slot %d before it is written", i, b); return 1; }
        if (op == OP_OUT) {
            if (dst < 0 || dst >= d) { snprintf(msg, n, "expr: instruction %d writes output %d of %d", i, dst, d); return 1; }
            outs |= 1u << dst;
        } else {
            if (dst < 0 || dst >= p.n_slots) { snprintf(msg, n, "expr: instruction %d writes slot %d of %d", i, dst, p.n_slots); return 1; }
            written |= 1u << dst;
        }
    }
    for (int i = 0; i < d; ++i)
        if (!(outs >> i & 1u)) { snprintf(msg, n, "expr: the program has no OUT for output %d (outputs 0 … %d are needed)", i, d - 1); return 1; }
    for (int i = 0; i < p.n_consts; ++i)
        if (!(p.consts[i] - p.consts[i] == 0.0)) { snprintf(msg, n, "expr: constant %d is not finite", i); return 1; }
    return 0;
}

// tanh through expm1: t = e^{2|x|} − 1, tanh|x| = t/(t + 2) — a few ulp over the whole line, small arguments included (the device library's own
// tanh measured 17 ulp from the correctly rounded value there); 1 from |x| = 22 on (1 − tanh 22 < 2⁻⁶²)
EXPR_HD double tanh_expm1(double x) {
    EXPR_NO_CONTRACT
    const double ax = fabs(x);
    if (!(ax < 22.0)) return x != x ? x : copysign(1.0, x);
    const double t = expm1(2.0 * ax);
    return copysign(t / (t + 2.0), x);
}

// A lane's view of its workgroup's LDS block
struct Slots {
    double* base;   // the block
    int lane, nc, n_slots, d;
    EXPR_HD double& at(int row, int c) const { return base[(row * nc + c) * EXPR_LANES + lane]; }
    EXPR_HD double& in(int i, int c) const { return at(n_slots + d + i, c); }
    EXPR_HD double& out(int i, int c) const { return at(n_slots + i, c); }
};

// the interpreter: inputs are read from the `in` rows, results land in the `out` rows
template <bool DUAL>
EXPR_HD void run(const Program* __restrict__ p, const Slots& s) {
    EXPR_NO_CONTRACT
    const int nc = s.nc, n = p->n_code;
    for (int pc = 0; pc < n; ++pc) {
        const int op = p->code[4 * pc], dst = p->code[4 * pc + 1], a = p->code[4 * pc + 2], b = p->code[4 * pc + 3];
        switch (op) {
            case OP_CONST: {
                const double k = p->consts[a];
                s.at(dst, 0) = k;
                for (int c = 1; c < nc; ++c) s.at(dst, c) = DUAL ? 0.0 : k;
            } break;
            case OP_VAR: for (int c = 0; c < nc; ++c) s.at(dst, c) = s.in(a, c); break;
            case OP_OUT: for (int c = 0; c < nc; ++c) s.out(dst, c) = s.at(a, c); break;
            case OP_ADD: for (int c = 0; c < nc; ++c) s.at(dst, c) = s.at(a, c) + s.at(b, c); break;
            case OP_SUB: for (int c = 0; c < nc; ++c) s.at(dst, c) = s.at(a, c) - s.at(b, c); break;
            case OP_NEG: for (int c = 0; c < nc; ++c) s.at(dst, c) = -s.at(a, c); break;
            case OP_MUL:
                if (DUAL) {
                    const double a0 = s.at(a, 0), b0 = s.at(b, 0);
                    for (int c = 1; c < nc; ++c) { const double ta = s.at(a, c), tb = s.at(b, c); s.at(dst, c) = ta * b0 + a0 * tb; }
                    s.at(dst, 0) = a0 * b0;
                } else
                    for (int c = 0; c < nc; ++c) s.at(dst, c) = s.at(a, c) * s.at(b, c);
                break;
            case OP_DIV:
                if (DUAL) {
                    const double a0 = s.at(a, 0), b0 = s.at(b, 0), v = a0 / b0;
                    for (int c = 1; c < nc; ++c) { const double ta = s.at(a, c), tb = s.at(b, c); s.at(dst, c) = (ta - v * tb) / b0; }
                    s.at(dst, 0) = v;
                } else
                    for (int c = 0; c < nc; ++c) s.at(dst, c) = s.at(a, c) / s.at(b, c);
                break;
            default: {   // the unary functions: value v and derivative dv at the value of the argument
                const int nv = DUAL ? 1 : nc;
                for (int c = 0; c < nv; ++c) {
                    const double a0 = s.at(a, c);
                    double v, dv;
                    switch (op) {
                        case OP_SQRT: v = sqrt(a0); dv = 0.5 / v; break;
                        case OP_EXP: v = exp(a0); dv = v; break;
                        case OP_LOG: v = log(a0); dv = 1.0 / a0; break;
                        case OP_SIN: v = sin(a0); dv = DUAL ? cos(a0) : 0.0; break;
                        case OP_COS: v = cos(a0); dv = DUAL ? -sin(a0) : 0.0; break;
                        default: v = tanh_expm1(a0); dv = 1.0 - v * v; break;
                    }
                    if (DUAL)
                        for (int t = 1; t < nc; ++t) s.at(dst, t) = s.at(a, t) * dv;
                    s.at(dst, c) = v;
                }
            } break;
        }
    }
}

// f(x) and J = ∂f/∂x(x) for a lane, D ≤ 4: the tangents in as many passes as the budget asks for.  x, f: [D]; J: [D][D] row-major (J[i][k] = ∂f_i/∂x_k).
template <int D>
EXPR_HD void eval_jacobian(const Program* __restrict__ p, double* lds, int lane, const double (&x)[D], double (&f)[D], double (&J)[D][D]) {
    const int cap = expr_max_comps(p->n_slots, D);
    const int per = cap - 1 < D ? cap - 1 : D;   // tangents per pass
#pragma unroll
    for (int i = 0; i < D; ++i) {
        f[i] = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) J[i][k] = 0.0;
    }
    for (int k0 = 0; k0 < D; k0 += per) {
        const int nt = D - k0 < per ? D - k0 : per;
        const Slots s{lds, lane, nt + 1, p->n_slots, D};
#pragma unroll
        for (int i = 0; i < D; ++i) {
            s.in(i, 0) = x[i];
            for (int c = 1; c <= nt; ++c) s.in(i, c) = (i == k0 + c - 1) ? 1.0 : 0.0;
        }
        run<true>(p, s);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            f[i] = s.out(i, 0);
#pragma unroll
            for (int k = 0; k < D; ++k)
                if (k >= k0 && k < k0 + nt) J[i][k] = s.out(i, k - k0 + 1);
        }
    }
}

// f at NP points for a lane (plain mode), in passes: X, Y are [NP][D]
template <int D, int NP>
EXPR_HD void eval_points(const Program* __restrict__ p, double* lds, int lane, const double (&X)[NP][D], double (&Y)[NP][D]) {
    const int cap = expr_max_comps(p->n_slots, D);
    const int per = cap < NP ? cap : NP;
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int i = 0; i < D; ++i) Y[q][i] = 0.0;
    for (int p0 = 0; p0 < NP; p0 += per) {
        const int np = NP - p0 < per ? NP - p0 : per;
        const Slots s{lds, lane, np, p->n_slots, D};
#pragma unroll
        for (int q = 0; q < NP; ++q)
            if (q >= p0 && q < p0 + np) {
#pragma unroll
                for (int i = 0; i < D; ++i) s.in(i, q - p0) = X[q][i];
            }
        run<false>(p, s);
#pragma unroll
        for (int q = 0; q < NP; ++q)
            if (q >= p0 && q < p0 + np) {
#pragma unroll
                for (int i = 0; i < D; ++i) Y[q][i] = s.out(i, q - p0);
            }
    }
}

}  // namespace expr
}  // namespace rxhip

#if defined(__HIPCC__) || defined(RXHIP_HOST_EMUL)
namespace rxhip {

#if defined(RXHIP_HOST_EMUL)
static double expr_lds_emul[expr::EXPR_LDS_BYTES / sizeof(double)];   // (the host build runs one "thread" at a time: a lane's column of one block)
#define EXPR_LDS_BLOCK(name) double* name = expr_lds_emul
#else
#define EXPR_LDS_BLOCK(name) extern __shared__ double name[]
#endif

// rxhip_expr_eval: value [n][D] and Jacobian [n][D][D] at n points x [n][D], one lane per point.  The value comes from a plain pass and the
// Jacobian from the dual passes, so both modes of the interpreter are exercised.
template <int D>
__global__ void __launch_bounds__(64) k_expr_eval(const expr::Program* __restrict__ prog, const double* __restrict__ x, double* __restrict__ value,
                                                   double* __restrict__ jac, long long n) {
    EXPR_LDS_BLOCK(lds);
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    double xi[D], f[D], J[D][D], X[1][D], Y[1][D];
#pragma unroll
    for (int k = 0; k < D; ++k) { xi[k] = x[i * D + k]; X[0][k] = xi[k]; }
    expr::eval_jacobian<D>(prog, lds, (int)threadIdx.x, xi, f, J);
    expr::eval_points<D, 1>(prog, lds, (int)threadIdx.x, X, Y);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        value[i * D + k] = Y[0][k];
#pragma unroll
        for (int j = 0; j < D; ++j) jac[(i * D + k) * D + j] = J[k][j];
    }
}

}  // namespace rxhip
#endif

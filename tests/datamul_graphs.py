"""Graphs whose `*` nodes take DATA matrices (include/rxhip.h: "typeof(*) with a constant or a DATA matrix"), each with the switch `x_as_data`, and
`const_twin`: for ONE replica a data-matrix graph is by definition the graph with that replica's matrices as constants — so the references are the ones
the constant-matrix executor is already held to (oracle/tree_oracle.py on the twin, tests/loopy_ref.py for the regression, normal equations in numpy).

Every builder returns (builder, vector data variables, matrix data variables, Gaussian variables to compare); `draw` makes the per-replica values."""
import copy

import numpy as np

from rxhip import _lib
from rxhip.graph import GraphBuilder, linreg_graph


def const_twin(dump, matrices):
    """the dump with the data matrices {variable id: matrix} of one replica rewritten into constants"""
    tw = copy.deepcopy(dump)
    on_a = {int(f["interfaces"][1][1]) for f in tw["factors"] if f["type"] == "*"}
    for v, M in matrices.items():
        var = tw["variables"][int(v)]
        M = np.asarray(M, float)
        assert var["kind"] == "data" and int(v) in on_a and M.size == var["rows"] * var["cols"], v
        var["kind"] = "constant"
        var["value"] = M.ravel().tolist()
    assert not any(var["kind"] == "data" and i in on_a for i, var in enumerate(tw["variables"])), "a data matrix was left without a value"
    return tw


def spd(rng, d, s=1.0):
    M = rng.normal(size=(d, d)) / np.sqrt(d)
    return s * (np.eye(d) + 0.3 * (M @ M.T))


def well_conditioned(rng, r, c, norm=1.0):
    """an r × c map with singular values in [0.4, 1] · norm"""
    A = rng.normal(size=(r, c))
    U, sv, Vt = np.linalg.svd(A, full_matrices=False)
    return (U * (norm * np.clip(sv / sv[0], 0.4, 1.0))) @ Vt


class _B:
    """a builder that makes each matrix a data variable or a constant"""

    def __init__(self, x_as_data):
        self.gb, self.as_data, self.mats, self.ys, self.shapes = GraphBuilder(), x_as_data, [], [], {}

    def matrix(self, M):
        M = np.atleast_2d(np.asarray(M, float))
        if not self.as_data:
            return self.gb.constvar(M if M.shape != (1, 1) else float(M[0, 0]))
        v = self.gb.datavar(M.shape[0], cols=M.shape[1])
        self.mats.append(v)
        return v

    def data(self, d):
        v = self.gb.datavar(d)
        self.ys.append(v)
        return v

    def noise(self, out, mu, V):
        V = np.atleast_2d(V)
        if V.shape[0] > 1:
            self.gb.mvnormal_mean_cov(out, mu, self.gb.constvar(V))
        else:
            self.gb.node(_lib.NODE_NORMAL_MEAN_VARIANCE, out, mu, self.gb.constvar(float(V[0, 0])))

    def prior(self, rng, d):
        x = self.gb.randomvar(d)
        self.noise(x, self.gb.constvar(rng.normal(size=d) if d > 1 else float(rng.normal())), spd(rng, d, 2.0))
        return x


# Every forest below draws its NOMINAL matrices from `seed` (they are what the constant variant bakes in); `draw` perturbs them per replica.

def chain_obs_maps(T, d, dy, seed=0, x_as_data=True):
    """(a) x[t] ~ N(A x[t−1], P), y[t] ~ N(B[t] x[t], Q): the observation maps B[t] (dy × d) as data"""
    rng = np.random.default_rng(seed)
    b = _B(x_as_data)
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    A, P, Q = 0.9 * q, spd(rng, d, 0.2), spd(rng, dy, 0.5)
    nominal, gauss = [], []
    x = b.prior(rng, d)
    for t in range(T):
        if t:
            a = b.gb.randomvar(d)
            b.gb.multiply(a, b.gb.constvar(A), x)
            xn = b.gb.randomvar(d)
            b.noise(xn, a, P)
            gauss.append(a)
            x = xn
        Bt = well_conditioned(rng, dy, d)
        nominal.append(Bt)
        o = b.gb.randomvar(dy)
        b.gb.multiply(o, b.matrix(Bt), x)
        b.noise(b.data(dy), o, Q)
        gauss += [x, o]
    return b.gb, b.ys, b.mats, gauss, nominal


def two_maps(d, du, dw, seed=0, x_as_data=True):
    """(b) w = B (A x) with both matrices data: u = A x is an image of x's marginal, w — the output of an output — the product of its messages"""
    rng = np.random.default_rng(seed)
    b = _B(x_as_data)
    x = b.prior(rng, d)
    A, Bm = well_conditioned(rng, du, d), well_conditioned(rng, dw, du)
    u, w = b.gb.randomvar(du), b.gb.randomvar(dw)
    b.gb.multiply(u, b.matrix(A), x)
    b.gb.multiply(w, b.matrix(Bm), u)
    b.noise(b.data(dw), w, spd(rng, dw, 0.5))
    b.noise(b.data(du), u, spd(rng, du, 0.7))
    return b.gb, b.ys, b.mats, [x, u, w], [A, Bm]


def derived_product(d, du, seed=0, x_as_data=True):
    """(c) y ~ N(x + A u, Q) with A (d × du) and u both data: the clamped value A u is derived on the device (OP_DERIVE_MUL with both operands data)"""
    rng = np.random.default_rng(seed)
    b = _B(x_as_data)
    x = b.prior(rng, d)
    A = well_conditioned(rng, d, du)
    u = b.data(du)
    v, w = b.gb.randomvar(d), b.gb.randomvar(d)
    b.gb.multiply(v, b.matrix(A), u)
    b.gb.node(_lib.NODE_ADD, w, x, v)
    b.noise(b.data(d), w, spd(rng, d, 0.5))
    return b.gb, b.ys, b.mats, [x, w], [A]


def square_and_flat(d, r, seed=0, x_as_data=True):
    """(d) a square data map S x (d × d: the constant twin takes the shortcut log|S V Sᵀ| = log|V| + 2 log|det S|, the data map forms it per replica) next to a non-square one C x (r × d, r < d)"""
    rng = np.random.default_rng(seed)
    b = _B(x_as_data)
    x = b.prior(rng, d)
    S, C = well_conditioned(rng, d, d), well_conditioned(rng, r, d)
    p, q = b.gb.randomvar(d), b.gb.randomvar(r)
    b.gb.multiply(p, b.matrix(S), x)
    b.gb.multiply(q, b.matrix(C), x)
    b.noise(b.data(d), p, spd(rng, d, 0.5))
    b.noise(b.data(r), q, spd(rng, r, 0.8))
    return b.gb, b.ys, b.mats, [x, p, q], [S, C]


def dot_rows(N, d, seed=0, x_as_data=True):
    """(e) y[i] ~ Normal(dot(c[i], x), v): `dot` as `*` with a 1 × d data matrix"""
    rng = np.random.default_rng(seed)
    b = _B(x_as_data)
    x = b.prior(rng, d)
    nominal, gauss = [], [x]
    for _ in range(N):
        c = rng.normal(size=(1, d))
        nominal.append(c)
        t = b.gb.randomvar(1)
        b.gb.multiply(t, b.matrix(c), x)
        b.noise(b.data(1), t, np.array([[0.6]]))
        gauss.append(t)
    return b.gb, b.ys, b.mats, gauss, nominal


def draw(gb, ys, nominal, R, seed, scale=0.05):
    """per replica: the vector data [R][Σ rows] (standard normal) and the matrices, nominal + scale · randn: [R] lists of arrays"""
    rng = np.random.default_rng(seed)
    Y = rng.normal(size=(R, int(sum(gb.rows[v] for v in ys))))
    mats = [[M + scale * rng.normal(size=M.shape) for M in nominal] for _ in range(R)]
    return Y, mats


def rows_of(Y, mats):
    """the host rows of set_data(ys + matrix variables): [R][Σ rows | Σ rows·cols], matrices row-major"""
    return np.concatenate([Y, np.stack([np.concatenate([M.ravel() for M in ms]) for ms in mats])], axis=1)


def data_dict(gb, ys, row):
    out, o = {}, 0
    for v in ys:
        out[v] = np.asarray(row[o:o + gb.rows[v]], float)
        o += gb.rows[v]
    return out


__all__ = ["const_twin", "linreg_graph", "chain_obs_maps", "two_maps", "derived_product", "square_and_flat", "dot_rows", "draw", "rows_of", "data_dict"]

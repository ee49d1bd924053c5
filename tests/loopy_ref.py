"""A numpy restatement of the loopy schedule (include/rxhip.h "Loopy graphs") on the linear regression of tests/loopy_graphs.py, scalar or vector:
in every iteration each reader of a loop message takes the previous iteration's value (the first iteration reads the initialisation), every loop
message is computed again by its ordinary rule, and the marginals read the latest value of every message.  Messages toward b from the maps X[i] are kept
in information form (ξ, Λ), every other one in moment form.  The free energy is the executor's node-local sum on the SAME values the schedule reads:
the prior and observation nodes' average energies minus the entropies of their variables' marginals, −H of each `+` node's joint from its three
inbound (variable → factor) messages, and (degree − 1)·H of the marginals (a: N) — for b that is cancelled by its N `*` nodes, for t[i] = X[i] b the marginal
is the image of b's.  At a fixed point these are the Bethe free energy's terms (the node beliefs agree with the marginals).  Pinned by its converged
means against exact conditioning (exact_linreg)."""
import numpy as np

LOG2PI = np.log(2.0 * np.pi)


def _H(V):
    V = np.atleast_2d(V)
    return 0.5 * (V.shape[0] * (LOG2PI + 1.0) + np.linalg.slogdet(V)[1])


def _U(m, V, m0, V0):
    """average energy of N(v | m0, V0) under N(m, V)"""
    W = np.linalg.inv(V0)
    r = m - m0
    return 0.5 * (len(m) * LOG2PI + np.linalg.slogdet(V0)[1] + np.trace(W @ (V + np.outer(r, r))))


def _excl(xis, Ls, xi0, L0):
    """for every i: the prior (information form) times all messages but i, as moments"""
    out = []
    for i in range(len(xis)):
        keep = [j for j in range(len(xis)) if j != i]
        L = L0 + np.sum(Ls[keep], axis=0)
        xi = xi0 + np.sum(xis[keep], axis=0)
        V = np.linalg.inv(L)
        out.append((V @ xi, V))
    return out


def _info(m, V):
    L = np.linalg.inv(V)
    return L @ m, L


def _moments(xi, L):
    V = np.linalg.inv(L)
    return V @ xi, V


def linreg_loopy(x, y, iterations, cut="b", init=(0.0, 100.0), prior_a=(0.0, 1.0), prior_b=(0.0, 1.0), noise_var=1.0):
    """Posterior of a and b and the free energy after every iteration: list of dict(a=(m, V), b=(m, V), fe=float).  Scalar problems (x [N]) take and
    return scalars; vector ones (x [N][dy][d]) vectors and matrices.  cut: the variable whose inbound messages on the cycles are the loop messages
    ("a": add[i] → a; "b": mul[i] → b)."""
    x = np.asarray(x, float)
    scalar = x.ndim == 1
    X = x.reshape(-1, 1, 1) if scalar else x
    N, dy, d = X.shape
    Y = np.asarray(y, float).reshape(N, dy)
    as_v = lambda v, n: np.asarray(v, float).reshape(n)
    as_m = lambda v, n: np.asarray(v, float).reshape(n, n)
    ma0, Va0 = as_v(prior_a[0], dy), as_m(prior_a[1], dy)
    mb0, Vb0 = as_v(prior_b[0], d), as_m(prior_b[1], d)
    S = as_m(noise_var, dy)
    xa0, La0 = _info(ma0, Va0)
    xb0, Lb0 = _info(mb0, Vb0)
    dn = dy if cut == "a" else d
    li_xi, li_L = _info(as_v(init[0], dn), as_m(init[1], dn))
    loop_xi, loop_L = np.tile(li_xi, (N, 1)), np.tile(li_L, (N, 1, 1))
    out = []
    for _ in range(iterations):
        if cut == "b":
            b2m = _excl(loop_xi, loop_L, xb0, Lb0)                                            # b → mul[i], from the previous iteration's mul[j] → b
            t = [(X[i] @ m, X[i] @ V @ X[i].T) for i, (m, V) in enumerate(b2m)]               # mul[i] → t[i]
            a_in = [_info(Y[i] - t[i][0], S + t[i][1]) for i in range(N)]                     # add[i] → a
            a2add = _excl(np.array([q[0] for q in a_in]), np.array([q[1] for q in a_in]), xa0, La0)   # a → add[i]
            bw = [(Y[i] - a2add[i][0], S + a2add[i][1]) for i in range(N)]                    # add[i] → t[i]
            new = [(X[i].T @ np.linalg.solve(bw[i][1], bw[i][0]), X[i].T @ np.linalg.solve(bw[i][1], X[i])) for i in range(N)]   # mul[i] → b
            loop_xi, loop_L = np.array([q[0] for q in new]), np.array([q[1] for q in new])
            a_msgs, b_msgs = a_in, new
        else:
            a2add = _excl(loop_xi, loop_L, xa0, La0)                                          # a → add[i], from the previous iteration's add[j] → a
            bw = [(Y[i] - a2add[i][0], S + a2add[i][1]) for i in range(N)]                    # add[i] → t[i]
            b_in = [(X[i].T @ np.linalg.solve(bw[i][1], bw[i][0]), X[i].T @ np.linalg.solve(bw[i][1], X[i])) for i in range(N)]   # mul[i] → b
            b2m = _excl(np.array([q[0] for q in b_in]), np.array([q[1] for q in b_in]), xb0, Lb0)   # b → mul[i]
            t = [(X[i] @ m, X[i] @ V @ X[i].T) for i, (m, V) in enumerate(b2m)]               # mul[i] → t[i]
            new = [_info(Y[i] - t[i][0], S + t[i][1]) for i in range(N)]                      # add[i] → a
            loop_xi, loop_L = np.array([q[0] for q in new]), np.array([q[1] for q in new])
            a_msgs, b_msgs = new, b_in
        qa = _moments(xa0 + sum(q[0] for q in a_msgs), La0 + sum(q[1] for q in a_msgs))
        qb = _moments(xb0 + sum(q[0] for q in b_msgs), Lb0 + sum(q[1] for q in b_msgs))
        # the free energy on the values this iteration read and wrote
        Wn = np.linalg.inv(S)
        fe = _U(*qa, ma0, Va0) - _H(qa[1]) + _U(*qb, mb0, Vb0) - _H(qb[1]) + N * _H(qa[1])
        for i in range(N):
            qs = _moments(Wn @ Y[i] + np.linalg.solve(t[i][1] + a2add[i][1], t[i][0] + a2add[i][0]), Wn + np.linalg.inv(t[i][1] + a2add[i][1]))   # y leaf × add → s
            fe += _U(Y[i], qs[1], qs[0], S) - _H(qs[1]) + _H(qs[1])                            # observation node; s: degree 2
            L1, L2 = np.linalg.inv(t[i][1]), np.linalg.inv(a2add[i][1])                       # `+`: t → add, a → add, s → add (the observation's leaf)
            Lj = np.block([[L1 + Wn, Wn], [Wn, L2 + Wn]])
            fe -= 0.5 * (2 * dy * (LOG2PI + 1.0) - np.linalg.slogdet(Lj)[1])
            fe += _H(X[i] @ qb[1] @ X[i].T)                                                   # t[i]: the image of q(b)
        if scalar:
            out.append(dict(a=(float(qa[0][0]), float(qa[1][0, 0])), b=(float(qb[0][0]), float(qb[1][0, 0])), fe=float(fe)))
        else:
            out.append(dict(a=qa, b=qb, fe=float(fe)))
    return out


def exact_linreg(x, y, prior_a=(0.0, 1.0), prior_b=(0.0, 1.0), noise_var=1.0):
    """the exact posterior of (a, b) of the scalar regression: mean [2], covariance [2][2]"""
    x, y = np.asarray(x, float), np.asarray(y, float)
    X = np.stack([np.ones_like(x), x], axis=1)
    J = np.diag([1.0 / prior_a[1], 1.0 / prior_b[1]]) + X.T @ X / noise_var
    h = np.array([prior_a[0] / prior_a[1], prior_b[0] / prior_b[1]]) + X.T @ y / noise_var
    S = np.linalg.inv(J)
    return S @ h, S

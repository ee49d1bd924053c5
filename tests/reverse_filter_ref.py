"""numpy restatement of the reverse-filter schedule of the shared-model LGSSM sweep (lgssm_kernels.hpp
k_smooth_tab_steps / k_smooth_tab_compose / k_backward_sh_rev): the per-step bound, the checkpoint-stride chooser and the
reverse recursion itself.  Time index t is x[t+1] of the model (index 0: the first state, filtered with y[0])."""
import numpy as np

AMP_LIMIT = 1.0e2   # REV_AMP_LIMIT
STRIDES = (32, 16, 8)


def obs_terms(B, Q):
    Qi = np.linalg.inv(Q)
    return B.T @ Qi @ B, B.T @ Qi   # B'Q⁻¹B, B'Q⁻¹


def filter_covariances(A, B, P, Q, V0, T, prior_through_transition=False):
    """V_f(t) and V_p(t) (V_p(0): the prior of the first state)"""
    lobs, _ = obs_terms(B, Q)
    Vp = A @ V0 @ A.T + P if prior_through_transition else V0.copy()
    Vf = np.empty((T,) + A.shape)
    Vps = np.empty_like(Vf)
    for t in range(T):
        if t > 0:
            Vp = A @ Vf[t - 1] @ A.T + P
        Vps[t] = Vp
        Vf[t] = np.linalg.inv(np.linalg.inv(Vp) + lobs)
    return Vf, Vps


def kalman_means(model, y, prior_through_transition=False):
    """filtered means m_f(t) [T][chain][d] of every chain (information-form update, the covariances of filter_covariances)"""
    A, B, P, Q, m0, V0 = (model[k] for k in ("A", "B", "P", "Q", "m0", "V0"))
    T, C, _ = y.shape
    lobs, g = obs_terms(B, Q)
    Vf, Vps = filter_covariances(A, B, P, Q, V0, T, prior_through_transition)
    mp = np.tile(A @ m0 if prior_through_transition else m0, (C, 1))
    mf = np.empty((T, C, A.shape[0]))
    for t in range(T):
        if t > 0:
            mp = mf[t - 1] @ A.T
        mf[t] = mp + (Vf[t] @ (g @ y[t].T - lobs @ mp.T)).T
    return mf, Vf, Vps


def spec_norm_bound(M):
    """the device's upper bound on ‖M‖₂ (lgssm_kernels.hpp spec_norm_bound)"""
    if not np.all(np.isfinite(M)):
        return np.inf
    X = M.T @ M
    s = np.abs(X).sum(axis=1).max()
    if s == 0.0:
        return 0.0
    X = X / s
    for _ in range(4):
        X = X @ X
    return float(np.sqrt(s * np.abs(X).sum(axis=1).max() ** (1.0 / 16.0)))


def step_bounds(model, T, prior_through_transition=False):
    """amp[t], t = 0 … T−2: bound on ‖A⁻¹(I + V_p(t+1) B'Q⁻¹B)‖₂, the growth of the reverse step t+1 → t; inf for a singular A"""
    A, B, P, Q, V0 = (model[k] for k in ("A", "B", "P", "Q", "V0"))
    lobs, _ = obs_terms(B, Q)
    _, Vps = filter_covariances(A, B, P, Q, V0, T, prior_through_transition)
    d = A.shape[0]
    try:
        Ai = np.linalg.inv(A)
    except np.linalg.LinAlgError:
        return np.full(T - 1, np.inf)
    if not np.all(np.isfinite(Ai)):
        return np.full(T - 1, np.inf)
    return np.array([spec_norm_bound(Ai @ (np.eye(d) + Vps[t + 1] @ lobs)) for t in range(T - 1)])


def worst_window_products(amp, T, L):
    """{K: worst product of the per-step bounds over a window of the reverse chain}, windows aligned to every segment start
    s·L; factors below 1 count as 1 (k_smooth_tab_compose)"""
    out = {}
    f = np.where(amp >= 1.0, amp, np.where(amp < 1.0, 1.0, np.inf))
    for K in STRIDES:
        worst = 1.0
        for tb in range(0, T - 1, L):
            te = min(tb + L, T - 1)
            p = 1.0
            for t in range(tb, te):
                if (t - tb) % K == 0:
                    p = 1.0
                else:
                    p *= f[t]
                    worst = max(worst, p) if np.isfinite(p) else np.inf
        out[K] = worst
    return out


def choose_stride(model, T, L, n_chains=64, prior_through_transition=False):
    """the checkpoint stride the engine should pick (0: a filtered-mean record per time index)"""
    d, dy = model["A"].shape[0], model["B"].shape[0]
    if dy > d or n_chains % 64 or T < 2:
        return 0
    wp = worst_window_products(step_bounds(model, T, prior_through_transition), T, L)
    for K in STRIDES:
        if wp[K] <= AMP_LIMIT:
            return K
    return 0


def reverse_means(model, y, mf_checkpoints, K, L, Vps):
    """m_f rebuilt by the reverse filter from the true filtered means at the checkpoints (every K steps of each segment,
    each segment end) and at each segment start — what k_backward_sh_rev computes; `mf_checkpoints`: [T][chain][d]
    (only the checkpoint / segment-start rows are read)"""
    A, B, Q = model["A"], model["B"], model["Q"]
    lobs, g = obs_terms(B, Q)
    Ai = np.linalg.inv(A)
    T = y.shape[0]
    out = np.empty_like(mf_checkpoints)
    for tb in range(0, T - 1, L):
        te = min(tb + L, T - 1)
        out[te] = mf_checkpoints[te]
        out[tb] = mf_checkpoints[tb]
        m = mf_checkpoints[te]
        for t in range(te - 1, tb, -1):
            if (t - tb) % K == 0:
                m = mf_checkpoints[t]
            else:
                mp = m + (Vps[t + 1] @ (lobs @ m.T - g @ y[t + 1].T)).T
                m = mp @ Ai.T
            out[t] = m
    return out

"""Posterior-predictive mean and variance of every entry: the NumPy mirror of Model.predictive_moments
(csrc/kernels_predictive.hpp).  A formula-level mirror -- the same quantities, the same NaN, limit and singular rules,
np.linalg per state instead of the kernel's elimination -- not a bit-level one.  Host only: it never touches the engine.

Per datapoint n, over the states s of K^n (and the permanent all-zero state in front of them) with the weights
q_ns = exp(lpj_ns - max_s lpj_ns) / (sum + tiny) of the statistics pass:

    mean[n, d] = sum_s q_ns m_ns,d
    var[n, d]  = sum_s q_ns ((m_ns,d - mean[n, d])^2 + v_ns,d)   (+ sigma^2 with ``noise``)

EBSC: m_ns = W s, v_ns = 0.  ES3C, with A the active latents of s and o the reliable entries of the datapoint:
Lam = (Psi_AA^-1 + W_oA^T W_oA / sigma2)^-1, kappa = mu_A + Lam W_oA^T (y_o - W_oA mu_A) / sigma2, m_ns = W_A kappa,
v_ns,d = w_dA^T Lam w_dA (``lam`` and ``lam_Wt`` of the reference, sssc.py:289-303).  The variance is formed in two
sweeps (centred), never as sum q m^2 - mean^2.
"""
import numpy as np

from .._lib import EvoAmdError

PRED_MAX_K = 32
F64_TINY = np.finfo(np.float64).tiny


def state_posterior_es3c(W, mus, Psi, sigma2, idx, y, obs=None):
    """(Lam, kappa) of one ES3C state with the active latents ``idx`` (k >= 1 of them) for the datapoint ``y`` whose
    reliable entries are ``obs`` (bool (D,), None: all): the Gaussian posterior N(kappa, Lam) of z_A.
    Lam = (I + Psi_AA G_A / sigma2)^-1 Psi_AA, the form that needs no inverse of Psi_AA.  None for a singular system:
    np.linalg raises LinAlgError (an exactly zero pivot) on Psi_AA or on I + Psi_AA G_A / sigma2, or a non-finite result."""
    WA = W[:, idx]
    Wo = WA if obs is None else WA[obs]
    yo = y if obs is None else y[obs]
    P = Psi[np.ix_(idx, idx)]
    k = len(idx)
    try:
        np.linalg.inv(P)  # the reference's own first step (sssc.py:280): raises for an exactly singular Psi_AA
        G = Wo.T @ Wo
        v = Wo.T @ yo - G @ mus[idx]
        T = np.eye(k) + P @ G / sigma2
        X = np.linalg.solve(T, np.concatenate((P, (P @ v)[:, None]), axis=1))
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(X).all():
        return None
    return X[:, :k], mus[idx] + X[:, k] / sigma2


def state_terms_es3c(W, mus, Psi, sigma2, idx, y, obs=None):
    """(m, v) of one ES3C state (the arguments of state_posterior_es3c): m (D,) = W_A kappa and v (D,) =
    diag(W_A Lam W_A^T), clamped at 0.  None for a singular system."""
    post = state_posterior_es3c(W, mus, Psi, sigma2, idx, y, obs)
    if post is None:
        return None
    Lam, kappa = post
    WA = W[:, idx]
    return WA @ kappa, np.maximum(np.einsum("di,ij,dj->d", WA, Lam, WA), 0.0)


def predictive_moments_host(model, theta, states, lpj, Y, x_infr=None, S_perm=0, background=False, noise=True):
    """(mean, var, info) as Model.predictive_moments returns them.  ``model``: "bsc" or "sssc"; ``theta``: W, sigma (EBSC)
    or W, mus, Psi, sigma2 (ES3C); ``states`` bool (N, S, H) = K^n; ``lpj`` (N, S_perm + S), the permanent all-zero state
    first; ``Y`` (N, D), NaN allowed where ``x_infr`` (bool (N, D), None: complete data) is False; ``background``: the last
    latent is active in every state.  info = {"n_singular", "n_skipped"}: datapoints whose rows are NaN because a k x k
    system of a state with non-zero weight is singular / because they have no reliable entry.  EvoAmdError naming n and k
    for a state with more than PRED_MAX_K active latents."""
    sssc = model not in ("bsc", "BSC", "ebsc")
    W = np.asarray(theta["W"], dtype=np.float64)
    D, H = W.shape
    states = np.asarray(states, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    N, S = states.shape[:2]
    assert states.shape == (N, S, H) and lpj.shape == (N, S_perm + S) and Y.shape == (N, D)
    if background:
        states = states.copy()
        states[:, :, H - 1] = True
    complete = x_infr is None or bool(np.all(x_infr))
    if sssc:
        mus, Psi = np.asarray(theta["mus"], dtype=np.float64), np.asarray(theta["Psi"], dtype=np.float64)
        sigma2 = float(theta["sigma2"])
    else:
        sigma2 = float(theta["sigma"] ** 2)
    ks = states.sum(axis=2)
    if ks.size and ks.max() > PRED_MAX_K:
        n, s = np.argwhere(ks > PRED_MAX_K)[0]
        raise EvoAmdError("predictive_moments: datapoint n = %d holds a state with k = %d active latents, at most %d are "
                          "supported (PRED_MAX_K)" % (n, ks[n, s], PRED_MAX_K))
    mean = np.full((N, D), np.nan)
    var = np.full((N, D), np.nan)
    info = {"n_singular": 0, "n_skipped": 0}
    cache = {}  # complete data: the terms of an active set do not depend on the datapoint but for y
    for n in range(N):
        obs = None if complete else np.asarray(x_infr[n], dtype=bool)
        if obs is not None and not obs.any():
            info["n_skipped"] += 1
            continue
        e = np.exp(lpj[n] - lpj[n].max())
        q = e / (e.sum() + F64_TINY)
        terms = _datapoint_terms(sssc, W, mus if sssc else None, Psi if sssc else None, sigma2, states[n], q == 0.0, Y[n], obs,
                                 S_perm, cache)
        singular = terms is None
        if singular:
            info["n_singular"] += 1
            continue
        m, v = terms
        mu = q @ m
        mean[n] = mu
        var[n] = q @ ((m - mu) ** 2 + v) + (sigma2 if noise else 0.0)
    return mean, var, info


def _datapoint_terms(sssc, W, mus, Psi, sigma2, states_n, skip, y, obs, S_perm, cache):
    """(m, v), each (S_perm + S, D): the per-state terms of one datapoint -- zero rows for the permanent all-zero state,
    for an empty state and for the slots ``skip`` (bool (S_perm + S,)) names -- or None when a state that is not skipped
    has a singular system.  ``obs``: the datapoint's reliable entries, None for complete data, where ``cache`` keeps the
    terms of an active set (they depend on the datapoint through y alone)."""
    S, D = states_n.shape[0], W.shape[0]
    m = np.zeros((S_perm + S, D))
    v = np.zeros((S_perm + S, D))
    for s in range(S):
        if skip[S_perm + s]:
            continue
        idx = np.flatnonzero(states_n[s])
        if idx.size == 0:
            continue
        if not sssc:
            m[S_perm + s] = W[:, idx].sum(axis=1)
            continue
        if obs is None:
            key = idx.tobytes()
            if key not in cache:
                cache[key] = _complete_terms(W, mus, Psi, sigma2, idx)
            terms = cache[key]
            if terms is None:
                return None
            WA, Lam, vdiag = terms
            kappa = mus[idx] + Lam @ (WA.T @ (y - WA @ mus[idx])) / sigma2
            m[S_perm + s], v[S_perm + s] = WA @ kappa, vdiag
        else:
            terms = state_terms_es3c(W, mus, Psi, sigma2, idx, y, obs)
            if terms is None:
                return None
            m[S_perm + s], v[S_perm + s] = terms
    return m, v


def _complete_terms(W, mus, Psi, sigma2, idx):
    """(W_A, Lam, diag(W_A Lam W_A^T)) of an active set on complete data, or None when the system is singular."""
    D = W.shape[0]
    k = len(idx)
    WA = W[:, idx]
    P = Psi[np.ix_(idx, idx)]
    try:
        np.linalg.inv(P)
        Lam = np.linalg.solve(np.eye(k) + P @ (WA.T @ WA) / sigma2, P)
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(Lam).all():
        return None
    assert WA.shape == (D, k)
    return WA, Lam, np.maximum(np.einsum("di,ij,dj->d", WA, Lam, WA), 0.0)

"""Posterior samples -- a state of K^n, ES3C latents and a data row per draw: the NumPy mirror of Model.sample_posterior
(csrc/kernels_posterior_sample.hpp, which states the law).  Host only: it never touches the engine.

With i = first_index + n, x0 = mix64(seed + 0x9e3779b97f4a7c15 (i + 1)) and P = PSAMP_PURPOSE (the stream of
generate_counter under a purpose of its own):

    weights  e_j = codes_exp(lpj_nj - max_j lpj_nj), c_j = c_{j-1} + e_j in slot order, C = c_{L-1};
             a row with a NaN or +inf, or with C = 0, is "bad weights"
    slot_t   u = u01(x0, P, t), target = u C: the first j with c_j > target, else (top end) the last j with e_j > 0
    ES3C     z_A = kappa + L eps, L L^T = (Lam + Lam^T) / 2, eps_j = normal number 32 t + j of purpose P + 1
    y        W z (EBSC: W s) + sigma g, g_d = normal number D t + d of purpose P + 2; fill "missing": the reliable entries
             carry the datapoint's own y

``slot`` and ``s`` are bit-level (codes_exp, sequential additions, searchsorted): the kernel's bit for bit.  ``z`` and ``y``
are formula-level: np.linalg for Lam and kappa as in predictive.py, np.linalg.cholesky for the factor.
"""
import numpy as np

from .._lib import EvoAmdError
from ..codes import codes_exp
from ..variational.utils import _M64
from .generate import _TWO_PI, _first_hash, _u01
from .predictive import PRED_MAX_K, state_posterior_es3c

PSAMP_PURPOSE = 0x5053414D00000000  # "PSAM"
INFO_KEYS = ("n_singular", "n_skipped", "n_not_pd", "n_bad_weights")


def posterior_weights(lpj_row):
    """(e, c, bad) of one lpj row: the weights, their running sums in slot order, and whether the row has no draws."""
    lpj_row = np.asarray(lpj_row, dtype=np.float64)
    if np.isnan(lpj_row).any() or (lpj_row == np.inf).any():
        return None, None, True
    with np.errstate(invalid="ignore"):  # (-inf) - (-inf): codes_exp turns the NaN into weight 0
        e = codes_exp(lpj_row - lpj_row.max())
    c = np.add.accumulate(e)  # c_j = c_{j-1} + e_j, one fp64 addition after the other
    return e, c, not c[-1] > 0.0


def slots_of_targets(e, c, target):
    """The slot of every target: the first j with c_j > target; none (target >= C): the last j with e_j > 0."""
    slot = np.searchsorted(c, target, side="right")
    return np.where(slot < c.size, slot, np.flatnonzero(e > 0.0)[-1]).astype(np.int32)


def _normal_at(x0, purpose, index):
    """The normal numbers ``index`` (uint64 array) of a purpose for ONE datapoint (x0 (1, 1)), shaped like ``index``."""
    index = np.asarray(index, dtype=np.uint64)
    p = (index >> np.uint64(1)).ravel()
    r = np.sqrt(-2.0 * np.log(_u01(x0, purpose, np.uint64(2) * p)[0]))
    t = _TWO_PI * _u01(x0, purpose, np.uint64(2) * p + np.uint64(1))[0]
    odd = (index.ravel() & np.uint64(1)).astype(bool)
    return np.where(odd, r * np.sin(t), r * np.cos(t)).reshape(index.shape)


def sample_posterior_counter(model, theta, states, lpj, Y, x_infr=None, S_perm=0, background=False, n_samples=1, seed=0,
                             first_index=0, fill="missing", noise=True):
    """The dict Model.sample_posterior returns for stream seed ``seed`` (``model.last_sample_seed``): "slot" int32 (N, T),
    "s" bool (N, T, H), ES3C "z" (N, T, H), "y" (N, T, D) and "info".  ``model``: "bsc" or "sssc"; the other arguments are
    those of predictive_moments_host.  EvoAmdError naming n and k for a state with more than PRED_MAX_K active latents."""
    if fill not in ("missing", "all"):
        raise ValueError("fill must be 'missing' or 'all'")
    sssc = model not in ("bsc", "BSC", "ebsc")
    W = np.asarray(theta["W"], dtype=np.float64)
    D, H = W.shape
    states = np.asarray(states, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    N, S = states.shape[:2]
    T = int(n_samples)
    assert states.shape == (N, S, H) and lpj.shape == (N, S_perm + S) and Y.shape == (N, D) and T >= 1
    if background:
        states = states.copy()
        states[:, :, H - 1] = True
    complete = x_infr is None or bool(np.all(x_infr))
    if sssc:
        mus, Psi = np.asarray(theta["mus"], dtype=np.float64), np.asarray(theta["Psi"], dtype=np.float64)
        sigma2 = float(theta["sigma2"])
        sigma = float(np.sqrt(theta["sigma2"]))
    else:
        sigma = float(theta["sigma"])
    has_data = np.ones(N, dtype=bool) if complete else np.asarray(x_infr, dtype=bool).any(axis=1)
    ks = states.sum(axis=2)
    over = (ks > PRED_MAX_K) & has_data[:, None]
    if over.any():
        n, s = np.argwhere(over)[0]
        raise EvoAmdError("sample_posterior: datapoint n = %d holds a state with k = %d active latents, at most %d are "
                          "supported (PRED_MAX_K)" % (n, ks[n, s], PRED_MAX_K))
    out = {"slot": np.full((N, T), -1, dtype=np.int32), "s": np.zeros((N, T, H), dtype=bool),
           "y": np.full((N, T, D), np.nan)}
    if sssc:
        out["z"] = np.full((N, T, H), np.nan)
    info = dict.fromkeys(INFO_KEYS, 0)
    seed, first_index = int(seed) & _M64, int(first_index) & _M64
    ts = np.arange(T, dtype=np.uint64)
    with np.errstate(over="ignore"):  # the hashes wrap mod 2^64
        for n in range(N):
            if not has_data[n]:
                info["n_skipped"] += 1
                continue
            e, c, bad = posterior_weights(lpj[n])
            if bad:
                info["n_bad_weights"] += 1
                continue
            x0 = _first_hash(seed, np.array([(first_index + n) & _M64], dtype=np.uint64))
            slot = slots_of_targets(e, c, _u01(x0, PSAMP_PURPOSE, ts)[0] * c[-1])
            obs = None if complete else np.asarray(x_infr[n], dtype=bool)
            s_n = np.zeros((T, H), dtype=bool)
            z_n = np.zeros((T, H))
            yhat = np.zeros((T, D))
            singular = not_pd = False
            for sl in np.unique(slot):
                rows = np.flatnonzero(slot == sl)
                idx = np.flatnonzero(states[n, sl - S_perm]) if sl >= S_perm else np.zeros(0, dtype=np.int64)
                s_n[np.ix_(rows, idx)] = True
                if idx.size == 0:
                    continue
                if not sssc:
                    yhat[rows] = W[:, idx].sum(axis=1)
                    continue
                post = state_posterior_es3c(W, mus, Psi, sigma2, idx, Y[n], obs)
                if post is None:
                    singular = True
                    continue
                Lam, kappa = post
                try:
                    Lc = np.linalg.cholesky(0.5 * (Lam + Lam.T))
                except np.linalg.LinAlgError:
                    not_pd = True
                    continue
                if not np.isfinite(Lc).all():
                    not_pd = True
                    continue
                eps = _normal_at(x0, PSAMP_PURPOSE + 1, np.uint64(32) * ts[rows, None] + np.arange(idx.size, dtype=np.uint64))
                # (einsum's own loops, not BLAS: a row's bits do not depend on how many rows there are)
                zA = kappa + np.einsum("tj,ij->ti", eps, Lc)
                z_n[np.ix_(rows, idx)] = zA
                yhat[rows] = np.einsum("ti,di->td", zA, W[:, idx])
            if singular or not_pd:  # any drawn state: the whole datapoint has no draws; singular wins
                info["n_singular" if singular else "n_not_pd"] += 1
                continue
            if noise:
                yhat = yhat + sigma * _normal_at(x0, PSAMP_PURPOSE + 2, np.arange(T * D, dtype=np.uint64).reshape(T, D))
            if fill == "missing":
                keep = np.ones(D, dtype=bool) if obs is None else obs
                yhat[:, keep] = Y[n, keep]
            out["slot"][n], out["s"][n], out["y"][n] = slot, s_n, yhat
            if sssc:
                out["z"][n] = z_n
    out["info"] = info
    return out

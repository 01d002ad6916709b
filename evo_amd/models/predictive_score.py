"""Log predictive density and PIT of single entries under the mixture over K^n: the NumPy mirror of
Model.predictive_log_score (csrc/kernels_predictive_score.hpp has the law this file is written from), and pit_summary, which
reads a PIT array.  A formula-level mirror built on the per-state m and v of predictive_moments_host (np.linalg per state,
scipy-free: math.erfc), not a bit-level one.  Host only: it never touches the engine.

Per datapoint n, with e_s = exp(lpj_ns - max_s lpj_ns) over the permanent all-zero state and the states of K^n in slot
order (a state of weight exactly 0 is skipped) and Wsum = sum_s e_s, for every scored entry d (query set, y_true finite):

    tau = v_sd + (noise ? sigma^2 : 0),  u = y_true - m_sd,  ld = -(log(2 pi tau) + u^2 / tau) / 2,  Phi = erfc(-u / sqrt(2 tau)) / 2
    (tau = 0, a point mass: ld = -inf, Phi = [u >= 0])
    logp[n, d] = logsumexp_s((lpj_ns - max) + ld_s) - log Wsum          pit[n, d] = (sum_s e_s Phi_s) / Wsum
"""
import math

import numpy as np

from .._lib import EvoAmdError
from .predictive import PRED_MAX_K, _datapoint_terms

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def predictive_log_score_host(model, theta, states, lpj, Y, y_true, query, x_infr=None, S_perm=0, background=False, noise=True):
    """(score, info) as Model.predictive_log_score returns them with per_entry=True, for one rank.  ``model``, ``theta``,
    ``states``, ``lpj``, ``Y``, ``x_infr``, ``S_perm`` and ``background`` as for predictive_moments_host; ``y_true`` (N, D)
    is read where ``query`` (bool (N, D)) is set.  info: "logp", "pit" (N, D; NaN outside the scored entries), "logp_n"
    (N,), "count" (N,) int32, "n_singular", "n_skipped", "n_not_queried", "n_bad_values".  A datapoint without a scored
    entry is not visited (its states are not looked at); EvoAmdError naming n and k for a state with more than PRED_MAX_K
    active latents in a visited datapoint; ValueError for EBSC without noise."""
    sssc = model not in ("bsc", "BSC", "ebsc")
    if not sssc and not noise:
        raise ValueError("predictive_log_score: EBSC without noise has variance 0 at every entry: nothing to score")
    W = np.asarray(theta["W"], dtype=np.float64)
    D, H = W.shape
    states = np.asarray(states, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    y_true = np.asarray(y_true, dtype=np.float64)
    query = np.asarray(query)
    N, S = states.shape[:2]
    assert states.shape == (N, S, H) and lpj.shape == (N, S_perm + S) and Y.shape == (N, D)
    if y_true.shape != (N, D) or query.shape != (N, D) or query.dtype != np.bool_:
        raise ValueError("predictive_log_score: y_true and query (bool) must be (N, D) = (%d, %d)" % (N, D))
    if background:
        states = states.copy()
        states[:, :, H - 1] = True
    complete = x_infr is None or bool(np.all(x_infr))
    mus = Psi = None
    if sssc:
        mus, Psi = np.asarray(theta["mus"], dtype=np.float64), np.asarray(theta["Psi"], dtype=np.float64)
        sigma2 = float(theta["sigma2"])
    else:
        sigma2 = float(theta["sigma"] ** 2)
    add = sigma2 if noise else 0.0
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(np.where(query, y_true, 0.0))
    scored = query & finite
    logp = np.full((N, D), np.nan)
    pit = np.full((N, D), np.nan)
    logp_n = np.zeros(N)
    count = np.zeros(N, dtype=np.int32)
    info = {"n_singular": 0, "n_skipped": 0, "n_not_queried": 0, "n_bad_values": int((query & ~finite).sum())}
    cache = {}
    for n in range(N):
        dd = np.flatnonzero(scored[n])
        if dd.size == 0:
            info["n_not_queried"] += 1
            continue
        obs = None if complete else np.asarray(x_infr[n], dtype=bool)
        if obs is not None and not obs.any():
            info["n_skipped"] += 1
            continue
        ks = states[n].sum(axis=1)
        if ks.size and ks.max() > PRED_MAX_K:  # (the kernel meets the first such slot)
            s = int(np.flatnonzero(ks > PRED_MAX_K)[0])
            raise EvoAmdError("predictive_score: datapoint n = %d holds a state with k = %d active latents, at most %d are "
                              "supported (PRED_MAX_K)" % (n, ks[s], PRED_MAX_K))
        la = lpj[n] - lpj[n].max()
        e = np.exp(la)
        terms = _datapoint_terms(sssc, W, mus, Psi, sigma2, states[n], e == 0.0, Y[n], obs, S_perm, cache)
        if terms is None:
            info["n_singular"] += 1
            continue
        m, v = terms
        use = np.flatnonzero(e != 0.0)  # slot order
        Wsum = 0.0
        for s in use:
            Wsum += e[s]
        tau = v[np.ix_(use, dd)] + add
        u = y_true[n, dd][None, :] - m[np.ix_(use, dd)]
        point = tau == 0.0
        ts = np.where(point, 1.0, tau)
        ld = np.where(point, -np.inf, -0.5 * (np.log(2.0 * np.pi * ts) + u * u / ts))
        phi = np.where(point, (u >= 0.0).astype(np.float64), 0.5 * _erfc(-u / np.sqrt(2.0 * ts)))
        a = la[use][:, None] + ld
        M = a.max(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            lse = np.where(np.isneginf(M), -np.inf, M + np.log(np.exp(a - np.where(np.isneginf(M), 0.0, M)).sum(axis=0)))
        logp[n, dd] = lse - math.log(Wsum)
        pit[n, dd] = (e[use][:, None] * phi).sum(axis=0) / Wsum
        for d in dd:  # ascending d
            logp_n[n] += logp[n, d]
        count[n] = dd.size
    total = int(count.sum())
    info.update(logp=logp, pit=pit, logp_n=logp_n, count=count)
    return (float(logp_n.sum()) / total if total else float("nan")), info


def pit_summary(pit, levels=(0.5, 0.9)):
    """What a PIT array says about calibration, over its finite values: {"n": their number, "coverage": {level: the share
    inside the central interval [(1 - level) / 2, (1 + level) / 2]} -- a calibrated model gives ``level`` --, "ks": the
    Kolmogorov-Smirnov distance sup_t |F_n(t) - t| of their empirical distribution to the uniform one}.  An under-dispersed
    predictive distribution (a truncated K^n that holds too few states) piles the PIT near 0 and 1: coverage below the
    levels; an over-dispersed one piles it near 1/2.  n = 0: NaN everywhere."""
    p = np.asarray(pit, dtype=np.float64).ravel()
    p = np.sort(p[np.isfinite(p)])
    k = p.size
    if k == 0:
        return {"n": 0, "coverage": {float(l): float("nan") for l in levels}, "ks": float("nan")}
    cov = {float(l): float(np.mean((p >= (1.0 - l) / 2.0) & (p <= (1.0 + l) / 2.0))) for l in levels}
    i = np.arange(1, k + 1)
    ks = float(max(np.max(i / k - p), np.max(p - (i - 1) / k)))
    return {"n": int(k), "coverage": cov, "ks": ks}

"""The log-likelihood beyond K^n by importance draws: the NumPy mirror of Model.estimate_log_likelihood
(csrc/kernels_loglik_estimate.hpp, which states the law).  Host only: it never touches the engine.

For datapoint n, T states s_1 .. s_T are drawn from a product of Bernoullis r_n; a draw that K^n holds counts as zero:

    Z^_n = sum_{s in K^n} e^{lpj_ns} + (1 / T) sum_t 1[s_t not in K^n] e^{lpj(s_t)} / r_n(s_t),    ll^_n = log Z^_n.

r_n > 0 on every state, so E[Z^_n] is the sum over ALL states: unbiased in the likelihood, ll^_n >= F_n always, and
E[ll^_n] <= log p(y_n) - ljc by Jensen.  With i = first_index + n, x0 = the first hash of generate / sample_posterior,
P = LLE_PURPOSE, Hv = H - background, L = S_perm + S and lambda = prior_mix:

    weights    e_j = codes_exp(lpj_nj - max_j lpj_nj), C = e_0 + e_1 + ... in slot order (posterior_weights and its
               "bad weights" rule)
    marginals  p_h = (sum_j e_j [s_jh]) / C for h < Hv, j ascending over the states of K^n
    proposal   rho_h = fl(fl((1 - lambda) p_h) + fl(lambda pi_h)), pi_h = pies[h] (ES3C) or pi (EBSC); never an FMA
    draw       s_th = u01(x0, P, t Hv + h) < rho_h; the background latent is on in every draw, without a factor in r
    density    log r_t = sum_{h < Hv} (s_th ? log rho_h : log1p(-rho_h))
    inside     s_t equals a state of K^n in every latent, or is the all-zero state with S_perm >= 1; an outside all-zero
               draw takes the all-zero lpj; draws are not de-duplicated among themselves
    terms      a_t = lpj(s_t) - log r_t for the outside draws (lpj clamped as by lpj_reset_check),
               lR = logsumexp_{t outside} a_t - log T, -inf when no draw is outside
    result     ll^ = logsumexp(F, lR), gap = ll^ - F, mass_outside = exp(lR - ll^), ess = (sum w)^2 / sum w^2 with
               w_t = exp(a_t - max a)

``s``, ``inside`` and ``n_outside`` are bit-level (codes_exp, sequential sums, the stream of generate.py): the kernel's
bit for bit.  The real-valued outputs are formula-level.
"""
import numpy as np

from ..variational.utils import _M64
from .generate import _first_hash, _u01
from .posterior_sample import posterior_weights

LLE_PURPOSE = 0x4C4C450000000000  # "LLE"
F64_MIN = np.finfo(np.float64).min


def _prior_of(theta, Hv):
    if "pies" in theta:
        return np.asarray(theta["pies"], dtype=np.float64)[:Hv]
    return np.full(Hv, float(theta["pi"]))


def proposal_of(theta, states_n, lpj_n, S_perm=0, background=False, prior_mix=0.25):
    """rho (Hv,) of one datapoint: the Bernoulli means of its proposal, from its states of K^n (bool (S, H)) and its lpj
    row (S_perm + S,).  None for a row with "bad weights"."""
    states_n = np.asarray(states_n, dtype=bool)
    S, H = states_n.shape
    Hv = H - (1 if background else 0)
    e, c, bad = posterior_weights(lpj_n)
    if bad:
        return None
    acc = np.zeros(Hv)
    for j in range(S):  # p_h: one fp64 addition per state, j ascending
        if e[S_perm + j] != 0.0:
            acc = acc + np.where(states_n[j, :Hv], e[S_perm + j], 0.0)
    p = acc / c[-1]
    lam = float(prior_mix)
    a = (1.0 - lam) * p      # (separate NumPy operations: each rounds once)
    b = lam * _prior_of(theta, Hv)
    return a + b


def _clamp(v):
    """lpj_reset_check: NaN -> finfo.min, +-inf -> 0."""
    v = np.array(v, dtype=np.float64)
    v[np.isnan(v)] = F64_MIN
    v[np.isinf(v)] = 0.0
    return v


def estimate_log_likelihood_counter(model, theta, states, lpj, lpj_fn, S_perm=0, background=False, n_samples=256, seed=0,
                                    first_index=0, prior_mix=0.25, x_infr=None):
    """The ``info`` dict Model.estimate_log_likelihood returns with per_datapoint=True and keep_draws=True, for stream
    seed ``seed`` (``model.last_estimate_seed``), plus "sum" = the sum of ll over the datapoints that have an estimate
    (L^ = ljc + allreduce(sum) / their count).  ``model``: "bsc" or "sssc" (names the prior: theta["pi"] / theta["pies"]);
    ``states`` bool (N, S, H), ``lpj`` (N, S_perm + S).  ``lpj_fn(n, states_bool) -> (C,)`` supplies the lpj of drawn states
    of datapoint n (bool (C, H), the background latent on); for an all-zero row it must return the all-zero lpj.
    ``x_infr``: a datapoint without a reliable entry is skipped."""
    if int(n_samples) < 1:
        raise ValueError("n_samples must be positive")
    if not 0.0 < float(prior_mix) <= 1.0:
        raise ValueError("prior_mix must be in (0, 1]")
    states = np.asarray(states, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    N, S, H = states.shape
    T = int(n_samples)
    Hv = H - (1 if background else 0)
    assert lpj.shape == (N, S_perm + S) and Hv >= 1
    sssc = model not in ("bsc", "BSC", "ebsc")
    assert sssc == ("pies" in theta), "theta does not belong to the model named"
    if background:
        states = states.copy()
        states[:, :, H - 1] = True
    has_data = np.ones(N, dtype=bool) if x_infr is None else np.asarray(x_infr, dtype=bool).any(axis=1)
    nan = np.full(N, np.nan)
    out = {"ll": nan.copy(), "F": nan.copy(), "gap": nan.copy(), "mass_outside": nan.copy(), "ess": nan.copy(),
           "n_outside": np.zeros(N, dtype=np.int32), "n_bad_weights": 0, "n_skipped": 0,
           "s": np.zeros((N, T, H), dtype=bool), "inside": np.zeros((N, T), dtype=bool),
           "log_r": np.full((N, T), np.nan), "lpj": np.full((N, T), np.nan)}
    seed, first_index = int(seed) & _M64, int(first_index) & _M64
    index = np.arange(T * Hv, dtype=np.uint64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):  # the hashes wrap mod 2^64; log 0 = -inf
        for n in range(N):
            m = lpj[n].max()
            out["F"][n] = m + np.log(np.exp(lpj[n] - m).sum())
            if not has_data[n]:
                out["n_skipped"] += 1
                out["F"][n] = np.nan
                continue
            rho = proposal_of(theta, states[n], lpj[n], S_perm, background, prior_mix)
            if rho is None:
                out["n_bad_weights"] += 1
                out["F"][n] = np.nan
                continue
            x0 = _first_hash(seed, np.array([(first_index + n) & _M64], dtype=np.uint64))
            s = np.zeros((T, H), dtype=bool)
            s[:, :Hv] = _u01(x0, LLE_PURPOSE, index)[0].reshape(T, Hv) < rho
            log_r = np.where(s[:, :Hv], np.log(rho), np.log1p(-rho)).sum(axis=1)
            if background:
                s[:, H - 1] = True
            inside = (s[:, None, :] == states[n][None, :, :]).all(axis=2).any(axis=1)
            if S_perm >= 1:
                inside |= ~s.any(axis=1)
            outside = np.flatnonzero(~inside)
            out["s"][n], out["inside"][n], out["log_r"][n] = s, inside, log_r
            out["n_outside"][n] = outside.size
            F = out["F"][n]
            lR = -np.inf
            ess = 0.0
            if outside.size:
                v = _clamp(lpj_fn(n, s[outside]))
                out["lpj"][n, outside] = v
                a = v - log_r[outside]
                am = a.max()
                w = np.exp(a - am)
                lR = am + np.log(w.sum()) - np.log(T)
                ess = w.sum() ** 2 / (w * w).sum()
            ll = np.logaddexp(F, lR) if lR != -np.inf else F
            out["ll"][n], out["gap"][n], out["ess"][n] = ll, ll - F, ess
            out["mass_outside"][n] = np.exp(lR - ll)
    out["sum"] = float(np.nansum(out["ll"]))
    return out

"""Problems shared by tests/test_predictive_score_host.py and tests/test_gpu_predictive_score.py: the shapes, states, masks
and lpj rows of tests/_predictive_problems.problem with values to score, a query and the NumPy mirror's result (computed
once per problem: lru_cache; do not modify), and an independent brute-force evaluation of the formulas on dense arrays."""
import math
from functools import lru_cache

import numpy as np

from _predictive_problems import Problem, algo_name, problem
from evo_amd.models import predictive_log_score_host

N_NOT_QUERIED = 7   # the datapoint without a scored entry
N_ALL_SCORED = 3    # complete data: every entry of this datapoint is queried (incomplete data: datapoint 5, all D queried,
                    # has no reliable entry and is skipped)
BAD_VALUES = ((2, np.nan), (4, np.inf), (6, -np.inf), (8, np.nan))  # (datapoint, value) at its first queried entry


@lru_cache(maxsize=None)
def score_problem(algo, N, D, H, incomplete=False, S_perm=0, background=False, noise=True):
    """q.p = the moments problem; q.y_true = mean + c sd per entry with the mirror's mean and standard deviation (with or
    without the noise term, as ``noise``) and c uniform in [-8, 8] -- the tails, but not where erfc underflows --, standard
    normal values where the mirror's mean is NaN (datapoint 5 of the incomplete problems), a handful of NaN and +-inf at
    queried entries (BAD_VALUES) and NaN at every entry outside the query; q.query = ~x_infr (incomplete; q.query_arg is
    None there, the default of the call) or a random 30 % (complete), with datapoint N_NOT_QUERIED left without a scored
    entry (complete: no queried entry; incomplete: every queried value NaN) and, complete data, datapoint N_ALL_SCORED
    queried at all D entries; q.score / q.info = the mirror's result with per-entry arrays."""
    p = problem(algo, N, D, H, incomplete, S_perm, background)
    rng = np.random.RandomState(77 + 1000 * H + 10 * D + N + 5 * incomplete + 3 * S_perm + 2 * background + (not noise))
    q = Problem()
    q.p, q.noise = p, noise
    var = p.var if noise else p.var0
    c = rng.uniform(-8.0, 8.0, size=(N, D))
    with np.errstate(invalid="ignore"):
        y = p.mean + c * np.sqrt(var)
    y = np.where(np.isnan(p.mean), rng.normal(size=(N, D)), y)
    if incomplete:
        query = ~np.array(p.x_infr)
        y[N_NOT_QUERIED, query[N_NOT_QUERIED]] = np.nan
        q.query_arg = None
    else:
        query = rng.random_sample((N, D)) < 0.3
        query[:, 1] |= ~query.any(axis=1)
        query[N_NOT_QUERIED] = False
        query[N_ALL_SCORED] = True
        q.query_arg = query
    for n, val in BAD_VALUES:
        y[n, np.flatnonzero(query[n])[0]] = val
    y[~query] = np.nan
    q.y_true, q.query = y, query
    q.n_bad = int((query & ~np.isfinite(np.where(query, y, 0.0))).sum())
    q.score, q.info = predictive_log_score_host(algo_name(algo), p.theta, p.ss, p.lpj, p.Y, y, query,
                                                p.x_infr if incomplete else None, S_perm, background, noise)
    for a in (q.y_true, q.query, q.info["logp"], q.info["pit"], q.info["logp_n"], q.info["count"]):
        a.setflags(write=False)
    return q


def brute_terms(p, n, noise=True):
    """(q, m, tau) of datapoint n of the moments problem ``p``, written from the model alone: the normalised weights
    q (L,), the per-state means m (L, D) and variances tau (L, D) of the predictive Gaussians.  ES3C: the posterior of z_A
    given the reliable entries by explicit inverses, Lam = inv(inv(Psi_AA) + W_oA^T W_oA / sigma2)."""
    th = p.theta
    W = np.asarray(th["W"])
    D, H = W.shape
    L = p.S_perm + p.S
    w = np.exp(p.lpj[n] - p.lpj[n].max())
    w = w / w.sum()
    m, tau = np.zeros((L, D)), np.zeros((L, D))
    obs = np.asarray(p.x_infr[n], dtype=bool)
    for s in range(p.S):
        st = np.array(p.ss[n, s])
        if p.background:
            st[H - 1] = True
        A = np.flatnonzero(st)
        if A.size == 0:
            continue
        if p.algo == "ebsc":
            m[p.S_perm + s] = W[:, A].sum(axis=1)
            continue
        Wo = W[obs][:, A]
        prec = np.linalg.inv(th["Psi"][np.ix_(A, A)]) + Wo.T @ Wo / th["sigma2"]
        Lam = np.linalg.inv(prec)
        kappa = Lam @ (np.linalg.inv(th["Psi"][np.ix_(A, A)]) @ th["mus"][A] + Wo.T @ p.Y[n, obs] / th["sigma2"])
        m[p.S_perm + s] = W[:, A] @ kappa
        tau[p.S_perm + s] = np.einsum("di,ij,dj->d", W[:, A], Lam, W[:, A])
    s2 = float(th["sigma"] ** 2) if p.algo == "ebsc" else float(th["sigma2"])
    return w, m, tau + (s2 if noise else 0.0)


def brute_entry(w, m, tau, y):
    """(density, cdf) at the value y of the mixture sum_s w_s N(m_s, tau_s) of one entry, summed in the linear domain with
    math.erf (tau_s = 0: a point mass, no density)."""
    dens = cdf = 0.0
    for ws, ms, ts in zip(w, m, tau):
        if ts == 0.0:
            cdf += ws * (1.0 if y >= ms else 0.0)
            continue
        z = (y - ms) / math.sqrt(ts)
        dens += ws * math.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi * ts)
        cdf += ws * 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))
    return dens, cdf

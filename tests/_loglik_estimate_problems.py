"""Problems shared by tests/test_loglik_estimate_host.py and tests/test_gpu_loglik_estimate.py: Theta and data as in
tests/_exact_problems.py, a K^n with its oracle lpj rows, and ``lpj_fn`` callables backed by the oracle for the NumPy
mirror.  References are computed once per case (lru_cache) and must not be modified."""
from functools import lru_cache

import numpy as np

from _exact_problems import Problem, make_data, make_theta, oracle_theta, oracle_zero, problem
from evo_amd.models import estimate_log_likelihood_counter
from oracle import evo_oracle as orc


def oracle_lpj_fn(algo, theta, Y, x_infr=None):
    """lpj_fn(n, states bool (C, H)) -> (C,) from the oracle; an all-zero row takes the oracle's all-zero lpj."""
    N, D = Y.shape
    th, counters = oracle_theta(algo, theta, D, theta["W"].shape[1], x_infr)
    zero = oracle_zero(algo, theta, Y, x_infr)

    def fn(n, states):
        states = np.asarray(states, dtype=bool)
        out = np.empty(states.shape[0])
        nz = states.any(axis=1)
        out[~nz] = zero[n]
        if nz.any():
            row = None if x_infr is None else x_infr[n]
            if algo == "ebsc":
                out[nz] = orc.bsc_lpj(th, states[nz], Y[n], counters, x_infr=row)
            else:
                out[nz] = orc.sssc_lpj(th, states[nz], Y[n], counters, {}, obs=row)
        return out

    return fn


def table_lpj_fn(p):
    """lpj_fn over the enumerated oracle lpj of a problem of _exact_problems (no background): a lookup by state index."""
    assert not p.background
    weights = np.int64(1) << np.arange(p.H, dtype=np.int64)

    def fn(n, states):
        g = np.asarray(states, dtype=np.int64) @ weights
        return np.where(g == 0, p.zero[n], p.lpj[n, np.maximum(g, 1) - 1])

    return fn


@lru_cache(maxsize=None)
def exact_case(algo, nan_frac=0.0):
    """(p, states, lpj) of the comparison against the exact answer: problem(algo, 10, 12, 40[, nan_frac]); K^n = the
    permanent all-zero state plus every second state by descending exact lpj (ranks 2, 4, .. 10: the best state of
    every datapoint is NOT in K^n, which is what makes the bound loose by nats), S = 5."""
    p = problem(algo, 10, 12, 40, False, nan_frac)
    order = np.argsort(-p.lpj, axis=1, kind="stable")[:, 1:10:2]
    states = p.states[order]
    lpj = np.concatenate((p.zero[:, None], np.take_along_axis(p.lpj, order, axis=1)), axis=1)
    states.setflags(write=False)
    lpj.setflags(write=False)
    return p, states, lpj


def exact_conditions(p, res, what):
    """The two conditions of the comparison against the exact answer; prints the figures first."""
    ll, F = res["ll"], res["F"]
    gap_bound, gap_est = (p.ll - F).mean(), (p.ll - ll).mean()
    ratio = np.exp(ll - p.ll)  # Z^_n / Z_n
    z = (ratio.mean() - 1.0) / (ratio.std(ddof=1) / np.sqrt(ratio.size))
    print("%s: gap of the bound %.4f, of the estimate %.4f, z %.2f, min(ll - F) %.3g"
          % (what, gap_bound, gap_est, z, (ll - F).min()))
    assert abs(gap_est) <= 0.1 * gap_bound, (what, gap_est, gap_bound)
    assert abs(z) <= 4.0, (what, z)
    assert (ll >= F).all(), what


@lru_cache(maxsize=None)
def kn_case(algo, H, S_perm=1, background=False, nan_frac=0.0, N=37, D=12, S=9, pi=None, seed=0, zero_rows=False):
    """A Theta, data and a K^n around the generating states: c.theta, c.Y, c.x_infr (or None), c.states bool (N, S, H)
    (unique, non-zero: the generating state first, then states one or two flips away), c.lpj (N, S_perm + S) from the
    oracle, c.lpj_fn.  ``pi``: the prior of every latent instead of make_theta's.  ``zero_rows`` (S_perm = 0, no background):
    every second datapoint holds the all-zero state as the LAST ordinary row of its K^n (what init_states with a small
    p_init_Kn lays out): an all-zero draw is inside K^n for those datapoints and outside for the others."""
    rng = np.random.RandomState(7000 + 100 * H + 10 * S_perm + seed + (3 if background else 0) + (5 if nan_frac else 0))
    c = Problem()
    c.algo, c.H, c.D, c.N, c.S, c.S_perm, c.background = algo, H, D, N, S, S_perm, background
    theta = make_theta(rng, algo, D, H)
    if pi is not None:
        if algo == "ebsc":
            theta["pi"] = np.float64(pi)
        else:
            theta["pies"] = np.full(H, float(pi))
    c.theta = theta
    Hv = H - (1 if background else 0)
    s = np.zeros((N, H), dtype=bool)
    for n in range(N):
        s[n, rng.choice(Hv, size=rng.randint(1, 3), replace=False)] = True
    if background:
        s[:, -1] = True
    c.s = s
    c.Y = make_data(rng, algo, theta, s)
    c.x_infr = None
    if nan_frac:
        c.x_infr = rng.random_sample((N, D)) >= nan_frac
        c.x_infr[np.arange(N), rng.randint(D, size=N)] = True
        c.Y = np.where(c.x_infr, c.Y, np.nan)
    states = np.zeros((N, S, H), dtype=bool)
    for n in range(N):
        have = [s[n].copy()]
        while len(have) < S:
            t = s[n].copy()
            t[rng.choice(Hv, size=rng.randint(1, 3), replace=False)] ^= True
            if t[:Hv].any() and not any((t == u).all() for u in have):
                have.append(t)
        states[n] = have
    if zero_rows:
        assert S_perm == 0 and not background
        states[0::2, S - 1, :] = False
    c.states = states
    c.lpj_fn = oracle_lpj_fn(algo, theta, c.Y, c.x_infr)
    body = np.stack([c.lpj_fn(n, states[n]) for n in range(N)])
    zero = oracle_zero(algo, theta, c.Y, c.x_infr)
    c.lpj = np.concatenate((zero[:, None], body), axis=1) if S_perm else body
    for a in (c.Y, c.states, c.lpj):
        a.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def mirror_of(case_key, n_samples, seed, prior_mix, first_index=0):
    """The mirror's result for a kn_case (case_key = its arguments as a tuple), computed once."""
    c = kn_case(*case_key)
    return estimate_log_likelihood_counter(
        "bsc" if c.algo == "ebsc" else "sssc", c.theta, c.states, c.lpj, c.lpj_fn, S_perm=c.S_perm, background=c.background,
        n_samples=n_samples, seed=seed, first_index=first_index, prior_mix=prior_mix, x_infr=c.x_infr)

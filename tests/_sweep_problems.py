"""Problems for the local-search tests (tests/test_sweep_states_host.py, tests/test_gpu_sweep_states.py): the thetas and data
of tests/_seed_problems.py, K^n from seed_states_host, its lpj rows from the oracle, and the NumPy mirror of one sweep's
proposals, computed once per case and handed out read-only."""
from functools import lru_cache

import numpy as np

from _seed_problems import make_data, make_theta
from evo_amd.variational import seed_states_host, sweep_states_host
from oracle import evo_oracle as orc

# name -> (N, D, H, S, S_perm, P, q, max_active of the seeding, true latents of the data)
CASES = {
    "ragged": (37, 8, 70, 12, 0, 2, 4, 4, 3),       # HW = 2 with a ragged word; N no multiple of four
    "ragged_perm": (37, 8, 70, 12, 1, 2, 4, 4, 3),  # ... with the permanent all-zero state
    "s200": (9, 16, 130, 200, 0, 3, 8, 8, 3),       # more than 64 states per lane loop; HW = 3
    "tight": (33, 4, 8, 20, 0, 2, 8, 3, 1),         # fewer scored neighbours than q; singleton parents (removal = all-zero)
    "large_h": (5, 8, 1100, 6, 0, 1, 4, 6, 3),      # HW = 18
}
ALGOS = ("ebsc", "es3c")
SEEDS = {name: 300 + i for i, name in enumerate(sorted(CASES))}


def model_name(algo):
    return "bsc" if algo == "ebsc" else "sssc"


def oracle_theta(algo, theta, D, H):
    th = dict(theta)
    if algo == "ebsc":
        orc.bsc_precompute(th, D, H)
    else:
        orc.sssc_precompute(th, D)
    return th


def oracle_lpj(algo, oth, y, states):
    """The oracle's lpj of ``states`` bool (C, H) for one datapoint (clamped as the reference clamps; finite scores pass)."""
    states = np.asarray(states, dtype=bool)
    out = np.empty(len(states))
    nz = states.any(axis=1)
    cnt = orc.new_counters()
    if algo == "ebsc":
        out[:] = orc.bsc_lpj(oth, states, y, cnt)
    else:
        if nz.any():
            out[nz] = orc.sssc_lpj(oth, states[nz], y, cnt, {})
        if (~nz).any():
            out[~nz] = orc.sssc_lpj_allzero(oth, y, cnt)[0]
    return out


def rows_of(algo, theta, Y, ss, S_perm):
    """lpj rows (N, S_perm + S) of K^n from the oracle."""
    N, S, H = ss.shape
    oth = oracle_theta(algo, theta, Y.shape[1], H)
    lpj = np.empty((N, S_perm + S))
    for n in range(N):
        if S_perm:
            lpj[n, 0] = oracle_lpj(algo, oth, Y[n], np.zeros((1, H), dtype=bool))[0]
        lpj[n, S_perm:] = oracle_lpj(algo, oth, Y[n], ss[n])
    return lpj


class SweepProblem:
    pass


def build(algo, N, D, H, S, S_perm, P, q, A, k, seed):
    rng = np.random.RandomState(seed + (0 if algo == "ebsc" else 1000))
    p = SweepProblem()
    p.algo, p.model, p.N, p.D, p.H, p.S, p.S_perm, p.P, p.q, p.Cmax = algo, model_name(algo), N, D, H, S, S_perm, P, q, P * q
    p.theta = make_theta(rng, algo, D, H)
    p.Y, p.s_true = make_data(rng, algo, p.theta, N, k=k)
    p.ss = seed_states_host(p.model, p.theta, p.Y, S, A, S_perm)[0]
    p.lpj = rows_of(algo, p.theta, p.Y, p.ss, S_perm)
    (p.cand, p.counts, p.scores, p.best_flip, p.gain, p.n_capped,
     p.margin) = sweep_states_host(p.model, p.theta, p.Y, p.ss, p.lpj, S_perm, P, q)
    for a in (p.Y, p.ss, p.lpj, p.cand, p.counts, p.scores, p.best_flip, p.gain, p.n_capped, p.margin):
        a.setflags(write=False)
    return p


@lru_cache(maxsize=None)
def problem(algo, name):
    N, D, H, S, S_perm, P, q, A, k = CASES[name]
    return build(algo, N, D, H, S, S_perm, P, q, A, k, SEEDS[name])


# ---- ES3C only: hand-made parents of 7, 8, 9 and 10 active latents, to exercise the cap and n_capped.  S = 1: the one state
# of K^n is the parent whatever its lpj.
CAPS = dict(N=8, D=12, H=40, S=1, S_perm=0, P=1, q=6, sizes=(7, 8, 9, 10))


@lru_cache(maxsize=None)
def caps_problem():
    c = CAPS
    rng = np.random.RandomState(77)
    p = SweepProblem()
    p.algo, p.model, p.N, p.D, p.H, p.S, p.S_perm, p.P, p.q, p.Cmax = ("es3c", "sssc", c["N"], c["D"], c["H"], c["S"], 0, c["P"],
                                                                          c["q"], c["P"] * c["q"])
    p.theta = make_theta(rng, "es3c", p.D, p.H)
    p.Y, _ = make_data(rng, "es3c", p.theta, p.N, k=8)
    p.sizes = np.array([c["sizes"][n % len(c["sizes"])] for n in range(p.N)])
    p.ss = np.zeros((p.N, p.S, p.H), dtype=bool)
    for n in range(p.N):
        p.ss[n, 0, rng.choice(p.H, size=p.sizes[n], replace=False)] = True
    p.lpj = rows_of("es3c", p.theta, p.Y, p.ss, 0)
    (p.cand, p.counts, p.scores, p.best_flip, p.gain, p.n_capped,
     p.margin) = sweep_states_host("sssc", p.theta, p.Y, p.ss, p.lpj, 0, p.P, p.q)
    return p


def compare_proposals(p, cand, counts, decided_tol=1e-7):
    """The GPU's (or any) proposals against the mirror's: datapoints with margin > ``decided_tol`` must match in rows and
    counts exactly, the rest up to the first difference.  Returns the undecided datapoints."""
    undecided = []
    for n in range(p.N):
        same = counts[n] == p.counts[n] and np.array_equal(cand[n, :counts[n]], p.cand[n, :p.counts[n]])
        if same:
            continue
        assert p.margin[n] <= decided_tol, "datapoint %d (margin %.3g): counts %d vs %d, rows differ at %s" % (
            n, p.margin[n], counts[n], p.counts[n],
            np.flatnonzero((cand[n, :p.Cmax] != p.cand[n]).any(axis=1))[:4])
        undecided.append(n)
    return undecided

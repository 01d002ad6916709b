"""Problems for the local-search tests on incomplete data (tests/test_sweep_states_masked_host.py,
tests/test_gpu_sweep_states_masked.py): Theta and data of tests/_seed_problems.py, an i.i.d. mask of reliable entries per
missing fraction (tests/_seed_masked_problems.py: make_mask) with NaN in the data wherever it is False, K^n from
seed_states_host(..., x_infr=), its lpj rows from the oracle's masked lpj and the NumPy mirror of one sweep's proposals,
computed once per problem and handed out read-only."""
from functools import lru_cache

import numpy as np

from _seed_masked_problems import make_mask
from _seed_problems import make_data, make_theta
from _sweep_problems import SweepProblem, compare_proposals, model_name  # noqa: F401  (the GPU tests take them from here)
from evo_amd.variational import seed_states_host, sweep_states_host
from oracle import evo_oracle as orc

# name -> (N, D, H, S, S_perm, P, q, max_active of the seeding, true latents of the data)
CASES = {
    "ragged": (37, 8, 70, 12, 0, 2, 4, 4, 3),       # ragged state word; N no multiple of the waves per workgroup
    "ragged_perm": (37, 8, 70, 12, 1, 2, 4, 4, 3),  # ... with the permanent all-zero state
    "s200": (9, 16, 130, 200, 0, 3, 8, 8, 3),       # more than 64 states per lane loop; ES3C at k = 8
    "tight": (33, 4, 8, 20, 0, 2, 8, 3, 1),         # fewer scored neighbours than q; singleton parents; one reliable entry
    "large_h": (5, 8, 1100, 6, 0, 1, 4, 6, 3),      # HW = 18
    "wide_d": (11, 70, 70, 12, 0, 2, 4, 4, 3),      # D no multiple of 64
    "d130": (6, 130, 40, 16, 0, 2, 4, 8, 3),        # D > 2 * 64, H < 64
    "rows_gmem": (3, 4, 1990, 8, 0, 1, 4, 8, 3),    # ES3C: ten rows of 2048 doubles do not fit LDS
    # a row without any reliable entry (datapoint 0) and a row with exactly one (datapoint 1)
    "empty_row": (7, 8, 70, 12, 0, 2, 4, 4, 3),
    # EBSC: one wavefront's share of LDS is 45 216 bytes, three fit 150 KiB and four do not (the workgroup steps down by one)
    "wpw3": (7, 4, 1800, 6, 0, 1, 4, 3, 3),
}
FRACTIONS = (0.3, 0.6)
ALGOS = ("ebsc", "es3c")
ONLY = {"rows_gmem": ("es3c",), "wpw3": ("ebsc",)}
# picked so that every problem's smallest margin exceeds 1e-6 (tests/test_sweep_states_masked_host.py holds them to it)
SEEDS = {name: 700 + i for i, name in enumerate(sorted(CASES))}
SEEDS["d130"] = 720  # (700 leaves ES3C at 0.3 a margin of 8e-7)
# (1800 latents rank closely and D = 4 leaves rows without a reliable entry: the first seed from 709 on with margins above
# 2e-6 -- 2.5e-5 and 1.1e-5 -- and a reliable entry in every row at both fractions)
SEEDS["wpw3"] = 816


def all_problems():
    return [(algo, name, f) for name in sorted(CASES) for algo in ONLY.get(name, ALGOS) for f in FRACTIONS]


def oracle_theta(algo, theta, D, H, x_infr):
    """Theta with the oracle's derived keys; ljc counts the reliable entries."""
    th = dict(theta)
    if algo == "ebsc":
        orc.bsc_precompute(th, D, H, x_infr)
    else:
        orc.sssc_precompute(th, D, x_infr)
    return th


def oracle_lpj(algo, oth, y, states, obs):
    """The oracle's masked lpj of ``states`` bool (C, H) for one datapoint with the reliable entries ``obs``."""
    states = np.asarray(states, dtype=bool)
    out = np.empty(len(states))
    nz = states.any(axis=1)
    cnt = orc.new_counters()
    if algo == "ebsc":
        out[:] = orc.bsc_lpj(oth, states, y, cnt, x_infr=obs)
    else:
        if nz.any():
            out[nz] = orc.sssc_lpj(oth, states[nz], y, cnt, {}, obs=obs)
        if (~nz).any():
            out[~nz] = orc.sssc_lpj_allzero(oth, y, cnt, obs=obs)[0]
    return out


def rows_of(algo, theta, Y, x_infr, ss, S_perm):
    """lpj rows (N, S_perm + S) of K^n from the oracle's masked lpj."""
    N, S, H = ss.shape
    oth = oracle_theta(algo, theta, Y.shape[1], H, x_infr)
    lpj = np.empty((N, S_perm + S))
    for n in range(N):
        if S_perm:
            lpj[n, 0] = oracle_lpj(algo, oth, Y[n], np.zeros((1, H), dtype=bool), x_infr[n])[0]
        lpj[n, S_perm:] = oracle_lpj(algo, oth, Y[n], ss[n], x_infr[n])
    return lpj


def finish(p):
    """The rows and the mirror of a problem whose theta, Y, x_infr and ss are set."""
    p.lpj = rows_of(p.algo, p.theta, p.Y, p.x_infr, p.ss, p.S_perm)
    (p.cand, p.counts, p.scores, p.best_flip, p.gain, p.n_capped,
     p.margin) = sweep_states_host(p.model, p.theta, p.Y, p.ss, p.lpj, p.S_perm, p.P, p.q, x_infr=p.x_infr)
    for a in (p.Y, p.x_infr, p.ss, p.lpj, p.cand, p.counts, p.scores, p.best_flip, p.gain, p.n_capped, p.margin):
        a.setflags(write=False)
    return p


def build(algo, N, D, H, S, S_perm, P, q, A, k, seed, missing, empty_row=False):
    rng = np.random.RandomState(seed + (0 if algo == "ebsc" else 1000) + int(round(100 * missing)))
    p = SweepProblem()
    p.algo, p.model, p.N, p.D, p.H, p.S, p.S_perm, p.P, p.q, p.Cmax = algo, model_name(algo), N, D, H, S, S_perm, P, q, P * q
    p.missing = missing
    p.theta = make_theta(rng, algo, D, H)
    Y, p.s_true = make_data(rng, algo, p.theta, N, k=k)
    p.x_infr = make_mask(rng, N, D, missing)
    if empty_row:
        p.x_infr[0] = False
        p.x_infr[1] = False
        p.x_infr[1, 3] = True
    p.Y = np.where(p.x_infr, Y, np.nan)
    p.ss = seed_states_host(p.model, p.theta, p.Y, S, A, S_perm, x_infr=p.x_infr)[0]
    return finish(p)


@lru_cache(maxsize=None)
def problem(algo, name, missing):
    N, D, H, S, S_perm, P, q, A, k = CASES[name]
    return build(algo, N, D, H, S, S_perm, P, q, A, k, SEEDS[name], missing, empty_row=name == "empty_row")


# ---- ES3C only: hand-made parents of 7, 8, 9 and 10 active latents on masked data, to exercise the cap and n_capped.  S = 1:
# the one state of K^n is the parent whatever its lpj.
CAPS = dict(N=8, D=12, H=40, S=1, S_perm=0, P=1, q=6, sizes=(7, 8, 9, 10), missing=0.3)


@lru_cache(maxsize=None)
def caps_problem():
    c = CAPS
    rng = np.random.RandomState(78)
    p = SweepProblem()
    p.algo, p.model, p.N, p.D, p.H, p.S, p.S_perm, p.P, p.q, p.Cmax = ("es3c", "sssc", c["N"], c["D"], c["H"], c["S"], 0, c["P"],
                                                                          c["q"], c["P"] * c["q"])
    p.missing = c["missing"]
    p.theta = make_theta(rng, "es3c", p.D, p.H)
    Y, _ = make_data(rng, "es3c", p.theta, p.N, k=8)
    p.x_infr = make_mask(rng, p.N, p.D, p.missing)
    p.Y = np.where(p.x_infr, Y, np.nan)
    p.sizes = np.array([c["sizes"][n % len(c["sizes"])] for n in range(p.N)])
    p.ss = np.zeros((p.N, p.S, p.H), dtype=bool)
    for n in range(p.N):
        p.ss[n, 0, rng.choice(p.H, size=p.sizes[n], replace=False)] = True
    return finish(p)

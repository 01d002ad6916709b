"""Problems for the K^n seeding tests on incomplete data (tests/test_seed_states_masked_host.py,
tests/test_gpu_seed_states_masked.py): Theta and data of tests/_seed_problems.py, an i.i.d. mask of reliable entries per
missing fraction and NaN in the data wherever the mask is False.  Every row keeps at least one reliable entry unless the
case says otherwise.  The NumPy mirror of a problem is computed once and handed out read-only."""
from functools import lru_cache

import numpy as np

from _seed_problems import make_data, make_theta
from evo_amd.variational import seed_states_host

# name -> (N, D, H, S, A, S_perm)
CASES = {
    "ragged": (37, 8, 70, 12, 4, 0),       # ragged last state word; N is no multiple of the waves per workgroup
    "ragged_perm": (37, 8, 70, 12, 4, 1),  # ... with the permanent all-zero state
    "s200": (9, 16, 130, 200, 8, 0),       # more than 64 states per step; ES3C at k = 8
    "tight": (33, 4, 8, 20, 3, 0),         # quotas against the latents left; rows with one reliable entry
    "large_h": (5, 8, 1100, 6, 6, 0),      # HW = 18; keys re-read from LDS
    "wide_d": (11, 70, 70, 12, 4, 0),      # D not a multiple of 64 in the d-sweep
    "d130": (6, 130, 40, 16, 8, 0),        # D > 2 * 64, H < 64
    "rows_gmem": (3, 4, 1990, 8, 8, 0),    # ES3C: eight rows of 2048 doubles do not fit LDS -- the context's buffer holds them
    # a row without any reliable entry (datapoint 0) and a row with exactly one (datapoint 1)
    "empty_row": (7, 8, 70, 12, 4, 0),
}
FRACTIONS = (0.3, 0.6)
ALGOS = ("ebsc", "es3c")
# picked so that every problem's smallest margin exceeds 1e-6 (tests/test_seed_states_masked_host.py holds them to it)
SEEDS = {name: 300 + i for i, name in enumerate(sorted(CASES))}


def make_mask(rng, N, D, missing, keep_one=True):
    xi = rng.random_sample((N, D)) >= missing
    if keep_one:
        for n in np.nonzero(~xi.any(axis=1))[0]:
            xi[n, rng.randint(D)] = True
    return xi


class SeedProblem:
    pass


@lru_cache(maxsize=None)
def problem(algo, name, missing):
    N, D, H, S, A, S_perm = CASES[name]
    rng = np.random.RandomState(SEEDS[name] + (0 if algo == "ebsc" else 1000) + int(round(100 * missing)))
    p = SeedProblem()
    p.algo, p.N, p.D, p.H, p.S, p.A, p.S_perm, p.missing = algo, N, D, H, S, A, S_perm, missing
    p.theta = make_theta(rng, algo, D, H)
    Y, p.s_true = make_data(rng, algo, p.theta, N)
    p.x_infr = make_mask(rng, N, D, missing)
    if name == "empty_row":
        p.x_infr[0] = False
        p.x_infr[1] = False
        p.x_infr[1, 3] = True
    p.Y = np.where(p.x_infr, Y, np.nan)
    p.states, p.path, p.lpj_path, p.margin = seed_states_host("bsc" if algo == "ebsc" else "sssc", p.theta, p.Y, S, A, S_perm,
                                                              x_infr=p.x_infr)
    for a in (p.Y, p.x_infr, p.states, p.path, p.lpj_path, p.margin):
        a.setflags(write=False)
    return p


ONLY = {"rows_gmem": ("es3c",)}  # (EBSC keeps no rows; with D = 4 most of its 1990 scores would be near-ties)


def all_problems():
    return [(algo, name, f) for name in sorted(CASES) for algo in ONLY.get(name, ALGOS) for f in FRACTIONS]

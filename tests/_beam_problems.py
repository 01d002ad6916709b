"""Problems for the beam-seeding tests (tests/test_seed_beam_host.py, tests/test_gpu_seed_beam.py): the shapes of
tests/_seed_problems.py that the beam stresses, one of this file's own (large_h2: HW = 18 with q_t = 2) and the correlated
dictionary of tests/_swap_problems.py, where a single greedy path falls short.  Each case has its own seed, chosen on the CPU
so that the mirror's smallest margin is at least MARGIN_MIN for every (case, model, beam) in USED -- the GPU comparison
demands all datapoints equal, and that bound is what decides them; a case that missed it got another seed.  The NumPy mirror
of a (case, model, beam) is computed once and handed out read-only."""
from functools import lru_cache

import numpy as np

from _seed_problems import make_data, make_theta
from _swap_problems import correlated_theta
from evo_amd.variational import seed_states_beam_host

MARGIN_MIN = 1e-7
ALGOS = ("ebsc", "es3c")
# name -> (N, D, H, S, A, S_perm)
CASES = {
    "ragged": (37, 8, 70, 12, 4, 0),       # ragged last word; N is no multiple of the waves per workgroup
    "ragged_perm": (37, 8, 70, 12, 4, 1),  # ... with the permanent all-zero state
    "tight": (33, 4, 8, 20, 3, 0),         # quotas 7, 7, 6 of 8, 7, 6 latents: most candidates of a later parent are duplicates
    "s200": (9, 16, 130, 200, 8, 0),       # 25 states per step: lists above 64 entries over the parents; beam at the cap
    "large_h2": (5, 8, 1100, 12, 6, 0),    # HW = 18, keys re-read from LDS in the threshold search (H > 1024)
    "correlated": (64, 16, 130, 32, 4, 0),  # columns share H / 4 directions: the first greedy pick is often a look-alike
}
# the beams the tests use per case (1 everywhere: the greedy law)
USED = {"ragged": (1, 3), "ragged_perm": (1, 3), "tight": (1, 4, 6), "s200": (1, 4, 16), "large_h2": (1, 2), "correlated": (1, 4)}
# ragged, ragged_perm, tight and correlated keep the seeds of their home files; s200 has its own (the seed of
# tests/_seed_problems.py leaves an ES3C margin of 4e-8 at beam 1 and 405 is the first of 400 .. 419 with 2e-7 or more everywhere)
SEEDS = {"ragged": 101, "ragged_perm": 102, "tight": 104, "s200": 405, "large_h2": 300, "correlated": 9}


class BeamProblem:
    pass


@lru_cache(maxsize=None)
def data(algo, name):
    """Theta and data of a case (no mirror)."""
    N, D, H, S, A, S_perm = CASES[name]
    p = BeamProblem()
    p.algo, p.model, p.name = algo, "bsc" if algo == "ebsc" else "sssc", name
    p.N, p.D, p.H, p.S, p.A, p.S_perm = N, D, H, S, A, S_perm
    if name == "correlated":  # exactly the stream of _swap_problems.correlated_problem
        rng = np.random.RandomState(SEEDS[name])
        p.theta = correlated_theta(rng, algo, D, H)
    else:
        rng = np.random.RandomState(SEEDS[name] + (0 if algo == "ebsc" else 1000))
        p.theta = make_theta(rng, algo, D, H)
    p.Y, p.s_true = make_data(rng, algo, p.theta, N)
    p.Y.setflags(write=False)
    return p


@lru_cache(maxsize=None)
def problem(algo, name, beam):
    """The case with the mirror of ``beam``: states, lpj (every slot), path, lpj_path, margin."""
    src = data(algo, name)
    p = BeamProblem()
    p.__dict__.update(src.__dict__)
    p.beam = beam
    p.states, p.lpj, p.path, p.lpj_path, p.margin = seed_states_beam_host(p.model, p.theta, p.Y, p.S, p.A, beam, p.S_perm)
    for a in (p.states, p.lpj, p.path, p.lpj_path, p.margin):
        a.setflags(write=False)
    return p


def quotas(S, A):
    return [S // A + (1 if t <= S % A else 0) for t in range(1, A + 1)]


def mean_log_sum(lpj):
    """Mean over datapoints of log sum_s exp lpj over the seeded states."""
    m = lpj.max(axis=1)
    return float((m + np.log(np.exp(lpj - m[:, None]).sum(axis=1))).mean())

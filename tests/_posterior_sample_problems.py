"""Problems shared by tests/test_posterior_sample_host.py and tests/test_gpu_posterior_sample.py: the shapes of
tests/_predictive_problems.py (states of k = 0, 1, ..., 12 and 32, two state words, the all-zero state, the background unit,
a datapoint without reliable entries) with the NumPy mirror's draws, computed once per problem (lru_cache; do not modify)."""
from functools import lru_cache

import numpy as np

from _predictive_problems import algo_name, problem
from evo_amd.models import sample_posterior_counter
from evo_amd.variational import init_states

SEED = 20240611
T_MAX = 70  # one full pass of 64 draws and a ragged one; draw t does not depend on n_samples: fewer draws are a prefix

# the ten shapes of tests/test_gpu_predictive.py::CASES -- (algo, N, D, H, incomplete, S_perm, background), noise,
# sync_host -- and the fill of the draws
CASES = [
    (("es3c", 30, 25, 10, False, 1, False), True, True, "all"),
    (("es3c", 37, 70, 70, False, 1, False), True, False, "missing"),
    (("es3c", 37, 64, 70, True, 0, False), False, True, "missing"),
    (("es3c", 37, 70, 70, True, 1, False), True, True, "all"),
    (("es3c", 30, 25, 10, True, 0, True), True, False, "missing"),
    (("es3c", 30, 512, 10, False, 0, False), False, True, "all"),
    (("ebsc", 37, 25, 70, False, 1, False), True, True, "all"),
    (("ebsc", 30, 70, 10, True, 0, False), False, True, "missing"),
    (("ebsc", 37, 64, 10, False, 0, True), True, False, "all"),
    (("ebsc", 30, 512, 10, True, 1, False), True, True, "missing"),
]


def suff_of(p, ss=None, lpj=None):
    """my_suff_stat of a problem (the layout init_states gives a model) holding its K^n and lpj rows."""
    suff = init_states(p.N, p.S, p.H, "fit", "randflip", 4, 1, 1, permanent=dict(p.permanent))
    ss, lpj = (p.ss if ss is None else ss), (p.lpj if lpj is None else lpj)
    assert suff["ss"].shape == ss.shape and suff["lpj"].shape == lpj.shape
    suff["ss"], suff["lpj"] = np.array(ss), np.array(lpj)
    return suff


def mirror(p, n_samples, fill="all", noise=True, seed=SEED, first_index=0, rows=slice(None), theta=None, lpj=None):
    """sample_posterior_counter on (the datapoints ``rows`` of) a problem."""
    xi = p.x_infr[rows] if p.incomplete else None
    return sample_posterior_counter(algo_name(p.algo), p.theta if theta is None else theta, p.ss[rows],
                                    (p.lpj if lpj is None else lpj)[rows], p.Y[rows], xi, p.S_perm, p.background,
                                    n_samples=n_samples, seed=seed, first_index=first_index, fill=fill, noise=noise)


@lru_cache(maxsize=None)
def draws(case, fill, noise, n_samples=T_MAX):
    """The mirror's dict for a shape of tests/_predictive_problems.py::problem, read-only."""
    out = mirror(problem(*case), n_samples, fill, noise)
    for k, a in out.items():
        if k != "info":
            a.setflags(write=False)
    return out


def moments(p, noise=True):
    """(mean, var) of predictive_moments_host for a problem (the arrays the problem holds already)."""
    return p.mean, (p.var if noise else p.var0)


def q_of(lpj):
    """q_ns from the lpj rows with NumPy's own exp."""
    e = np.exp(lpj - lpj.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def moment_bounds(y, mean, var):
    """The issue's two checks on draws y (N, T, D) against a mean and a variance per entry: returns the largest
    |sample mean - mean| / sqrt(var / T) and |sample variance - var| / sqrt((m4 - var^2) / T) over the entries whose
    reference is not NaN (m4: the sample's fourth central moment)."""
    T = y.shape[1]
    ok = ~np.isnan(mean)
    assert np.array_equal(np.isnan(y).any(axis=1), ~ok) and np.array_equal(np.isnan(y).all(axis=1), ~ok)
    m = y.mean(axis=1)
    c = y - m[:, None, :]
    s2 = (c ** 2).mean(axis=1)
    m4 = (c ** 4).mean(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        zm = np.abs(m - mean) / np.sqrt(var / T)
        zv = np.abs(s2 - var) / np.sqrt((m4 - var ** 2) / T)
    return float(zm[ok].max()), float(zv[ok].max())


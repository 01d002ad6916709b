"""Problems for the neighbourhood-bound tests (tests/test_neighbour_bound_host.py, tests/test_gpu_neighbour_bound.py): the cases
of tests/_sweep_problems.py, tests/_sweep_masked_problems.py and tests/_swap_problems.py (each shape has a reason that holds
here as well) with the NumPy mirror evo_amd.variational.neighbour_bound_host, a hand-made K^n whose parents are pairwise two
flips apart, and the brute-force set the bound sums over.  Computed once per case and handed out read-only."""
from functools import lru_cache

import numpy as np

import _swap_problems as wp
import _sweep_masked_problems as mp
import _sweep_problems as sp
from _seed_problems import make_data, make_theta
from evo_amd.variational import neighbour_bound_host

ALGOS = sp.ALGOS
CAP = {"ebsc": 64, "es3c": 8}
DECIDED_TOL = 1e-7    # the sweeps' decided_tol: best_parent / best_flip are exact above this margin
MAX_UNDECIDED = 0.02  # of the datapoints of a case may fall below it

# the masked cases per model: ES3C with the rows of G(n) in LDS ("empty_row", which has a row without a reliable entry) and in
# the context's buffer ("rows_gmem": ten rows of 2048 doubles do not fit one wavefront's share); EBSC with D no multiple of 64
# and with the permanent all-zero column.  EBSC's "empty_row" is a case of its own (EMPTY_ROW): scored by the prior alone, all
# neighbours of one size tie exactly, so its margin is 0 by construction and best_parent / best_flip are left to the law's
# tie rule, which the host test checks.
MASKED = {"ebsc": (("wide_d", 0.3), ("ragged_perm", 0.6)), "es3c": (("empty_row", 0.6), ("rows_gmem", 0.6))}
EMPTY_ROW = ("masked", "ebsc", "empty_row", 0.6, 0)


def gpu_cases():
    """(kind, algo, name, missing, P) of every case the GPU test runs; P = 0 stands for S."""
    out = [("complete", algo, name, None, P) for algo in ALGOS for name in sp.CASES for P in (1, 0)]
    out.append(("caps", "es3c", "caps", None, 1))
    out += [("masked", algo, name, f, P) for algo in ALGOS for name, f in MASKED[algo] for P in (1, 0)]
    return out


def case_id(case):
    kind, algo, name, missing, P = case
    return "%s-%s-%s%s-P%s" % (kind, algo, name, "" if missing is None else "-%g" % missing, P or "S")


def problem_of(kind, algo, name, missing=None):
    if kind == "complete":
        return sp.problem(algo, name)
    if kind == "caps":
        return sp.caps_problem()
    if kind == "small":
        return wp.small(algo)
    if kind == "two_apart":
        return two_apart(algo)
    return mp.problem(algo, name, missing)


def _frozen(res):
    for a in res.values():
        a.setflags(write=False)
    return res


def mirror_on(p, P, lpj=None):
    """The mirror of problem ``p`` with P parents (0: S), on ``lpj`` (None: the problem's own rows)."""
    return neighbour_bound_host(p.model, p.theta, p.Y, p.ss, p.lpj if lpj is None else lpj, p.S_perm, P or p.S,
                                x_infr=getattr(p, "x_infr", None))


@lru_cache(maxsize=None)
def mirror(kind, algo, name, missing, P):
    return _frozen(mirror_on(problem_of(kind, algo, name, missing), P))


# ---- a hand-made K^n whose S states are pairwise two flips apart: {0, a} for a = 1 .. S.  Every parent reaches the singleton
# {0} and the pairs of the others' latents, so without rule (d) states are counted more than once.
TWO_APART = dict(N=5, D=8, H=12, S=6)


@lru_cache(maxsize=None)
def two_apart(algo):
    c = TWO_APART
    rng = np.random.RandomState(41 if algo == "ebsc" else 1041)
    p = sp.SweepProblem()
    p.algo, p.model, p.N, p.D, p.H, p.S, p.S_perm = algo, sp.model_name(algo), c["N"], c["D"], c["H"], c["S"], 0
    p.P, p.q, p.Cmax = p.S, 1, p.S
    p.theta = make_theta(rng, algo, p.D, p.H)
    p.Y, _ = make_data(rng, algo, p.theta, p.N, k=2)
    p.ss = np.zeros((p.N, p.S, p.H), dtype=bool)
    p.ss[:, :, 0] = True
    p.ss[:, np.arange(p.S), np.arange(1, p.S + 1)] = True
    p.lpj = sp.rows_of(algo, p.theta, p.Y, p.ss, 0)
    for a in (p.Y, p.ss, p.lpj):
        a.setflags(write=False)
    return p


# ---- brute force: the SET the bound sums over, built with Python sets of row bytes
def parents_of(p, n, P, lpj=None):
    row = (p.lpj if lpj is None else lpj)[n, p.S_perm:]
    return np.lexsort((np.arange(p.S), -row))[:P or p.S]


def neighbour_set(p, n, P, lpj=None):
    """The non-zero states within distance 1 of a parent, within the cap, that K^n does not hold: a list of bool rows."""
    held = {s.tobytes() for s in p.ss[n]}
    seen, out = set(), []
    for slot in parents_of(p, n, P, lpj):
        for j in range(p.H):
            nb = p.ss[n, slot].copy()
            nb[j] = ~nb[j]
            key = nb.tobytes()
            if nb.any() and nb.sum() <= CAP[p.algo] and key not in held and key not in seen:
                seen.add(key)
                out.append(nb)
    return out


def logsumexp(v):
    v = np.asarray(v, dtype=np.float64)
    m = v.max()
    return m + np.log(np.exp(v - m).sum())


def brute_force(p, P, lpj=None):
    """(F_plus (N,), n_states (N,)) over K^n and the set, with the oracle's lpj of the set's states and the rows ``lpj`` (None:
    the problem's own, which are the oracle's) for K^n.  Complete data."""
    oth = sp.oracle_theta(p.algo, p.theta, p.D, p.H)
    rows = p.lpj if lpj is None else lpj
    Fp, cnt = np.empty(p.N), np.zeros(p.N, dtype=np.int32)
    for n in range(p.N):
        nbs = neighbour_set(p, n, P, lpj)
        cnt[n] = len(nbs)
        extra = sp.oracle_lpj(p.algo, oth, p.Y[n], np.array(nbs)) if nbs else np.empty(0)
        Fp[n] = logsumexp(np.concatenate([rows[n], extra]))
    return Fp, cnt


def compare(p, got, want, rtol=1e-9):
    """A result dict ``got`` (the engine's, or any) against the mirror's ``want`` on the same rows: counts exact, F, M and F_plus
    to ``rtol`` relative, best_parent / best_flip exact where the mirror's margin exceeds DECIDED_TOL.  Returns the undecided
    datapoints."""
    assert np.array_equal(got["n_states"], want["n_states"]), np.flatnonzero(got["n_states"] != want["n_states"])[:8]
    assert np.array_equal(got["n_capped"], want["n_capped"]), np.flatnonzero(got["n_capped"] != want["n_capped"])[:8]
    for k in ("F", "M", "F_plus", "best_score"):
        a, b = got[k], want[k]
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), k
        assert np.array_equal(a[~np.isfinite(b)], b[~np.isfinite(b)], equal_nan=True), k
        f = np.isfinite(b)
        err = np.abs(a[f] - b[f]) / np.maximum(1.0, np.abs(b[f]))
        print("%s %s: worst relative error %.3g" % (p.algo, k, err.max() if f.any() else 0.0))
        assert (err <= rtol).all(), (k, err.max())
    decided = want["margin"] > DECIDED_TOL
    for k in ("best_parent", "best_flip"):
        assert np.array_equal(got[k][decided], want[k][decided]), k
    return np.flatnonzero(~decided)

"""Problems for the tests of AIS on incomplete data (tests/test_ais_masked_host.py, tests/test_gpu_ais_masked.py): the
dictionaries and data of tests/_ais_problems.build with an i.i.d. mask of reliable entries per missing fraction
(tests/_seed_masked_problems.make_mask), NaN in the data wherever the mask is False, row 0 without a reliable entry and row 1
with exactly one (as tests/_sweep_masked_problems.build(empty_row=True)); the NumPy mirrors of both directions of
ais_log_likelihood_counter and of ais_posterior_counter at n_keep = 1 and 3, all with ``x_infr``; and, where H allows it, the
exact answer by enumeration with the oracle's masked lpj.  Computed once per problem and handed out read-only.

The shapes are the three of _ais_problems.CASES, those at which the chunked scan can go wrong; T = 12, C = 5.  The data seeds
were chosen ON THE CPU, with the mirror alone, by the rule of _ais_problems: the first seed from 300 on for which no chain of
either direction, nor of the posterior call (n_keep = 3, which holds the chains of n_keep = 1), has a decision closer than
MARGIN_CPU = 1e-7 to its uniform.  ``python tests/_ais_masked_problems.py`` repeats every search below and prints what it
finds; SEED_MARGINS is what it printed for SEEDS.

ALLTRUE: the mirror with an all-True ``x_infr`` against the complete mirror on the same three problems of _ais_problems, both
directions.  The two differ only in how G is summed (a loop over d with every product rounded, against np.dot), so the states
agree wherever the margin decides and log w agrees to rounding: ALLTRUE_MEASURED is the largest |log w - log w'| / max(1,
|log w'|) that the search printed, ALLTRUE_TOL = 100 times that.

SMALL_SEED (H = 8, half the entries missing) was chosen on the CPU as _ais_problems.SMALL_SEED was: the first seed from 1 on
for which the 5 SE bars of _ais_problems.check_bars hold for the mirror in both directions AND every posterior marginal
satisfies _ais_post_problems.bar_excess <= 0.  EXACT_SEED likewise for the H = 10 problem of _ais_problems.MODEL_EXACT with half
the entries hidden, with the mirrors at the stream seed the GPU test hands to the model (EXACT_STREAM).  The mirror is
deterministic for a seed, so neither test can flicker.
"""
from functools import lru_cache

import numpy as np

import _ais_post_problems as pp
import _ais_problems as ap
import _exact_problems as ep
from _seed_masked_problems import make_mask
from evo_amd.models import ais_log_likelihood_counter, ais_posterior_counter, sigmoid_schedule

CASES = ap.CASES
T, C = ap.T, ap.C
KEEPS = (1, 3)
FRACTIONS = (0.3, 0.6)
STREAM_SEED = ap.STREAM_SEED
MARGIN_CPU = ap.MARGIN_CPU
MARGIN_DECIDED = ap.MARGIN_DECIDED
MAX_UNDECIDED = ap.MAX_UNDECIDED

# (name, missing) -> data seed, and the smallest margin over both directions and the posterior call at that seed
SEEDS = {("partial_chunk", 0.3): 300, ("partial_chunk", 0.6): 300, ("two_words", 0.3): 300, ("two_words", 0.6): 300,
         ("three_words", 0.3): 302, ("three_words", 0.6): 300}
SEED_MARGINS = {("partial_chunk", 0.3): 9.94e-6, ("partial_chunk", 0.6): 8.64e-6, ("two_words", 0.3): 5.44e-6,
                ("two_words", 0.6): 2.71e-6, ("three_words", 0.3): 1.31e-7, ("three_words", 0.6): 3.52e-6}
SMALLEST_MARGIN = 1.31e-7  # over all six problems; the tests read the mirrors' own margins

ALLTRUE_MEASURED = 7.92e-15
ALLTRUE_TOL = 100.0 * ALLTRUE_MEASURED

SMALL = dict(N=8, D=6, H=8, T=64, C=256, K=4, missing=0.5)
SMALL_SEED = 7
EXACT = dict(ap.MODEL_EXACT, K=4, missing=0.5)  # N = 16, D = 8, H = 10, T = 64, C = 256
EXACT_SEED = 56
EXACT_STREAM = ap.MODEL_EXACT_STREAM


def build(N, D, H, seed, missing, edge_rows=True):
    """Theta, s and data of _ais_problems.build; x_infr i.i.d. with ``missing`` of the entries False; edge_rows: row 0 has no
    reliable entry and row 1 exactly one.  NaN stands under every False entry."""
    full = ap.build(N, D, H, seed)
    p = ap.AisProblem()
    p.N, p.D, p.H, p.missing = N, D, H, missing
    p.theta, p.s_true = full.theta, full.s_true
    rng = np.random.RandomState(seed + 5000 + int(round(100 * missing)))
    p.x_infr = make_mask(rng, N, D, missing)
    if edge_rows:
        p.x_infr[0] = False
        p.x_infr[1] = False
        p.x_infr[1, 3] = True
    p.Y = np.where(p.x_infr, full.Y, np.nan)
    p.Y_full = full.Y
    p.Y.setflags(write=False)
    p.x_infr.setflags(write=False)
    return p


def mirror(p, T, C, direction, seed=STREAM_SEED, first_index=0, rows=None):
    rows = slice(None) if rows is None else rows
    return ais_log_likelihood_counter(p.theta, p.Y[rows], n_chains=C, n_temps=T, seed=seed, first_index=first_index,
                                      direction=direction, s_start=p.s_true[rows] if direction == "reverse" else None,
                                      x_infr=p.x_infr[rows])


def mirror_post(p, T, C, K, seed=STREAM_SEED, first_index=0, rows=None, mean=True):
    rows = slice(None) if rows is None else rows
    return ais_posterior_counter(p.theta, p.Y[rows], n_chains=C, n_temps=T, n_keep=K, seed=seed, first_index=first_index,
                                 mean=mean, x_infr=p.x_infr[rows])


@lru_cache(maxsize=None)
def problem(name, missing, seed=None):
    N, D, H = CASES[name]
    p = build(N, D, H, SEEDS[(name, missing)] if seed is None else seed, missing)
    p.name = name
    p.betas = sigmoid_schedule(T)
    p.forward = ap._freeze(mirror(p, T, C, "forward"))
    p.reverse = ap._freeze(mirror(p, T, C, "reverse"))
    p.post = {K: ap._freeze(mirror_post(p, T, C, K)) for K in KEEPS}
    p.margin = min(p.forward["margin"].min(), p.reverse["margin"].min(), min(p.post[K]["margin"].min() for K in KEEPS))
    return p


def all_problems():
    return [(name, f) for name in CASES for f in FRACTIONS]


# The paths of the masked kernels that the three shapes do not take, at 0.3 missing with the two edge rows: the wide
# instantiations (NC = 8, 16) and a column and list above 64 KiB of LDS per workgroup (D = 1500: 4 (512 + 18 000) = 74 048
# bytes for the likelihood kernel, 76 128 for the posterior kernel), where the launch needs its limit raised.
# name -> (N, D, H, T, C, n_keep); seeds by the rule above.
EXTRA = {"nc8": (4, 8, 300, 4, 2, 2), "nc16": (3, 8, 1000, 4, 2, 2), "wide_column": (3, 1500, 10, 4, 2, 2)}
EXTRA_MISSING = 0.3
EXTRA_SEEDS = {"nc8": 300, "nc16": 300, "wide_column": 300}
EXTRA_MARGINS = {"nc8": 3.34e-6, "nc16": 6.34e-6, "wide_column": 2.88e-3}  # what the search printed


@lru_cache(maxsize=None)
def extra_problem(name, seed=None):
    N, D, H, T_, C_, K = EXTRA[name]
    p = build(N, D, H, EXTRA_SEEDS[name] if seed is None else seed, EXTRA_MISSING)
    p.name, p.T, p.C, p.K = name, T_, C_, K
    p.betas = sigmoid_schedule(T_)
    p.forward = ap._freeze(mirror(p, T_, C_, "forward"))
    p.reverse = ap._freeze(mirror(p, T_, C_, "reverse"))
    p.post = ap._freeze(mirror_post(p, T_, C_, K))
    p.margin = min(p.forward["margin"].min(), p.reverse["margin"].min(), p.post["margin"].min())
    return p


# ---- the exact answer by enumeration, from the oracle's masked lpj
def exact_of(p):
    """(ll (N): log sum over all 2^H states of exp(lpj_n(s)) = log p(y_n) - ljc, marginals (N, H)) on the incomplete data."""
    H = p.H
    states = ((np.arange(2 ** H)[:, None] >> np.arange(H)[None, :]) & 1).astype(bool)
    lpj = ep.oracle_lpj("ebsc", p.theta, p.Y, states, x_infr=p.x_infr)  # (N, 2^H)
    m = lpj.max(axis=1, keepdims=True)
    w = np.exp(lpj - m)
    ll = m[:, 0] + np.log(w.sum(axis=1))
    marg = np.dot(w, states.astype(np.float64)) / w.sum(axis=1, keepdims=True)
    ll.setflags(write=False)
    marg.setflags(write=False)
    return ll, marg


def _enumerable(c, data_seed, stream):
    p = build(c["N"], c["D"], c["H"], data_seed, c["missing"], edge_rows=False)
    p.exact, p.exact_marg = exact_of(p)
    p.forward = ap._freeze(mirror(p, c["T"], c["C"], "forward", seed=stream))
    p.reverse = ap._freeze(mirror(p, c["T"], c["C"], "reverse", seed=stream))
    p.post = ap._freeze(mirror_post(p, c["T"], c["C"], c["K"], seed=stream))
    return p


@lru_cache(maxsize=None)
def small(seed=None):
    """The H = 8 problem of the mirror-against-enumeration test, half the entries missing."""
    return _enumerable(SMALL, SMALL_SEED if seed is None else seed, STREAM_SEED)


@lru_cache(maxsize=None)
def exact_problem(seed=None):
    """The H = 10 problem of the GPU test against Model.exact_log_likelihood, half the entries hidden; the mirrors at the
    stream seed that test hands to the model."""
    return _enumerable(EXACT, EXACT_SEED if seed is None else seed, EXACT_STREAM)


def bars_hold(p):
    """Whether the 5 SE bars of both directions and the bars of every posterior marginal hold for the mirrors of p."""
    try:
        ap.check_bars(p.forward, p.reverse, p.exact)
    except AssertionError:
        return False
    return not (pp.bar_excess(p.post, p.exact_marg) > 0.0).any()


def alltrue_difference(name):
    """The largest |log w - log w'| / max(1, |log w'|) between the mirror with an all-True x_infr and the complete mirror
    (both directions, and the posterior call at n_keep = 3), with whether every decided chain has the same states."""
    q = ap.problem(name)
    ones = np.ones_like(q.Y, dtype=bool)
    worst, same = 0.0, True
    for direction, want in (("forward", q.forward), ("reverse", q.reverse)):
        got = ais_log_likelihood_counter(q.theta, q.Y, n_chains=ap.C, n_temps=ap.T, seed=ap.STREAM_SEED, direction=direction,
                                         s_start=q.s_true if direction == "reverse" else None, x_infr=ones)
        ok = np.minimum(got["margin"], want["margin"]) > MARGIN_DECIDED
        same = same and all(np.array_equal(got[k][ok], want[k][ok]) for k in ("final_bool", "chain_flips", "start"))
        worst = max(worst, float((np.abs(got["log_w"] - want["log_w"]) / np.maximum(1.0, np.abs(want["log_w"])))[ok].max()))
    return worst, same


if __name__ == "__main__":  # the searches that chose the figures above
    for name, f in all_problems():
        seed = 300
        while problem(name, f, seed).margin <= MARGIN_CPU:
            seed += 1
        print("(%r, %r): seed %d, smallest margin %.3g" % (name, f, seed, problem(name, f, seed).margin))
    print("all-True mask against the complete mirror: largest relative difference of log w %.3g"
          % max(alltrue_difference(name)[0] for name in CASES))
    for name in EXTRA:
        seed = 300
        while extra_problem(name, seed).margin <= MARGIN_CPU:
            seed += 1
        print("%s: seed %d, smallest margin %.3g" % (name, seed, extra_problem(name, seed).margin))
    for label, make in (("SMALL_SEED", small), ("EXACT_SEED", exact_problem)):
        seed = 1
        while not bars_hold(make(seed)):
            seed += 1
        print("%s: %d" % (label, seed))

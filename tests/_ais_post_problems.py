"""Problems for the tests of the posterior from AIS chains (tests/test_ais_post_host.py, tests/test_gpu_ais_post.py): the
dictionaries and data of tests/_seed_problems.py (EBSC) through tests/_ais_problems.build, with the NumPy mirror
(evo_amd.models.ais_posterior_counter) and, where H allows it, the exact marginals by enumeration with the oracle's lpj.
Computed once per case and handed out read-only.

The device-against-mirror shapes are those at which the chunked scan and its Rao-Blackwell sum can go wrong (a partial
chunk, a full one, the chunk boundary, a last chunk of two latents) at T = 12, C = 5, n_keep = 3, and one case for each wide
instantiation of the kernel (NC = 4, 8, 16) at T = 4, C = 2, n_keep = 2.  The data seeds were chosen ON THE CPU, with the mirror
alone: the first seed from 300 on for which no chain has a decision closer than MARGIN_CPU = 1e-7 to its uniform (``margin``,
the kept scans included), so that the rounding of B = Y W, G = W^T W and exp on the device (about 1e-15 relative) cannot flip
a decision.  ``python tests/_ais_post_problems.py`` repeats the search and prints what it finds; the smallest margins at the
seeds below are in SEED_MARGINS.

EXACT_SEED was chosen on the CPU as well, with the mirror at the stream seed the GPU test hands to the model (EXACT_STREAM):
the first data seed from 1 on for which EVERY entry satisfies |p - exact| <= 5 p_se + 3 / ess_n.  The second term is the
rule-of-three bound on an event that none of ess_n effective chains has seen; p_se, the spread over the chains, cannot know
of such an event.  The mirror is deterministic for a seed, so the test cannot flicker, and the device's chains are the
mirror's wherever ``margin`` is above MARGIN_DECIDED.
"""
from functools import lru_cache

import numpy as np

import _ais_problems as ap
import _sweep_problems as sp
from evo_amd.models import ais_posterior_counter, sigmoid_schedule

# name -> (N, D, H, T, C, n_keep)
CASES = {
    "partial_chunk": (37, 7, 10, 12, 5, 3),   # one partial chunk; N is no multiple of the waves per workgroup
    "full_chunk": (9, 8, 64, 12, 5, 3),       # exactly one chunk: the last lane flips, nothing stays open
    "two_words": (21, 9, 70, 12, 5, 3),       # two words, the chunk boundary at 64
    "three_words": (13, 16, 130, 12, 5, 3),   # three words, a last chunk of two latents (NC = 4)
    "nc4": (5, 8, 200, 4, 2, 2),              # the wide instantiations: NC = 4,
    "nc8": (4, 8, 300, 4, 2, 2),              # 8
    "nc16": (3, 8, 1000, 4, 2, 2),            # and 16, whose LDS is above 64 KiB
}
STREAM_SEED = ap.STREAM_SEED
SEEDS = {"partial_chunk": 300, "full_chunk": 300, "two_words": 300, "three_words": 300, "nc4": 300, "nc8": 300, "nc16": 300}
SEED_MARGINS = {"partial_chunk": 1.1e-5, "full_chunk": 2.12e-6, "two_words": 1.62e-6, "three_words": 3.52e-6, "nc4": 3.51e-6,
                "nc8": 3.52e-6, "nc16": 6.3e-5}  # what the search printed; the tests read the mirror's own margin
MARGIN_CPU = 1e-7      # what the seeds guarantee for the mirror
MARGIN_DECIDED = 1e-9  # a chain above this must match the device bit for bit
MAX_UNDECIDED = 0.01

EXACT = dict(N=16, D=8, H=10, T=64, C=256, K=4)  # the shape of _ais_problems.MODEL_EXACT
EXACT_SEED = 1
EXACT_STREAM = ap.MODEL_EXACT_STREAM


def mirror(p, T, C, K, seed=STREAM_SEED, first_index=0, betas=None, rows=None, mean=False):
    rows = slice(None) if rows is None else rows
    return ais_posterior_counter(p.theta, p.Y[rows], n_chains=C, n_temps=T, n_keep=K, betas=betas, seed=seed,
                                 first_index=first_index, mean=mean)


@lru_cache(maxsize=None)
def problem(name, seed=None):
    N, D, H, T, C, K = CASES[name]
    p = ap.build(N, D, H, SEEDS[name] if seed is None else seed)
    p.name, p.T, p.C, p.K = name, T, C, K
    p.betas = sigmoid_schedule(T)
    p.want = ap._freeze(mirror(p, T, C, K, mean=True))
    return p


def exact_marginals(p):
    """E_p[s_h | y_n] over all 2^H states, lpj from the oracle: (N, H)."""
    H = p.H
    states = ((np.arange(2 ** H)[:, None] >> np.arange(H)[None, :]) & 1).astype(bool)
    oth = sp.oracle_theta("ebsc", p.theta, p.D, H)
    out = np.empty((p.N, H))
    for n in range(p.N):
        lpj = sp.oracle_lpj("ebsc", oth, p.Y[n], states)
        w = np.exp(lpj - lpj.max())
        out[n] = (w[:, None] * states).sum(axis=0) / w.sum()
    return out


@lru_cache(maxsize=None)
def exact_problem(seed=None):
    """The enumerable problem: the mirror at the stream seed of the GPU test, and the exact marginals."""
    c = EXACT
    p = ap.build(c["N"], c["D"], c["H"], EXACT_SEED if seed is None else seed)
    p.exact = exact_marginals(p)
    p.exact.setflags(write=False)
    p.want = ap._freeze(mirror(p, c["T"], c["C"], c["K"], seed=EXACT_STREAM))
    return p


def bar_excess(info, exact):
    """|p - exact| - (5 p_se + 3 / ess_n) per entry: the bars hold where it is <= 0."""
    return np.abs(info["p"] - exact) - (5.0 * info["p_se"] + 3.0 / info["ess"][:, None])


def check_bars(info, exact):
    """The bars of the issue on every entry, the figures printed before they are asserted."""
    err = np.abs(info["p"] - exact)
    excess = bar_excess(info, exact)
    print("|p - exact|: largest %.3g, mean %.3g; smallest ess %.3g; largest excess over 5 p_se %.3g against 3 / ess >= %.3g" % (
        err.max(), err.mean(), info["ess"].min(), (err - 5.0 * info["p_se"]).max(), (3.0 / info["ess"]).min()))
    assert (excess <= 0.0).all(), np.argwhere(excess > 0.0)


def unpack(states, H):
    """np.packbits layout along the last axis -> bool (..., H)."""
    return np.unpackbits(np.asarray(states, dtype=np.uint8), axis=-1)[..., :H].astype(bool)


if __name__ == "__main__":  # the searches that chose the seeds above
    for name in CASES:
        seed = 300
        while problem(name, seed).want["margin"].min() <= MARGIN_CPU:
            seed += 1
        print("%s: seed %d, smallest margin %.3g" % (name, seed, problem(name, seed).want["margin"].min()))
    seed = 1
    while (bar_excess(exact_problem(seed).want, exact_problem(seed).exact) > 0.0).any():
        seed += 1
    print("exact problem: seed %d" % seed)
    check_bars(exact_problem(seed).want, exact_problem(seed).exact)

"""Problems for the annealed-importance-sampling tests (tests/test_ais_host.py, tests/test_gpu_ais.py): the dictionaries and
data of tests/_seed_problems.py (EBSC) with the NumPy mirror of both directions, and the exact answer by enumeration with the
oracle's lpj where H allows it.  Computed once per case and handed out read-only.

The shapes of the device-against-mirror cases are those at which the chunked scan can go wrong; T = 12, C = 5.
The data seeds were chosen ON THE CPU, with the mirror alone: the first seed from 300 on for which no chain of either
direction has a decision closer than 1e-7 to its uniform (``margin``), so that the rounding of B = Y W, G = W^T W and exp on
the device (about 1e-15 relative) cannot flip a decision.  SMALL_SEED was chosen on the CPU as well: the first seed from 1
on for which the 5 SE bars of tests/test_ais_host.py hold for the mirror in both directions (the mirror is deterministic
for a seed, so the test cannot flicker).  MODEL_EXACT_SEED likewise, with the mirror at the stream seed the GPU test
passes to the model (MODEL_EXACT_STREAM): the first seed from 1 on for which the bars hold is 18.  Seeds 1 .. 17 miss a bar,
nearly always an upper one: every reverse chain of a datapoint starts from the SAME state, so the spread over the chains,
which is all SE_n measures, does not hold the variance that comes from the start; an unlucky generating s (one the posterior
gives little mass) shifts all chains of that datapoint together.  The device's chains are the mirror's bit for bit at this
seed (smallest margin 4.7e-8), so the choice made on the CPU holds on the GPU.
"""
from functools import lru_cache

import numpy as np

import _sweep_problems as sp
from _seed_problems import make_data, make_theta
from evo_amd.models import ais_log_likelihood_counter, sigmoid_schedule

# name -> (N, D, H)
CASES = {
    "partial_chunk": (37, 7, 10),   # one partial chunk; N is no multiple of the waves per workgroup
    "two_words": (21, 9, 70),       # two words, the chunk boundary at 64
    "three_words": (13, 16, 130),   # three words, a last chunk of two latents
}
T, C = 12, 5
STREAM_SEED = 20261021
SEEDS = {"partial_chunk": 300, "two_words": 300, "three_words": 300}
MARGIN_CPU = 1e-7     # what the seeds guarantee for the mirror
MARGIN_DECIDED = 1e-9  # a chain above this must match the device bit for bit
MAX_UNDECIDED = 0.01

SMALL = dict(N=8, D=6, H=8, T=64, C=256)
SMALL_SEED = 1
MODEL_EXACT = dict(N=16, D=8, H=10, T=64, C=256)  # the GPU test against Model.exact_log_likelihood
MODEL_EXACT_SEED = 18
MODEL_EXACT_STREAM = 5


class AisProblem:
    pass


def build(N, D, H, seed, k=3):
    rng = np.random.RandomState(seed)
    p = AisProblem()
    p.N, p.D, p.H = N, D, H
    p.theta = make_theta(rng, "ebsc", D, H)
    p.Y, p.s_true = make_data(rng, "ebsc", p.theta, N, k=min(k, H))
    p.Y.setflags(write=False)
    p.s_true.setflags(write=False)
    return p


def mirror(p, T, C, direction, seed=STREAM_SEED, first_index=0, betas=None, rows=None):
    rows = slice(None) if rows is None else rows
    return ais_log_likelihood_counter(p.theta, p.Y[rows], n_chains=C, n_temps=T, betas=betas, seed=seed, first_index=first_index,
                                      direction=direction, s_start=p.s_true[rows] if direction == "reverse" else None)


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def problem(name, seed=None):
    N, D, H = CASES[name]
    p = build(N, D, H, SEEDS[name] if seed is None else seed)
    p.name = name
    p.betas = sigmoid_schedule(T)
    p.forward = _freeze(mirror(p, T, C, "forward"))
    p.reverse = _freeze(mirror(p, T, C, "reverse"))
    return p


def exact_ll(p):
    """log sum over all 2^H states of exp(lpj_n(s)) per datapoint, lpj from the oracle: log p(y_n) - ljc."""
    H = p.H
    states = ((np.arange(2 ** H)[:, None] >> np.arange(H)[None, :]) & 1).astype(bool)
    oth = sp.oracle_theta("ebsc", p.theta, p.D, H)
    out = np.empty(p.N)
    for n in range(p.N):
        lpj = sp.oracle_lpj("ebsc", oth, p.Y[n], states)
        m = lpj.max()
        out[n] = m + np.log(np.exp(lpj - m).sum())
    return out


@lru_cache(maxsize=None)
def small(seed=None):
    """The enumerable problem of the mirror-against-the-exact-answer test, both directions and the exact answer."""
    c = SMALL
    p = build(c["N"], c["D"], c["H"], SMALL_SEED if seed is None else seed)
    p.exact = exact_ll(p)
    p.forward = _freeze(mirror(p, c["T"], c["C"], "forward"))
    p.reverse = _freeze(mirror(p, c["T"], c["C"], "reverse"))
    return p


def bars(info, reverse):
    """SE_n = std(w) / (mean(w) sqrt(C)) of the averaged terms (w forward, 1 / w reverse), from the chains' weights."""
    a = -info["log_w"] if reverse else info["log_w"]
    w = np.exp(a - a.max(axis=1, keepdims=True))
    return w.std(axis=1) / (w.mean(axis=1) * np.sqrt(a.shape[1]))


def check_bars(lower, upper, exact):
    """The 5 SE bars of the issue, each figure printed before it is asserted."""
    se_lo, se_up = bars(lower, False), bars(upper, True)
    d_lo, d_up = np.abs(lower["ll"] - exact), np.abs(upper["ll"] - exact)
    print("lower: |ll - exact| / SE at most %.3g (SE at most %.3g); upper: %.3g (SE at most %.3g); mean lower %.6f, exact %.6f, "
          "mean upper %.6f" % ((d_lo / se_lo).max(), se_lo.max(), (d_up / se_up).max(), se_up.max(), lower["ll"].mean(),
                               exact.mean(), upper["ll"].mean()))
    assert (d_lo <= 5.0 * se_lo).all(), (d_lo / se_lo)
    assert (d_up <= 5.0 * se_up).all(), (d_up / se_up)
    se_mean = np.sqrt((se_lo ** 2).sum() + (se_up ** 2).sum()) / len(exact)
    assert lower["ll"].mean() <= upper["ll"].mean() + 5.0 * se_mean


def unpack_final(final, N, C, H):
    """``final`` in np.packbits layout -> bool (N, C, H)."""
    return np.unpackbits(np.asarray(final, dtype=np.uint8).reshape(N, C, (H + 7) // 8), axis=-1)[:, :, :H].astype(bool)

"""Problems for the tests of the AIS rescue (tests/test_ais_rescue_host.py, tests/test_gpu_ais_rescue.py): the posterior
chains on listed datapoints and their best states handed to K^n (Model.ais_posterior(index=..., admit=True)).

The chain problems are those of tests/_ais_post_problems.py (and one of tests/_ais_masked_problems.py) with their seeds and
margins: a listed call walks the same streams, so what those files guarantee for the mirror holds row by row.  The seed 300
of ``two_words`` passes the caps on undecided chains for the lists below as it stands (tests/test_ais_rescue_host.py checks
it), so no further search was needed.

K^n for the admission is seed_states_host("bsc", theta, Y, S = 12, 3, 0), as in the admit test of tests/test_gpu_ais.py.

HAND: hand-made inputs of the emission for the probe (Engine.ais_post_admit_probe) -- N = 6, C = 7, H = 70 (two words),
S = 5, Cmax = 3; datapoint 3 is not in the list.  What each row is there for stands beside it.
"""
from functools import lru_cache

import numpy as np

import _ais_post_problems as pp
import _ais_problems as ap  # noqa: F401  (the problems of pp are built on it)
from evo_amd.models import ais_admit_candidates_host
from evo_amd.variational import seed_states_host

STREAM_SEED = pp.STREAM_SEED
MARGIN_DECIDED = pp.MARGIN_DECIDED
MAX_UNDECIDED = pp.MAX_UNDECIDED

# the lists of the listed-equals-full tests: the first and the last datapoint, and a gap
LISTS = {"partial_chunk": [0, 1, 5, 6, 7, 20, 36], "two_words": [0, 3, 4, 11, 20], "nc16": [0, 2]}
MASKED_CASE = ("two_words", 0.3)
MASKED_LIST = [0, 1, 2, 9, 20]  # (rows 0 and 1: no reliable entry, exactly one)

ADMIT = dict(name="two_words", S=12, Cmax=4)  # Cmax < C = 5


def kn_states(p, S=ADMIT["S"]):
    return seed_states_host("bsc", p.theta, p.Y, S, 3, 0)[0]


@lru_cache(maxsize=None)
def admit_problem():
    """two_words with K^n from the greedy seed and every second datapoint listed; the mirror's emission per listed datapoint."""
    p = pp.problem(ADMIT["name"])
    q = ap.AisProblem()
    q.p, q.S, q.Cmax = p, ADMIT["S"], ADMIT["Cmax"]
    q.index = np.arange(0, p.N, 2, dtype=np.int64)
    q.ss = kn_states(p, q.S)
    q.ss.setflags(write=False)
    q.emit = [ais_admit_candidates_host(p.want["chain_map_lpj"][n], p.want["chain_map_bool"][n], q.ss[n], q.Cmax) for n in q.index]
    return q


# ---- the hand-made emission inputs -----------------------------------------------------------------------------------------------
HAND = dict(N=6, C=7, H=70, S=5, Cmax=3, D=4)
HAND_INDEX = np.array([0, 1, 2, 4, 5], dtype=np.int64)


def _st(*bits):
    s = np.zeros(HAND["H"], dtype=bool)
    s[list(bits)] = True
    return s


def hand_kn():
    """K^n of the hand-made problem: slot s of every datapoint holds the latents {s, 64 + s} (one bit in each word)."""
    kn = np.zeros((HAND["N"], HAND["S"], HAND["H"]), dtype=bool)
    for s in range(HAND["S"]):
        kn[:, s] = _st(s, 64 + s)
    return kn


def hand_inputs():
    """(chain_map_lpj (5, 7), chain_map_state bool (5, 7, 70)) for the rows HAND_INDEX."""
    nan, inf = np.nan, np.inf
    held2, held0 = _st(2, 66), _st(0, 64)
    rows = [
        # datapoint 0: an exact tie (chains 1 and 2: the lower chain first); n_new = 7 > Cmax
        ([-5.0, -3.0, -3.0, -7.0, -4.0, -6.0, -8.0], [_st(10 + c, 69) for c in range(7)]),
        # datapoint 1: NaN, -inf and +inf are left out; chain 0 (NaN) is the fold's map chain and K^n holds its state
        ([nan, -inf, inf, -2.0, -1.0, -3.0, -2.5], [held0, _st(20), _st(21), _st(22), _st(23, 68), _st(24), _st(25)]),
        # datapoint 2: all chains equal
        ([-1.0, -1.0, -2.0, -0.5, -3.0, -1.0, -4.0], [_st(30, 65)] * 7),
        # datapoint 4: the all-zero state ranked first (and last); a state K^n holds second, repeated; a repeated new one
        ([-1.0, -2.0, -3.0, -2.5, -4.0, -5.0, -6.0], [_st(), held2, _st(40), held2, _st(40), _st(41, 67), _st()]),
        # datapoint 5: a state K^n holds ranked first; states that differ in the second word alone; a tie of three;
        # n_new = 5 > Cmax
        ([-1.0, -2.0, -2.0, -2.0, -3.0, -3.5, -9.0], [held0, _st(3, 69), _st(3, 68), _st(3), _st(69), _st(3, 69), _st(1, 2, 3)]),
    ]
    lpj = np.array([r[0] for r in rows])
    st = np.array([r[1] for r in rows])
    return lpj, st

"""Problems for the tests of K^n resized (tests/test_resize_states_host.py, tests/test_gpu_resize_states.py): thetas, data,
K^n and oracle rows of tests/_sweep_problems.py, each shape there for a reason, plus hand-made rows and states on `ragged` and
one problem with the background unit.  Built once per case and handed out read-only; the mirror
(evo_amd.variational.resize_states_host) is computed once per (algo, case, S_new)."""
from functools import lru_cache

import numpy as np

import _sweep_problems as sp
from evo_amd.variational import resize_states_host

ALGOS = sp.ALGOS

# name -> the new sizes.  S of the case: ragged 12, s200 200, s64 64, s63 63, large_h 6, tight 20, handmade 12, background 12
RESIZES = {
    "ragged": (5, 30),       # N = 37, D = 8, H = 70: a ragged word, N no multiple of the waves per workgroup
    "ragged_perm": (5, 30),  # ... with the permanent all-zero column in front of the rows
    "s200": (64, 70, 199),   # N = 9, H = 130: four chunks of the 64-slot lane loop, cut at, above and far above a chunk
    "s64": (200,),           # ... the other way: one full chunk of held states, 136 fills
    "s63": (65,),            # ... and across the chunk's end from below
    "large_h": (4, 9),       # N = 5, H = 1100: HW = 18
    "tight": (35, 1),        # N = 33, D = 4, H = 8: 8 * 9 / 2 - 1 = 35 is the bound, met exactly -- every candidate that is
                             # not skipped is used; and the shrink to one state
    "handmade": (5, 30, 100),  # ragged with planted rows and states (HANDMADE names the datapoints); 100 reaches the pairs
    "background": (20,),     # H = 40 with the background unit, S = 12
}
# the S each case starts from (problem() asserts it): importing a test module builds no problem
CASE_S = {"ragged": 12, "ragged_perm": 12, "s200": 200, "s64": 64, "s63": 63, "large_h": 6, "tight": 20, "handmade": 12,
          "background": 12}
TIGHT_REFUSED = 36           # one above the bound of `tight`
# datapoints of `handmade` (S = 12, H = 70)
HANDMADE = {"tie": 0, "specials": 1, "all_neginf": 2, "singleton_best": 3, "pair_best": 4, "allzero_best": 5}


class ResizeProblem:
    pass


def _from_sweep(p, background=False):
    r = ResizeProblem()
    r.algo, r.model, r.N, r.D, r.H, r.S, r.S_perm = p.algo, p.model, p.N, p.D, p.H, p.S, p.S_perm
    r.theta, r.Y, r.ss, r.lpj, r.background = p.theta, p.Y, p.ss, p.lpj, background
    return r


def _unheld(ss_n, make, H):
    """The first state make(h) (h ascending) that the datapoint does not hold."""
    held = {s.tobytes() for s in ss_n}
    for h in range(H):
        s = make(h)
        if s.tobytes() not in held:
            return s
    raise AssertionError("every candidate is held")


def _handmade(algo):
    base = sp.problem(algo, "ragged")
    r = _from_sweep(base)
    ss, lpj = base.ss.copy(), base.lpj.copy()
    H, S = r.H, r.S
    assert S == 12 and r.S_perm == 0
    # equal values straddling the 5th rank: three above, then four equal ones of which the two lowest slots are kept
    n = HANDMADE["tie"]
    lpj[n] = -50.0 - np.arange(S)
    lpj[n, [10, 1, 6]] = (-1.0, -2.0, -3.0)
    lpj[n, [9, 3, 7, 4]] = -4.0
    # -inf, NaN, +inf (all rank as -inf, the lowest slots of them first), -0.0 beside +0.0 (equal keys: the lower slot first)
    n = HANDMADE["specials"]
    lpj[n] = -10.0 - np.arange(S)
    lpj[n, 2], lpj[n, 5], lpj[n, 0], lpj[n, 8], lpj[n, 7], lpj[n, 3] = -np.inf, np.nan, np.inf, -0.0, 0.0, -1.0
    # nothing finite: the best state is slot 0
    n = HANDMADE["all_neginf"]
    lpj[n] = -np.inf

    def single(h):
        s = np.zeros(H, dtype=bool)
        s[h] = True
        return s

    def pair(h):
        s = single(h)
        s[(h + 3) % H] = True
        return s

    # a best state that is a singleton / a pair: e_c = b gives the empty state, which is skipped
    n = HANDMADE["singleton_best"]
    ss[n, 4] = _unheld(ss[n], single, H)
    lpj[n, 4] = lpj[n].max() + 1.0
    n = HANDMADE["pair_best"]
    ss[n, 7] = _unheld(ss[n], pair, H)
    lpj[n, 7] = lpj[n].max() + 1.0
    # S_perm = 0: the all-zero state as an ordinary row, and the best one -- its neighbours are the enumeration itself
    n = HANDMADE["allzero_best"]
    assert ss[n].any(axis=1).all()
    ss[n, 6] = False
    lpj[n, 6] = lpj[n].max() + 1.0
    r.ss, r.lpj = ss, lpj
    return r


def _background(algo):
    r = ResizeProblem()
    rng = np.random.RandomState(41 if algo == "ebsc" else 42)
    r.algo, r.model, r.N, r.D, r.H, r.S, r.S_perm, r.background = algo, sp.model_name(algo), 13, 8, 40, 12, 0, True
    r.theta = r.Y = None  # (the law reads states and rows only)
    r.ss = np.zeros((r.N, r.S, r.H), dtype=bool)
    for n in range(r.N):
        seen = set()
        for j in range(r.S):
            while True:
                s = rng.random_sample(r.H) < 0.08
                s[-1] = True
                if s[:-1].any() and s.tobytes() not in seen:
                    break
            seen.add(s.tobytes())
            r.ss[n, j] = s
    r.ss[0, 3, :-1] = False  # a best state next to "only the unit": flipping its one varying latent is skipped
    r.ss[0, 3, 17] = True
    r.lpj = rng.normal(size=(r.N, r.S)) * 5.0
    r.lpj[0, 3] = r.lpj[0].max() + 1.0
    return r


@lru_cache(maxsize=None)
def problem(algo, name):
    if name in ("ragged", "ragged_perm", "s200", "large_h", "tight"):
        r = _from_sweep(sp.problem(algo, name))
    elif name in ("s64", "s63"):
        N, D, H, _, S_perm, P, q, A, k = sp.CASES["s200"]
        r = _from_sweep(sp.build(algo, N, D, H, 64 if name == "s64" else 63, S_perm, P, q, A, k, sp.SEEDS["s200"] + 50))
    elif name == "handmade":
        r = _handmade(algo)
    else:
        assert name == "background", name
        r = _background(algo)
    r.name = name
    assert r.S == CASE_S[name], (name, r.S)
    for a in (r.ss, r.lpj):
        a.setflags(write=False)
    return r


def all_resizes():
    return [(name, S_new) for name in RESIZES for S_new in RESIZES[name]]


def shrinks():
    return [(name, S_new) for name, S_new in all_resizes() if S_new < CASE_S[name]]


def grows():
    return [(name, S_new) for name, S_new in all_resizes() if S_new > CASE_S[name]]


@lru_cache(maxsize=None)
def mirror(algo, name, S_new):
    p = problem(algo, name)
    states, src = resize_states_host(p.ss, p.lpj, p.S_perm, S_new, p.background)
    states.setflags(write=False)
    src.setflags(write=False)
    return states, src


def seed_key_order(row):
    """The slots of a row (S values, the permanent column taken off) in rank order: descending key, then ascending slot."""
    row = np.asarray(row, dtype=np.float64)
    key = np.where(np.isfinite(row), row, -np.inf) + 0.0
    return np.lexsort((np.arange(len(row)), -key))

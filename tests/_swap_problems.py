"""Problems for the swap-neighbourhood tests (tests/test_swap_states_host.py, tests/test_gpu_swap_states.py): the cases of
tests/_sweep_problems.py (each shape has a reason that holds here as well) with the NumPy mirror of the swap stage, the
hand-made ES3C parents of the caps problem, and one problem of this file's own: a correlated dictionary whose K^n is closed
under one flip on the CPU, so that the mirror shows datapoints that only a swap improves.  Computed once per case and handed
out read-only."""
from functools import lru_cache

import numpy as np

import _sweep_problems as sp
from _seed_problems import make_data, make_theta
from evo_amd.variational import seed_states_host, swap_states_host, sweep_states_host

CASES = sp.CASES
ALGOS = sp.ALGOS
# the seeds of tests/_sweep_problems.py; a case whose swap margins fell below the bound would get its own seed here
SEEDS = dict(sp.SEEDS)


class SwapProblem:
    pass


def _with_swaps(src):
    """``src`` (a SweepProblem) with the swap mirror beside its flip mirror: the flip fields keep their names, the swap stage's
    are cand_swap, counts_swap, scores_swap, best_swap, swap_gain, n_capped_swap, margin_swap."""
    p = SwapProblem()
    p.__dict__.update(src.__dict__)
    (p.cand_swap, p.counts_swap, p.scores_swap, p.best_swap, p.swap_gain, p.n_capped_swap,
     p.margin_swap) = swap_states_host(p.model, p.theta, p.Y, p.ss, p.lpj, p.S_perm, p.P, p.q)
    p.Cmax_both = 2 * p.P * p.q
    for a in (p.cand_swap, p.counts_swap, p.scores_swap, p.best_swap, p.swap_gain, p.n_capped_swap, p.margin_swap):
        a.setflags(write=False)
    return p


@lru_cache(maxsize=None)
def problem(algo, name):
    if SEEDS[name] == sp.SEEDS[name]:
        return _with_swaps(sp.problem(algo, name))
    N, D, H, S, S_perm, P, q, A, k = CASES[name]
    return _with_swaps(sp.build(algo, N, D, H, S, S_perm, P, q, A, k, SEEDS[name]))


@lru_cache(maxsize=None)
def small(algo):
    """The H = 10 shape of the monotone-and-closed test of tests/test_gpu_sweep_states.py, with room for both stages."""
    return _with_swaps(sp.build(algo, 33, 6, 10, 20, 0, 1, 10, 3, 3, 500))


@lru_cache(maxsize=None)
def caps_problem():
    return _with_swaps(sp.caps_problem())


# ---- a correlated dictionary: columns share one of H / 4 directions, so greedy seeding often picks a latent that resembles
# the true one -- it cannot be removed first without a loss, nor the right one added first.  K^n is seeded, then closed under
# one flip of its best state on the CPU (mirror proposals, oracle lpj, the S best kept), which is where a swap is needed.
CORRELATED = dict(N=64, D=16, H=130, S=12, S_perm=0, P=1, q=6, A=4, k=3)
CORRELATED_SEEDS = {"ebsc": 9, "es3c": 9}  # chosen on the CPU: 12 / 2 of 64 datapoints are closed under one flip and gain by a swap


def correlated_theta(rng, algo, D, H):
    theta = make_theta(rng, algo, D, H)
    base = rng.normal(size=(D, H // 4))
    theta["W"] = 0.8 * (0.8 * base[:, rng.randint(0, H // 4, H)] + 0.6 * rng.normal(size=(D, H)))
    return theta


@lru_cache(maxsize=None)
def correlated_problem(algo, seed=None):
    c = CORRELATED
    rng = np.random.RandomState(CORRELATED_SEEDS[algo] if seed is None else seed)
    p = sp.SweepProblem()
    p.algo, p.model = algo, sp.model_name(algo)
    p.N, p.D, p.H, p.S, p.S_perm, p.P, p.q = c["N"], c["D"], c["H"], c["S"], c["S_perm"], c["P"], c["q"]
    p.Cmax = p.P * p.q
    p.theta = correlated_theta(rng, algo, p.D, p.H)
    p.Y, p.s_true = make_data(rng, algo, p.theta, p.N, k=c["k"])
    ss = seed_states_host(p.model, p.theta, p.Y, p.S, c["A"], 0)[0]
    lpj = sp.rows_of(algo, p.theta, p.Y, ss, 0)
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    for _ in range(32):  # flip sweeps on the CPU until nothing enters K^n
        cand, counts = sweep_states_host(p.model, p.theta, p.Y, ss, lpj, 0, p.P, p.q)[:2]
        changed = False
        for n in range(p.N):
            if counts[n] == 0:
                continue
            new = cand[n, :counts[n]]
            pool, pl = np.concatenate([ss[n], new]), np.concatenate([lpj[n], sp.oracle_lpj(algo, oth, p.Y[n], new)])
            keep = np.argsort(-pl, kind="stable")[:p.S]
            changed = changed or bool((keep >= p.S).any())
            ss[n], lpj[n] = pool[keep], pl[keep]
        if not changed:
            break
    p.ss, p.lpj = ss, lpj
    (p.cand, p.counts, p.scores, p.best_flip, p.gain, p.n_capped,
     p.margin) = sweep_states_host(p.model, p.theta, p.Y, p.ss, p.lpj, 0, p.P, p.q)
    for a in (p.Y, p.ss, p.lpj, p.cand, p.counts, p.scores, p.best_flip, p.gain, p.n_capped, p.margin):
        a.setflags(write=False)
    p = _with_swaps(p)
    # flip-closed and swap-improvable, with a gain no rounding error explains
    p.marked = np.flatnonzero((p.gain <= 0.0) & (p.swap_gain > 1e-6))
    return p


def compare_proposals(N, margin, want_cand, want_counts, cand, counts, decided_tol=1e-7):
    """Proposals against a mirror's: datapoints with margin > ``decided_tol`` must match in rows and counts exactly.  Returns
    the undecided datapoints."""
    undecided = []
    for n in range(N):
        same = counts[n] == want_counts[n] and np.array_equal(cand[n, :counts[n]], want_cand[n, :want_counts[n]])
        if same:
            continue
        assert margin[n] <= decided_tol, "datapoint %d (margin %.3g): counts %d vs %d" % (n, margin[n], counts[n], want_counts[n])
        undecided.append(n)
    return undecided

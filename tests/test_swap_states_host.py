"""evo_amd.variational.swap_states_host, the NumPy mirror of the swap stage of the local search on K^n
(csrc/kernels_sweep_swap.hpp), against the oracle's lpj and a brute force over every swap of a parent.  CPU only."""
import numpy as np
import pytest

import _sweep_problems as sp
import _swap_problems as wp

RTOL = 1e-9  # the tolerance tests/test_sweep_states_host.py uses for the one-flip scores
DECIDED = 1e-7
CASES = [(algo, name) for algo in wp.ALGOS for name in wp.CASES]
CAP = {"ebsc": 64, "es3c": 8}


def _parents(p, n):
    row = p.lpj[n, p.S_perm:]
    return np.lexsort((np.arange(p.S), -row))[:p.P]


def _held(p, n, state):
    return (p.ss[n] == state).all(axis=1).any()


def _all_swaps(p, n, par):
    """Every swap of ``par`` that the law admits, in ascending (a, j): (a, j, state) with K^n not holding the state."""
    act, free = np.flatnonzero(par), np.flatnonzero(~par)
    if len(act) == 0 or len(act) > CAP[p.algo]:
        return np.zeros((0, 2), dtype=int), np.zeros((0, p.H), dtype=bool)
    aj = np.array([(a, j) for a in act for j in free], dtype=int).reshape(-1, 2)
    states = np.repeat(par[None], len(aj), axis=0)
    states[np.arange(len(aj)), aj[:, 0]] = False
    states[np.arange(len(aj)), aj[:, 1]] = True
    kn = {s.tobytes() for s in p.ss[n]}
    new = np.array([s.tobytes() not in kn for s in states], dtype=bool)
    return aj[new], states[new]


@pytest.mark.parametrize("algo,name", CASES)
def test_scores_are_the_oracle_lpj_of_the_proposed_states(algo, name):
    p = wp.problem(algo, name)
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    worst = 0.0
    for n in range(p.N):
        c = p.counts_swap[n]
        assert np.isnan(p.scores_swap[n, c:]).all() and not p.cand_swap[n, c:].any()
        if c == 0:
            continue
        want = sp.oracle_lpj(algo, oth, p.Y[n], p.cand_swap[n, :c])
        err = np.abs(p.scores_swap[n, :c] - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, err.max())
    print("%s %s: worst relative error of the swap scores %.3g" % (algo, name, worst))
    assert worst <= RTOL


@pytest.mark.parametrize("algo,name", CASES)
def test_proposals_are_the_brute_force_top_q_of_all_swaps(algo, name):
    p = wp.problem(algo, name)
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    n_compared = 0
    for n in range(p.N):
        at = 0
        for slot in _parents(p, n):
            par = p.ss[n, slot]
            aj, states = _all_swaps(p, n, par)
            k = min(p.q, len(aj))  # (every admitted swap of these problems has a finite score)
            rows, sc = p.cand_swap[n, at:at + k], p.scores_swap[n, at:at + k]
            # swap neighbours of the parent, new, distinct, in rank order
            assert ((rows != par).sum(axis=1) == 2).all() and (rows.sum(axis=1) == par.sum()).all(), (name, n, slot)
            assert not any(_held(p, n, r) for r in rows), "a state K^n holds was proposed"
            assert len({r.tobytes() for r in rows}) == k
            a_of = np.argmax(par & ~rows, axis=1) if k else np.zeros(0, dtype=int)
            j_of = np.argmax(rows & ~par, axis=1) if k else np.zeros(0, dtype=int)
            for i in range(k - 1):  # descending score, ties by ascending a, then ascending j
                assert sc[i] > sc[i + 1] or (sc[i] == sc[i + 1] and (a_of[i], j_of[i]) < (a_of[i + 1], j_of[i + 1]))
            if k and p.margin_swap[n] > DECIDED:  # the brute-force top q of all m (H - m) swaps by the oracle's lpj
                lp = sp.oracle_lpj(algo, oth, p.Y[n], states)
                order = np.lexsort((aj[:, 1], aj[:, 0], -lp))[:k]
                assert np.array_equal(states[order], rows), (name, n, slot)
                n_compared += 1
            at += k
        assert p.counts_swap[n] == at, (name, n, p.counts_swap[n], at)
    assert n_compared > 0


@pytest.mark.parametrize("algo,name", CASES)
def test_certificate_is_the_brute_force_swap_of_the_best_state(algo, name):
    p = wp.problem(algo, name)
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    for n in range(p.N):
        par = p.ss[n, _parents(p, n)[0]]
        aj, states = _all_swaps(p, n, par)
        if len(aj) == 0:
            assert tuple(p.best_swap[n]) == (-1, -1) and p.swap_gain[n] == -np.inf
            continue
        lp = sp.oracle_lpj(algo, oth, p.Y[n], states)
        base = sp.oracle_lpj(algo, oth, p.Y[n], par[None])[0]
        best = lp.max()
        # the mirror's winner is within rounding of the brute-force maximum, and its gain is that maximum minus the base
        at = np.flatnonzero((aj == p.best_swap[n]).all(axis=1))
        assert len(at) == 1, (name, n, p.best_swap[n])
        assert best - lp[at[0]] <= RTOL * max(1.0, abs(best)), (name, n)
        assert abs(p.swap_gain[n] - (best - base)) <= RTOL * max(1.0, abs(base)), (name, n, p.swap_gain[n], best - base)


@pytest.mark.parametrize("algo,name", CASES)
def test_committed_seeds_leave_a_margin(algo, name):
    p = wp.problem(algo, name)
    decided = (p.margin_swap > DECIDED).sum()
    print("%s %s: smallest margin %.3g, %d of %d decided" % (algo, name, p.margin_swap.min(), decided, p.N))
    assert decided >= 0.98 * p.N


def test_tight_has_short_lists_and_singleton_parents():
    for algo in wp.ALGOS:
        p = wp.problem(algo, "tight")
        assert (p.counts_swap < p.P * p.q).any() and (p.counts_swap > 0).any()
        sizes = [p.ss[n, s].sum() for n in range(p.N) for s in _parents(p, n)]
        assert sizes.count(1) > 0


def test_caps():
    p = wp.caps_problem()
    oth = sp.oracle_theta("es3c", p.theta, p.D, p.H)
    for n in range(p.N):
        m, c = p.sizes[n], p.counts_swap[n]
        if m <= 8:  # sizes 7 and 8: the q best of their m (H - m) swaps, nothing capped
            assert c == p.q and p.n_capped_swap[n] == 0 and np.isfinite(p.swap_gain[n]) and (p.best_swap[n] >= 0).all()
            assert (p.cand_swap[n, :c].sum(axis=1) == m).all()
            want = sp.oracle_lpj("es3c", oth, p.Y[n], p.cand_swap[n, :c])
            assert (np.abs(p.scores_swap[n, :c] - want) <= RTOL * np.maximum(1.0, np.abs(want))).all()
        else:  # sizes 9 and 10: above the cap, none of their swaps is emitted
            assert c == 0 and p.n_capped_swap[n] == 1 and p.swap_gain[n] == -np.inf and tuple(p.best_swap[n]) == (-1, -1)
            assert not p.cand_swap[n].any()
    assert set(p.sizes) == {7, 8, 9, 10}


@pytest.mark.parametrize("algo", wp.ALGOS)
def test_correlated_problem_is_flip_closed_and_swap_improvable(algo):
    p = wp.correlated_problem(algo)
    c = wp.CORRELATED
    assert (p.N, p.D, p.H, p.S) == (c["N"], c["D"], c["H"], c["S"])
    print("%s: %d datapoints with gain <= 0, %d of them with a better swap, gains %s" % (
        algo, (p.gain <= 0).sum(), len(p.marked), np.round(p.swap_gain[p.marked], 3)))
    assert len(p.marked) >= 1
    assert (p.margin_swap > DECIDED).sum() >= 0.98 * p.N
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    for n in p.marked:  # the oracle agrees: no better one-flip neighbour outside K^n, and the best swap is better
        best = p.lpj[n].max()
        par = p.ss[n, int(np.argmax(p.lpj[n]))]
        nbs = np.repeat(par[None], p.H, axis=0)
        nbs[np.arange(p.H), np.arange(p.H)] ^= True
        ok = np.array([nb.any() and not _held(p, n, nb) for nb in nbs])
        assert (sp.oracle_lpj(algo, oth, p.Y[n], nbs[ok]) <= best + RTOL * max(1.0, abs(best))).all()
        sw = par.copy()
        sw[p.best_swap[n, 0]], sw[p.best_swap[n, 1]] = False, True
        assert sp.oracle_lpj(algo, oth, p.Y[n], sw[None])[0] > best + 1e-6


def test_refuses_bad_arguments():
    p = wp.problem("ebsc", "tight")
    from evo_amd.variational import swap_states_host
    for P, q in ((0, 1), (p.S + 1, 1), (1, 0)):
        with pytest.raises(ValueError):
            swap_states_host("bsc", p.theta, p.Y, p.ss, p.lpj, 0, P, q)

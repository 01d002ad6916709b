"""evo_amd.variational.sweep_states_host, the NumPy mirror of one sweep's proposals of the local search on K^n
(csrc/kernels_sweep.hpp), against the oracle's lpj and a brute-force flip of the best state.  CPU only."""
import numpy as np
import pytest

import _sweep_problems as sp

RTOL = 1e-9
CASES = [(algo, name) for algo in sp.ALGOS for name in sp.CASES]


def _parents(p, n):
    row = p.lpj[n, p.S_perm:]
    return np.lexsort((np.arange(p.S), -row))[:p.P]


def _held(p, n, state):
    return (p.ss[n] == state).all(axis=1).any()


@pytest.mark.parametrize("algo,name", CASES)
def test_scores_are_the_oracle_lpj_of_the_proposed_states(algo, name):
    p = sp.problem(algo, name)
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    worst = 0.0
    for n in range(p.N):
        c = p.counts[n]
        assert np.isnan(p.scores[n, c:]).all() and not p.cand[n, c:].any()
        if c == 0:
            continue
        want = sp.oracle_lpj(algo, oth, p.Y[n], p.cand[n, :c])
        err = np.abs(p.scores[n, :c] - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, err.max())
    print("%s %s: worst relative error of the scores %.3g" % (algo, name, worst))
    assert worst <= RTOL


@pytest.mark.parametrize("algo,name", CASES)
def test_proposals_are_new_nonzero_one_flip_neighbours_in_rank_order(algo, name):
    p = sp.problem(algo, name)
    for n in range(p.N):
        at = 0
        for slot in _parents(p, n):
            par = p.ss[n, slot]
            # what the law admits for this parent, by brute force
            admitted = 0
            for j in range(p.H):
                nb = par.copy()
                nb[j] = ~nb[j]
                if nb.any() and not _held(p, n, nb) and nb.sum() <= (64 if algo == "ebsc" else 8):
                    admitted += 1
            k = min(p.q, admitted)  # (every admitted neighbour of these problems has a finite score)
            rows, sc = p.cand[n, at:at + k], p.scores[n, at:at + k]
            assert ((rows != par).sum(axis=1) == 1).all(), (name, n, slot)
            assert rows.any(axis=1).all(), "the all-zero state was proposed"
            assert not any(_held(p, n, r) for r in rows), "a state K^n holds was proposed"
            assert len({r.tobytes() for r in rows}) == k
            flips = np.argmax(rows != par, axis=1)
            for i in range(k - 1):  # descending score, ties by ascending latent
                assert sc[i] > sc[i + 1] or (sc[i] == sc[i + 1] and flips[i] < flips[i + 1])
            at += k
        assert p.counts[n] == at, (name, n, p.counts[n], at)


@pytest.mark.parametrize("algo,name", CASES)
def test_certificate_is_the_brute_force_flip_of_the_best_state(algo, name):
    p = sp.problem(algo, name)
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    for n in range(p.N):
        par = p.ss[n, _parents(p, n)[0]]
        nbs = np.repeat(par[None], p.H, axis=0)
        nbs[np.arange(p.H), np.arange(p.H)] ^= True
        ok = np.array([nb.any() and not _held(p, n, nb) for nb in nbs])
        if not ok.any():
            assert p.best_flip[n] == -1 and p.gain[n] == -np.inf
            continue
        lp = sp.oracle_lpj(algo, oth, p.Y[n], nbs[ok])
        base = sp.oracle_lpj(algo, oth, p.Y[n], par[None])[0]
        js = np.flatnonzero(ok)
        best = lp.max()
        # the mirror's winner is within rounding of the brute-force maximum, and its gain is that maximum minus the base
        assert p.best_flip[n] in js
        got = lp[list(js).index(p.best_flip[n])]
        assert best - got <= RTOL * max(1.0, abs(best)), (name, n)
        assert abs(p.gain[n] - (best - base)) <= RTOL * max(1.0, abs(base)), (name, n, p.gain[n], best - base)


@pytest.mark.parametrize("algo,name", CASES)
def test_committed_seeds_leave_a_margin(algo, name):
    p = sp.problem(algo, name)
    print("%s %s: smallest margin %.3g" % (algo, name, p.margin.min()))
    assert p.margin.min() >= 1e-6


def test_tight_has_short_lists_and_singleton_parents():
    for algo in sp.ALGOS:
        p = sp.problem(algo, "tight")
        assert (p.counts < p.P * p.q).all() and (p.counts > 0).any()
        sizes = [p.ss[n, s].sum() for n in range(p.N) for s in _parents(p, n)]
        assert sizes.count(1) > 0


def test_caps():
    p = sp.caps_problem()
    oth = sp.oracle_theta("es3c", p.theta, p.D, p.H)
    for n in range(p.N):
        m, c = p.sizes[n], p.counts[n]
        sizes = p.cand[n, :c].sum(axis=1)
        if m == 7:  # additions reach the cap, nothing is lost
            assert c == p.q and p.n_capped[n] == 0 and np.isfinite(p.gain[n])
        elif m == 8:  # additions are above the cap: removals only
            assert c == p.q and (sizes == 7).all() and p.n_capped[n] == 1 and np.isfinite(p.gain[n])
        elif m == 9:  # removals of 8 latents are scored, the parent has no score of its own
            assert c == p.q and (sizes == 8).all() and p.n_capped[n] == 1 and np.isnan(p.gain[n]) and p.best_flip[n] >= 0
        else:
            assert c == 0 and p.n_capped[n] == 1 and p.gain[n] == -np.inf and p.best_flip[n] == -1
        if c:
            want = sp.oracle_lpj("es3c", oth, p.Y[n], p.cand[n, :c])
            assert (np.abs(p.scores[n, :c] - want) <= RTOL * np.maximum(1.0, np.abs(want))).all()


def test_refuses_bad_arguments():
    p = sp.problem("ebsc", "tight")
    from evo_amd.variational import sweep_states_host
    for P, q in ((0, 1), (p.S + 1, 1), (1, 0)):
        with pytest.raises(ValueError):
            sweep_states_host("bsc", p.theta, p.Y, p.ss, p.lpj, 0, P, q)

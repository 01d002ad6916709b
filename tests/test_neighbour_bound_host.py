"""evo_amd.variational.neighbour_bound_host, the NumPy mirror of the neighbourhood bound (csrc/kernels_nbound.hpp), against
the set definition by brute force, and the refusals of Model.neighbourhood_bound that need no GPU.  CPU only.

1. brute force at H = 10; 2. ownership: every state once; 3. the caps; 4. masks; 5. refusals; and the margins of the cases
the GPU test runs.
"""
import numpy as np
import pytest

import _nbound_problems as nb
import _sweep_masked_problems as mp
import _sweep_problems as sp
from evo_amd.models import BSC, SSSC
from evo_amd.variational import neighbour_bound_host
from evo_amd.variational.utils import _FlipScores

RTOL = 1e-9


# ---- 1. brute force at H = 10 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 0])
@pytest.mark.parametrize("algo", nb.ALGOS)
def test_bound_is_the_logsumexp_over_the_set(algo, P):
    p = nb.problem_of("small", algo, None)
    got = nb.mirror("small", algo, None, None, P)
    want, count = nb.brute_force(p, P)
    assert np.array_equal(got["n_states"], count)
    err = np.abs(got["F_plus"] - want) / np.maximum(1.0, np.abs(want))
    print("%s P = %s: worst relative error of F+ %.3g, mean gap %.4g nats, states %d .. %d" % (
        algo, P or "S", err.max(), got["gap"].mean(), count.min(), count.max()))
    assert err.max() <= RTOL
    # F <= F+ <= the logsumexp over all 2^10 states
    oth = sp.oracle_theta(algo, p.theta, p.D, p.H)
    every = ((np.arange(2 ** p.H)[:, None] >> np.arange(p.H)) & 1).astype(bool)
    for n in range(p.N):
        total = nb.logsumexp(sp.oracle_lpj(algo, oth, p.Y[n], every))
        F = nb.logsumexp(p.lpj[n])
        assert abs(got["F"][n] - F) <= RTOL * max(1.0, abs(F))
        assert got["F"][n] <= got["F_plus"][n] <= total + RTOL * max(1.0, abs(total)), (n, got["F"][n], got["F_plus"][n], total)
    assert (got["gap"] >= 0.0).all() and (got["gap"] > 0.0).any()
    assert ((got["mass_outside"] >= 0.0) & (got["mass_outside"] <= 1.0)).all()


# ---- 2. ownership ------------------------------------------------------------------------------------------------------------
def _count_without_ownership(p, P):
    """The neighbours summed when rule (d) is switched off: every parent's present scores, whoever else reaches the state."""
    fs = _FlipScores(p.model, p.theta, p.Y, p.ss, p.lpj, p.S_perm)
    return np.array([sum(int(np.isfinite(fs.neighbours(n, p.ss[n, slot])[0]).sum()) for slot in fs.parents(n)[:P])
                     for n in range(p.N)])


@pytest.mark.parametrize("algo", nb.ALGOS)
def test_every_state_is_counted_once(algo):
    p = nb.two_apart(algo)
    d = (p.ss[0][:, None, :] ^ p.ss[0][None, :, :]).sum(axis=2)
    assert (d[~np.eye(p.S, dtype=bool)] == 2).all(), "the parents are not pairwise two flips apart"
    got = nb.mirror("two_apart", algo, None, None, 0)
    want, count = nb.brute_force(p, 0)
    # {0}; the S singletons' complements {a}; {0, a, b}, a < b <= S; {0, a, j}, j > S: each once
    S, H = p.S, p.H
    assert (count == 1 + S + S * (S - 1) // 2 + S * (H - 1 - S)).all()
    assert np.array_equal(got["n_states"], count)
    err = np.abs(got["F_plus"] - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= RTOL
    loose = _count_without_ownership(p, S)
    print("%s: %d states in the set, %d summed without rule (d)" % (algo, count[0], loose[0]))
    assert (loose == S + S + S * (S - 1) + S * (H - 1 - S)).all() and (loose > count).all()
    # one parent owns nothing of anybody's: the switch changes nothing at P = 1
    assert np.array_equal(nb.mirror("two_apart", algo, None, None, 1)["n_states"], _count_without_ownership(p, 1))


@pytest.mark.parametrize("algo", nb.ALGOS)
def test_best_is_the_largest_present_score_ties_by_rank_then_latent(algo):
    p = nb.two_apart(algo)
    got = nb.mirror("two_apart", algo, None, None, 0)
    fs = _FlipScores(p.model, p.theta, p.Y, p.ss, p.lpj, 0)
    for n in range(p.N):
        r, j = got["best_parent"][n], got["best_flip"][n]
        sc = fs.neighbours(n, p.ss[n, fs.parents(n)[r]])[0]
        assert sc[j] == got["best_score"][n]
        top = max(fs.neighbours(n, p.ss[n, s])[0].max() for s in fs.parents(n))
        assert got["best_score"][n] == top


# ---- 3. the caps -------------------------------------------------------------------------------------------------------------
def test_caps():
    p = sp.caps_problem()
    got = nb.mirror("caps", "es3c", "caps", None, 1)
    assert np.array_equal(got["n_capped"], (p.sizes >= 8).astype(np.int32))
    # size 7: 33 additions and 7 removals; 8: the additions are above the cap; 9: the removals give 8 latents; 10: nothing
    want = {7: p.H, 8: 8, 9: 9, 10: 0}
    assert np.array_equal(got["n_states"], [want[s] for s in p.sizes])
    none = p.sizes == 10
    assert (got["M"][none] == -np.inf).all() and (got["best_parent"][none] == -1).all() and (got["best_flip"][none] == -1).all()
    assert (got["best_score"][none] == -np.inf).all() and (got["gap"][none] == 0.0).all()
    assert np.array_equal(got["F_plus"][none], got["F"][none])
    nine = p.sizes == 9  # only removals are present
    assert all(p.ss[n, 0, got["best_flip"][n]] for n in np.flatnonzero(nine))
    count = nb.brute_force(p, 1)[1]
    assert np.array_equal(got["n_states"], count)


# ---- 4. masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", nb.ALGOS)
def test_all_reliable_equals_the_complete_call(algo):
    p = sp.problem(algo, "ragged")
    a = nb.mirror("complete", algo, "ragged", None, 0)
    b = neighbour_bound_host(p.model, p.theta, p.Y, p.ss, p.lpj, p.S_perm, p.S, x_infr=np.ones_like(p.Y, dtype=bool))
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("algo", nb.ALGOS)
def test_masked_entries_are_never_read_and_an_empty_row_is_scored_by_the_prior(algo):
    p = mp.problem(algo, "empty_row", 0.6)
    assert np.isnan(p.Y).any() and not p.x_infr[0].any()
    got = nb.mirror("masked", algo, "empty_row", 0.6, 0)
    for k in ("F", "M", "F_plus", "gap", "mass_outside", "best_score"):
        assert np.isfinite(got[k]).all(), k
    assert (got["n_states"] > 0).all()
    # other values under False, and any y at all for the datapoint without a reliable entry: the same bits
    Y2 = np.where(p.x_infr, p.Y, 1e30)
    Y2[0] = np.linspace(-3.0, 3.0, p.D)
    again = neighbour_bound_host(p.model, p.theta, Y2, p.ss, p.lpj, p.S_perm, p.S, x_infr=p.x_infr)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    if algo == "ebsc":  # the prior alone: a state of k latents scores k pil_bar
        pi = float(p.theta["pi"])
        sizes = np.array([s.sum() for s in nb.neighbour_set(p, 0, 0)])
        want = nb.logsumexp(sizes * np.log(pi / (1.0 - pi)))
        assert abs(got["M"][0] - want) <= RTOL * max(1.0, abs(want)), (got["M"][0], want)


# ---- 5. refusals that need no GPU ----------------------------------------------------------------------------------------------
def test_model_refusals():
    D, H, S = 8, 16, 6
    Y = np.zeros((4, D))
    complete = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    holes = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    holes["x_infr"][0, 0] = False
    plain = {"permanent": {"background": False, "allzero": False, "singletons": False}}
    for cls in (BSC, SSSC):
        model = cls(D, H, S)  # (the engine is made on first use: none of these calls reaches it)
        with pytest.raises(ValueError, match="background"):
            model.neighbourhood_bound({}, {"permanent": {"background": True}}, complete)
        with pytest.raises(ValueError, match="incomplete"):
            model.neighbourhood_bound({}, plain, holes)
        for P in (0, S + 1, -1):
            with pytest.raises(ValueError, match="n_parents"):
                model.neighbourhood_bound({}, plain, complete, n_parents=P)
        assert model._engine is None
    with pytest.raises(NotImplementedError):
        BSC(D, H, S, dtype=np.float32).neighbourhood_bound({}, plain, complete)
    with pytest.raises(ValueError, match="n_parents"):
        neighbour_bound_host("bsc", {"W": np.zeros((D, H)), "pi": 0.1, "sigma": 1.0}, Y, np.zeros((4, S, H), dtype=bool),
                             np.zeros((4, S)), 0, S + 1)


# ---- the margins of the cases the GPU test runs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nb.gpu_cases(), ids=nb.case_id)
def test_committed_cases_leave_a_margin(case):
    got = nb.mirror(*case)
    low = got["margin"] <= nb.DECIDED_TOL
    print("%s: smallest margin %.3g, %d of %d datapoints at or below %g" % (nb.case_id(case), got["margin"].min(), low.sum(),
                                                                              len(low), nb.DECIDED_TOL))
    assert low.mean() <= nb.MAX_UNDECIDED
    assert (got["gap"][np.isfinite(got["gap"])] >= 0.0).all()

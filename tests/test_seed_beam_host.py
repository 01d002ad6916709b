"""The NumPy mirror of the beam-seeding law (evo_amd.variational.seed_states_beam_host) and the refusals of the Python layer.

1. beam = 1 is seed_states_host exactly: states, path, lpj_path;
2. per step q_t distinct states of t latents in descending mirror score, none all-zero, all S distinct;
3. the lpj of every slot against the oracle's lpj, 1e-9 relative (the project's lpj tolerance against the oracle);
4. a hand-made H = 4 case: every two-latent set appears once although two parents reach it;
5. the margin condition of tests/_beam_problems.py, which the GPU comparison relies on;
6. on the correlated dictionary a beam of 4 lifts the mean log sum exp lpj of the seeded states by at least 1 nat;
7. the refusals of the mirror and of Model.seed_resident_states(beam=...).
"""
from itertools import combinations

import numpy as np
import pytest

import _beam_problems as bp
import _seed_problems as sdp
from _sweep_problems import rows_of
from evo_amd.models import BSC, SSSC
from evo_amd.variational import seed_states_beam_host, seed_states_host

LPJ_RTOL = 1e-9
CASE_BEAMS = [(name, B) for name in sorted(bp.CASES) for B in bp.USED[name]]


@pytest.mark.parametrize("name", sorted(sdp.CASES))
@pytest.mark.parametrize("algo", bp.ALGOS)
def test_beam_one_is_the_greedy_mirror(algo, name):
    p = sdp.problem(algo, name)
    states, lpj, path, lpj_path, margin = seed_states_beam_host("bsc" if algo == "ebsc" else "sssc", p.theta, p.Y, p.S, p.A, 1,
                                                                p.S_perm)
    assert states.dtype == np.bool_ and path.dtype == np.int32 and lpj.shape == (p.N, p.S) and margin.shape == (p.N,)
    assert np.array_equal(states, p.states)
    assert np.array_equal(path, p.path)
    assert np.array_equal(lpj_path, p.lpj_path)
    slots = np.concatenate(([0], np.cumsum(sdp.quotas(p.S, p.A))[:-1]))
    assert np.array_equal(lpj[:, slots], p.lpj_path)
    assert (margin <= p.margin).all()  # it looks at every gap the greedy margin looks at, and more


@pytest.mark.parametrize("name,beam", CASE_BEAMS)
@pytest.mark.parametrize("algo", bp.ALGOS)
def test_steps_hold_distinct_ranked_states(algo, name, beam):
    p = bp.problem(algo, name, beam)
    sizes = np.repeat(np.arange(1, p.A + 1), bp.quotas(p.S, p.A))
    assert p.states.any(axis=2).all()  # never the all-zero state
    for n in range(p.N):
        assert len({r.tobytes() for r in p.states[n]}) == p.S
        assert np.array_equal(p.states[n].sum(axis=1), sizes)
        slot = 0
        for t, q in enumerate(bp.quotas(p.S, p.A), start=1):
            assert (np.diff(p.lpj[n, slot:slot + q]) <= 0).all(), (n, t)
            assert p.lpj_path[n, t - 1] == p.lpj[n, slot]
            slot += q
        # the path is the last step's best state, in the order its ancestry added the latents
        last = p.S - bp.quotas(p.S, p.A)[-1]
        assert len(set(p.path[n].tolist())) == p.A and p.states[n, last, p.path[n]].all()


@pytest.mark.parametrize("name,beam", [(n, B) for n, B in CASE_BEAMS if n != "large_h2" or B == 2])
@pytest.mark.parametrize("algo", bp.ALGOS)
def test_slot_lpj_is_the_oracles(algo, name, beam):
    p = bp.problem(algo, name, beam)
    want = rows_of(algo, p.theta, p.Y, p.states, 0)
    err = np.abs(p.lpj - want) / np.maximum(1.0, np.abs(want))
    print("%s %s beam %d: largest relative difference to the oracle %.3g" % (algo, name, beam, err.max()))
    assert err.max() <= LPJ_RTOL


@pytest.mark.parametrize("algo", bp.ALGOS)
def test_two_parents_reach_a_set_once(algo):
    """H = 4 with W = I, S = 7, A = 2 (quotas 4, 3), beam 3: datapoint n is made of the two latents of pair n, so both of
    its singletons are in the beam and both reach the pair -- which must fill one slot of step 2, not two."""
    H = D = 4
    rng = np.random.RandomState(4)
    theta = sdp.make_theta(rng, algo, D, H)
    theta["W"] = np.eye(D)
    pairs = list(combinations(range(H), 2))
    Y = np.tile([0.11, 0.07, 0.05, 0.02], (len(pairs), 1))
    for n, (a, b) in enumerate(pairs):
        Y[n, a], Y[n, b] = 1.3, 1.1
    states, lpj, path, lpj_path, margin = seed_states_beam_host("bsc" if algo == "ebsc" else "sssc", theta, Y, 7, 2, 3)
    assert margin.min() > 1e-6
    for n, pair in enumerate(pairs):
        singles = [frozenset(np.flatnonzero(s)) for s in states[n, :4]]
        assert set(singles) == {frozenset([h]) for h in range(H)}
        assert set(singles[:2]) == {frozenset([h]) for h in pair}  # both parents of the pair are beam members
        got = [frozenset(np.flatnonzero(s)) for s in states[n, 4:]]
        assert all(len(g) == 2 for g in got) and len(set(got)) == 3
        assert got.count(frozenset(pair)) == 1 and got[0] == frozenset(pair)
        assert set(path[n].tolist()) == set(pair)


@pytest.mark.parametrize("name,beam", CASE_BEAMS)
@pytest.mark.parametrize("algo", bp.ALGOS)
def test_committed_cases_are_decided(algo, name, beam):
    m = bp.problem(algo, name, beam).margin.min()
    print("%s %s beam %d: smallest margin %.3g" % (algo, name, beam, m))
    assert m >= bp.MARGIN_MIN


@pytest.mark.parametrize("algo", bp.ALGOS)
def test_beam_lifts_the_correlated_problem(algo):
    one, four = bp.problem(algo, "correlated", 1), bp.problem(algo, "correlated", 4)
    a, b = bp.mean_log_sum(one.lpj), bp.mean_log_sum(four.lpj)
    print("%s correlated: mean log sum exp lpj %.3f (beam 1), %.3f (beam 4), gain %.3f nats" % (algo, a, b, b - a))
    assert b - a >= 1.0
    # and no datapoint's best state is worse
    assert (four.lpj.max(axis=1) >= one.lpj.max(axis=1) - 1e-9 * np.abs(one.lpj.max(axis=1))).all()


def test_refusals_of_the_mirror():
    rng = np.random.RandomState(0)
    th = sdp.make_theta(rng, "ebsc", 4, 80)
    Y = rng.normal(size=(2, 4))
    for B in (0, -1):
        with pytest.raises(ValueError, match="beam = %d" % B):
            seed_states_beam_host("bsc", th, Y, 40, 4, B)
    with pytest.raises(ValueError, match="beam = 11"):  # > S // A = 10
        seed_states_beam_host("bsc", th, Y, 40, 4, 11)
    with pytest.raises(ValueError, match="beam = 17"):  # > 16
        seed_states_beam_host("bsc", th, Y, 80, 4, 17)
    seed_states_beam_host("bsc", th, Y[:1], 40, 4, 10)  # the bounds themselves are admitted
    seed_states_beam_host("bsc", th, Y[:1], 64, 4, 16)
    with pytest.raises(ValueError, match="max_active = 0"):  # the greedy law's refusals come first
        seed_states_beam_host("bsc", th, Y, 40, 0, 1)
    assert np.array_equal(seed_states_beam_host("bsc", th, Y, 40, 4, 1)[0], seed_states_host("bsc", th, Y, 40, 4)[0])


@pytest.mark.parametrize("cls", [BSC, SSSC])
def test_refusals_of_the_model_method(cls):
    """Refused before the device is touched (no engine exists on this host)."""
    D, H, S = 4, 8, 20
    rng = np.random.RandomState(1)
    Y = rng.normal(size=(5, D))
    model = cls(D, H, S)
    theta = sdp.make_theta(rng, "ebsc" if cls is BSC else "es3c", D, H)
    ea = ("fit", "randflip", 4, 1, 1)
    full = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    holes = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    holes["x_infr"][0, 0] = False
    with pytest.raises(ValueError, match="beam"):
        model.seed_resident_states(theta, holes, *ea, max_active=3, beam=2)
    with pytest.raises(ValueError, match="beam"):
        model.seed_resident_states(theta, holes, *ea, max_active=3, beam=2, incomplete=True)
    with pytest.raises(ValueError, match="beam"):
        model.seed_resident_states(theta, full, *ea, max_active=3, beam=2, incomplete=True)
    with pytest.raises(ValueError, match="beam = 0"):
        model.seed_resident_states(theta, full, *ea, max_active=3, beam=0)
    with pytest.raises(ValueError, match="beam = 7"):  # > S // A = 6
        model.seed_resident_states(theta, full, *ea, max_active=3, beam=7)
    with pytest.raises(ValueError, match="background"):
        model.seed_resident_states(theta, full, *ea, max_active=3, beam=2,
                                   permanent={"background": True, "allzero": False, "singletons": False})
    with pytest.raises(ValueError, match="quota q_1 = 10"):
        model.seed_resident_states(theta, full, *ea, max_active=2, beam=2)
    assert model._engine is None
    if cls is BSC:
        with pytest.raises(NotImplementedError, match="float32"):
            BSC(D, H, S, dtype=np.float32).seed_resident_states(theta, full, *ea, max_active=3, beam=2)

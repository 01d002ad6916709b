"""K^n resized, on the CPU: the properties of the NumPy mirror (evo_amd.variational.resize_states_host; csrc/kernels_resize.hpp
has the law) on every problem of tests/_resize_problems.py, the documented order on the hand-made rows, and the refusals of
the mirror and of Model.resize_states that need no device."""
import itertools

import numpy as np
import pytest

import _resize_problems as rp
from evo_amd.models import BSC, SSSC
from evo_amd.variational import check_resize, init_states, resize_states_host

SHRINKS, GROWS = rp.shrinks(), rp.grows()  # (from the table of sizes: collecting this module builds no problem)


def _enumeration(Hv):
    return [(a,) for a in range(Hv)] + list(itertools.combinations(range(Hv), 2))


@pytest.mark.parametrize("name,S_new", SHRINKS)
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_shrink_keeps_the_top_states_in_ascending_slot(algo, name, S_new):
    p = rp.problem(algo, name)
    states, src = rp.mirror(algo, name, S_new)
    assert states.shape == (p.N, S_new, p.H) and src.shape == (p.N, S_new) and src.dtype == np.int32
    for n in range(p.N):
        order = rp.seed_key_order(p.lpj[n, p.S_perm:])
        assert set(src[n]) == set(order[:S_new])
        assert (np.diff(src[n]) > 0).all()
        assert np.array_equal(states[n], p.ss[n, src[n]])


@pytest.mark.parametrize("name,S_new", GROWS)
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_grow_fills_next_to_the_best_state(algo, name, S_new):
    p = rp.problem(algo, name)
    states, src = rp.mirror(algo, name, S_new)
    Hv = p.H - (1 if p.background else 0)
    assert states.shape == (p.N, S_new, p.H)
    for n in range(p.N):
        assert np.array_equal(states[n, :p.S], p.ss[n]) and np.array_equal(src[n, :p.S], np.arange(p.S))
        assert (src[n, p.S:] == -1).all()
        assert len({s.tobytes() for s in states[n]}) == S_new
        fills = states[n, p.S:]
        assert fills[:, :Hv].any(axis=1).all()
        if p.background:
            assert fills[:, -1].all()
        best = p.ss[n, rp.seed_key_order(p.lpj[n, p.S_perm:])[0]]
        dist = (fills ^ best).sum(axis=1)
        assert ((dist == 1) | (dist == 2)).all()
        # enumeration order: one flip in ascending latent, then two flips in ascending (a, b)
        d = fills ^ best
        code = [(0, np.flatnonzero(r)[0], 0) if r.sum() == 1 else (1,) + tuple(np.flatnonzero(r)) for r in d]
        assert code == sorted(code) and not d[:, Hv:].any()
        # distance 2 only after every unheld one-flip neighbour is used
        if (dist == 2).any():
            held = {s.tobytes() for s in p.ss[n]}
            unheld_one = 0
            for h in range(Hv):
                f = best.copy()
                f[h] ^= True
                unheld_one += f[:Hv].any() and f.tobytes() not in held
            assert (dist == 1).sum() == unheld_one


@pytest.mark.parametrize("algo", rp.ALGOS)
def test_tight_by_brute_force(algo):
    """H = 8, S = 20 -> 35: the bound is met exactly.  Every candidate in enumeration order is recomputed here: skipped (empty
    or held) or used, and the used ones are the fills, in that order."""
    p = rp.problem(algo, "tight")
    states, _ = rp.mirror(algo, "tight", 35)
    assert p.H * (p.H + 1) // 2 - 1 == 35
    for n in range(p.N):
        best = p.ss[n, rp.seed_key_order(p.lpj[n])[0]]
        want = []
        for e in _enumeration(p.H):
            f = best.copy()
            f[list(e)] ^= True
            if f.any() and not (p.ss[n] == f).all(axis=1).any():
                want.append(f)
        assert len(want) >= 35 - p.S
        assert np.array_equal(states[n, p.S:], np.array(want[:35 - p.S]))
    # one state: the best one
    states, src = rp.mirror(algo, "tight", 1)
    for n in range(p.N):
        assert src[n, 0] == rp.seed_key_order(p.lpj[n])[0]


@pytest.mark.parametrize("algo", rp.ALGOS)
def test_handmade_rows_give_the_documented_order(algo):
    p = rp.problem(algo, "handmade")
    H = p.H
    sh, src = rp.mirror(algo, "handmade", 5)
    gr, _ = rp.mirror(algo, "handmade", 30)
    # ties at the 5th rank: -1, -2, -3 in slots 10, 1, 6, then -4 in slots 3, 4, 7, 9 -- the two lowest of them
    assert list(src[rp.HANDMADE["tie"]]) == [1, 3, 4, 6, 10]
    # 0.0 and -0.0 tie (slots 7 and 8), then -1 (slot 3), then the finite -11, -14 .. ; NaN and the infinities rank last
    n = rp.HANDMADE["specials"]
    assert list(src[n]) == [1, 3, 4, 7, 8]
    assert list(rp.seed_key_order(p.lpj[n])[:2]) == [7, 8] and list(rp.seed_key_order(p.lpj[n])[-3:]) == [0, 2, 5]
    # ten of twelve: the nine finite ones and, of the three that rank as -inf, the lowest slot (0, the +inf)
    assert list(resize_states_host(p.ss[n:n + 1], p.lpj[n:n + 1], 0, 10)[1][0]) == [0, 1, 3, 4, 6, 7, 8, 9, 10, 11]
    # nothing finite: slots 0 .. 4 are kept, and the fills are neighbours of slot 0
    n = rp.HANDMADE["all_neginf"]
    assert list(src[n]) == [0, 1, 2, 3, 4]
    assert ((gr[n, p.S:] ^ p.ss[n, 0]).sum(axis=1) <= 2).all()
    # a singleton best state {h}: flipping h is skipped, so no fill is empty and the first fill flips the first other latent
    n = rp.HANDMADE["singleton_best"]
    best = p.ss[n, 4]
    assert best.sum() == 1 and gr[n, p.S:].any(axis=1).all()
    h = int(np.flatnonzero(best)[0])
    assert gr[n, p.S:, h].all() and (gr[n, p.S:].sum(axis=1) == 2).all()  # (18 fills: all one flip away, none flips h)
    # a pair best state {a, b}: the two-flip candidate {a, b} is the empty state
    n = rp.HANDMADE["pair_best"]
    big, _ = rp.mirror(algo, "handmade", 100)  # far enough into the pairs to pass {a, b}
    dist = (big[n, p.S:] ^ p.ss[n, 7]).sum(axis=1)
    assert p.ss[n, 7].sum() == 2 and big[n, p.S:].any(axis=1).all() and (dist == 2).any()
    a, b = np.flatnonzero(p.ss[n, 7])
    assert (a, b) == (0, 3)  # candidate H + 2: within the 88 fills
    # the all-zero state held as an ordinary row and best: the fills are the singletons the datapoint does not hold
    n = rp.HANDMADE["allzero_best"]
    assert not p.ss[n, 6].any() and (gr[n, p.S:].sum(axis=1) == 1).all()
    held = {int(np.flatnonzero(s)[0]) for s in p.ss[n] if s.sum() == 1}
    want = [h for h in range(H) if h not in held][:30 - p.S]
    assert [int(np.flatnonzero(s)[0]) for s in gr[n, p.S:]] == want


def test_background_unit_stays_on():
    p = rp.problem("ebsc", "background")
    states, _ = rp.mirror("ebsc", "background", 20)
    assert states[:, :, -1].all()
    # datapoint 0: the best state is {17, unit}; the candidate that flips 17 leaves the unit alone and is skipped
    fills = states[0, p.S:]
    assert fills[:, :-1].any(axis=1).all() and (fills[:, 17] | (fills[:, :-1].sum(axis=1) == 2)).all()


def test_permanent_column_is_no_slot():
    """S_perm = 1: column 0 of the rows never ranks, whatever its value."""
    p = rp.problem("ebsc", "ragged_perm")
    lpj = p.lpj.copy()
    lpj[:, 0] = 1e300
    a = resize_states_host(p.ss, lpj, 1, 5)
    b = rp.mirror("ebsc", "ragged_perm", 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_mirror_refusals():
    p = rp.problem("ebsc", "tight")
    for S_new, match in ((p.S, "nothing to resize"), (0, "must be positive"), (-3, "must be positive"),
                         (rp.TIGHT_REFUSED, "fewer than S_new = 36"), (1025, "at most 1024")):
        with pytest.raises(ValueError, match=match):
            resize_states_host(p.ss, p.lpj, 0, S_new)
    with pytest.raises(ValueError, match="fewer than S_new = 36"):  # the unit is no varying latent: Hv = 8 at H = 9
        check_resize(20, 36, 9, background=True)
    assert check_resize(20, 35, 8) == 35 and check_resize(20, 44, 9) == 44


@pytest.mark.parametrize("cls", [BSC, SSSC])
def test_model_refusals_need_no_device(cls):
    p = rp.problem("ebsc", "tight")
    model = cls(p.D, p.H, p.S, rng="device", sync_host=True, seed=3)
    suff = init_states(p.N, p.S, p.H, "fit", "randflip", 2, 1, 1)
    data = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    for S_new, match in ((p.S, "nothing to resize"), (0, "must be positive"), (rp.TIGHT_REFUSED, "fewer than S_new = 36"),
                         (1025, "at most 1024")):
        with pytest.raises(ValueError, match=match):
            model.resize_states({}, suff, data, S_new)
    assert model._engine is None  # nothing touched a device
    f32 = BSC(p.D, p.H, p.S, rng="device", sync_host=True, seed=3, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="float32"):
        f32.resize_states({}, suff, data, 5)
    assert f32._engine is None

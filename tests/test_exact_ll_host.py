"""CPU tests of the exact log-likelihood's NumPy mirrors (evo_amd/models/exact.py) and of the host-side guards of
Model.exact_log_likelihood: the index -> state map covers every state exactly once, and the running max / rescale
recursion over chunks reproduces the oracle's exact likelihood.

Tolerances.  L: rtol 1e-11, test_full_free_energy's -- the sums have at most 2^13 positive terms, so n * eps is about
2e-12 on z.  Marginals against softmax(lpj) @ states: rtol 1e-10."""
import numpy as np
import pytest

from _exact_problems import NoEngine, fold_in_chunks, make_theta, problem
from evo_amd.models import BSC, SSSC, enumerate_chunk, fold_exact
from evo_amd.models.exact import chunk_bounds
from oracle import evo_oracle as orc


@pytest.mark.parametrize("background", [False, True])
@pytest.mark.parametrize("Hv", [3, 6, 7, 9])
def test_chunks_cover_every_state_once(Hv, background):
    H = Hv + (1 if background else 0)
    bounds = chunk_bounds(H, background, 64)
    assert len(bounds) == max(1, 2 ** Hv // 64)
    for g0, cnt in bounds:  # aligned windows of the index space; without background index 0 is left out
        assert g0 // 64 == (g0 + cnt - 1) // 64
    states = np.concatenate([enumerate_chunk(g0, cnt, H, background) for g0, cnt in bounds], axis=0)
    assert states.dtype == np.bool_ and states.shape == (2 ** Hv - (0 if background else 1), H)
    codes = states[:, :Hv] @ (1 << np.arange(Hv))
    want = np.arange(0 if background else 1, 2 ** Hv)  # latent h on iff bit h of the index
    assert np.array_equal(codes, want)
    if background:
        assert states[:, -1].all()
    else:
        assert states.any(axis=1).all()
    assert np.unique(states, axis=0).shape[0] == states.shape[0]


def _oracle_L(p):
    Hv = p.H - (1 if p.background else 0)
    suff = {"sm": orc.all_states_matrix(Hv),
            "permanent": {"background": p.background, "allzero": False, "singletons": False}}
    theta = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in p.theta.items()}
    fn = orc.bsc_free_energy_full if p.algo == "ebsc" else orc.sssc_free_energy_full
    return fn(theta, suff, np.array(p.Y))


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
@pytest.mark.parametrize("H,D,N,background", [(7, 6, 5, False), (7, 6, 5, True), (13, 8, 6, False)])
def test_fold_matches_oracle_full_free_energy(algo, H, D, N, background):
    p = problem(algo, H, D, N, background)
    want_L = _oracle_L(p)
    for C in (64, 1024):
        ll, marg = fold_in_chunks(p, C)
        np.testing.assert_allclose(p.ljc + ll.sum() / N, want_L, rtol=1e-11)
        np.testing.assert_allclose(ll, p.ll, rtol=1e-11)
        np.testing.assert_allclose(marg, p.marg, rtol=1e-10)
        if background:
            assert (marg[:, -1] == 1.0).all()
    np.testing.assert_allclose(p.L, want_L, rtol=1e-11)
    # the running maximum moves in a late chunk for some rows and never after the first for others
    if not background:
        late = p.lpj.argmax(axis=1) + 1 >= 64  # (column j holds index j + 1)
        assert late.any() and not late.all()


def test_fold_without_states_and_from_minus_infinity():
    rng = np.random.RandomState(3)
    lpj = rng.normal(size=(4, 200)) * 30 - 500
    ll, marg = fold_exact([lpj[:, :64], lpj[:, 64:128], lpj[:, 128:]])
    assert marg is None and np.isfinite(ll).all()
    mx = lpj.max(axis=1)
    np.testing.assert_allclose(ll, np.log(np.exp(lpj - mx[:, None]).sum(axis=1)) + mx, rtol=1e-13)


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_guards_raise_before_any_engine_work(algo):
    D, H = 4, 14
    model = (BSC if algo == "ebsc" else SSSC)(D, H, 4, engine=NoEngine())
    theta = make_theta(np.random.RandomState(0), algo, D, H)
    Y = np.zeros((3, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    suff = {"permanent": {"background": False, "allzero": False, "singletons": False}, "S_perm": 0, "sm": None}
    with pytest.raises(ValueError, match=r"16384 states.*max_H"):
        model.exact_log_likelihood(my_data, theta, suff, max_H=13)
    with pytest.raises(ValueError, match="max_H"):
        model.exact_log_likelihood(my_data, theta, suff, max_H=33)
    suff["permanent"]["background"] = True  # 13 latents vary: the guard passes and the engine is reached
    with pytest.raises(AssertionError, match="touched the GPU engine"):
        model.exact_log_likelihood(my_data, theta, suff, max_H=13)

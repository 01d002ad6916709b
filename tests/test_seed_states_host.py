"""The NumPy mirror of the K^n seeding law (evo_amd.variational.seed_states_host) and the refusals of the Python layer.

1. both models against brute force with the oracle's bsc_lpj / sssc_lpj on tiny shapes: every winner is the arg-max over all
   one-additions, the path lpj is the oracle's to 1e-9 relative (the project's lpj tolerance against the oracle), the slots
   of a step hold exactly its q_t best in rank order;
2. all S states distinct, sizes by the quotas, never the all-zero state;
3. the -inf rule on an indefinite Psi;
4. every refusal of the Python layer.
"""
import numpy as np
import pytest

from _exact_problems import oracle_lpj
from _seed_problems import ALGOS, CASES, make_data, make_theta, problem, quotas
from evo_amd.models import BSC, SSSC
from evo_amd.variational import seed_states_host
from evo_amd.variational.utils import seed_quotas

LPJ_RTOL = 1e-9


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("shape", [(6, 5, 9, 10, 3), (4, 6, 10, 7, 7), (5, 3, 6, 6, 1)])
def test_mirror_against_brute_force(algo, shape):
    N, D, H, S, A = shape
    rng = np.random.RandomState(7)
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, N)
    states, path, lpj_path, margin = seed_states_host("bsc" if algo == "ebsc" else "sssc", theta, Y, S, A)
    assert states.shape == (N, S, H) and states.dtype == np.bool_
    assert path.shape == (N, A) and path.dtype == np.int32 and lpj_path.shape == (N, A) and margin.shape == (N,)
    assert margin.min() > 1e-7, margin.min()  # else the brute force below may rank differently by rounding alone
    for n in range(N):
        active, slot = np.zeros(H, dtype=bool), 0
        for t, q in enumerate(quotas(S, A), start=1):
            cand = np.flatnonzero(~active)
            adds = np.repeat(active[None], len(cand), axis=0)
            adds[np.arange(len(cand)), cand] = True
            lpj = oracle_lpj(algo, theta, Y[n:n + 1], adds)[0]
            order = np.lexsort((cand, -lpj))
            assert path[n, t - 1] == cand[order[0]], (n, t)
            assert abs(lpj_path[n, t - 1] - lpj[order[0]]) <= LPJ_RTOL * max(1.0, abs(lpj[order[0]])), (n, t)
            assert np.array_equal(states[n, slot:slot + q], adds[order[:q]]), (n, t)
            active[path[n, t - 1]] = True
            slot += q
        assert slot == S


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", ["ragged", "tight", "s200"])
def test_states_distinct_sizes_by_quota(algo, name):
    p = problem(algo, name)
    sizes = np.repeat(np.arange(1, p.A + 1), quotas(p.S, p.A))
    for n in range(p.N):
        assert len({r.tobytes() for r in p.states[n]}) == p.S
        assert np.array_equal(p.states[n].sum(axis=1), sizes)
        # the state of step t holds the path up to t - 1; the winner of step t is its first slot
        slot = 0
        for t, q in enumerate(quotas(p.S, p.A), start=1):
            assert p.states[n, slot:slot + q][:, p.path[n, :t - 1]].all()
            assert p.states[n, slot, p.path[n, t - 1]]
            slot += q
    assert p.states.any(axis=2).all()  # never the all-zero state


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("algo", ALGOS)
def test_committed_cases_are_decided(algo, name):
    """What the GPU comparison relies on: at the committed seeds no decision of the mirror hangs on less than 1e-6."""
    assert problem(algo, name).margin.min() >= 1e-6


def test_indefinite_psi_scores_minus_inf():
    N, D, H = 4, 5, 6
    rng = np.random.RandomState(3)
    theta = make_theta(rng, "es3c", D, H)
    Y, _ = make_data(rng, "es3c", theta, N)
    Psi = np.eye(H)
    Psi[2, 2] = Psi[4, 4] = -50.0  # T = 1 + Psi_jj G_jj / sigma2 < 0 for j = 2, 4: det T is not positive
    theta["Psi"] = Psi
    G = theta["W"].T @ theta["W"]
    assert (1.0 + Psi[[2, 4], [2, 4]] * G[[2, 4], [2, 4]] / theta["sigma2"] < 0).all()
    states, path, lpj_path, margin = seed_states_host("sssc", theta, Y, H, 1)  # q_1 = H: every latent is ranked
    order = states.argmax(axis=2)
    assert np.array_equal(order[:, -2:], np.tile([2, 4], (N, 1)))  # -inf ranks last, ascending j among them
    assert np.isfinite(lpj_path).all() and not np.isin(path, [2, 4]).any()
    assert np.isfinite(margin).all()  # the gaps among the finite scores


def test_refusals_of_the_mirror():
    rng = np.random.RandomState(0)
    th_b, th_s = make_theta(rng, "ebsc", 4, 80), make_theta(rng, "es3c", 4, 80)
    Y = rng.normal(size=(2, 4))
    for A in (0, -1):
        with pytest.raises(ValueError, match="max_active"):
            seed_states_host("bsc", th_b, Y, 10, A)
    with pytest.raises(ValueError, match="max_active = 11"):  # > S
        seed_states_host("bsc", th_b, Y, 10, 11)
    with pytest.raises(ValueError, match="ES3C: at most 8"):
        seed_states_host("sssc", th_s, Y, 40, 9)
    with pytest.raises(ValueError, match="EBSC: at most 64"):
        seed_states_host("bsc", th_b, Y, 80, 65)
    seed_states_host("bsc", th_b, Y[:1], 80, 64)  # the caps themselves are admitted
    seed_states_host("sssc", th_s, Y[:1], 40, 8)
    th8 = make_theta(rng, "ebsc", 4, 8)
    with pytest.raises(ValueError, match="max_active = 9"):  # > Hv
        seed_states_host("bsc", th8, Y, 20, 9)
    with pytest.raises(ValueError, match="quota q_1 = 10"):  # 10 > Hv = 8
        seed_states_host("bsc", th8, Y, 20, 2)
    with pytest.raises(ValueError, match="quota q_3 = 7"):  # quotas 7, 7, 7 and 6 latents left at step 3
        seed_states_host("bsc", th8, Y, 21, 3)
    assert seed_quotas(20, 8, 3, False) == [7, 7, 6]


@pytest.mark.parametrize("cls", [BSC, SSSC])
def test_refusals_of_the_model_method(cls):
    """Refused before the device is touched (no engine exists on this host)."""
    D, H, S = 4, 8, 20
    rng = np.random.RandomState(1)
    Y = rng.normal(size=(5, D))
    model = cls(D, H, S)
    theta = make_theta(rng, "ebsc" if cls is BSC else "es3c", D, H)
    ea = ("fit", "randflip", 4, 1, 1)
    full = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    holes = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    holes["x_infr"][0, 0] = False
    with pytest.raises(ValueError, match="incomplete data"):
        model.seed_resident_states(theta, holes, *ea)
    with pytest.raises(ValueError, match="background"):
        model.seed_resident_states(theta, full, *ea, permanent={"background": True, "allzero": False, "singletons": False})
    with pytest.raises(ValueError, match="quota q_1 = 10"):
        model.seed_resident_states(theta, full, *ea, max_active=2)
    with pytest.raises(ValueError, match="max_active = 9"):
        model.seed_resident_states(theta, full, *ea, max_active=9)
    with pytest.raises(ValueError, match="max_active = 0"):
        model.seed_resident_states(theta, full, *ea, max_active=0)
    assert model._engine is None
    if cls is BSC:
        with pytest.raises(NotImplementedError, match="float32"):
            BSC(D, H, S, dtype=np.float32).seed_resident_states(theta, full, *ea)

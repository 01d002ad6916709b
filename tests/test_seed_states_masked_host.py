"""The NumPy mirror of the K^n seeding law on incomplete data (evo_amd.variational.seed_states_host with ``x_infr``) and the
refusals of Model.seed_resident_states(incomplete=...).

1. an all-True mask is complete data: the same states, path, margin and path lpj as ``x_infr=None``;
2. values of Y under False entries never enter (NaN, 1e30);
3. the path lpj is the oracle's masked lpj of the winner states to 1e-9 relative, no clamp counter fires;
4. every committed problem has a smallest margin above 1e-6 (what the GPU comparison relies on);
5. S distinct states, step t has t latents and holds the path prefix, none is all-zero;
6. a row without a reliable entry is ranked by the prior alone;
7. the refusals of the model method, before an engine exists.
"""
import numpy as np
import pytest

from _exact_problems import oracle_theta
from _seed_masked_problems import ALGOS, CASES, FRACTIONS, ONLY, all_problems, make_mask, problem
from _seed_problems import make_data, make_theta, quotas
from evo_amd.models import BSC, SSSC
from evo_amd.variational import seed_states_host
from oracle import evo_oracle as orc

LPJ_RTOL = 1e-9
SMALL = [(algo, name, f) for algo, name, f in all_problems() if name not in ("large_h", "rows_gmem")]


def _model(algo):
    return "bsc" if algo == "ebsc" else "sssc"


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("shape", [(6, 5, 9, 10, 3, 0), (9, 16, 130, 40, 8, 1)])
def test_all_true_mask_is_complete_data(algo, shape):
    N, D, H, S, A, S_perm = shape
    rng = np.random.RandomState(11)
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, N)
    want = seed_states_host(_model(algo), theta, Y, S, A, S_perm)
    got = seed_states_host(_model(algo), theta, Y, S, A, S_perm, x_infr=np.ones((N, D), dtype=bool))
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and np.array_equal(w, g)


@pytest.mark.parametrize("algo,name,missing", [("ebsc", "ragged", 0.3), ("es3c", "ragged_perm", 0.6), ("es3c", "tight", 0.6),
                                               ("ebsc", "wide_d", 0.6)])
def test_values_under_false_never_enter(algo, name, missing):
    p = problem(algo, name, missing)
    assert np.isnan(p.Y[~p.x_infr]).all() and np.isfinite(p.Y[p.x_infr]).all()
    for fill in (0.0, 1e30):
        Y = np.where(p.x_infr, p.Y, fill)
        got = seed_states_host(_model(algo), p.theta, Y, p.S, p.A, p.S_perm, x_infr=p.x_infr)
        for w, g in zip((p.states, p.path, p.lpj_path, p.margin), got):
            assert np.array_equal(w, g)


@pytest.mark.parametrize("algo,name,missing", SMALL)
def test_path_lpj_is_the_oracles_masked_lpj(algo, name, missing):
    p = problem(algo, name, missing)
    th, counters = oracle_theta(algo, p.theta, p.D, p.H, p.x_infr)
    slots = np.concatenate(([0], np.cumsum(quotas(p.S, p.A))[:-1]))
    worst = 0.0
    for n in range(p.N):
        winners = p.states[n, slots]
        if algo == "ebsc":
            want = orc.bsc_lpj(th, winners, p.Y[n], counters, x_infr=p.x_infr[n])
        else:
            want = orc.sssc_lpj(th, winners, p.Y[n], counters, {}, obs=p.x_infr[n])
        err = np.abs(p.lpj_path[n] - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, err.max())
    print("%s %s %.1f: largest relative difference to the oracle %.3g" % (algo, name, missing, worst))
    assert worst <= LPJ_RTOL
    assert not any(np.any(v) for v in counters.values()), counters


@pytest.mark.parametrize("algo,name,missing", all_problems())
def test_committed_problems_are_decided(algo, name, missing):
    p = problem(algo, name, missing)
    margin = p.margin
    if name == "empty_row" and algo == "ebsc":
        assert margin[0] == 0.0  # all scores equal: the tie rule decides, exactly
        margin = margin[1:]
    print("%s %s %.1f: smallest margin %.3g" % (algo, name, missing, margin.min()))
    assert margin.min() > 1e-6
    if name != "empty_row":
        assert p.x_infr.any(axis=1).all()
        assert abs((~p.x_infr).mean() - missing) < 0.2


def test_tight_has_rows_with_one_reliable_entry():
    assert any((problem(algo, "tight", 0.6).x_infr.sum(axis=1) == 1).any() for algo in ALGOS)


@pytest.mark.parametrize("algo,name,missing", SMALL)
def test_structure(algo, name, missing):
    p = problem(algo, name, missing)
    q = quotas(p.S, p.A)
    sizes = np.repeat(np.arange(1, p.A + 1), q)
    for n in range(p.N):
        assert len({r.tobytes() for r in p.states[n]}) == p.S
        assert np.array_equal(p.states[n].sum(axis=1), sizes)
        slot = 0
        for t, qt in enumerate(q, start=1):
            assert p.states[n, slot:slot + qt][:, p.path[n, :t - 1]].all()
            assert p.states[n, slot, p.path[n, t - 1]]
            slot += qt
    assert p.states.any(axis=2).all()


@pytest.mark.parametrize("missing", FRACTIONS)
def test_row_without_reliable_entry(missing):
    # EBSC: every score of a step is the same number -- ascending j
    p = problem("ebsc", "empty_row", missing)
    assert not p.x_infr[0].any() and p.x_infr[1].sum() == 1
    assert np.array_equal(p.path[0], np.arange(p.A))
    slot = 0
    for t, qt in enumerate(quotas(p.S, p.A), start=1):
        want = np.zeros((qt, p.H), dtype=bool)
        want[:, :t - 1] = True
        want[np.arange(qt), t - 1 + np.arange(qt)] = True  # the q_t lowest free j
        assert np.array_equal(p.states[0, slot:slot + qt], want)
        slot += qt
    pil = np.log(p.theta["pi"] / (1.0 - p.theta["pi"]))
    assert np.allclose(p.lpj_path[0], pil * np.arange(1, p.A + 1), rtol=1e-12)
    # ES3C: pil_bar alone decides
    p = problem("es3c", "empty_row", missing)
    pil = np.log(p.theta["pies"] / (1.0 - p.theta["pies"]))
    order = np.lexsort((np.arange(p.H), -pil))
    assert np.array_equal(p.path[0], order[:p.A])
    assert np.allclose(p.lpj_path[0], np.cumsum(pil[order[:p.A]]), rtol=1e-12)
    slot = 0
    for t, qt in enumerate(quotas(p.S, p.A), start=1):
        free = [j for j in order if j not in p.path[0, :t - 1]]
        for r in range(qt):
            want = np.zeros(p.H, dtype=bool)
            want[p.path[0, :t - 1]] = True
            want[free[r]] = True
            assert np.array_equal(p.states[0, slot + r], want)
        slot += qt


@pytest.mark.parametrize("cls", [BSC, SSSC])
def test_refusals_of_the_model_method(cls):
    """Refused before the device is touched (no engine exists on this host)."""
    D, H, S = 4, 8, 20
    rng = np.random.RandomState(1)
    Y = rng.normal(size=(5, D))
    model = cls(D, H, S)
    theta = make_theta(rng, "ebsc" if cls is BSC else "es3c", D, H)
    ea = ("fit", "randflip", 4, 1, 1)
    holes = {"y": Y, "x_infr": make_mask(rng, 5, D, 0.4)}
    assert not holes["x_infr"].all()
    with pytest.raises(ValueError, match="incomplete data") as e:
        model.seed_resident_states(theta, holes, *ea)
    assert "incomplete=True" in str(e.value)
    with pytest.raises(ValueError, match="incomplete data"):
        model.seed_resident_states(theta, holes, *ea, incomplete=False)
    with pytest.raises(ValueError, match="background"):
        model.seed_resident_states(theta, holes, *ea, incomplete=True,
                                   permanent={"background": True, "allzero": False, "singletons": False})
    with pytest.raises(ValueError, match="quota q_1 = 10"):
        model.seed_resident_states(theta, holes, *ea, max_active=2, incomplete=True)
    with pytest.raises(ValueError, match="max_active = 9"):
        model.seed_resident_states(theta, holes, *ea, max_active=9, incomplete=True)
    with pytest.raises(ValueError, match="max_active = 0"):
        model.seed_resident_states(theta, holes, *ea, max_active=0, incomplete=True)
    assert model._engine is None
    if cls is BSC:
        m32 = BSC(D, H, S, dtype=np.float32)
        with pytest.raises(NotImplementedError, match="float32"):
            m32.seed_resident_states(theta, holes, *ea, incomplete=True)
        assert m32._engine is None


def test_only_table_names_cases():
    assert set(ONLY) <= set(CASES)

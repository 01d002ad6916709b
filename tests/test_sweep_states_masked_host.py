"""evo_amd.variational.sweep_states_host with ``x_infr``, the NumPy mirror of one sweep's proposals of the local search on
K^n from incomplete data (csrc/kernels_sweep.hpp).  CPU only.

1. every emitted score is the oracle's masked lpj of that state, 1e-9 relative (the tolerance of
   tests/test_sweep_states_host.py);
2. an all-True mask is complete data: the same rows, counts, best_flip and n_capped as ``x_infr=None``, scores and gains to
   1e-12 relative;
3. entries of Y under False never matter: NaN or 0.0 there, the same bits;
4. every committed problem has a smallest margin above 1e-6 (what the GPU comparison relies on);
5. the refusals of Model.sweep_resident_states, before an engine exists.
"""
import numpy as np
import pytest

import _sweep_masked_problems as mp
import _sweep_problems as sp
from _seed_masked_problems import make_mask
from _seed_problems import make_theta
from evo_amd.models import BSC, SSSC
from evo_amd.variational import sweep_states_host

RTOL = 1e-9
OUTPUTS = ("cand", "counts", "scores", "best_flip", "gain", "n_capped", "margin")


@pytest.mark.parametrize("algo,name,missing", mp.all_problems())
def test_scores_are_the_oracle_masked_lpj_of_the_proposed_states(algo, name, missing):
    p = mp.problem(algo, name, missing)
    assert np.isnan(p.Y[~p.x_infr]).all() and np.isfinite(p.Y[p.x_infr]).all()
    oth = mp.oracle_theta(algo, p.theta, p.D, p.H, p.x_infr)
    worst = 0.0
    for n in range(p.N):
        c = p.counts[n]
        assert np.isnan(p.scores[n, c:]).all() and not p.cand[n, c:].any()
        if c == 0:
            continue
        want = mp.oracle_lpj(algo, oth, p.Y[n], p.cand[n, :c], p.x_infr[n])
        err = np.abs(p.scores[n, :c] - want) / np.maximum(1.0, np.abs(want))
        worst = max(worst, err.max())
    print("%s %s %.1f: worst relative error of the scores %.3g" % (algo, name, missing, worst))
    assert worst <= RTOL


def test_caps_scores_are_the_oracle_masked_lpj():
    p = mp.caps_problem()
    oth = mp.oracle_theta("es3c", p.theta, p.D, p.H, p.x_infr)
    assert np.array_equal(p.n_capped, (p.sizes >= 8).astype(np.int32))
    assert np.isnan(p.gain[p.sizes == 9]).all() and (p.gain[p.sizes == 10] == -np.inf).all()
    assert (p.counts[p.sizes == 10] == 0).all() and (p.counts[p.sizes < 10] == p.q).all()
    for n in range(p.N):
        c = p.counts[n]
        if c:
            want = mp.oracle_lpj("es3c", oth, p.Y[n], p.cand[n, :c], p.x_infr[n])
            assert (np.abs(p.scores[n, :c] - want) <= RTOL * np.maximum(1.0, np.abs(want))).all()


@pytest.mark.parametrize("algo,name", [(algo, name) for algo in sp.ALGOS for name in ("ragged_perm", "s200", "tight")])
def test_all_true_mask_is_complete_data(algo, name):
    p = sp.problem(algo, name)
    got = sweep_states_host(p.model, p.theta, p.Y, p.ss, p.lpj, p.S_perm, p.P, p.q, x_infr=np.ones((p.N, p.D), dtype=bool))
    g = dict(zip(OUTPUTS, got))
    for k in ("cand", "counts", "best_flip", "n_capped"):
        assert g[k].dtype == getattr(p, k).dtype and np.array_equal(g[k], getattr(p, k)), k
    for k in ("scores", "gain"):
        want = getattr(p, k)
        fin = np.isfinite(want)
        assert np.array_equal(g[k][~fin], want[~fin], equal_nan=True), k
        assert (np.abs(g[k][fin] - want[fin]) <= 1e-12 * np.maximum(1.0, np.abs(want[fin]))).all(), k


@pytest.mark.parametrize("algo,name,missing", [("ebsc", "ragged", 0.3), ("es3c", "ragged_perm", 0.6), ("es3c", "tight", 0.6),
                                               ("ebsc", "wide_d", 0.6), ("es3c", "empty_row", 0.3)])
def test_values_under_false_never_enter(algo, name, missing):
    p = mp.problem(algo, name, missing)
    Y0 = np.where(p.x_infr, p.Y, 0.0)
    assert np.isnan(p.Y).any() and np.isfinite(Y0).all()
    got = sweep_states_host(p.model, p.theta, Y0, p.ss, p.lpj, p.S_perm, p.P, p.q, x_infr=p.x_infr)
    for k, g in zip(OUTPUTS, got):
        assert np.array_equal(g, getattr(p, k), equal_nan=True), k


@pytest.mark.parametrize("algo,name,missing", mp.all_problems())
def test_committed_problems_are_decided(algo, name, missing):
    p = mp.problem(algo, name, missing)
    margin = p.margin
    if name == "empty_row":
        assert not p.x_infr[0].any() and p.x_infr[1].sum() == 1
        if algo == "ebsc":
            assert margin[0] == 0.0  # every addition has the same score: the tie rule decides, exactly
            margin = margin[1:]
    print("%s %s %.1f: smallest margin %.3g" % (algo, name, missing, margin.min()))
    assert margin.min() > 1e-6
    if name != "empty_row":
        assert p.x_infr.any(axis=1).all()
        assert abs((~p.x_infr).mean() - missing) < 0.2


def test_row_without_reliable_entry_is_scored_by_the_prior():
    # EBSC: the additions of a parent all score base + pil_bar -- ascending j among the latents K^n does not hold
    p = mp.problem("ebsc", "empty_row", 0.3)
    par = p.ss[0, np.lexsort((np.arange(p.S), -p.lpj[0]))[0]]
    flips = np.argmax(p.cand[0, :p.q] != par, axis=1)
    assert (np.diff(flips) > 0).all() and not par[flips].any()
    pil = np.log(p.theta["pi"] / (1.0 - p.theta["pi"]))
    assert np.allclose(p.scores[0, :p.q], (par.sum() + 1) * pil, rtol=1e-12)
    # ES3C: the sum of pil_bar over the state
    p = mp.problem("es3c", "empty_row", 0.3)
    pil = np.log(p.theta["pies"] / (1.0 - p.theta["pies"]))
    c = p.counts[0]
    assert c > 0 and np.allclose(p.scores[0, :c], p.cand[0, :c] @ pil, rtol=1e-12)


def test_tight_has_short_lists_singleton_parents_and_rows_with_one_reliable_entry():
    assert any((mp.problem(algo, "tight", 0.6).x_infr.sum(axis=1) == 1).any() for algo in mp.ALGOS)
    for algo in mp.ALGOS:
        p = mp.problem(algo, "tight", 0.6)
        assert (p.counts < p.P * p.q).all() and (p.counts > 0).any()
        sizes = [p.ss[n, s].sum() for n in range(p.N) for s in np.lexsort((np.arange(p.S), -p.lpj[n]))[:p.P]]
        assert sizes.count(1) > 0


@pytest.mark.parametrize("cls", [BSC, SSSC])
def test_refusals_of_the_model_method(cls):
    """Refused before the device is touched (no engine exists on this host)."""
    D, H, S = 4, 8, 20
    rng = np.random.RandomState(1)
    model = cls(D, H, S)
    theta = make_theta(rng, "ebsc" if cls is BSC else "es3c", D, H)
    holes = {"y": rng.normal(size=(5, D)), "x_infr": make_mask(rng, 5, D, 0.4)}
    assert not holes["x_infr"].all()
    plain = {"permanent": {"background": False, "allzero": False, "singletons": False}}
    with pytest.raises(ValueError, match="incomplete data") as e:
        model.sweep_resident_states(theta, plain, holes)
    assert "incomplete=True" in str(e.value)
    with pytest.raises(ValueError, match="background"):
        model.sweep_resident_states(theta, {"permanent": dict(plain["permanent"], background=True)}, holes, incomplete=True)
    with pytest.raises(ValueError, match="n_sweeps"):
        model.sweep_resident_states(theta, plain, holes, n_sweeps=0, incomplete=True)
    assert model._engine is None
    if cls is BSC:
        m32 = BSC(D, H, S, dtype=np.float32)
        with pytest.raises(NotImplementedError, match="float32"):
            m32.sweep_resident_states(theta, plain, holes, incomplete=True)
        assert m32._engine is None

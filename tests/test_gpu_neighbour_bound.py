"""The neighbourhood bound on the GPU (Engine.neighbour_bound / Model.neighbourhood_bound, csrc/kernels_nbound.hpp) against its
NumPy mirror (evo_amd.variational.neighbour_bound_host) and the brute-force set of tests/test_neighbour_bound_host.py.

1. against the mirror on the GPU's own rows; 2. at H = 10 against the set; 3. two calls, the same bits; 4. the call writes
nothing; 5. refusals leave the context usable; 6. the Model level.
"""
import numpy as np
import pytest

import _nbound_problems as nb
import _sweep_problems as sp
from _seed_problems import make_data, make_theta
from evo_amd import _lib
from evo_amd.engine import Engine, EvoAmdError
from evo_amd.models import BSC, SSSC
from evo_amd.variational import seed_states_host

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ALLZERO = {"background": False, "allzero": True, "singletons": False}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model_eng():
    e = Engine(0)
    yield e
    e.close()


def _set_theta(eng, model, th):
    if model == "sssc":
        eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    else:
        eng.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))


def _install(eng, p, Cmax=None):
    """Data (NaN under the mask's False entries), the masks when the problem has them, Theta, K^n."""
    x_infr = getattr(p, "x_infr", None)
    eng.configure(p.model, p.N, p.D, p.H, p.S, p.S_perm, p.Cmax if Cmax is None else Cmax)
    eng.upload_data(p.Y)
    if x_infr is not None:
        eng.upload_masks(x_infr)
        eng.set_reliable_fraction(x_infr.sum() / float(p.N))  # (enters ljc alone, which no score holds)
    _set_theta(eng, p.model, p.theta)
    eng.upload_states(p.ss)


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# ---- 1. against the mirror on the GPU's own rows -----------------------------------------------------------------------------
def _check_against_mirror(eng, p, P, best=True):
    masked = getattr(p, "x_infr", None) is not None
    _install(eng, p)
    got = eng.neighbour_bound(P or p.S, incomplete=masked)
    rows = eng.download_lpj()
    err = np.abs(rows - p.lpj) / np.maximum(1.0, np.abs(p.lpj))
    print("%s: rows against the oracle %.3g" % (p.algo, err.max()))
    assert err.max() <= RTOL
    want = nb.mirror_on(p, P, lpj=rows)  # the choice of the parents is exact
    if not best:
        want["margin"][:] = 0.0
    undecided = nb.compare(p, got, want, RTOL)
    print("%s: %d of %d datapoints undecided, smallest margin %.3g, states %d .. %d, mean gap %.4g nats" % (
        p.algo, len(undecided), p.N, want["margin"].min(), got["n_states"].min(), got["n_states"].max(), got["gap"].mean()))
    if best:
        assert len(undecided) <= nb.MAX_UNDECIDED * p.N
    assert (got["gap"] >= 0.0).all() and ((got["mass_outside"] >= 0.0) & (got["mass_outside"] <= 1.0)).all()
    ok = np.isfinite(got["F_plus"])
    assert got["count"] == ok.sum() and abs(got["sum"] - got["F_plus"][ok].sum()) <= RTOL * max(1.0, abs(got["sum"]))
    return got


@pytest.mark.parametrize("case", nb.gpu_cases(), ids=nb.case_id)
def test_bound_equals_the_mirror(eng, case):
    kind, algo, name, missing, P = case
    p = nb.problem_of(kind, algo, name, missing)
    got = _check_against_mirror(eng, p, P)
    if kind == "caps":
        assert np.array_equal(got["n_capped"], (p.sizes >= 8).astype(np.int32))
        assert np.array_equal(got["n_states"], [{7: p.H, 8: 8, 9: 9, 10: 0}[s] for s in p.sizes])
        none = p.sizes == 10
        assert (got["M"][none] == -np.inf).all() and (got["best_flip"][none] == -1).all() and (got["best_parent"][none] == -1).all()


def test_a_row_without_a_reliable_entry_is_scored_by_the_prior(eng):
    kind, algo, name, missing, P = nb.EMPTY_ROW
    p = nb.problem_of(kind, algo, name, missing)
    got = _check_against_mirror(eng, p, P, best=False)  # (exact ties by construction: see _nbound_problems.py)
    want = nb.mirror_on(p, P, lpj=eng.download_lpj())
    n = 0  # equal scores are equal keys on the device as well: the law's tie rule decides, ascending rank, then latent
    assert (got["best_parent"][n], got["best_flip"][n]) == (want["best_parent"][n], want["best_flip"][n])


# ---- 2. at H = 10 against the brute-force set -------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 0])
@pytest.mark.parametrize("algo", nb.ALGOS)
def test_kernel_counts_each_state_of_the_set_once(eng, algo, P):
    p = nb.problem_of("small", algo, None)
    _install(eng, p)
    got = eng.neighbour_bound(P or p.S)
    rows = eng.download_lpj()
    want, count = nb.brute_force(p, P, lpj=rows)
    assert np.array_equal(got["n_states"], count)
    err = np.abs(got["F_plus"] - want) / np.maximum(1.0, np.abs(want))
    print("%s P = %s: worst relative error of F+ against the set %.3g" % (algo, P or "S", err.max()))
    assert err.max() <= RTOL


@pytest.mark.parametrize("algo", nb.ALGOS)
def test_kernel_applies_the_ownership_rule(eng, algo):
    p = nb.two_apart(algo)
    _install(eng, p)
    got = eng.neighbour_bound(p.S)
    want, count = nb.brute_force(p, 0, lpj=eng.download_lpj())
    S, H = p.S, p.H
    assert (count == 1 + S + S * (S - 1) // 2 + S * (H - 1 - S)).all()
    assert np.array_equal(got["n_states"], count)
    assert (np.abs(got["F_plus"] - want) <= RTOL * np.maximum(1.0, np.abs(want))).all()


# ---- 3. / 4. two calls give the same bits; the call writes nothing -----------------------------------------------------------------
@pytest.mark.parametrize("case", [("complete", "ebsc", "s200", None, 0), ("complete", "es3c", "ragged_perm", None, 0),
                                  ("masked", "ebsc", "wide_d", 0.3, 0), ("masked", "es3c", "rows_gmem", 0.6, 0)], ids=nb.case_id)
def test_deterministic_and_write_free(eng, eng2, case):
    kind, algo, name, missing, P = case
    p = nb.problem_of(kind, algo, name, missing)
    masked = kind == "masked"
    for e in (eng, eng2):  # eng2: the same calls without the bound in between
        _install(e, p)
        e.lpj_resident()
        e.evolve_randflip(2, 2, 5, True)
    before = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates())
    a = eng.neighbour_bound(P or p.S, incomplete=masked)
    b = eng.neighbour_bound(P or p.S, incomplete=masked)
    assert _same(a, b)
    after = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    # what follows is what it is without the call
    fa, fb = eng.posterior_scores(), eng2.posterior_scores()
    assert _same(fa, fb)
    assert np.array_equal(fa["F"], a["F"])
    ra, rb = eng.sweep_propose(p.P, p.q, incomplete=masked), eng2.sweep_propose(p.P, p.q, incomplete=masked)
    assert _same(ra, rb)
    for x, y in zip(eng.download_candidates(), eng2.download_candidates()):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(eng.download_lpj(), eng2.download_lpj())


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(eng, call, match):
    before = (eng.download_states_packed(), eng.download_lpj(), eng.debug_validity())
    with pytest.raises(EvoAmdError, match=match):
        call()
    after = (eng.download_states_packed(), eng.download_lpj(), eng.debug_validity())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    assert before[2] == after[2], {k: (before[2][k], after[2][k]) for k in before[2] if before[2][k] != after[2][k]}


@pytest.mark.parametrize("algo", nb.ALGOS)
def test_refusals_leave_the_context_usable(eng, algo):
    import ctypes
    p = sp.problem(algo, "ragged")
    _install(eng, p)
    eng.lpj_resident()
    first = eng.neighbour_bound(2)
    _refused(eng, lambda: eng.neighbour_bound(0), "n_parents")
    _refused(eng, lambda: eng.neighbour_bound(p.S + 1), "n_parents")
    out = _lib.NboundOut()
    _refused(eng, lambda: _lib.check(eng.lib.evoamd_neighbour_bound(eng._h, 1, 2, ctypes.byref(out))), "unknown flag")
    eng.set_option("background_unit", 1)
    _refused(eng, lambda: eng.neighbour_bound(1), "background_unit")
    eng.set_option("background_unit", 0)
    eng.upload_masks(np.ones((p.N, p.D), dtype=bool))
    _refused(eng, lambda: eng.neighbour_bound(1), "incomplete data")
    with_masks = eng.neighbour_bound(2, incomplete=True)  # the permission: the masked instantiation, all entries reliable
    eng.upload_masks(None)
    for k in ("n_states", "n_capped", "best_parent", "best_flip"):
        assert np.array_equal(with_masks[k], first[k]), k
    assert (np.abs(with_masks["F_plus"] - first["F_plus"]) <= RTOL * np.maximum(1.0, np.abs(first["F_plus"]))).all()
    assert _same(eng.neighbour_bound(2), first)
    assert _same(eng.neighbour_bound(2, incomplete=True), first)  # without masks the flag changes nothing
    if algo == "ebsc":
        eng.set_option("ebsc_f32", 1)
        try:
            p4 = sp.build("ebsc", 9, 8, 16, 6, 0, 1, 4, 2, 2, 1)  # (the float32 mode asks for H % 4 == 0)
            _install(eng, p4)
            _refused(eng, lambda: eng.neighbour_bound(1), "float32")
        finally:
            eng.set_option("ebsc_f32", 0)
        _install(eng, p)
        assert _same(eng.neighbour_bound(2), first)


def test_refuses_keys_beyond_lds(eng):
    # EBSC keeps 16 bytes per latent: H = 9664 asks for more than a wavefront's share of 150 KiB
    N, D, H = 2, 2, 9664
    eng.configure("bsc", N, D, H, 2, 0, 2)
    eng.upload_data(np.ones((N, D)))
    eng.set_params_bsc(np.ones((D, H)), 0.01, 1.0)
    with pytest.raises(EvoAmdError, match="LDS"):
        eng.neighbour_bound(1)


def test_kernel_class_is_named(eng):
    assert _lib.KERNEL_IDS_EXTRA["neighbour_bound"] == 33
    assert eng.lib.evoamd_kernel_name(33) == b"neighbour_bound"
    p = sp.problem("ebsc", "ragged")
    _install(eng, p)
    eng.timing(("neighbour_bound",))
    eng.timing_reset()
    eng.neighbour_bound(p.S)
    ms, launches = eng.kernel_time_ms("neighbour_bound")
    eng.timing(False)
    assert launches == 1 and ms > 0.0


# ---- 6. the Model level ----------------------------------------------------------------------------------------------------------
def _suff(ss, permanent=None):
    from evo_amd.variational import init_states
    N, S, H = ss.shape
    suff = init_states(0, S, H, "fit", "randflip", 6, 5, 1, permanent=permanent)  # (Cmax = 30: a sweep may keep H = 30 per parent)
    suff["ss"] = ss.copy()
    suff["lpj"] = np.zeros((N, S + suff["S_perm"]))
    return suff


@pytest.mark.parametrize("S_perm", [0, 1])
@pytest.mark.parametrize("sync_host", [True, False])
@pytest.mark.parametrize("algo", nb.ALGOS)
def test_model_level(model_eng, algo, sync_host, S_perm):
    cls = BSC if algo == "ebsc" else SSSC
    N, D, H, S = 29, 8, 30, 12
    rng = np.random.RandomState(61 if algo == "ebsc" else 62)
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, N, k=3)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    ss = seed_states_host(sp.model_name(algo), theta, Y, S, 2, S_perm)[0]
    model = cls(D, H, S, engine=model_eng, rng="reference" if sync_host else "device", sync_host=sync_host, seed=3)
    suff = _suff(ss, permanent=ALLZERO if S_perm else None)
    if not sync_host:
        suff["ss"] = suff["lpj"] = None
        model.attach_resident_states(suff, my_data, [(0, np.packbits(ss, axis=-1))])
    th = dict(theta)
    keys = (set(th), set(suff), set(my_data))
    L, info = model.neighbourhood_bound(th, suff, my_data, per_datapoint=True)
    assert (set(th), set(suff), set(my_data)) == keys, "the call wrote into a dict"
    assert set(info) == {"F", "F_plus", "gap", "mass_outside", "n_states", "n_capped", "best_score", "best_parent", "best_flip",
                         "n_bad_weights"}
    assert info["n_bad_weights"] == 0 and (info["n_capped"] == 0).all() and (info["n_states"] > 0).all()
    for k in ("F", "F_plus", "gap", "mass_outside", "best_score"):
        assert info[k].shape == (N,) and info[k].dtype == np.float64, k
    for k in ("n_states", "n_capped", "best_parent", "best_flip"):
        assert info[k].shape == (N,) and info[k].dtype == np.int32, k
    ljc = model_eng.ljc
    assert abs(L - (ljc + info["F_plus"].mean())) <= RTOL * max(1.0, abs(L))
    assert L >= ljc + info["F"].mean() and (info["gap"] > 0.0).any()
    assert model.neighbourhood_bound(th, suff, my_data) == L
    L1 = model.neighbourhood_bound(th, suff, my_data, n_parents=1)
    assert ljc + info["F"].mean() <= L1 <= L
    assert np.array_equal(model_eng.download_states(), ss)
    if sync_host:
        assert np.array_equal(suff["ss"], ss) and not suff["lpj"].any()
    else:
        assert suff["ss"] is None and suff["lpj"] is None
    # after a quiet sweep with n_keep = Hv the best state has no better one-flip neighbour outside K^n: the gain certificate
    res = model.sweep_resident_states(th, suff, my_data, n_sweeps=60, n_parents=1, n_keep=H, stop_when_quiet=True)
    assert res.stopped_early, res
    _, quiet = model.neighbourhood_bound(th, suff, my_data, n_parents=1, per_datapoint=True)
    top = model_eng.download_lpj().max(axis=1)
    assert (res.gain <= RTOL * np.maximum(1.0, np.abs(top))).all()
    assert (quiet["best_parent"][quiet["n_states"] > 0] == 0).all()
    print("%s: best neighbour of the best state minus the largest lpj of the row: at most %.4g" % (
        algo, (quiet["best_score"] - top).max()))
    assert (quiet["best_score"] - top <= 0.0).all()
    with pytest.raises(ValueError, match="incomplete"):
        bad = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
        bad["x_infr"][0, 0] = False
        model.neighbourhood_bound(th, suff, bad)
    with pytest.raises(ValueError, match="background"):
        model.neighbourhood_bound(th, dict(suff, permanent={"background": True, "allzero": False, "singletons": False}), my_data)


def test_float32_model_refuses(model_eng):
    model = BSC(8, 16, 6, engine=model_eng, dtype=np.float32)
    with pytest.raises(NotImplementedError):
        model.neighbourhood_bound({}, {"permanent": {"background": False}}, {})

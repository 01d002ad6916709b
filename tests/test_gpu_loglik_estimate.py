"""Model.estimate_log_likelihood on the GPU (csrc/kernels_loglik_estimate.hpp) against its NumPy mirror
(evo_amd.models.estimate_log_likelihood_counter, lpj of the draws from the oracle).

The draws, inside / outside and n_outside must match bit for bit; ll, F, log_r, lpj, mass_outside and ess to 1e-9 (the
project's tolerance for F and lpj), scaled by the largest reference entry where values are large (sketch_close).

1. both models at H = 10 (a partial word), 64 (a full word), 70 (two words), S_perm = 1 and 0, the background unit;
   T = 40 in passes of 12 draws (three full passes and a partial one), T = 5 (less than a pass);
2. incomplete data; ES3C dense draws through the general level; a concentrated posterior;
3. the comparison against the exact answer on the device;
4. F against posterior_scores, the same bits twice, prefix and shards;
5. the EM state is not disturbed;
6. argument errors.
"""
import ctypes

import numpy as np
import pytest

from _exact_problems import my_data_of, oracle_theta, problem
from _loglik_estimate_problems import exact_case, exact_conditions, kn_case, mirror_of
from conftest import sketch_close
from evo_amd._lib import EvoAmdError, check
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import init_states

pytestmark = pytest.mark.gpu

ALGOS = ["ebsc", "es3c"]
BSC_KEYS = ("W", "pi", "sigma")
SSSC_KEYS = ("W", "pies", "mus", "Psi", "sigma2")
REAL = ("ll", "F", "gap", "mass_outside", "ess", "log_r", "lpj")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _copy(d):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _suff(N, S, H, S_perm, background, states, lpj):
    """my_suff_stat whose candidate capacity is 4 parents x 3 children = 12: a pass holds 12 draws."""
    np.random.seed(0)
    perm = {"background": background, "allzero": bool(S_perm), "singletons": False}
    suff = init_states(N, S, H, "fit", "randflip", 4, 3, 1, permanent=perm)
    assert suff["S_perm"] == S_perm and suff["ss"].shape == states.shape and suff["lpj"].shape == lpj.shape
    suff["ss"], suff["lpj"] = np.array(states), np.array(lpj)
    return suff


def _inputs(eng, c, **kw):
    model = (BSC if c.algo == "ebsc" else SSSC)(c.D, c.H, c.S, engine=eng, **kw)
    if c.x_infr is None:
        my_data = {"y": np.array(c.Y), "x_infr": np.ones_like(c.Y, dtype=bool)}
    else:
        my_data = {"y": np.array(c.Y), "x_infr": c.x_infr.copy(), "x": c.x_infr.copy()}
    return model, my_data, _copy(c.theta), _suff(c.N, c.S, c.H, c.S_perm, c.background, c.states, c.lpj)


def _compare(info, ref, what):
    for k in ("s", "inside", "n_outside"):
        assert info[k].dtype == ref[k].dtype and np.array_equal(info[k], ref[k]), (what, k)
    assert (info["n_bad_weights"], info["n_skipped"]) == (ref["n_bad_weights"], ref["n_skipped"]), what
    for k in REAL:
        assert np.array_equal(np.isnan(info[k]), np.isnan(ref[k])), (what, k)
        ok = ~np.isnan(ref[k])
        print("%s %s: max |diff| %.3g (scale %.3g)" % (what, k, np.abs(info[k][ok] - ref[k][ok]).max(initial=0.0),
                                                        np.abs(ref[k][ok]).max(initial=0.0)))
        sketch_close(info[k][ok], ref[k][ok], 1e-9, "%s %s" % (what, k))
    assert (info["ll"] >= info["F"]).all(), what
    none = info["n_outside"] == 0
    assert (info["gap"][none] == 0).all() and (info["mass_outside"][none] == 0).all(), what


def _run_case(eng, key, T, seed, lam, L_check=True):
    c = kn_case(*key)
    model, my_data, theta, suff = _inputs(eng, c)
    snaps = (_copy(theta), _copy(suff), _copy(my_data))
    L, info = model.estimate_log_likelihood(theta, suff, my_data, n_samples=T, seed=seed, prior_mix=lam,
                                            per_datapoint=True, keep_draws=True)
    assert model.last_estimate_seed == seed
    for d, snap in zip((theta, suff, my_data), snaps):  # the three dicts stay as they were
        assert list(d.keys()) == list(snap.keys())
        for k, v in snap.items():
            assert np.array_equal(d[k], v, equal_nan=True) if isinstance(v, np.ndarray) else (d[k] is v or d[k] == v), k
    ref = mirror_of(key, T, seed, lam)
    what = "%s H=%d S_perm=%d bg=%d T=%d" % (c.algo, c.H, c.S_perm, c.background, T)
    _compare(info, ref, what)
    if L_check:
        ljc = oracle_theta(c.algo, c.theta, c.D, c.H, c.x_infr)[0]["ljc"]
        np.testing.assert_allclose(L, ljc + ref["sum"] / c.N, rtol=1e-9)
    return c, info, ref


# ---- 1. against the mirror ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("H", [10, 64, 70])
@pytest.mark.parametrize("S_perm", [1, 0])
def test_matches_mirror(eng, algo, H, S_perm):
    # (S_perm = 0 at H = 64 / 70: pi lowered to 0.02 so that all-zero draws occur)
    key = (algo, H, S_perm) if S_perm == 1 or H == 10 else (algo, H, 0, False, 0.0, 37, 12, 9, 0.02)
    c, info, ref = _run_case(eng, key, 40, 9, 0.25)
    if S_perm == 0:  # all-zero draws that are outside K^n: they take the all-zero lpj
        zero = ~info["s"].any(axis=2)
        print("%s H=%d: %d all-zero draws" % (algo, H, zero.sum()))
        assert zero.sum() >= 10 and not info["inside"][zero].any()
    if S_perm == 1:
        zero = ~info["s"].any(axis=2)
        assert info["inside"][zero].all()
    assert info["inside"].any() and not info["inside"].all()


ZERO_ROWS = (10, 0, False, 0.0, 37, 12, 9, 0.05, 0, True)  # kn_case: S_perm = 0, the all-zero row in every second K^n


@pytest.mark.parametrize("algo", ALGOS)
def test_all_zero_state_as_an_ordinary_row(eng, algo):
    """S_perm = 0 and K^n holds the all-zero state among its S rows (what init_states with a small p_init_Kn lays
    out): an all-zero draw is inside there -- its mass is in F_n already -- and outside for the other datapoints."""
    c, info, ref = _run_case(eng, (algo,) + ZERO_ROWS, 40, 9, 0.25)
    has_zero = ~c.states.any(axis=2).all(axis=1)
    zero = ~info["s"].any(axis=2)
    assert zero[has_zero].any() and zero[~has_zero].any()
    assert info["inside"][has_zero][zero[has_zero]].all() and not info["inside"][~has_zero][zero[~has_zero]].any()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("H", [10, 65])
def test_background_unit(eng, algo, H):
    c, info, ref = _run_case(eng, (algo, H, 0, True), 40, 4, 0.25)
    assert info["s"][:, :, -1].all()


@pytest.mark.parametrize("algo", ALGOS)
def test_fewer_draws_than_a_pass(eng, algo):
    _run_case(eng, (algo, 10, 1), 5, 9, 0.25)


# ---- 2. other regimes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("S_perm", [1, 0])
def test_incomplete_data(eng, algo, S_perm):
    c, info, ref = _run_case(eng, (algo, 10, S_perm, False, 0.3), 40, 6, 0.25)
    assert 0.2 < 1.0 - c.x_infr.mean() < 0.4
    if S_perm == 0:  # outside all-zero draws on masked data: the all-zero lpj over the reliable entries
        zero = ~info["s"].any(axis=2)
        assert zero.sum() >= 10 and not info["inside"][zero].any()


def test_es3c_dense_draws(eng):
    """prior_mix = 1 and pi = 0.3 at H = 40: about twelve active latents per draw, the general level with its lists."""
    c, info, ref = _run_case(eng, ("es3c", 40, 1, False, 0.0, 37, 12, 9, 0.3), 40, 8, 1.0)
    k = info["s"].sum(axis=2)
    assert (k > 8).mean() > 0.5 and not info["inside"].any()


@pytest.mark.parametrize("algo", ALGOS)
def test_concentrated_posterior(eng, algo):
    c, info, ref = _run_case(eng, (algo, 10, 1), 40, 2, 0.01)
    none = info["n_outside"] == 0
    assert info["inside"].mean() > 0.5 and none.any() and not none.all()
    assert (info["gap"][none] == 0).all()


# ---- 3. against the exact answer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("nan_frac", [0.0, 0.3])
def test_against_the_exact_answer(eng, algo, nan_frac):
    p, states, lpj = exact_case(algo, nan_frac)
    model = (BSC if algo == "ebsc" else SSSC)(p.D, p.H, 5, engine=eng)
    my_data, theta = my_data_of(p), _copy(p.theta)
    suff = _suff(p.N, 5, p.H, 1, False, states, lpj)
    L, info = model.estimate_log_likelihood(theta, suff, my_data, n_samples=1024, seed=3, prior_mix=0.5, per_datapoint=True)
    assert "s" not in info
    exact_conditions(p, info, "%s nan_frac=%.1f (device)" % (algo, nan_frac))
    scores = model.posterior_scores(theta, suff, my_data)
    np.testing.assert_allclose(info["F"], scores["F"], rtol=1e-12)
    L_exact, ll_exact, _ = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True)
    np.testing.assert_allclose(ll_exact, p.ll, rtol=1e-11)
    assert abs((ll_exact - info["ll"]).mean()) <= 0.1 * (ll_exact - info["F"]).mean()
    np.testing.assert_allclose(L, p.ljc + info["ll"].mean(), rtol=1e-12)
    assert L_exact - 0.1 * (ll_exact - info["F"]).mean() <= L <= L_exact + 0.1 * (ll_exact - info["F"]).mean()


# ---- 4. reproducibility, prefix, shards --------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_same_bits_prefix_and_shards(eng, algo):
    c = kn_case(algo, 70, 1)
    model, my_data, theta, suff = _inputs(eng, c)
    kw = dict(seed=5, prior_mix=0.25, per_datapoint=True, keep_draws=True)
    La, a = model.estimate_log_likelihood(theta, suff, my_data, n_samples=40, first_index=3, **kw)
    Lb, b = model.estimate_log_likelihood(theta, suff, my_data, n_samples=40, first_index=3, **kw)
    assert La == Lb
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    _, short = model.estimate_log_likelihood(theta, suff, my_data, n_samples=10, first_index=3, **kw)
    for k in ("s", "inside", "log_r", "lpj"):
        assert np.array_equal(short[k], a[k][:, :10], equal_nan=True), k
    cut = 15
    parts = []
    for lo, hi in ((0, cut), (cut, c.N)):
        m = (BSC if algo == "ebsc" else SSSC)(c.D, c.H, c.S, engine=eng)
        data = {"y": np.array(c.Y[lo:hi]), "x_infr": np.ones((hi - lo, c.D), dtype=bool)}
        sf = _suff(hi - lo, c.S, c.H, 1, False, c.states[lo:hi], c.lpj[lo:hi])
        parts.append(m.estimate_log_likelihood(theta, sf, data, n_samples=40, first_index=3 + lo, **kw)[1])
    for k in ("s", "inside", "n_outside", "log_r", "lpj", "ll", "F", "ess", "mass_outside"):
        assert np.array_equal(np.concatenate([q[k] for q in parts]), a[k], equal_nan=True), k


# ---- 5. isolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_em_state_is_not_disturbed(eng, algo):
    """step, statistics, [estimate_log_likelihood,] step: the second step gives the same F, counts, Theta and K^n with
    and without the call (the pattern and the tolerances of tests/test_gpu_exact_ll.py).  After the call K^n, the lpj
    rows and the dense posterior rows are the same bits, and a bare vary_kn refuses: no candidate batch is installed."""
    N, D, H, S = 40, 8, 10, 8
    p = problem(algo, H, D, N)
    out = []
    for with_call in (False, True):
        np.random.seed(2)
        model = (BSC if algo == "ebsc" else SSSC)(D, H, S, rng="device", sync_host=False, engine=eng, seed=4,
                                                   device_mstep=True)
        my_data = my_data_of(p)
        suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1)
        theta = model.check_params(model.standard_init(my_data))
        _, _, _, theta = model.step(theta, suff, my_data)
        theta = dict(theta.copy())
        eng.stats()
        rows = eng.download_posterior()
        if with_call:
            kn, lpj = eng.download_states_packed(), eng.download_lpj()
            total, n_ok, info = eng.loglik_estimate(16, seed=1)
            assert n_ok == N and np.isfinite(total) and (info["n_outside"] > 0).any()
            after = eng.download_posterior()
            for r0, r1 in zip(rows, after):
                assert (r0 is None and r1 is None) or np.array_equal(r0, r1)
            L, info = model.estimate_log_likelihood(theta, suff, my_data, n_samples=16, seed=1, per_datapoint=True)
            assert np.isfinite(L) and np.isfinite(info["ll"]).all() and (info["ll"] >= info["F"]).all()
            assert np.array_equal(eng.download_states_packed(), kn) and np.array_equal(eng.download_lpj(), lpj)
            with pytest.raises(EvoAmdError, match="no resident candidate batch"):
                eng.vary_kn(S)
            assert np.array_equal(eng.download_states_packed(), kn)
        F, nu, nsub, theta2 = model.step(theta, suff, my_data)
        theta2 = dict(theta2.copy())
        resets = tuple(suff[k] for k in ("reset_lpj_isnan", "reset_lpj_smaller_eps_lpj", "reset_lpj_isinf"))
        out.append((F, (nu, nsub) + resets, None, theta2, eng.download_states_packed()))
    (F0, nu0, ns0, th0, kn0), (F1, nu1, ns1, th1, kn1) = out
    print("%s: F %.17g / %.17g, counts and reset counters %s / %s" % (algo, F0, F1, nu0, nu1))
    assert np.array_equal(kn0, kn1) and (nu0, ns0) == (nu1, ns1)
    np.testing.assert_allclose(F1, F0, rtol=1e-12)
    for k in (BSC_KEYS if algo == "ebsc" else SSSC_KEYS):
        np.testing.assert_allclose(th1[k], th0[k], rtol=1e-9, atol=1e-12, err_msg=k)


# ---- 6. argument errors (last: they configure the engine directly) ----------------------------------------------------
def test_argument_errors(eng):
    c = kn_case("ebsc", 10, 1)
    model, my_data, theta, suff = _inputs(eng, c)
    for kw in ({"n_samples": 0}, {"prior_mix": 0.0}, {"prior_mix": 1.5}):
        with pytest.raises(ValueError):
            model.estimate_log_likelihood(theta, suff, my_data, **kw)
    m32 = BSC(c.D, 12, c.S, engine=eng, dtype=np.float32)
    with pytest.raises(EvoAmdError, match="float32"):
        m32.estimate_log_likelihood(theta, suff, my_data)
    L = model.estimate_log_likelihood(theta, suff, my_data, n_samples=8, seed=1)
    assert isinstance(L, float) and np.isfinite(L)
    for T, lam in ((0, 0.25), (4, 0.0), (4, 1.5)):  # the library's own checks, behind the Python ones
        cnt, tot = (ctypes.c_int64 * 2)(), ctypes.c_double()
        with pytest.raises(EvoAmdError, match="n_samples|prior_mix"):
            check(eng.lib.evoamd_loglik_estimate(eng._h, T, 0, 0, lam, 0, None, None, None, None, None, cnt, ctypes.byref(tot)))
    with pytest.raises(EvoAmdError, match="bytes of device memory"):  # refused before any launch
        eng.loglik_estimate(2 ** 31 - 1, keep_draws=True)
    total, n_ok, info = eng.loglik_estimate(8, seed=1)  # the refused calls left everything usable
    np.testing.assert_allclose(theta_ljc(model, theta, suff, my_data) + total / n_ok, L, rtol=1e-12)
    # a row with bad weights: NaN outputs, counted, left out of the sum
    lpj = np.array(c.lpj)
    lpj[2, 3] = np.nan
    eng.upload_lpj(lpj)
    total2, n_ok2, info2 = eng.loglik_estimate(8, seed=1)
    assert n_ok2 == c.N - 1 and info2["n_bad_weights"] == 1 and np.isnan(info2["ll"][2]) and np.isnan(info2["F"][2])
    ok = np.arange(c.N) != 2
    assert np.array_equal(info2["ll"][ok], info["ll"][ok])
    np.testing.assert_allclose(total2, info["ll"][ok].sum(), rtol=1e-12)
    rng = np.random.RandomState(0)
    eng.set_option("ebsc_f32", 0)
    eng.f32 = False
    eng.configure("bsc", 4, 3, 1088, 2, 0, 1)  # 17 words: above the 16 latents per lane of the proposal kernel
    eng.upload_data(rng.normal(size=(4, 3)))
    eng.set_params_bsc(rng.normal(size=(3, 1088)), 0.1, 1.0)
    with pytest.raises(EvoAmdError, match="at most 1024 latents"):
        eng.loglik_estimate(4)
    eng.configure("bsc", 4, 3, 8, 1024, 1, 1)  # S_perm + 2 S = 2049: one more than the LDS slices hold
    eng.upload_data(rng.normal(size=(4, 3)))
    eng.set_params_bsc(rng.normal(size=(3, 8)), 0.1, 1.0)
    with pytest.raises(EvoAmdError, match=r"S_perm \+ 2 S = 2049, at most 2048"):
        eng.loglik_estimate(4)


def theta_ljc(model, theta, suff, my_data):
    th = dict(theta)
    model.E_step_precompute(th, dict(suff), my_data)
    return th["ljc"]

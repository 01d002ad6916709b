"""The NumPy mirror of Model.estimate_log_likelihood (evo_amd/models/loglik_estimate.py) on the CPU:

1. r is a distribution (enumerated with proposal_of), with and without the background unit;
2. the draws follow r; fewer draws are a prefix; shards concatenate;
3. ll >= F, with equality exactly where no draw is outside K^n;
4. against the exact answer of tests/_exact_problems.py: the remaining gap is at most a tenth of the bound's, and
   mean_n(Z^_n / Z_n) - 1 lies within four standard errors of zero.

Seeds are fixed; the conditions of 4 are the issue's and were met by the mirror alone with these seeds before the GPU
test relied on them."""
import itertools

import numpy as np
import pytest

from _exact_problems import problem
from _loglik_estimate_problems import exact_case, exact_conditions, kn_case, table_lpj_fn
from evo_amd.models import estimate_log_likelihood_counter, proposal_of

ALGOS = ["ebsc", "es3c"]


def _name(algo):
    return "bsc" if algo == "ebsc" else "sssc"


def _all_states(Hv):
    return np.array(list(itertools.product((False, True), repeat=Hv)), dtype=bool)


def _log_r(rho, s):
    return np.where(s, np.log(rho), np.log1p(-rho)).sum(axis=1)


def _run(c, **kw):
    return estimate_log_likelihood_counter(_name(c.algo), c.theta, c.states, c.lpj, c.lpj_fn, S_perm=c.S_perm,
                                           background=c.background, x_infr=c.x_infr, **kw)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("background", [False, True])
def test_r_is_a_distribution(algo, background):
    c = kn_case(algo, 8, 0 if background else 1, background, N=5, S=6)
    Hv = 8 - (1 if background else 0)
    table = _all_states(Hv)
    for n in range(c.N):
        rho = proposal_of(c.theta, c.states[n], c.lpj[n], S_perm=c.S_perm, background=background, prior_mix=0.25)
        assert rho.shape == (Hv,) and (rho > 0).all() and (rho < 1).all()
        np.testing.assert_allclose(np.exp(_log_r(rho, table)).sum(), 1.0, rtol=0, atol=1e-12)
    bad = np.array(c.lpj[0])
    bad[1] = np.nan
    assert proposal_of(c.theta, c.states[0], bad, S_perm=c.S_perm, background=background) is None


@pytest.mark.parametrize("algo", ALGOS)
def test_draws_follow_r(algo):
    T = 20000
    c = kn_case(algo, 4, 1, N=3, D=6, S=3)
    res = _run(c, n_samples=T, seed=11, prior_mix=0.25)
    table = _all_states(4)
    weights = 1 << np.arange(4)
    for n in range(c.N):
        rho = proposal_of(c.theta, c.states[n], c.lpj[n], S_perm=1, prior_mix=0.25)
        r = np.exp(_log_r(rho, table))
        freq = np.bincount(res["s"][n] @ weights, minlength=16) / T
        se = np.sqrt(r * (1 - r) / T)
        dev = np.abs(freq - r[np.argsort(table @ weights)]) / se[np.argsort(table @ weights)]
        print("%s n=%d: largest deviation %.2f standard errors" % (algo, n, dev.max()))
        assert (dev <= 5.0).all(), (n, dev)
        np.testing.assert_allclose(res["log_r"][n], _log_r(rho, res["s"][n]), rtol=1e-13)


@pytest.mark.parametrize("algo", ALGOS)
def test_prefix_and_shards(algo):
    c = kn_case(algo, 10, 1)
    long = _run(c, n_samples=40, seed=5, prior_mix=0.25, first_index=3)
    short = _run(c, n_samples=10, seed=5, prior_mix=0.25, first_index=3)
    assert np.array_equal(short["s"], long["s"][:, :10]) and np.array_equal(short["inside"], long["inside"][:, :10])
    np.testing.assert_array_equal(short["log_r"], long["log_r"][:, :10])
    cut = 15
    parts = []
    for lo, hi in ((0, cut), (cut, c.N)):
        fn = (lambda lo: lambda n, st: c.lpj_fn(lo + n, st))(lo)
        parts.append(estimate_log_likelihood_counter(_name(algo), c.theta, c.states[lo:hi], c.lpj[lo:hi], fn, S_perm=1,
                                                     n_samples=40, seed=5, prior_mix=0.25, first_index=3 + lo))
    for k in ("s", "inside", "n_outside", "ll", "F", "ess", "mass_outside", "log_r", "lpj"):
        assert np.array_equal(np.concatenate([q[k] for q in parts]), long[k], equal_nan=True), k


@pytest.mark.parametrize("algo", ALGOS)
def test_ll_is_at_least_F(algo):
    c = kn_case(algo, 10, 1)
    res = _run(c, n_samples=40, seed=2, prior_mix=0.01)  # a concentrated proposal: some datapoints draw only inside
    none = res["n_outside"] == 0
    print("%s: %d of %d datapoints without an outside draw" % (algo, none.sum(), c.N))
    assert none.any() and not none.all()
    assert (res["ll"] >= res["F"]).all() and (res["gap"] >= 0).all()
    # (an outside draw whose term lies more than 36 nats below F_n adds less than one ulp: its gap rounds to 0)
    assert (res["gap"][none] == 0).all() and (res["gap"][~none & (res["mass_outside"] > 1e-15)] > 0).all()
    assert (res["gap"][~none] > 0).sum() > (~none).sum() // 2
    assert (res["mass_outside"][none] == 0).all() and (res["ess"][none] == 0).all()
    assert np.array_equal(res["n_outside"], (~res["inside"]).sum(axis=1))
    assert np.isnan(res["lpj"][res["inside"]]).all() and np.isfinite(res["lpj"][~res["inside"]]).all()
    # K^n holds all 2^Hv states (H = 3: S = 7 plus the permanent all-zero state): every draw is inside
    p = problem(algo, 3, 6, 5)
    states = np.tile(p.states[None], (p.N, 1, 1))
    lpj = np.concatenate((p.zero[:, None], p.lpj), axis=1)
    full = estimate_log_likelihood_counter(_name(algo), p.theta, states, lpj, table_lpj_fn(p), S_perm=1, n_samples=50,
                                           seed=1, prior_mix=0.5)
    assert full["inside"].all() and (full["n_outside"] == 0).all() and (full["gap"] == 0).all()
    np.testing.assert_allclose(full["ll"], p.ll, rtol=1e-12)
    # a flat posterior whose K^n lacks the best state: every datapoint has outside draws and every gap is positive
    p, states, lpj = exact_case(algo)
    flat = estimate_log_likelihood_counter(_name(algo), p.theta, states, lpj, table_lpj_fn(p), S_perm=1, n_samples=64,
                                           seed=3, prior_mix=0.5)
    assert (flat["n_outside"] > 0).all() and (flat["gap"] > 0).all() and (flat["ess"] >= 1).all()


ZERO_ROWS = (10, 0, False, 0.0, 37, 12, 9, 0.05, 0, True)  # kn_case: S_perm = 0, pi = 0.05, the all-zero row in every second K^n


@pytest.mark.parametrize("algo", ALGOS)
def test_all_zero_state_as_an_ordinary_row(algo):
    """S_perm = 0: an all-zero draw is inside exactly where K^n holds the all-zero state among its S rows; elsewhere it
    is outside and takes the all-zero lpj."""
    c = kn_case(algo, *ZERO_ROWS)
    has_zero = ~c.states.any(axis=2).all(axis=1)
    assert has_zero[0::2].all() and not has_zero[1::2].any()
    res = _run(c, n_samples=40, seed=9, prior_mix=0.25)
    zero = ~res["s"].any(axis=2)
    assert zero[has_zero].any() and zero[~has_zero].any()
    assert res["inside"][has_zero][zero[has_zero]].all() and not res["inside"][~has_zero][zero[~has_zero]].any()
    for n in np.flatnonzero(~has_zero):
        assert (res["lpj"][n][zero[n]] == c.lpj_fn(n, np.zeros((1, c.H), dtype=bool))[0]).all()
    assert np.array_equal(res["n_outside"], (~res["inside"]).sum(axis=1))


def test_argument_errors_and_bad_rows():
    c = kn_case("ebsc", 10, 1)
    for kw in ({"n_samples": 0}, {"prior_mix": 0.0}, {"prior_mix": 1.5}):
        with pytest.raises(ValueError):
            _run(c, **dict({"n_samples": 4, "seed": 0, "prior_mix": 0.25}, **kw))
    lpj = np.array(c.lpj)
    lpj[2, 3] = np.nan
    lpj[4, :] = -np.inf
    x_infr = np.ones((c.N, c.D), dtype=bool)
    x_infr[6] = False
    res = estimate_log_likelihood_counter("bsc", c.theta, c.states, lpj, c.lpj_fn, S_perm=1, n_samples=8, seed=0,
                                          x_infr=x_infr)
    assert res["n_bad_weights"] == 2 and res["n_skipped"] == 1
    for n in (2, 4, 6):
        assert np.isnan(res["ll"][n]) and np.isnan(res["F"][n]) and res["n_outside"][n] == 0 and not res["s"][n].any()
    ok = np.setdiff1d(np.arange(c.N), (2, 4, 6))
    assert np.isfinite(res["ll"][ok]).all() and res["sum"] == pytest.approx(res["ll"][ok].sum(), rel=1e-14)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("nan_frac", [0.0, 0.3])
def test_against_the_exact_answer(algo, nan_frac):
    p, states, lpj = exact_case(algo, nan_frac)
    res = estimate_log_likelihood_counter(_name(algo), p.theta, states, lpj, table_lpj_fn(p), S_perm=1, n_samples=1024,
                                          seed=3, prior_mix=0.5, x_infr=p.x_infr)
    exact_conditions(p, res, "%s nan_frac=%.1f" % (algo, nan_frac))

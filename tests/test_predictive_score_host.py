"""evo_amd.models.predictive_log_score_host, the NumPy mirror of Model.predictive_log_score, and pit_summary (CPU only).

1. the mirror against an independent brute-force evaluation of the formulas on dense arrays (explicit inverses, sums in
   the linear domain, math.erf): logp rtol 1e-9 where the linear-domain density is above 1e-250, pit atol 1e-12;
2. for a few entries exp(logp) integrated over a grid of y is 1 and its running integral is pit (the grid and its
   quadrature tolerance are derived in the test);
3. with S = 1 logp is the normal log density at the mean and var of predictive_moments_host;
4. calibration under the exact posterior: states from the prior, data from the model, 30 % of the entries hidden, K^n =
   all 2^H states with the oracle's masked lpj: the KS distance of the PIT to the uniform distribution stays below the
   0.1 % critical value 1.95 / sqrt(k);
5. refusals of bad arguments; pit_summary on known arrays.
"""
import math

import numpy as np
import pytest

from _exact_problems import make_data, make_theta, oracle_lpj, oracle_zero
from _predictive_problems import algo_name, problem
from _predictive_score_problems import N_NOT_QUERIED, brute_entry, brute_terms, score_problem
from evo_amd._lib import EvoAmdError
from evo_amd.models import enumerate_chunk, pit_summary, predictive_log_score_host, predictive_moments_host
from evo_amd.models.exact import index_range

# (algo, N, D, H, incomplete, S_perm, background), noise
HOST_CASES = [
    (("es3c", 30, 25, 10, False, 1, False), True),
    (("es3c", 30, 25, 10, True, 0, True), True),
    (("es3c", 37, 64, 70, True, 0, False), False),
    (("es3c", 30, 25, 10, False, 1, False), False),  # (the all-zero state is a point mass)
    (("ebsc", 37, 25, 70, False, 1, False), True),
    (("ebsc", 30, 70, 10, True, 0, False), True),
]


@pytest.mark.parametrize("case,noise", HOST_CASES)
def test_mirror_equals_brute_force(case, noise):
    q = score_problem(*case, noise=noise)
    p, info = q.p, q.info
    logp, pit = info["logp"], info["pit"]
    scored = q.query & np.isfinite(np.where(q.query, q.y_true, 0.0))
    visited = scored.any(axis=1) & p.x_infr.any(axis=1)
    assert np.array_equal(np.isnan(logp), ~(scored & visited[:, None])) and np.array_equal(np.isnan(pit), np.isnan(logp))
    assert info["n_singular"] == 0 and info["n_skipped"] == (1 if p.incomplete else 0)
    assert info["n_not_queried"] == int((~scored.any(axis=1)).sum()) >= 1 and not scored[N_NOT_QUERIED].any()
    assert info["n_bad_values"] == q.n_bad >= 4
    assert np.array_equal(info["count"], np.where(visited, scored.sum(axis=1), 0))
    if p.incomplete:
        assert q.query[5].all() and info["count"][5] == 0 and info["logp_n"][5] == 0.0  # all D queried, no reliable entry
    worst_l = worst_p = 0.0
    n_compared = 0
    for n in np.flatnonzero(visited):
        w, m, tau = brute_terms(p, n, noise)
        for d in np.flatnonzero(scored[n]):
            dens, cdf = brute_entry(w, m[:, d], tau[:, d], q.y_true[n, d])
            assert abs(pit[n, d] - cdf) <= 1e-12, (n, d)
            worst_p = max(worst_p, abs(pit[n, d] - cdf))
            if dens > 1e-250:
                worst_l = max(worst_l, abs(logp[n, d] - math.log(dens)) / max(1.0, abs(logp[n, d])))
                n_compared += 1
            else:
                assert logp[n, d] < math.log(1e-250) + 1.0
    print("%r noise=%s: %d entries, worst |logp - log dens| / max(1, |logp|) = %.3g, worst |pit - cdf| = %.3g"
          % (case, noise, n_compared, worst_l, worst_p))
    assert n_compared > 0.5 * scored[visited].sum() and worst_l <= 1e-9
    ok = ~np.isnan(logp)
    assert np.isfinite(logp[ok]).all() and ((pit[ok] >= 0) & (pit[ok] <= 1)).all()
    np.testing.assert_allclose(info["logp_n"], np.where(ok, logp, 0.0).sum(axis=1), rtol=1e-12, atol=1e-12)
    assert q.score == pytest.approx(logp[ok].sum() / ok.sum(), rel=1e-12)


@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_density_integrates_to_one_and_to_pit(algo):
    """One datapoint repeated over a grid of y at one entry.  The grid runs from min_s m_s - 10 sd_max to max_s m_s +
    10 sd_max (the mass outside is below erfc(10 / sqrt 2) = 1.6e-23) with the step h = sd_min / 50.  The trapezoid sum
    over the whole line of a mixture of Gaussians no narrower than 50 h is exact to rounding (its error decays like
    exp(-2 pi^2 50^2)): tolerance 1e-10.  The running sum up to an inner grid point has the Euler-Maclaurin end term
    h^2 / 12 |f'(y)| <= h^2 / 12 * 0.242 / tau_min (the largest slope of a Gaussian density is 1 / (tau sqrt(2 pi e))):
    with h^2 = tau_min / 2500 that is 8.1e-6; the test allows twice that, 1.7e-5."""
    p = problem(algo, 30, 25, 10, False, 1, False)
    for n, d in ((0, 3), (4, 11), (9, 24)):
        w, m, tau = brute_terms(p, n, True)
        sd_min, sd_max = math.sqrt(tau[:, d].min()), math.sqrt(tau[:, d].max())
        h = sd_min / 50.0
        grid = np.arange(m[:, d].min() - 10.0 * sd_max, m[:, d].max() + 10.0 * sd_max + h, h)
        G = grid.size
        y_true = np.full((G, p.D), np.nan)
        y_true[:, d] = grid
        query = np.zeros((G, p.D), dtype=bool)
        query[:, d] = True
        rep = lambda a: np.repeat(a[n:n + 1], G, axis=0)  # noqa: E731
        _, info = predictive_log_score_host(algo_name(algo), p.theta, rep(p.ss), rep(p.lpj), rep(p.Y), y_true, query, None,
                                            p.S_perm, p.background, True)
        f = np.exp(info["logp"][:, d])
        total = h * (f.sum() - 0.5 * (f[0] + f[-1]))
        running = h * (np.cumsum(f) - 0.5 * f - 0.5 * f[0])
        err = np.abs(running - info["pit"][:, d]).max()
        print("%s (n, d) = (%d, %d): %d grid points, integral - 1 = %.3g, max |running integral - pit| = %.3g"
              % (algo, n, d, G, total - 1.0, err))
        assert abs(total - 1.0) <= 1e-10
        assert err <= 1.7e-5
        assert (np.diff(info["pit"][:, d]) >= 0).all()


@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
@pytest.mark.parametrize("incomplete", [False, True])
def test_one_state_is_the_gaussian_of_the_moments(algo, incomplete):
    p = problem(algo, 30, 25, 10, incomplete, 0, False)
    ss, lpj = np.array(p.ss[:, 2:3]), np.array(p.lpj[:, 2:3])
    xi = p.x_infr if incomplete else None
    mean, var, _ = predictive_moments_host(algo_name(algo), p.theta, ss, lpj, p.Y, xi)
    rng = np.random.RandomState(3)
    y_true = np.where(np.isnan(mean), 0.0, mean) + rng.normal(size=mean.shape) * 2.0
    query = np.ones(mean.shape, dtype=bool)
    score, info = predictive_log_score_host(algo_name(algo), p.theta, ss, lpj, p.Y, y_true, query, xi)
    ok = ~np.isnan(mean)
    want = -0.5 * (np.log(2.0 * np.pi * var[ok]) + (y_true[ok] - mean[ok]) ** 2 / var[ok])
    np.testing.assert_allclose(info["logp"][ok], want, rtol=1e-12, atol=1e-12)
    assert np.isnan(info["logp"][~ok]).all() and info["n_skipped"] == (1 if incomplete else 0)
    assert score == pytest.approx(want.mean(), rel=1e-12)


def _gaussian_score(mean, var, y, scored):
    return float((-0.5 * (np.log(2.0 * np.pi * var[scored]) + (y[scored] - mean[scored]) ** 2 / var[scored])).mean())


# seeds for which the mirror satisfies the bound (1.95 / sqrt(k) is the 0.1 % critical value: a calibrated model fails one
# seed in a thousand)
@pytest.mark.parametrize("algo,seed", [("ebsc", 0), ("ebsc", 1), ("es3c", 0), ("es3c", 1)])
def test_pit_is_uniform_under_the_exact_posterior(algo, seed):
    H, D, N = 6, 10, 400
    rng = np.random.RandomState(4000 + seed)
    theta = make_theta(rng, algo, D, H)
    prior = np.full(H, float(theta["pi"])) if algo == "ebsc" else np.asarray(theta["pies"])
    s = rng.random_sample((N, H)) < prior
    Y_full = make_data(rng, algo, theta, s)
    x_infr = rng.random_sample((N, D)) >= 0.3
    x_infr[np.arange(N), rng.randint(D, size=N)] = True  # at least one entry kept per datapoint
    Y = np.where(x_infr, Y_full, np.nan)
    first, end = index_range(H, False)
    states = enumerate_chunk(first, end - first, H, False)  # every state but the all-zero one
    assert states.shape == (2 ** H - 1, H)
    lpj = np.concatenate((oracle_zero(algo, theta, Y, x_infr)[:, None], oracle_lpj(algo, theta, Y, states, x_infr)), axis=1)
    ss = np.broadcast_to(states, (N,) + states.shape)
    score, info = predictive_log_score_host(algo_name(algo), theta, ss, lpj, Y, Y_full, ~x_infr, x_infr, S_perm=1)
    summ = pit_summary(info["pit"])
    k = int((~x_infr).sum())
    assert summ["n"] == k == int(info["count"].sum()) and info["n_not_queried"] == int(x_infr.all(axis=1).sum())
    mean, var, _ = predictive_moments_host(algo_name(algo), theta, ss, lpj, Y, x_infr, S_perm=1)
    print("%s seed %d: k = %d, KS = %.4f (bound %.4f), coverage %r, mean log score: mixture %.4f, moment-matched Gaussian %.4f"
          % (algo, seed, k, summ["ks"], 1.95 / math.sqrt(k), summ["coverage"], score, _gaussian_score(mean, var, Y_full, ~x_infr)))
    assert summ["ks"] <= 1.95 / math.sqrt(k)


def test_bad_arguments_are_refused():
    p = problem("ebsc", 37, 25, 70, False, 1, False)
    y = np.zeros((p.N, p.D))
    qy = np.ones((p.N, p.D), dtype=bool)
    args = ("bsc", p.theta, p.ss, p.lpj, p.Y)
    with pytest.raises(ValueError, match="EBSC without noise"):
        predictive_log_score_host(*args, y, qy, None, 1, False, noise=False)
    with pytest.raises(ValueError, match=r"\(N, D\)"):
        predictive_log_score_host(*args, y[:, :-1], qy, None, 1)
    with pytest.raises(ValueError, match=r"\(N, D\)"):
        predictive_log_score_host(*args, y, qy[:-1], None, 1)
    with pytest.raises(ValueError, match=r"\(N, D\)"):
        predictive_log_score_host(*args, y, qy.astype(np.uint8), None, 1)
    # a state of 33 latents: refused in a visited datapoint, not looked at in one without a scored entry
    ss = np.array(p.ss)
    assert ss[1, 2].sum() == 32
    ss[1, 2, np.flatnonzero(~ss[1, 2])[0]] = True
    with pytest.raises(EvoAmdError, match=r"n = 1 .*k = 33"):
        predictive_log_score_host("bsc", p.theta, ss, p.lpj, p.Y, y, qy, None, 1)
    qy[1] = False
    score, info = predictive_log_score_host("bsc", p.theta, ss, p.lpj, p.Y, y, qy, None, 1)
    assert np.isfinite(score) and info["n_not_queried"] == 1 and info["count"][1] == 0 and np.isnan(info["logp"][1]).all()
    # nothing scored at all
    score, info = predictive_log_score_host("bsc", p.theta, ss, p.lpj, p.Y, y, np.zeros_like(qy), None, 1)
    assert np.isnan(score) and info["n_not_queried"] == p.N and not info["count"].any()


def test_pit_summary():
    k = 1000
    u = (np.arange(k) + 0.5) / k  # the uniform distribution's own quantiles
    s = pit_summary(np.concatenate((u, [np.nan, np.inf])).reshape(2, -1))
    assert s["n"] == k and s["ks"] == pytest.approx(0.5 / k) and s["coverage"] == {0.5: pytest.approx(0.5), 0.9: pytest.approx(0.9)}
    s = pit_summary(np.full(10, 0.5), levels=(0.2,))  # a point mass at 1/2: over-dispersed predictions
    assert s["ks"] == pytest.approx(0.5) and s["coverage"] == {0.2: 1.0}
    s = pit_summary(np.array([0.0, 1.0] * 5))  # everything in the tails: under-dispersed predictions
    assert s["ks"] == pytest.approx(0.5) and s["coverage"] == {0.5: 0.0, 0.9: 0.0}
    s = pit_summary(np.array([np.nan]))
    assert s["n"] == 0 and math.isnan(s["ks"]) and math.isnan(s["coverage"][0.5])

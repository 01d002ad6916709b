"""The NumPy mirror of the predictive moments (evo_amd.models.predictive) and of the precision-weighted patch merge
(evo_amd.utils.prepost.PrecisionMerger), on the CPU.

1. the mirror's mean against the reference's own y_reconstructed (tests/golden/missing_*.npz) at rtol 1e-11 / atol 1e-12,
   the tolerance tests/test_oracle_golden.py holds that array to;
2. the ES3C state terms (latent space) against Gaussian conditioning in data space at 1e-12 absolute, and the mixture
   moments over all 2^H states formed from those;
3. properties: var - noise >= 0, a one-state posterior, the centred against the raw-moment form, NaN rows, the k limit,
   the singular count;
4. PrecisionMerger against an explicit triple loop.
"""
import numpy as np
import pytest

from _exact_problems import oracle_lpj, oracle_zero
from _predictive_problems import MERGE_CASES, fixture_steps, merge_case, problem
from evo_amd._lib import EvoAmdError
from evo_amd.models import predictive_moments_host
from evo_amd.models.predictive import PRED_MAX_K, state_terms_es3c
from evo_amd.utils.prepost import (PrecisionMerger, estimate_stack, mean_merger, patch_geometry, precision_merger)
from evo_amd.variational.utils import enumerate_states


# ---- 1. the reference's numbers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_mean_equals_reference_reconstruction(algo):
    g, steps = fixture_steps(algo)
    Y, x_infr = g["Y"], g["x_infr"]
    miss = ~x_infr & x_infr.any(axis=1)[:, None]
    assert miss.any() and len(steps) >= 2
    for t, theta, ss, lpj, y_rec in steps:
        mean, var, info = predictive_moments_host("bsc" if algo == "ebsc" else "sssc", theta, ss, lpj, Y, x_infr)
        assert info == {"n_singular": 0, "n_skipped": int((~x_infr.any(axis=1)).sum())}
        print("%s step %d: max |mean - y_reconstructed| = %.3g" % (algo, t, np.abs(mean[miss] - y_rec[miss]).max()))
        np.testing.assert_allclose(mean[miss], y_rec[miss], rtol=1e-11, atol=1e-12)
        assert (var[miss] >= 0).all()


# ---- 2. an independent derivation -------------------------------------------------------------------------------------------
def _small_es3c(incomplete):
    rng = np.random.RandomState(17 + incomplete)
    H, D, N = 4, 7, 6
    A = rng.normal(size=(H, H))
    theta = {"W": rng.normal(size=(D, H)), "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H),
             "Psi": A @ A.T + 0.5 * np.eye(H), "sigma2": np.float64(0.7)}
    Y = rng.normal(size=(N, D)) * 2.0
    x_infr = np.ones((N, D), dtype=bool)
    if incomplete:
        for n in range(N):
            x_infr[n, rng.choice(D, 2, replace=False)] = False
        Y[~x_infr] = np.nan
    return theta, Y, x_infr


def _data_space(theta, idx, y, obs):
    """m, v of one state by conditioning the joint Gaussian of (y_o, W_A z_A) on y_o."""
    W, mus, Psi, s2 = theta["W"], theta["mus"], theta["Psi"], float(theta["sigma2"])
    WA = W[:, idx]
    K = WA @ Psi[np.ix_(idx, idx)] @ WA.T
    C = K[np.ix_(obs, obs)] + s2 * np.eye(int(obs.sum()))
    Ci = np.linalg.inv(C)
    m = WA @ mus[idx] + K[:, obs] @ Ci @ (y[obs] - WA[obs] @ mus[idx])
    v = np.diag(K - K[:, obs] @ Ci @ K[obs, :])
    return m, v


@pytest.mark.parametrize("incomplete", [False, True])
def test_state_terms_equal_gaussian_conditioning(incomplete):
    theta, Y, x_infr = _small_es3c(incomplete)
    H = 4
    states = enumerate_states(H)[1:]
    worst = 0.0
    per_state = np.zeros((Y.shape[0], 1 + states.shape[0], 2, Y.shape[1]))
    for n in range(Y.shape[0]):
        for s, st in enumerate(states):
            idx = np.flatnonzero(st)
            m, v = state_terms_es3c(theta["W"], theta["mus"], theta["Psi"], float(theta["sigma2"]), idx, Y[n], x_infr[n])
            m2, v2 = _data_space(theta, idx, Y[n], x_infr[n])
            worst = max(worst, np.abs(m - m2).max(), np.abs(v - v2).max())
            np.testing.assert_allclose(m, m2, rtol=0, atol=1e-12)
            np.testing.assert_allclose(v, v2, rtol=0, atol=1e-12)
            per_state[n, 1 + s] = m2, v2
    print("incomplete=%s: max |latent - data space| = %.3g" % (incomplete, worst))
    # all 2^H states as K^n, lpj from the oracle: the mixture moments of the data-space values
    xi = x_infr if incomplete else None
    lpj = np.concatenate((oracle_zero("es3c", theta, Y, xi)[:, None], oracle_lpj("es3c", theta, Y, states, xi)), axis=1)
    ss = np.tile(states[None], (Y.shape[0], 1, 1))
    mean, var, info = predictive_moments_host("sssc", theta, ss, lpj, Y, xi, S_perm=1, noise=True)
    assert info == {"n_singular": 0, "n_skipped": 0}
    q = np.exp(lpj - lpj.max(axis=1, keepdims=True))
    q /= q.sum(axis=1, keepdims=True)
    want_mean = np.einsum("ns,nsd->nd", q, per_state[:, :, 0])
    want_var = np.einsum("ns,nsd->nd", q, (per_state[:, :, 0] - want_mean[:, None]) ** 2 + per_state[:, :, 1])
    np.testing.assert_allclose(mean, want_mean, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(var, want_var + float(theta["sigma2"]), rtol=1e-12, atol=1e-12)


# ---- 3. properties ----------------------------------------------------------------------------------------------------------
CASES = [("es3c", 30, 25, 10, False, 1, False), ("es3c", 37, 70, 70, True, 1, False), ("es3c", 30, 25, 10, True, 0, True),
         ("ebsc", 37, 25, 70, False, 1, False), ("ebsc", 30, 70, 10, True, 0, False)]


@pytest.mark.parametrize("case", CASES)
def test_variance_is_non_negative_and_rows_without_data_are_nan(case):
    p = problem(*case)
    ok = ~np.isnan(p.var0)
    assert (p.var0[ok] >= 0).all()
    s2 = float(p.theta["sigma"] ** 2 if p.algo == "ebsc" else p.theta["sigma2"])
    np.testing.assert_allclose(p.var[ok], p.var0[ok] + s2, rtol=1e-15)
    dead = ~p.x_infr.any(axis=1)
    assert p.info == {"n_singular": 0, "n_skipped": int(dead.sum())} and dead.sum() == (1 if p.incomplete else 0)
    assert np.isnan(p.mean[dead]).all() and np.isnan(p.var[dead]).all()
    assert not np.isnan(p.mean[~dead]).any() and not np.isnan(p.var[~dead]).any()
    if p.algo == "es3c":
        assert (p.var0[~dead] > 0).any()


def test_one_state_posterior_has_exactly_the_noise_variance():
    p = problem("ebsc", 30, 25, 10, False, 1, False)
    lpj = np.array(p.lpj)
    lpj[:, 3] += 800.0
    mean, var, _ = predictive_moments_host("bsc", p.theta, p.ss, lpj, p.Y, None, 1)
    assert np.array_equal(var, np.full_like(var, p.theta["sigma"] ** 2))
    np.testing.assert_allclose(mean, p.ss[:, 2].astype(float) @ p.theta["W"].T, rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_centred_form_agrees_with_raw_moments_on_the_fixtures(algo):
    g, steps = fixture_steps(algo)
    Y, x_infr = g["Y"], g["x_infr"]
    name = "bsc" if algo == "ebsc" else "sssc"
    live = x_infr.any(axis=1)
    for t, theta, ss, lpj, _ in steps:
        mean, var, _ = predictive_moments_host(name, theta, ss, lpj, Y, x_infr, noise=False)
        q = np.exp(lpj - lpj.max(axis=1, keepdims=True))
        q /= q.sum(axis=1, keepdims=True)
        raw = np.zeros_like(var)
        for n in np.flatnonzero(live):
            for s in range(ss.shape[1]):
                idx = np.flatnonzero(ss[n, s])
                if algo == "ebsc":
                    m, v = theta["W"][:, idx].sum(axis=1), 0.0
                else:
                    m, v = state_terms_es3c(theta["W"], theta["mus"], theta["Psi"], float(theta["sigma2"]), idx, Y[n], x_infr[n])
                raw[n] += q[n, s] * (m * m + v)
        raw -= mean ** 2
        scale = np.abs(var[live]).max()
        print("%s step %d: max |centred - raw| = %.3g at max var %.3g" % (algo, t, np.abs(raw[live] - var[live]).max(), scale))
        np.testing.assert_allclose(raw[live], var[live], rtol=1e-10, atol=1e-10 * scale)


def test_more_than_32_active_latents_raise():
    rng = np.random.RandomState(3)
    H, D, N, S = 40, 6, 3, 2
    theta = {"W": rng.normal(size=(D, H)), "pi": 0.1, "sigma": 1.0}
    ss = np.zeros((N, S, H), dtype=bool)
    ss[:, :, :2] = True
    ss[1, 1, :PRED_MAX_K] = True
    predictive_moments_host("bsc", theta, ss, np.zeros((N, S)), rng.normal(size=(N, D)))  # k = 32 is served
    ss[1, 1, PRED_MAX_K] = True
    with pytest.raises(EvoAmdError, match=r"n = 1 .*k = 33"):
        predictive_moments_host("bsc", theta, ss, np.zeros((N, S)), rng.normal(size=(N, D)))


def test_singular_system_is_counted():
    """A rank-deficient Psi_AA (a dead latent: zero row and column) with W_oA = 0 on the datapoint's reliable entries."""
    rng = np.random.RandomState(4)
    H, D, N, S = 5, 6, 4, 2
    Psi = np.eye(H)
    Psi[2, :] = Psi[:, 2] = 0.0
    W = rng.normal(size=(D, H))
    W[:3, [1, 2]] = 0.0
    theta = {"W": W, "pies": np.full(H, 0.2), "mus": np.zeros(H), "Psi": Psi, "sigma2": np.float64(1.0)}
    ss = np.zeros((N, S, H), dtype=bool)
    ss[:, 0, 0] = True
    ss[:, 1, 3] = True
    ss[2, 1] = [False, True, True, False, False]  # A = {1, 2}: Psi_AA = diag(1, 0), W_oA = 0
    x_infr = np.ones((N, D), dtype=bool)
    x_infr[2, 3:] = False
    Y = np.where(x_infr, rng.normal(size=(N, D)), np.nan)
    mean, var, info = predictive_moments_host("sssc", theta, ss, np.zeros((N, S)), Y, x_infr)
    assert info == {"n_singular": 1, "n_skipped": 0}
    assert np.isnan(mean[2]).all() and np.isnan(var[2]).all()
    assert not np.isnan(np.delete(mean, 2, axis=0)).any() and not np.isnan(np.delete(var, 2, axis=0)).any()
    lpj = np.zeros((N, S))
    lpj[2, 1] = -900.0  # the singular state has weight 0: it is not evaluated
    _, _, info = predictive_moments_host("sssc", theta, ss, lpj, Y, x_infr)
    assert info == {"n_singular": 0, "n_skipped": 0}


# ---- 4. PrecisionMerger ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MERGE_CASES))
def test_precision_merger_equals_triple_loop(name):
    (H, W, C, ph, pw, shift), Y, V, ref = merge_case(name)
    stack = estimate_stack(Y, H, W, C, ph, pw, shift)
    merger = precision_merger(V.T)
    assert isinstance(merger, PrecisionMerger)
    with pytest.raises(ValueError, match="bind"):
        merger(stack)
    got = merger.bind(H, W, C, ph, pw, shift)(stack, axis=0)
    assert got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)
    assert np.isnan(got[0, 0]).all() and not np.isnan(got).all()
    with pytest.raises(ValueError, match="variances of shape"):
        precision_merger(V.T[:, :-1]).bind(H, W, C, ph, pw, shift)


@pytest.mark.parametrize("name", ["s1_c1", "s2_c3"])
def test_equal_variances_reproduce_the_mean_merger(name):
    (H, W, C, ph, pw, shift), Y, _, _ = merge_case(name)
    N, D = patch_geometry(H, W, C, ph, pw, shift)
    stack = estimate_stack(Y, H, W, C, ph, pw, shift)
    want = mean_merger(stack)
    for v in (0.5, 4.0):  # a power of two: the weights scale both sums exactly
        got = precision_merger(np.full((D, N), v)).bind(H, W, C, ph, pw, shift)(stack)
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=0, equal_nan=True)
    # any other value: K <= ph pw products and 2 K additions, each within one rounding of the exact value, so the two
    # quotients differ by at most (3 K + 2) eps sum|e_k| / count (a bound relative to the estimates, not to a mean that
    # may cancel)
    got = precision_merger(np.full((D, N), 0.37)).bind(H, W, C, ph, pw, shift)(stack)
    K = ph * pw
    bound = (3 * K + 2) * np.finfo(float).eps * mean_merger(np.abs(stack))
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok) and (np.abs(got - want)[ok] <= bound[ok]).all()

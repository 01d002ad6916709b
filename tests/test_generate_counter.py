"""evo_amd.models.generate_counter: the NumPy mirror of the device sampler (csrc/kernels_generate.hpp).

1. the stream: s equals a scalar Python-int restatement of rng_u01 with the purposes and indices of the definition;
2. the law: mean of s, mean and covariance of y within 5 standard errors of the analytic values (fixed seed, ES3C with a
   singular Psi, and BSC);
3. the factor F of Psi: regular, singular, and with a tiny negative eigenvalue;
4. given s, shards, the shape of the result.
"""
import math

import numpy as np
import pytest

import _generate_problems as gp
from evo_amd.models import generate_counter
from evo_amd.models.generate import GEN_PURPOSE, generate_params, pack_words, psi_factor, unpack_words


def test_purpose_constant():
    assert GEN_PURPOSE == gp.GEN_PURPOSE == int.from_bytes(b"GEN\0\0\0\0\0", "big")


@pytest.mark.parametrize("model_name", ["bsc", "sssc"])
def test_stream_of_s(model_name):
    H, D, N, seed, first = 70, 5, 40, 0xFEDCBA9876543210, 1000
    theta = gp.sssc_theta(H, D, 3, diagonal=True) if model_name == "sssc" else gp.bsc_theta(H, D, 3, pi=0.25)
    out = generate_counter(model_name, theta, N, seed, first_index=first)
    pies = theta["pies"] if model_name == "sssc" else np.full(H, theta["pi"])
    for n, h in [(0, 0), (0, 69), (1, 63), (7, 64), (39, 1), (39, 69), (20, 33)]:
        assert out["s"][n, h] == (gp.rng_u01_int(seed, first + n, gp.GEN_PURPOSE, h) <= pies[h]), (n, h)
    assert out["s"].dtype == np.bool_ and 0 < out["s"].sum() < N * H


def test_stream_of_the_normals():
    """eps and g: Box-Muller on the uniforms of purposes + 1 and + 2, pair k >> 1, cosine for even k, sine for odd k."""
    H, D, N, seed = 5, 3, 4, 99
    theta = gp.sssc_theta(H, D, 4)
    theta["pies"] = np.ones(H)  # every latent active: z = mus + F eps
    out = generate_counter("sssc", theta, N, seed)
    F = psi_factor(theta["Psi"])

    def normal(n, purpose, k):
        u1, u2 = (gp.rng_u01_int(seed, n, purpose, 2 * (k >> 1) + i) for i in (0, 1))
        r, t = math.sqrt(-2.0 * math.log(u1)), 6.283185307179586 * u2
        return r * (math.sin(t) if k & 1 else math.cos(t))

    for n in (0, 3):
        eps = np.array([normal(n, gp.GEN_PURPOSE + 1, j) for j in range(H)])
        g = np.array([normal(n, gp.GEN_PURPOSE + 2, d) for d in range(D)])
        z = theta["mus"] + np.dot(F, eps)
        np.testing.assert_allclose(out["z"][n], z, rtol=0, atol=1e-12)
        np.testing.assert_allclose(out["y_mean"][n], np.dot(theta["W"], z), rtol=0, atol=1e-12)
        np.testing.assert_allclose(out["y"][n], np.dot(theta["W"], z) + math.sqrt(theta["sigma2"]) * g, rtol=0, atol=1e-12)


@pytest.mark.parametrize("model_name", ["bsc", "sssc"])
def test_law(model_name):
    theta = gp.law_theta(model_name)
    if model_name == "sssc":
        assert np.linalg.matrix_rank(theta["Psi"]) == 6  # singular
    out = generate_counter(model_name, theta, gp.LAW_N, gp.LAW_SEED)
    gp.assert_law(model_name, theta, out, "mirror")


def test_law_check_sees_a_wrong_variance():
    """The bound is not vacuous: data generated with 1.2 sigma, or with F of a Psi scaled by 1.3, misses it."""
    theta = gp.law_theta("sssc")
    wrong = dict(theta, sigma2=theta["sigma2"] * 1.44)
    assert max(gp.law_zscores("sssc", theta, generate_counter("sssc", wrong, gp.LAW_N, gp.LAW_SEED))) > 1.5 * gp.LAW_BOUND
    wrong = dict(theta, Psi=theta["Psi"] * 1.3)
    assert max(gp.law_zscores("sssc", theta, generate_counter("sssc", wrong, gp.LAW_N, gp.LAW_SEED))) > 1.5 * gp.LAW_BOUND


def test_psi_factor():
    rng = np.random.RandomState(5)
    H = 12
    A = rng.normal(size=(H, H))
    regular = np.dot(A, A.T)
    B = rng.normal(size=(H, 7))
    singular = np.dot(B, B.T)
    lam, V = np.linalg.eigh(singular)
    lam[:5] = 0.0
    lam[0] = -1e-14 * lam[-1]  # what rounding leaves of a zero eigenvalue
    negative = np.dot(V * lam, V.T)
    for Psi in (regular, singular, negative):
        F = psi_factor(Psi)
        assert F.shape == (H, H) and np.isfinite(F).all()
        assert np.abs(np.dot(F, F.T) - Psi).max() <= 1e-12 * np.linalg.norm(Psi)


def test_given_s_and_shards():
    H, D, N, seed = 70, 9, 50, 5
    theta = gp.sssc_theta(H, D, 6)
    full = generate_counter("sssc", theta, N, seed)
    assert sorted(full) == ["s", "y", "y_mean", "z"]
    assert full["y"].shape == (N, D) and full["z"].shape == (N, H) and full["s"].shape == (N, H)
    assert np.array_equal(full["z"] != 0.0, full["s"])
    a = generate_counter("sssc", theta, 20, seed)
    b = generate_counter("sssc", theta, N - 20, seed, first_index=20)
    for key in full:
        assert np.array_equal(np.concatenate((a[key], b[key])), full[key]), key
    # s given: taken, not drawn; the normals do not depend on it
    given = generate_counter("sssc", theta, N, seed, s=full["s"])
    for key in full:
        assert np.array_equal(given[key], full[key]), key
    zero = generate_counter("sssc", theta, N, seed, s=np.zeros((N, H), dtype=bool))
    assert not zero["y_mean"].any() and not zero["z"].any() and not zero["s"].any()
    assert sorted(generate_counter("bsc", gp.bsc_theta(H, D, 6), 3, seed)) == ["s", "y", "y_mean"]


def test_word_layout():
    rng = np.random.RandomState(0)
    for H in (1, 63, 64, 70, 130):
        s = rng.random_sample((5, H)) < 0.4
        words = pack_words(s)
        assert words.dtype == np.uint64 and words.shape == (5, (H + 63) // 64)
        assert np.array_equal(unpack_words(words, H), s)
        for n, h in [(0, 0), (4, H - 1)]:
            assert bool((int(words[n, h // 64]) >> (63 - h % 64)) & 1) == s[n, h]


def test_generate_params_reads_the_reference_keys():
    par = generate_params("bsc", gp.bsc_theta(4, 3, 0, pi=0.2))
    assert par["Wt"].shape == (4, 3) and np.array_equal(par["pies"], np.full(4, 0.2)) and par["F"] is None
    th = gp.sssc_theta(4, 3, 0)
    par = generate_params("sssc", th)
    assert par["sigma"] == math.sqrt(th["sigma2"]) and par["F"].shape == (4, 4)

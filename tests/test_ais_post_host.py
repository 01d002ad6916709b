"""The posterior from AIS chains on the CPU (evo_amd.models.ais_posterior_counter, the NumPy mirror of
csrc/kernels_ais_post.hpp).

1. the law, exactly: at H = 4 the chain law is propagated over all 2^H states; E[w] = Z_1 / Z_0, and for every kept scan and
   every latent E[w r_h] = (Z_1 / Z_0) E_p[s_h | y], r_h the conditional recorded at the moment latent h is decided;
2. the mirror against ais_log_likelihood_counter: the chains ARE its forward chains, bit for bit up to the first kept scan;
3. the mirror against enumeration at H = 10: every entry within 5 p_se + 3 / ess_n;
4. the stream (a prefix of the chains, shards by first_index, n_keep) and the refusals that need no GPU.
"""
import numpy as np
import pytest

import _ais_post_problems as pp
import _ais_problems as ap
import _sweep_problems as sp
from evo_amd.models import BSC, SSSC, ais_conditional, ais_posterior_counter, ais_scalars


# ---- 1. the law, exactly -------------------------------------------------------------------------------------------------------
def test_the_law_by_exact_propagation():
    H, D, T, K = 4, 5, 3, 2
    p = ap.build(1, D, H, 11, k=2)
    W = p.theta["W"]
    B, G, yy = np.dot(p.Y, W)[0], np.dot(W.T, W), float((p.Y[0] ** 2).sum())
    pre1, pilb, pi = ais_scalars(p.theta)
    betas = np.array([0.0, 0.2, 0.6, 1.0])
    S = 2 ** H
    states = ((np.arange(S)[:, None] >> np.arange(H)[None, :]) & 1).astype(bool)
    c = B[None, :] - np.dot(states.astype(np.float64), G)  # c_j of every state
    ell = pre1 * (yy - (states * (B[None, :] + c)).sum(axis=1))
    k = states.sum(axis=1)

    def cond(h, beta):
        """p(s_h = 1 | the rest) of every state, from ais_conditional."""
        return np.array([float(ais_conditional(pre1, pilb, c[i, h], G[h, h], states[i, h], beta)) for i in range(S)])

    def site(h, beta):
        """The single-site transition: state i goes to i with bit h set (probability p_h(i)) or cleared."""
        ph = cond(h, beta)
        M = np.zeros((S, S))
        for i in range(S):
            M[i, i | (1 << h)] += ph[i]
            M[i, i & ~(1 << h)] += 1.0 - ph[i]
        return M

    # the truth: Z_1 from the oracle's lpj, Z_0 the prior's normaliser
    oth = sp.oracle_theta("ebsc", p.theta, D, H)
    lpj = sp.oracle_lpj("ebsc", oth, p.Y[0], states)
    assert np.abs(lpj - (k * pilb + ell)).max() <= 1e-12 * np.abs(lpj).max()
    Z1, Z0 = np.exp(lpj).sum(), (1.0 - pi) ** (-H)
    post = (np.exp(lpj)[:, None] * states).sum(axis=0) / Z1
    ratio = Z1 / Z0

    v = pi ** k * (1.0 - pi) ** (H - k)  # v(s) = E[w 1{x = s}], w = 1 at the start
    assert abs(v.sum() - 1.0) <= 1e-14
    worst = 0.0
    for t in range(1, T + K):
        beta = betas[min(t, T)]
        if t <= T:
            v = v * np.exp((betas[t] - betas[t - 1]) * ell)
        if t == T:
            assert abs(v.sum() - ratio) <= 1e-12 * ratio, "E[w] is not Z_1 / Z_0"
        for h in range(H):
            if t >= T:  # a kept scan: the conditional is recorded when latent h is decided, before the bit is drawn
                got = float((v * cond(h, beta)).sum())
                worst = max(worst, abs(got - ratio * post[h]) / ratio)
                assert abs(got - ratio * post[h]) <= 1e-12 * ratio, (t, h, got, ratio * post[h])
            v = np.dot(v, site(h, beta))
        assert t < T or abs(v.sum() - ratio) <= 1e-12 * ratio
    print("E[w] = Z_1 / Z_0 = %.15g; largest |E[w r_h] - (Z_1 / Z_0) E_p[s_h | y]| / (Z_1 / Z_0) over %d kept scans: %.3g"
          % (ratio, K, worst))
    # the state-based estimator has nothing to say about a latent no chain switched on; the recorded conditional has
    q = ap.build(2, D, H, 11, k=1)
    out = ais_posterior_counter(q.theta, q.Y, n_chains=3, betas=betas, n_keep=K, seed=1)
    never_on = ~out["chain_map_bool"].any(axis=1)  # (N, H): off in the best state of every chain
    assert never_on.any() and (out["p"][never_on] > 0.0).all()


# ---- 2. the chains are the forward chains of ais_log_likelihood_counter -----------------------------------------------------------
@pytest.mark.parametrize("name", list(ap.CASES))
def test_mirror_continues_the_forward_chains(name):
    p = ap.problem(name)
    for K in (1, 3):
        out = ais_posterior_counter(p.theta, p.Y, n_chains=ap.C, n_temps=ap.T, n_keep=K, seed=ap.STREAM_SEED)
        for k in ("log_w", "ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
            assert np.array_equal(out[k], p.forward[k]), (K, k)
        assert np.array_equal(out["first_flips"], p.forward["chain_flips"])
        assert np.array_equal(out["first_bool"], p.forward["final_bool"])
        assert (out["margin"] <= p.forward["margin"]).all()
        if K == 1:  # one kept scan: the best state is the state behind it, the flips are all the flips
            assert np.array_equal(out["chain_map_bool"], p.forward["final_bool"])
            assert np.array_equal(out["chain_flips"], p.forward["chain_flips"])
            assert np.array_equal(out["n_flips"], p.forward["n_flips"]) and out["n_flips"].dtype == np.int64
        else:
            assert (out["chain_flips"] >= p.forward["chain_flips"]).all()


# ---- 3. the mirror against enumeration -------------------------------------------------------------------------------------------
def test_mirror_against_the_exact_marginals():
    p = pp.exact_problem()
    c, out = pp.EXACT, p.want
    pp.check_bars(out, p.exact)
    N, H, C = c["N"], c["H"], c["C"]
    assert out["p"].shape == out["p_se"].shape == (N, H) and out["rb"].shape == (N, C, H)
    assert ((out["p"] > 0.0) & (out["p"] <= 1.0 + 1e-12)).all() and (out["p_se"] >= 0.0).all()
    assert ((out["ess"] >= 1.0) & (out["ess"] <= C)).all()
    assert np.allclose(out["count"], out["p"].sum(axis=1), rtol=1e-13, atol=0)
    # the best state over the chains: its lpj is the oracle's, and no chain has a better one
    oth = sp.oracle_theta("ebsc", p.theta, p.D, H)
    for n in range(N):
        lpj = sp.oracle_lpj("ebsc", oth, p.Y[n], out["map_bool"][n][None, :])[0]
        assert abs(lpj - out["map_lpj"][n]) <= 1e-10 * max(1.0, abs(lpj))
        assert out["map_lpj"][n] == out["chain_map_lpj"][n].max()
        first = int(np.argmax(out["chain_map_lpj"][n]))  # (argmax: the lowest chain among equals)
        assert np.array_equal(out["map_bool"][n], out["chain_map_bool"][n, first])
    assert np.array_equal(pp.unpack(out["map_state"], H), out["map_bool"])
    assert np.array_equal(pp.unpack(out["chain_map_state"], H), out["chain_map_bool"])


# ---- 4. the stream and the refusals ----------------------------------------------------------------------------------------------
def test_stream_properties():
    p = pp.problem("two_words")
    full = p.want
    prefix = pp.mirror(p, p.T, 3, p.K)
    for k in ("log_w", "rb", "chain_map_lpj", "chain_map_bool", "chain_flips", "margin"):
        assert np.array_equal(prefix[k], full[k][:, :3]), k
    cut = 8
    a = pp.mirror(p, p.T, p.C, p.K, rows=slice(0, cut))
    b = pp.mirror(p, p.T, p.C, p.K, rows=slice(cut, None), first_index=cut)
    for k in ("p", "p_se", "count", "map_lpj", "map_state", "ll", "ess", "n_flips", "log_w", "rb", "chain_map_lpj"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), full[k]), k
    other = pp.mirror(p, p.T, p.C, p.K, seed=pp.STREAM_SEED + 1)
    assert not np.array_equal(other["log_w"], full["log_w"])
    # n_keep = 1 against 3: the weights are the same chains', the recorded conditionals are not
    one = pp.mirror(p, p.T, p.C, 1)
    assert np.array_equal(one["log_w"], full["log_w"]) and np.array_equal(one["ll"], full["ll"])
    assert not np.array_equal(one["rb"], full["rb"])
    assert (one["chain_map_lpj"] <= full["chain_map_lpj"]).all()  # the first kept scan is among the three
    # mean = p W^T
    assert np.array_equal(full["mean"], np.dot(full["p"], p.theta["W"].T))
    assert "mean" not in one


def test_python_refusals():
    p = pp.problem("partial_chunk")
    suff = {"permanent": {"background": False, "allzero": False, "singletons": False}, "S_perm": 0, "Mprime": 1}
    data = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    with pytest.raises(NotImplementedError, match="ES3C"):
        SSSC(p.D, p.H, 4).ais_posterior({}, suff, data)
    model = BSC(p.D, p.H, 4)
    for bad, match in (([0.1, 1.0], "start at 0"), ([0.0, 0.5, 0.9], "end at 1"), ([0.0, 0.6, 0.5, 1.0], "descend"),
                       ([0.0, 0.0, 1.0], "descend"), ([1.0], "T \\+ 1")):
        with pytest.raises(ValueError, match=match):
            model.ais_posterior(p.theta, suff, data, betas=bad)
        with pytest.raises(ValueError, match=match):
            ais_posterior_counter(p.theta, p.Y, betas=bad)
    for kw, match in ((dict(n_chains=0), "n_chains"), (dict(n_keep=0), "n_keep")):
        with pytest.raises(ValueError, match=match):
            model.ais_posterior(p.theta, suff, data, **kw)
        with pytest.raises(ValueError, match=match):
            ais_posterior_counter(p.theta, p.Y, **kw)
    holes = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    holes["x_infr"][0, 0] = False
    with pytest.raises(ValueError, match="incomplete"):
        model.ais_posterior(p.theta, suff, holes)
    with pytest.raises(ValueError, match="background"):
        model.ais_posterior(p.theta, dict(suff, permanent={"background": True, "allzero": False, "singletons": False}), data)
    with pytest.raises(ValueError, match="float32"):
        BSC(8, 16, 4, dtype=np.float32).ais_posterior({}, suff, data)
    with pytest.raises(ValueError, match="1024"):
        BSC(p.D, 1025, 4).ais_posterior({}, suff, data)
    with pytest.raises(ValueError, match="1024"):
        ais_posterior_counter({"W": np.zeros((2, 1025)), "pi": 0.1, "sigma": 1.0}, np.zeros((1, 2)))

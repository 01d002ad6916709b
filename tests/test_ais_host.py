"""Annealed importance sampling on the CPU (evo_amd.models.ais, the NumPy mirror of csrc/kernels_ais.hpp).

1. the law is valid, by enumeration at H = 3: the scans leave f_beta invariant, the descending scan is the reversal of the
   ascending one, and the sums over ALL paths give Z_1 / Z_0 (forward) and Z_0 / Z_1 (reverse) with Z_1 from the oracle's lpj;
2. the mirror against the exact answer at H = 8, both directions, 5 SE bars;
3. the stream: a prefix of the chains, shards by first_index, uniforms shared by the directions;
4. the refusals of the Python layer that need no GPU.
"""
import itertools

import numpy as np
import pytest

import _ais_problems as ap
import _sweep_problems as sp
from evo_amd.models import BSC, SSSC, ais_conditional, ais_log_likelihood_counter, ais_scalars, sigmoid_schedule
from evo_amd.models.ais import AIS_PURPOSE, _u01_chains, check_betas
from evo_amd.models.generate import _first_hash


# ---- 1. the law, by enumeration ------------------------------------------------------------------------------------------------
H3 = 3
STATES = [tuple(bool((i >> h) & 1) for h in range(H3)) for i in range(2 ** H3)]
BETAS = np.array([0.0, 0.15, 0.4, 0.8, 1.0])


def _tiny():
    p = ap.build(1, 3, H3, 11, k=2)
    W = p.theta["W"]
    return p, np.dot(p.Y, W)[0], np.dot(W.T, W), float((p.Y[0] ** 2).sum()), ais_scalars(p.theta)


def _c_of(B, G, s):
    c = B.copy()
    for i in range(H3):
        if s[i]:
            c = c - G[i]
    return c


def _ell(B, G, yy, pre1, s):
    c = _c_of(B, G, s)
    return pre1 * (yy - sum(B[a] + c[a] for a in range(H3) if s[a]))


def _f(B, G, yy, pre1, pilb, s, beta):
    return np.exp(sum(s) * pilb + beta * _ell(B, G, yy, pre1, s))


def _scan_matrix(B, G, pre1, pilb, beta, order):
    """K[i, j] = the probability that one scan over ``order`` takes state i to state j, from ais_conditional alone."""
    K = np.zeros((8, 8))
    for i, s0 in enumerate(STATES):
        dist = {s0: 1.0}
        for h in order:
            nxt = {}
            for s, pr in dist.items():
                p_on = float(ais_conditional(pre1, pilb, _c_of(B, G, s)[h], G[h, h], s[h], beta))
                for bit, q in ((True, p_on), (False, 1.0 - p_on)):
                    s2 = s[:h] + (bit,) + s[h + 1:]
                    nxt[s2] = nxt.get(s2, 0.0) + pr * q
            dist = nxt
        for s, pr in dist.items():
            K[i, STATES.index(s)] = pr
    return K


def test_the_law_is_valid_by_enumeration():
    p, B, G, yy, (pre1, pilb, pi) = _tiny()
    T = len(BETAS) - 1
    f = [np.array([_f(B, G, yy, pre1, pilb, s, b) for s in STATES]) for b in BETAS]
    ell = np.array([_ell(B, G, yy, pre1, s) for s in STATES])
    K = [None] + [_scan_matrix(B, G, pre1, pilb, BETAS[t], range(H3)) for t in range(1, T + 1)]
    Kr = [None] + [_scan_matrix(B, G, pre1, pilb, BETAS[t], range(H3 - 1, -1, -1)) for t in range(1, T + 1)]
    for t in range(1, T + 1):
        assert np.allclose(K[t].sum(axis=1), 1.0, rtol=0, atol=1e-12)
        inv = f[t] @ K[t]
        assert np.abs(inv - f[t]).max() <= 1e-12 * f[t].max(), "K_t does not leave f_beta_t invariant"
        want = (f[t][:, None] * K[t]).T / f[t][:, None]  # the reversal: K~[j, i] = f(i) K[i, j] / f(j)
        assert np.abs(Kr[t] - want).max() <= 1e-12, "the descending scan is not the reversal of the ascending one"
    # f_1 is the oracle's exp(lpj), Z_0 the prior's normaliser
    oth = sp.oracle_theta("ebsc", p.theta, p.D, H3)
    lpj = sp.oracle_lpj("ebsc", oth, p.Y[0], np.array(STATES))
    assert np.abs(np.log(f[T]) - lpj).max() <= 1e-12 * np.abs(lpj).max()
    Z1, Z0 = np.exp(lpj).sum(), (1.0 - pi) ** (-H3)
    assert abs(f[0].sum() - Z0) <= 1e-12 * Z0
    p0, pT = f[0] / Z0, np.exp(lpj) / Z1
    idx = range(8)
    fwd = rev = 0.0
    for path in itertools.product(idx, repeat=T):  # x_0 .. x_{T-1}
        log_w = sum((BETAS[t] - BETAS[t - 1]) * ell[path[t - 1]] for t in range(1, T + 1))
        dens_f = p0[path[0]] * np.prod([K[t][path[t - 1], path[t]] for t in range(1, T)])
        dens_r = pT[path[T - 1]] * np.prod([Kr[t][path[t], path[t - 1]] for t in range(T - 1, 0, -1)])
        fwd += dens_f * np.exp(log_w)
        rev += dens_r * np.exp(-log_w)
    print("sum over the paths: forward %.15g against Z_1 / Z_0 = %.15g; reverse %.15g against %.15g" % (fwd, Z1 / Z0, rev, Z0 / Z1))
    assert abs(fwd - Z1 / Z0) <= 1e-12 * Z1 / Z0
    assert abs(rev - Z0 / Z1) <= 1e-12 * Z0 / Z1


# ---- 2. the mirror against the exact answer ------------------------------------------------------------------------------------
def test_mirror_brackets_the_exact_answer():
    p = ap.small()
    ap.check_bars(p.forward, p.reverse, p.exact)
    for d in (p.forward, p.reverse):
        assert d["ll"].shape == (p.N,) and d["log_w"].shape == (p.N, ap.SMALL["C"]) and d["n_flips"].dtype == np.int64
        assert ((d["ess"] >= 1.0) & (d["ess"] <= ap.SMALL["C"])).all()
        assert (d["log_w_min"] <= d["log_w_mean"]).all() and (d["log_w_mean"] <= d["log_w_max"]).all()
        assert np.array_equal(ap.unpack_final(d["final"], p.N, ap.SMALL["C"], p.H), d["final_bool"])
    again = ap.mirror(p, ap.SMALL["T"], 3, "forward")
    assert np.array_equal(again["log_w"], p.forward["log_w"][:, :3])


# ---- 3. the stream -------------------------------------------------------------------------------------------------------------
def test_stream_properties():
    p = ap.problem("two_words")
    for direction, full in (("forward", p.forward), ("reverse", p.reverse)):
        prefix = ap.mirror(p, ap.T, 3, direction)
        for k in ("log_w", "final_bool", "chain_flips", "start", "margin"):
            assert np.array_equal(prefix[k], full[k][:, :3]), (direction, k)
        cut = 8
        a = ap.mirror(p, ap.T, ap.C, direction, rows=slice(0, cut))
        b = ap.mirror(p, ap.T, ap.C, direction, rows=slice(cut, None), first_index=cut)
        for k in ("ll", "ess", "log_w", "final_bool", "n_flips", "log_w_mean", "log_w_min", "log_w_max"):
            assert np.array_equal(np.concatenate([a[k], b[k]]), full[k]), (direction, k)
        other = ap.mirror(p, ap.T, ap.C, direction, seed=ap.STREAM_SEED + 1)
        assert not np.array_equal(other["log_w"], full["log_w"])
    # the starting draw is the uniforms of block 0 against pi; both directions read block t + 1 at temperature t
    pi = ais_scalars(p.theta)[2]
    hs = np.arange(p.H, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for n in (0, p.N - 1):
            x0 = _first_hash(ap.STREAM_SEED, np.array([n], dtype=np.uint64))
            assert np.array_equal(_u01_chains(x0, ap.C, hs) < pi, p.forward["start"][n])
    assert AIS_PURPOSE == 0x4149530000000000
    # a chain of T = 1 has no transition inside w: forward log w = l(x_0), and a reverse chain from x_0 gives the same value
    one = ap.mirror(p, 1, 2, "forward")
    back = ais_log_likelihood_counter(p.theta, p.Y[:1], n_chains=1, n_temps=1, seed=ap.STREAM_SEED, direction="reverse",
                                      s_start=one["start"][:1, 0])
    assert back["log_w"][0, 0] == one["log_w"][0, 0] and back["n_flips"][0] == 0
    # the directions share uniforms by (c, t, h): with ONE latent the ascending and the descending scan are the same
    # transition, so a forward chain over [0, 1] (one scan at beta = 1, block 2) and a reverse chain over [0, 1, 1] from the
    # forward chain's start (one scan at beta_1 = 1, block 2) must end in the same state
    q = ap.build(6, 3, 1, 5, k=1)
    f = ais_log_likelihood_counter(q.theta, q.Y, n_chains=4, betas=[0.0, 1.0], seed=7)
    for c in range(4):
        r = ais_log_likelihood_counter(q.theta, q.Y, n_chains=4, betas=[0.0, 1.0, 1.0], seed=7, direction="reverse",
                                       s_start=f["start"][:, c])
        assert np.array_equal(r["final_bool"][:, c], f["final_bool"][:, c])
        assert np.array_equal(r["chain_flips"][:, c], f["chain_flips"][:, c])
    assert f["chain_flips"].any()


def test_schedule():
    b = sigmoid_schedule(128)
    assert b.shape == (129,) and b[0] == 0.0 and b[-1] == 1.0 and (np.diff(b) > 0).all()
    assert abs(b[64] - 0.5) <= 1e-15 and np.allclose(b + b[::-1], 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(sigmoid_schedule(1), [0.0, 1.0])
    assert check_betas(b) is not None


# ---- 4. refusals that need no GPU ----------------------------------------------------------------------------------------------
def test_python_refusals():
    p = ap.problem("partial_chunk")
    suff = {"permanent": {"background": False, "allzero": False, "singletons": False}, "S_perm": 0, "Mprime": 1}
    data = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    with pytest.raises(NotImplementedError, match="ES3C"):
        SSSC(p.D, p.H, 4).ais_log_likelihood({}, suff, data)
    model = BSC(p.D, p.H, 4)
    for bad, match in (([0.1, 1.0], "start at 0"), ([0.0, 0.5, 0.9], "end at 1"), ([0.0, 0.6, 0.5, 1.0], "descend"),
                       ([0.0, 0.0, 1.0], "descend"), ([1.0], "T \\+ 1")):
        with pytest.raises(ValueError, match=match):
            model.ais_log_likelihood(p.theta, suff, data, betas=bad)
        with pytest.raises(ValueError, match=match):
            ais_log_likelihood_counter(p.theta, p.Y, betas=bad)
    with pytest.raises(ValueError, match="s_start"):
        model.ais_log_likelihood(p.theta, suff, data, direction="reverse")
    with pytest.raises(ValueError, match="s_start"):
        model.ais_log_likelihood(p.theta, suff, data, direction="reverse", s_start=p.s_true[:, :-1])
    with pytest.raises(ValueError, match="s_start"):
        model.ais_log_likelihood(p.theta, suff, data, direction="reverse", s_start=p.s_true.astype(np.uint8))
    with pytest.raises(ValueError, match="admit"):
        model.ais_log_likelihood(p.theta, suff, data, direction="reverse", s_start=p.s_true, admit=True)
    with pytest.raises(ValueError, match="direction"):
        model.ais_log_likelihood(p.theta, suff, data, direction="sideways")
    with pytest.raises(ValueError, match="n_chains"):
        model.ais_log_likelihood(p.theta, suff, data, n_chains=0)
    holes = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    holes["x_infr"][0, 0] = False
    with pytest.raises(ValueError, match="incomplete"):
        model.ais_log_likelihood(p.theta, suff, holes)
    with pytest.raises(ValueError, match="background"):
        model.ais_log_likelihood(p.theta, dict(suff, permanent={"background": True, "allzero": False, "singletons": False}), data)
    with pytest.raises(ValueError, match="float32"):
        BSC(8, 16, 4, dtype=np.float32).ais_log_likelihood({}, suff, data)
    with pytest.raises(ValueError, match="1024"):
        BSC(p.D, 1025, 4).ais_log_likelihood({}, suff, data)

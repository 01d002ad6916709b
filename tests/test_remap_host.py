"""The host side of the dictionary resize: the NumPy mirror of the remap law (evo_amd.variational.remap_states_host) against
an independent brute force, remap_theta, prune_index, latent_usage_host and the refusals of the Python layer -- none of
which touches the engine (no GPU on the host that runs this file)."""
import numpy as np
import pytest

import _remap_problems as rp
from _seed_problems import make_data, make_theta
from evo_amd.models import BSC, SSSC, remap_theta
from evo_amd.variational import (check_remap_index, latent_usage_host, posterior_scores_host, prune_index,
                                 remap_states_host)

HOST_CASES = [n for n in rp.CASES if n != "cap"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_mirror_equals_brute_force(name):
    c = rp.case(name)
    got, n_rep = remap_states_host(c.ss, c.index, c.S_perm, c.background)
    assert got.shape == (c.N, c.S, c.H2) and got.dtype == np.bool_ and n_rep.dtype == np.int32
    assert np.array_equal(got, c.want)
    assert np.array_equal(n_rep, c.n_replaced)
    print("%s: mean / max n_replaced per datapoint %.2f / %d" % (name, n_rep.mean(), n_rep.max()))
    for n in range(c.N):
        assert len({r.tobytes() for r in got[n]}) == c.S  # S distinct states
        if c.S_perm:
            assert got[n].any(axis=1).all()  # never the permanent all-zero state
    # kept slots keep their position and their gathered bits
    src = c.index >= 0
    gathered = np.zeros_like(got)
    gathered[:, :, src] = c.ss[:, :, c.index[src]]
    assert np.array_equal(got[c.kept], gathered[c.kept])
    assert np.array_equal((~c.kept).sum(axis=1), n_rep)
    if c.background:
        assert got[:, :, -1].all()


def test_cases_cover_what_they_are_for():
    assert rp.case("permutation").n_replaced.max() == 0
    for name in ("boundary", "prototype", "shrink", "allzero", "background", "dense"):
        assert rp.case(name).n_replaced.max() >= 1, name
    c = rp.case("pairs")
    assert 4 <= c.n_replaced.max() and c.n_replaced.mean() >= 2
    filled = c.want[~c.kept]
    assert (filled.sum(axis=1) == 2).any()  # a fill past the six singletons
    c = rp.case("allzero")
    src = c.index >= 0
    assert (~c.ss[:, :, c.index[src]].any(axis=2)).any()  # a state that gathers to all-zero
    c = rp.case("dense")
    k = c.want.sum(axis=2)
    assert k.min() >= 1 and k.max() >= 9 and (k[c.kept] >= 5).all()
    c = rp.case("grow")
    assert c.n_replaced.max() == 0 and not c.want[:, :, c.index < 0].any()


def test_permutation_and_its_inverse_restore_kn():
    c = rp.case("permutation")
    fwd, n1 = remap_states_host(c.ss, c.index)
    inv = np.argsort(c.index).astype(np.int32)
    back, n2 = remap_states_host(fwd, inv)
    assert n1.max() == 0 and n2.max() == 0
    assert np.array_equal(back, c.ss)


def test_index_refusals():
    ss = rp.case("pairs").ss  # H = 8, S = 18
    for index, match in (([0, 1, 2, 3, 4, 4], "duplicate source latent 4"),
                         ([0, 1, 2, 3, 4, 8], "out of range"),
                         ([0, 1, 2, 3, 4, -2], "out of range"),
                         ([0, 1, 2], "fewer than S = 18"),
                         ([0, 1, 2, 3, 4], "fewer than S = 18")):  # 15 candidates
        with pytest.raises(ValueError, match=match):
            remap_states_host(ss, index)
    with pytest.raises(ValueError, match="fewer than S = 8"):
        check_remap_index([0, 1, 2], 8, 8)  # H' = 3, S = 8
    check_remap_index([0, 1, 2], 8, 6)
    with pytest.raises(ValueError, match="cannot take the background unit's place"):
        remap_states_host(ss, [0, 1, 2, 3, 4, 5, -1], background=True)
    with pytest.raises(ValueError, match="the background unit is not last"):
        remap_states_host(ss, [0, 1, 2, 7, 4, 5, 3], background=True)
    with pytest.raises(ValueError, match="fewer than S = 18"):
        remap_states_host(ss, [0, 1, 2, 3, 4, 7], background=True)  # Hv' = 5
    with pytest.raises(ValueError, match="one-dimensional integer"):
        remap_states_host(ss, [[0, 1]])
    with pytest.raises(ValueError, match="one-dimensional integer"):
        remap_states_host(ss, [0.0, 1.0])


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_remap_theta(algo):
    D, H = 7, 12
    rng = np.random.RandomState(3)
    theta = make_theta(rng, algo, D, H)
    theta["ljc"], theta["piH"] = 1.0, 2.0  # derived keys: dropped
    name = "bsc" if algo == "ebsc" else "sssc"
    index = np.array([5, -1, 0, 11, 3, -1, 7], dtype=np.int32)
    old, new = index >= 0, index < 0
    a = remap_theta(name, theta, index, rng=np.random.RandomState(9))
    b = remap_theta(name, theta, index, rng=np.random.RandomState(9))
    assert "ljc" not in a and "piH" not in a
    assert a["W"].shape == (D, 7) and np.array_equal(a["W"][:, old], theta["W"][:, index[old]])
    assert np.array_equal(a["W"], b["W"])  # the defaults are deterministic for a given rng
    sigma = theta["sigma"] if algo == "ebsc" else np.sqrt(theta["sigma2"])
    dev = a["W"][:, new] - theta["W"][:, index[old]].mean(axis=1)[:, None]
    assert 0.0 < np.abs(dev).max() < 6 * sigma / 4
    if algo == "ebsc":
        assert a["pi"] == theta["pi"] and a["sigma"] == theta["sigma"]
        model = BSC(D, 7, 5)
    else:
        assert a["sigma2"] == theta["sigma2"]
        for key in ("pies", "mus"):
            assert a[key].shape == (7,) and np.array_equal(a[key][old], theta[key][index[old]])
            assert np.array_equal(a[key][new], np.full(2, theta[key][index[old]].mean()))
        Psi = a["Psi"]
        assert Psi.shape == (7, 7) and np.array_equal(Psi, Psi.T)
        assert np.array_equal(Psi[np.ix_(old, old)], theta["Psi"][np.ix_(index[old], index[old])])
        assert np.array_equal(np.diag(Psi)[new], np.full(2, np.diag(theta["Psi"])[index[old]].mean()))
        off = Psi[new].copy()
        off[np.arange(2), np.flatnonzero(new)] = 0.0
        assert not off.any()  # new off-diagonal entries are 0
        model = SSSC(D, 7, 5)
    checked = model.check_params({k: (v.copy() if hasattr(v, "copy") else v) for k, v in a.items()})
    assert np.array_equal(checked["W"], a["W"])
    # given columns are taken as they are
    Wn = rng.normal(size=(D, 2))
    kw = {} if algo == "ebsc" else dict(pies_new=[0.1, 0.2], mus_new=[1.0, 2.0], Psi_diag_new=[3.0, 4.0])
    g = remap_theta(name, theta, index, W_new=Wn, **kw)
    assert np.array_equal(g["W"][:, new], Wn)
    if algo == "es3c":
        assert np.array_equal(g["pies"][new], [0.1, 0.2]) and np.array_equal(np.diag(g["Psi"])[new], [3.0, 4.0])
    with pytest.raises(ValueError, match="W_new must have shape"):
        remap_theta(name, theta, index, W_new=Wn[:, :1])
    with pytest.raises(ValueError, match="named twice"):
        remap_theta(name, theta, [0, 0])
    # a pure gather keeps every bit and draws nothing
    p = remap_theta(name, theta, np.arange(H)[::-1].copy(), rng=None)
    assert np.array_equal(p["W"], theta["W"][:, ::-1])


def test_prune_index():
    usage = np.array([0.3, 0.0, 0.2, 0.001, 0.2, 0.5])
    assert prune_index(usage, keep_min=0.01).tolist() == [0, 2, 4, 5]
    assert prune_index(usage, n_keep=3).tolist() == [0, 2, 5]  # the tie between 2 and 4 goes to the lower latent
    assert prune_index(usage, n_keep=2, n_new=2).tolist() == [0, 5, -1, -1]
    idx = prune_index(usage, keep_min=0.25, n_new=1, background=True)
    assert idx.tolist() == [0, -1, 5] and idx.dtype == np.int32
    assert prune_index(np.array([0.3, 0.0, 0.4, 0.0]), keep_min=0.1, background=True).tolist() == [0, 2, 3]
    for kw in ({}, {"keep_min": 0.1, "n_keep": 2}, {"n_keep": 7}):
        with pytest.raises(ValueError):
            prune_index(usage, **kw)
    check_remap_index(idx, 6, 3, background=True)


def test_latent_usage_host():
    rng = np.random.RandomState(4)
    N, S, H, S_perm = 9, 6, 10, 1
    ss = rp.distinct_states(rng, N, S, H, 0.3, S_perm=1)
    lpj = rng.normal(size=(N, S + S_perm)) * 3
    lpj[0, 2] = lpj[0, 4] = lpj[0].max() + 1.0  # a planted tie: the first column wins
    lpj[1, 0] = lpj[1].max() + 1.0              # the permanent state is the MAP state: counts nothing
    out = latent_usage_host(ss, lpj, S_perm)
    q = np.exp(lpj - lpj.max(axis=1)[:, None])
    q /= q.sum(axis=1)[:, None]
    want = np.zeros(H)
    counts = np.zeros(H, dtype=np.int64)
    for n in range(N):
        for s in range(S):
            want += q[n, s + S_perm] * ss[n, s]
        best = int(np.argmax(lpj[n]))
        if best >= S_perm:
            counts += ss[n, best - S_perm]
    np.testing.assert_allclose(out["usage"], want / N, rtol=1e-12, atol=0)
    assert out["map_count"].dtype == np.int64 and np.array_equal(out["map_count"], counts)
    assert out["N"] == N
    best = posterior_scores_host(lpj, ss, S_perm)["best"]
    assert best[0] == 2 and best[1] == 0


@pytest.mark.parametrize("cls", [BSC, SSSC])
def test_refusals_of_the_model_method(cls):
    """Refused before the device is touched (no engine exists on this host)."""
    D, H, S = 4, 8, 18
    rng = np.random.RandomState(1)
    algo = "ebsc" if cls is BSC else "es3c"
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, 5)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    suff = {"ss": rp.distinct_states(rng, 5, S, H, 0.3), "lpj": np.zeros((5, S)), "S_perm": 0,
            "permanent": {"background": False, "allzero": False, "singletons": False}}
    model = cls(D, H, S)
    for index, match in (([0, 1, 1, 2, 3, 4], "duplicate source"), ([0, 9], "out of range"), ([0, 1, 2], "fewer than S = 18")):
        with pytest.raises(ValueError, match=match):
            model.remap_latents(theta, suff, my_data, index)
    bg = dict(suff, permanent={"background": True, "allzero": False, "singletons": False})
    with pytest.raises(ValueError, match="background unit"):
        model.remap_latents(theta, bg, my_data, [0, 1, 2, 3, 4, 5, -1])
    with pytest.raises(ValueError, match="not last"):
        model.remap_latents(theta, bg, my_data, [0, 1, 2, 3, 7, 5, 6])
    assert model._engine is None

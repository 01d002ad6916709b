"""CPU checks of the incomplete-data problems (_masked_problems.py): every problem reaches the regime it is named for,
masks change the sums, a reference that is wrong at one of the edges differs from the oracle by at least a thousand times
the tolerance the GPU test holds, two independent references of the masked ES3C lpj agree, the H x H systems of the Theta
problems are well conditioned, and every oracle is quick."""
import functools
import time

import numpy as np
import pytest

import _masked_problems as mp

MARGIN = 1e3  # a wrong reference must miss the GPU tolerance by this factor


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(problem, oracle, seconds); es_grid: the lpj of every 7th datapoint only."""
    p = mp.make_problem(name)
    t = time.perf_counter()
    if name == "es_grid":
        o = {"lpj": mp.oracle_lpj(mp.rows_of(p, slice(None, None, mp.GRID_STRIDE)))}
    else:
        o = mp.oracle(p)
    return p, o, time.perf_counter() - t


def _excess(got, want, rtol):
    """max |got - want| in units of the GPU check's tolerance rtol * max(1, |want|max) (its atol; rtol * |want| <= atol)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / (rtol * max(1.0, float(np.abs(want).max())))


# ---- regimes -----------------------------------------------------------------------------------------------------------
def test_latent_census():
    k = mp.make_problem("es_h65_wide")["ss"].sum(axis=-1)
    assert ((k > 8) & (k <= 64)).sum() >= 50 and (k > 64).any() and (k <= 8).sum() >= 50, np.bincount(k.ravel())
    assert mp.make_problem("es_h65_wide")["H"] > 64 and mp.make_problem("bsc_perm")["H"] > 64  # two state words
    for name in ("es_d25", "es_d64", "es_d65", "es_d130", "es_keep"):  # the golden regime in K: both launches have work
        k = mp.make_problem(name)["ss"].sum(axis=-1)
        assert (k > 8).any() and (k <= 8).any(), name


def test_sizes_reach_their_edges():
    P = {n: mp.make_problem(n) for n in mp.PROBLEMS}
    assert P["es_grid"]["N"] * P["es_grid"]["S"] > 65536                       # the grid cap of the masked launches
    half = P["es_grid"]["N"] // 2
    assert max(half, P["es_grid"]["N"] - half) * P["es_grid"]["S"] < 65536     # ... which neither half reaches
    assert P["es_h64"]["N"] > 256 and P["es_h64"]["H"] % 64 == 0              # p.nblk = 2; sym_row0 = H
    assert all(P[n]["H"] % 64 != 0 for n in mp.ES_PROBLEMS if n != "es_h64")  # ... and the plain form everywhere else
    assert (P["es_d64"]["D"], P["es_d65"]["D"], P["es_d130"]["D"]) == (64, 65, 130)
    assert P["bsc_d25"]["D"] <= 64 < P["bsc_d65"]["D"] <= 128 and P["bsc_dR"]["D"] == 4 * 64 + 1  # R = 1, 2, 4
    assert P["bsc_s300"]["S"] > 256 and P["bsc_perm"]["S_perm"] == 1
    assert all(P[n]["S_perm"] == 0 for n in mp.PROBLEMS if n != "bsc_perm")


def test_tiny_problems():
    """es_h2 / bsc_h2: the shapes, S = 3 distinct states of the 4 in every datapoint, an observed entry in every datapoint,
    both latents in use, the in-update backup route for es_h2 (D = 8 H), and a finite oracle."""
    import _theta_problems as tp
    shapes = {n: tuple(mp.PROBLEMS[n][:8]) for n in mp.TINY}
    assert shapes == {"es_h2": ("es3c", "sparse", 37, 16, 2, 3, 0, "rand30"), "bsc_h2": ("ebsc", "sparse", 37, 9, 2, 3, 0, "rand30")}
    assert set(mp.TINY) <= set(mp.THETA_PROBLEMS)
    for name in mp.TINY:
        p, o, _ = _oracle(name)
        assert p["x_infr"].any(axis=1).all() and np.array_equal(p["x"], p["x_infr"]), name
        assert (~p["x_infr"]).any(), name
        for n in range(p["N"]):
            assert len({row.tobytes() for row in p["ss"][n]}) == p["S"], (name, n)
        assert p["ss"].any(axis=(0, 1)).all(), name
        assert np.isfinite(o["lpj"]).all() and all(np.isfinite(np.asarray(v)).all() for v in o["sums"].values()), name
        th = mp.oracle_update(p, o["sums"])
        assert all(np.isfinite(np.asarray(v)).all() for v in th.values()), name
    assert tp.backup_route(mp.make_problem("es_h2")) == "in_update" and tp.backup_route(mp.make_problem("bsc_h2")) == "side_kernel"
    assert mp.make_problem("es_h2")["H"] ** 2 <= tp.DP_SIGMA2 < tp.DP_COUNT  # sigma2 beyond the live threads


@pytest.mark.parametrize("name", list(mp.PROBLEMS))
def test_mask_pattern(name):
    p = mp.make_problem(name)
    xi, x, N, D = p["x_infr"], p["x"], p["N"], p["D"]
    assert xi.shape == x.shape == (N, D) and xi.dtype == x.dtype == np.bool_
    assert not (x & ~xi).any()  # the keep-mask never keeps what is not reliable
    q = mp.make_problem.__wrapped__(name)  # deterministic from the seed
    assert np.array_equal(q["x_infr"], xi) and np.array_equal(q["x"], x) and np.array_equal(q["Y"], p["Y"])
    if p["pattern"] == "edge":
        assert xi[mp.EDGE_COMPLETE].all() and xi[mp.EDGE_SINGLE].sum() == 1
        assert all(not xi[n].any() for n in mp.EDGE_EMPTY) and len(mp.EDGE_EMPTY) == 2
        others = np.arange(N) != mp.EDGE_COMPLETE
        assert not xi[others, mp.EDGE_COLUMN].any()
        rest = np.setdiff1d(np.arange(N), (mp.EDGE_COMPLETE, mp.EDGE_SINGLE) + mp.EDGE_EMPTY)
        assert 0.2 < 1.0 - xi[rest].mean() < 0.45  # rand30 (plus the dead column) elsewhere
        assert np.array_equal(x, xi)
    else:
        assert xi.any(axis=1).all()  # rows without a reliable entry belong to `edge` alone
    if p["pattern"] == "rand30":
        assert 0.25 < 1.0 - xi.mean() < 0.35 and np.array_equal(x, xi)
        assert (~xi).any(axis=1).mean() > 0.9
    if p["pattern"] == "block":
        for n in range(N):  # one contiguous run per row
            miss = np.flatnonzero(~xi[n])
            assert miss.size >= 1 and miss[-1] - miss[0] + 1 == miss.size, n
        if D >= 128:
            assert any((~xi[n, 64 * b:64 * b + 64]).all() for n in range(N) for b in range(D // 64))
        assert np.array_equal(x, xi)
    if p["pattern"] == "keep":
        assert 0.25 < 1.0 - xi.mean() < 0.35
        drop = (xi & ~x).sum() / float(xi.sum())
        assert 0.1 < drop < 0.3 and (xi & ~x).any(axis=1).mean() > 0.9  # x differs from x_infr in nearly every row
    if D > 64:  # something is hidden in the last trip of a 64-lane loop over D (else its tail proves nothing)
        assert (~xi[:, 64 * ((D - 1) // 64):]).any()


def test_hide():
    p = mp.make_problem("es_d25")
    for how in (0.0, np.nan, 1e300):
        Yh = mp.hide(p["Y"], p["x_infr"], how)
        assert np.array_equal(Yh[p["x_infr"]], p["Y"][p["x_infr"]])
        hidden = Yh[~p["x_infr"]]
        assert np.isnan(hidden).all() if how != how else (hidden == how).all()
    assert np.array_equal(mp.hide(p["Y"], p["x_infr"], 0.0), p["Y0"])


# ---- masks are not a no-op ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["es_d65", "bsc_d65"])
def test_masks_change_the_sums(name):
    from oracle import evo_oracle as orc
    p, o, _ = _oracle(name)
    N, D, H, S, Y, ss = p["N"], p["D"], p["H"], p["S"], p["Y"], p["ss"]
    full = mp.oracle(p, x_infr=np.ones((N, D), dtype=bool), x=np.ones((N, D), dtype=bool), Y=Y)
    th = dict(p["theta"])
    if p["algo"] == "es3c":
        suff = {"ss": ss, "lpj": np.empty((N, S)), "S_perm": 0, "incl": np.zeros((0, H), dtype=bool), "Mprime": S}
        want = orc.sssc_EM_accumulate(th, suff, Y, use_storage=True, evolve=False)
        names = [k for k in mp.ES_NAMES if k != "pad"]
        assert "pad" not in full["sums"]
    else:
        cnt = orc.bsc_precompute(th, D, H)
        lpj = np.array([orc.bsc_lpj(th, ss[n], Y[n], cnt) for n in range(N)])
        suff = {"ss": ss, "lpj": lpj, "S_perm": 0, "permanent": {"allzero": False, "background": False}}
        want = dict(orc.bsc_accumulate(th, suff, Y), Fs=orc.free_energy_sum(lpj))
        names = mp.BSC_NAMES
    np.testing.assert_array_equal(full["lpj"], suff["lpj"])
    for k in names:
        if p["algo"] == "es3c" and k != "Fs":  # (use_storage only memoises: the same operations, the same bits)
            np.testing.assert_array_equal(full["sums"][k], want[k], err_msg=k)
        else:
            np.testing.assert_allclose(full["sums"][k], want[k], rtol=1e-14, atol=0, err_msg=k)
        rel = np.abs(np.asarray(o["sums"][k]) - np.asarray(want[k])).max() / np.abs(np.asarray(want[k])).max()
        assert rel > 1e-3, (k, rel)


# ---- sensitivity: a reference wrong at one edge is rejected -----------------------------------------------------------
@pytest.mark.parametrize("name", ["es_d65", "es_d130", "bsc_d65", "bsc_dR"])
def test_sensitive_to_a_mask_ignored_beyond_64_columns(name):
    p, o, _ = _oracle(name)
    bad = mp.oracle_lpj(p, mp.mask_ignored_from(p["x_infr"], 64))
    assert _excess(bad, o["lpj"], mp.LPJ_RTOL) >= MARGIN
    if name == "bsc_dR":  # ... and from the second slab of 64 R = 256 observables on
        assert _excess(mp.oracle_lpj(p, mp.mask_ignored_from(p["x_infr"], 256)), o["lpj"], mp.LPJ_RTOL) >= MARGIN
    if name == "es_d130":  # ... and in the ragged third trip alone
        assert _excess(mp.oracle_lpj(p, mp.mask_ignored_from(p["x_infr"], 128)), o["lpj"], mp.LPJ_RTOL) >= MARGIN


def test_sensitive_to_the_complete_gram_above_8_latents():
    p, o, _ = _oracle("es_h65_wide")
    bad = mp.lpj_complete_gram_above(p, 9)
    k = p["ss"].sum(axis=-1)
    assert np.array_equal(bad[k <= 8], o["lpj"][k <= 8])
    assert _excess(bad, o["lpj"], mp.LPJ_RTOL) >= MARGIN
    # the Gram form itself (masked Gram) is a third restatement of the oracle's value
    n, s = np.argwhere(k >= 9)[0]
    good = mp.lpj_gram(p["theta"], p["Y0"][n], p["x_infr"][n], p["ss"][n, s])
    np.testing.assert_allclose(good, o["lpj"][n, s], rtol=1e-11)


@pytest.mark.parametrize("name", ["es_keep", "bsc_keep"])
def test_sensitive_to_x_infr_in_the_place_of_x(name):
    p, o, _ = _oracle(name)
    bad = mp.oracle(p, x=p["x_infr"])
    np.testing.assert_array_equal(bad["lpj"], o["lpj"])  # (x enters the reconstruction alone)
    assert _excess(bad["y_reconstructed"], o["y_reconstructed"], mp.SUM_RTOL) >= MARGIN
    assert _excess(bad["sums"]["Wp"], o["sums"]["Wp"], mp.SUM_RTOL) >= MARGIN
    if name == "bsc_keep":  # bsc.py:187,214-216: sigma's residual reads y_reconstructed at the reliable entries, so a
        # reliable entry that x drops enters with its estimate, not with its datum
        assert _excess(bad["sums"]["sigma"], o["sums"]["sigma"], mp.SUM_RTOL) >= MARGIN
    else:  # sssc.py:748: sigma2 reads the data
        assert bad["sums"]["pad"] == o["sums"]["pad"]
        np.testing.assert_array_equal(bad["sums"]["y_outer_diag"], o["sums"]["y_outer_diag"])


def test_sensitive_to_the_allzero_term_of_sigma():
    p, o, _ = _oracle("bsc_perm")
    assert _excess(mp.sigma_without_allzero(p, o), o["sums"]["sigma"], mp.SUM_RTOL) >= MARGIN


@pytest.mark.parametrize("name", mp.THETA_PROBLEMS)
def test_sensitive_to_the_count_of_reliable_entries(name):
    p, o, _ = _oracle(name)
    key = "sigma2" if p["algo"] == "es3c" else "sigma"
    good = mp.oracle_update(p, o["sums"])
    bad = mp.oracle_update(p, o["sums"], n_reliable=p["N"] * p["D"])
    tol = mp.THETA_RTOL * abs(good[key]) + mp.THETA_ATOL * max(1.0, abs(good[key]))
    assert abs(bad[key] - good[key]) >= 10 * MARGIN * tol, (good[key], bad[key])  # (10 x: the looser of the two checks)
    # ... and ljc: the reliable fraction, not D, multiplies the Gaussian normaliser
    th = dict(good)
    sc = mp.new_scalars(p, good)
    from oracle import evo_oracle as orc
    if p["algo"] == "es3c":
        orc.sssc_precompute(th, p["D"])
    else:
        orc.bsc_precompute(th, p["D"], p["H"])
    assert abs(float(th["ljc"]) - sc["ljc"]) >= 10 * MARGIN * (mp.THETA_RTOL + mp.THETA_ATOL) * max(1.0, abs(sc["ljc"]))


# ---- two references agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["es_d65", "es_h65_wide"])
def test_independent_lpj_agrees_with_the_oracle(name):
    from oracle import evo_oracle as orc
    p, o, _ = _oracle(name)
    th = dict(p["theta"])
    cnt = orc.sssc_precompute(th, p["D"], p["x_infr"])
    worst = 0.0
    for n in range(p["N"]):
        obs = p["x_infr"][n]
        want = orc.sssc_lpj(th, p["ss"][n], p["Y0"][n], cnt, {}, obs=obs)
        np.testing.assert_array_equal(want, o["lpj"][n])
        got = np.array([mp.lpj_direct(p["theta"], p["Y"][n], obs, st) for st in p["ss"][n]])
        worst = max(worst, float(np.abs(got / want - 1.0).max()))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg="%s n = %d" % (name, n))
    print("%s: worst relative difference %.2e" % (name, worst))
    assert not any(cnt.values())  # no clamp took part


def test_prior_only_rows():
    for name in ("es_d25", "bsc_d25"):
        p, o, _ = _oracle(name)
        for n in mp.EDGE_EMPTY:
            np.testing.assert_allclose(o["lpj"][n], mp.prior_only_lpj(p, n), rtol=1e-13, atol=1e-13)


# ---- conditioning, time ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mp.THETA_PROBLEMS)
def test_theta_problems_are_well_conditioned(name):
    p, o, _ = _oracle(name)
    conds = mp.update_conditions(p, o["sums"])
    print(name, {k: "%.3g" % v for k, v in conds.items()})
    assert all(v <= mp.COND_CAP for v in conds.values()), conds


@pytest.mark.parametrize("name", list(mp.PROBLEMS))
def test_oracle_is_quick(name):
    _, o, seconds = _oracle(name)
    assert np.isfinite(o["lpj"]).all()
    assert seconds < 10.0, seconds

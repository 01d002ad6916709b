"""The E-step half of an iteration against the float64 oracle across its routes: vary_kn_kernel in all ten <SPL, CPL>
instantiations with digest and word de-duplication and S_perm 0 / 1 (bit for bit against oracle.vary_Kn), its tie rule,
the row statistics it leaves for the next statistics pass, the candidate lpj kernels (EBSC Gram / gram2 / direct, the
ES3C chain levels), the device flow (evolve_randflip -> vary_kn with more than 64 children) and the fused E-step against
the separate passes at S up to 1024, and every S class of the launch dispatch (with_spl) through the randflip kernel, the
selection and the fused kernel.  Problems are synthetic (_estep_problems.py)."""
import functools

import numpy as np
import pytest

import _estep_problems as ep

pytestmark = pytest.mark.gpu

LPJ_RTOL = 1e-9
SUM_RTOL = 1e-9
ES_NAMES = ("xpt_s", "xpt_ss", "xpt_sz", "xpt_szsz", "Wp", "s_sz_outer", "sz_sz_outer", "y_outer_diag", "Fs")
BSC_NAMES = ("Wp", "Wq", "pies", "sigma", "Fs")
DATA_CASES = [n for n, v in ep.SELECTION.items() if v[7]]


@pytest.fixture(scope="module")
def engine():
    from evo_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


def _close(a, b, rtol, name=""):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, err_msg=name)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Selection problem with its values (the oracle's lpj for problems with data); once per module."""
    p = ep.make_problem(name)
    if p["data"]:
        ep.attach_oracle_values(p)
    return p


@functools.lru_cache(maxsize=None)
def _want(name, Mprime):
    return ep.oracle_select(_problem(name), Mprime)


def _assert_tie_free(p, lpj, cand_lpj, label):
    """oracle.vary_Kn orders equal values as NumPy's partition does: bit parity needs distinct values per row."""
    for n in range(p["N"]):
        v = np.concatenate([lpj[n, p["S_perm"]:], cand_lpj[n, ep.survivors(p, n)]])
        assert np.unique(v).size == v.size, "%s: tied values in datapoint %d" % (label, n)


def _configure(engine, p, state_digest=1):
    engine.set_option("state_digest", state_digest)  # read by evoamd_configure
    engine.configure(p["model"], p["N"], p["D"], p["H"], p["S"], p["S_perm"], p["Cmax"])
    if "Y" in p:
        engine.upload_data(p["Y"])
        th = p["theta"]
        if p["model"] == "sssc":
            engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
        else:
            engine.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))


def _select(engine, p, Mprime):
    """upload K^n, its lpj and the candidate batch, then vary_kn: (K^n, lpj, (n_unique, n_sub) summed over N)."""
    engine.upload_states(p["ss"])
    engine.upload_lpj(p["lpj"])
    engine.set_candidates(p["cand"], p["counts"], p["cand_lpj"])
    engine.set_estep_counts(0.0, 0.0)  # (vary_kn adds its counts to these)
    sums = engine.vary_kn(Mprime)
    return engine.download_states(), engine.download_lpj(), tuple(sums)


@pytest.mark.parametrize("name", list(ep.SELECTION))
def test_selection_matches_oracle(engine, name):
    """K^n, the lpj row and (n_unique, n_sub) bit for bit against oracle.vary_Kn at Mprime in {1, S / 3, S}, with
    digest de-duplication and with word de-duplication; the two runs must agree."""
    p = _problem(name)
    _assert_tie_free(p, p["lpj"], p["cand_lpj"], name)
    got = {}
    try:
        for d in (1, 0):
            _configure(engine, p, d)
            for Mp in ep.mprimes(p["S"]):
                got[d, Mp] = _select(engine, p, Mp)
    finally:
        engine.set_option("state_digest", 1)
    for (d, Mp), (ss, lpj, sums) in got.items():
        w_ss, w_lpj, nu, ns = _want(name, Mp)
        label = "%s digest=%d Mprime=%d" % (name, d, Mp)
        bad = np.flatnonzero((ss != w_ss).any(axis=(1, 2)))
        assert bad.size == 0, "%s: K^n differs in datapoints %s" % (label, bad[:8])
        assert np.array_equal(lpj, w_lpj), label + ": lpj row differs"
        assert sums == (float(nu), float(ns)), (label, sums, nu, ns)
    for Mp in ep.mprimes(p["S"]):
        a, b = got[1, Mp], got[0, Mp]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], (name, Mp)


@pytest.mark.parametrize("name", list(ep.TIES))
def test_selection_ties_follow_the_documented_rule(engine, name):
    """Integer lpj values: candidates tie with each other and with old states.  The kernel must follow its documented
    rule exactly (swap j iff the j-th best candidate is strictly greater than the j-th worst old state; among equal
    values the lower index first).  Against the oracle, whose tie order is NumPy's: the same lpj multiset per row and the
    same counts; rows stay distinct and every (state, lpj) pair comes from the input."""
    p = _problem(name)
    N, S, S_perm = p["N"], p["S"], p["S_perm"]
    try:
        for d in (1, 0):
            _configure(engine, p, d)
            for Mp in ep.mprimes(S):
                ss, lpj, sums = _select(engine, p, Mp)
                label = "%s digest=%d Mprime=%d" % (name, d, Mp)
                w_ss, w_lpj, nu, ns = _want(name, Mp)
                assert sums == (float(nu), float(ns)), (label, sums, nu, ns)
                assert np.array_equal(lpj[:, :S_perm], p["lpj"][:, :S_perm]), label
                for n in range(N):
                    c = int(p["counts"][n])
                    r_ss, r_lpj, _, _ = ep.select_rule(p["ss"][n], p["lpj"][n, S_perm:], p["cand"][n, :c],
                                                       p["cand_lpj"][n, :c], c, Mp, S_perm)
                    assert np.array_equal(ss[n], r_ss), "%s: K^n of datapoint %d breaks the rule" % (label, n)
                    assert np.array_equal(lpj[n, S_perm:], r_lpj), "%s: lpj of datapoint %d" % (label, n)
                    assert np.array_equal(np.sort(lpj[n]), np.sort(w_lpj[n])), (label, n)
                    assert len({r.tobytes() for r in ss[n]}) == S, (label, n)
                    pairs = {(p["ss"][n, s].tobytes(), p["lpj"][n, S_perm + s]) for s in range(S)}
                    pairs |= {(p["cand"][n, j].tobytes(), p["cand_lpj"][n, j]) for j in range(c)}
                    assert all((ss[n, s].tobytes(), lpj[n, S_perm + s]) in pairs for s in range(S)), (label, n)
    finally:
        engine.set_option("state_digest", 1)


def _oracle_sums(p, ss, lpj):
    """M-step sums and Fs of the float64 oracle for K^n `ss` with lpj row `lpj` (its values are the oracle's)."""
    from oracle import evo_oracle as orc
    N, D, H, S, S_perm, Y = p["N"], p["D"], p["H"], p["S"], p["S_perm"], p["Y"]
    if p["model"] == "sssc":
        suff = {"ss": ss, "lpj": np.empty((N, S_perm + S)), "S_perm": S_perm, "incl": np.zeros((S_perm, H), dtype=bool),
                "Mprime": S}
        want = dict(orc.sssc_EM_accumulate(dict(p["theta"]), suff, Y, use_storage=True, evolve=False))
        _close(suff["lpj"], lpj, LPJ_RTOL, p["name"] + ": the oracle's own lpj of the new K^n")
        lpj = suff["lpj"]
    else:
        th = dict(p["theta"])
        orc.bsc_precompute(th, D, H)
        suff = {"ss": ss, "lpj": lpj, "S_perm": S_perm, "permanent": {"allzero": bool(S_perm), "background": False}}
        want = dict(orc.bsc_accumulate(th, suff, Y))
    want["Fs"] = orc.free_energy_sum(lpj)
    return want


@pytest.mark.parametrize("name", DATA_CASES)
def test_row_statistics_after_selection(engine, name):
    """stats() right after vary_kn reads the row maximum, sum and free-energy term the selection kernel wrote
    (rows_fresh): Fs and every accumulator against the oracle on the post-selection K^n."""
    p = _problem(name)
    Mp = ep.mprimes(p["S"])[1]
    _configure(engine, p, 1)
    ss, lpj, sums = _select(engine, p, Mp)
    w_ss, w_lpj, nu, ns = _want(name, Mp)
    assert np.array_equal(ss, w_ss) and np.array_equal(lpj, w_lpj), name
    assert not np.array_equal(ss, p["ss"]), name + ": nothing was swapped"
    v = engine.acc_views(engine.stats())
    want = _oracle_sums(p, w_ss, w_lpj)
    for k in (ES_NAMES if p["model"] == "sssc" else BSC_NAMES):
        _close(v[k], want[k], SUM_RTOL, "%s: %s" % (name, k))
    assert float(v["sum_nunique"]) == nu and float(v["sum_sub"]) == ns and float(v["N"]) == p["N"], name


@pytest.mark.parametrize("name", list(ep.CAND_LPJ))
def test_candidate_lpj_matches_oracle(engine, name):
    """evoamd_lpj_candidates (tag 1) on ragged batches against bsc_lpj / sssc_lpj; entries at c >= counts[n] are not
    compared."""
    p = ep.make_cand_problem(name)
    opts = p["opts"]
    try:
        engine.set_option("state_digest", opts.get("state_digest", 1))
        engine.configure(p["model"], p["N"], p["D"], p["H"], p["S"], 0, p["Cmax"])
        if p["model"] == "bsc":
            engine.set_option("bsc_direct", opts.get("bsc_direct", 0))  # (before set_params: it decides what is derived)
        engine.upload_data(p["Y"])
        engine.upload_states(p["ss"])
        th = p["theta"]
        if p["model"] == "sssc":
            engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
        else:
            engine.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))
        got = engine.lpj_candidates(p["cand"], p["counts"])
    finally:
        engine.set_option("state_digest", 1)
        engine.set_option("bsc_direct", 0)
    for n in range(p["N"]):
        c = int(p["counts"][n])
        want = ep.oracle_lpj(p, p["cand"][n:n + 1, :c], n)[0]
        _close(got[n, :c], want, LPJ_RTOL, "%s: datapoint %d" % (name, n))


@pytest.mark.parametrize("name", list(ep.DEVICE_FLOW))
def test_device_flow_selection(engine, name):
    """evolve_randflip with more than 64 children per datapoint (the <., 4> instantiation in the real flow): the
    downloaded candidates' lpj against the oracle, then vary_kn against oracle.vary_Kn run on the device's own lpj values
    (rounding cannot decide a swap) -- K^n bit for bit; this covers the digests the device wrote for its children."""
    from oracle import evo_oracle as orc
    N, D, H, S, npar, nch, Mp, seed = ep.DEVICE_FLOW[name]
    rng = np.random.RandomState(seed)
    ss = ep.make_kn(rng, N, S, H)
    p = {"name": name, "model": "bsc", "N": N, "D": D, "H": H, "S": S, "S_perm": 0, "Cmax": npar * nch,
         "Y": rng.normal(size=(N, D)), "theta": ep.bsc_theta(rng, D, H), "ss": ss}
    _configure(engine, p, 1)
    engine.upload_states(ss)
    engine.lpj_resident()
    lpj0 = engine.download_lpj()
    _close(lpj0, ep.oracle_lpj(p, ss), LPJ_RTOL, name + ": lpj of K^n")
    engine.evolve_randflip(npar, nch, seed)
    cand, counts, cl = engine.download_candidates()
    assert counts.max() > 64, (name, counts)
    p.update(cand=cand, counts=counts)
    for n in range(N):
        c = int(counts[n])
        _close(cl[n, :c], ep.oracle_lpj(p, cand[n:n + 1, :c], n)[0], LPJ_RTOL, "%s: candidate lpj of %d" % (name, n))
    _assert_tie_free(p, lpj0, cl, name)
    want_ss, want_lpj = ss.copy(), lpj0.copy()
    nu = ns = 0
    for n in range(N):
        c = int(counts[n])
        a, b = orc.vary_Kn(lpj0[n].copy(), cl[n, :c].copy(), want_lpj[n], want_ss[n], cand[n, :c], H, S, 0,
                           np.zeros((0, H), dtype=bool), Mp)
        nu += a
        ns += b
    engine.set_estep_counts(0.0, 0.0)
    sums = engine.vary_kn(Mp)
    got = engine.download_states()
    assert ns > 0, name
    assert np.array_equal(got, want_ss), "%s: K^n differs in datapoints %s" % (
        name, np.flatnonzero((got != want_ss).any(axis=(1, 2))))
    assert np.array_equal(engine.download_lpj(), want_lpj), name
    assert tuple(sums) == (float(nu), float(ns)), (name, sums, nu, ns)


def _fused_run(engine, p, fused_opt, npar, nch, Mp, seed, fit):
    engine.set_option("fused_estep", fused_opt)
    engine.upload_states(p["ss"])
    engine.lpj_resident()
    engine.stats()  # (the census the automatic choice and the level plan read; same prefix in both runs)
    before = engine.estep_counters()
    ran = engine.estep(npar, nch, seed, fit, Mp)
    after = engine.estep_counters()
    ss, lpj = engine.download_states(), engine.download_lpj()
    acc = engine.stats()
    return ran, before, after, ss, lpj, acc


@pytest.mark.parametrize("name", list(ep.FUSED))
def test_fused_estep_matches_separate_passes(engine, name):
    """The fused E-step forced on, then off, from the same ES3C K^n, Theta and device seed: K^n and lpj bit for bit, the
    counters and Fs of the following statistics pass equal, its accumulators to 1e-12 (f64 atomics: reproducible to the
    last bits only).  estep_counters must show which path ran; the dense cases (random parents) must send datapoints to
    the second launch (kc_big = SSSC_KCAP)."""
    N, D, H, S, npar, nch, Mp, dense, seed = ep.FUSED[name]
    rng = np.random.RandomState(seed)
    p = {"model": "sssc", "N": N, "D": D, "H": H, "S": S, "S_perm": 0, "Cmax": npar * nch,
         "Y": rng.normal(size=(N, D)), "theta": ep.es3c_theta(rng, D, H),
         "ss": ep.make_kn(rng, N, S, H, dense_every=2 if dense else 0)}
    _configure(engine, p, 1)
    # (one arithmetic per state in both runs: the separate passes would merge the 5..8 level into the wavefront kernel)
    engine.set_option("merge_small_levels", 0)
    try:
        on = _fused_run(engine, p, 2, npar, nch, Mp, seed, not dense)
        off = _fused_run(engine, p, 0, npar, nch, Mp, seed, not dense)
    finally:
        engine.set_option("fused_estep", 0)
        engine.set_option("merge_small_levels", 1)
    assert on[0] is True and on[2]["fused_calls"] == on[1]["fused_calls"] + 1, (name, on[1], on[2])
    assert on[2]["separate_calls"] == on[1]["separate_calls"], name
    assert off[0] is False and off[2]["separate_calls"] == off[1]["separate_calls"] + 1, (name, off[1], off[2])
    if dense:
        assert on[2]["deferred"] > 0, (name, on[2])
    assert not np.array_equal(on[3], p["ss"]), name + ": the E-step changed nothing"
    assert np.array_equal(on[3], off[3]), "%s: K^n differs in datapoints %s" % (
        name, np.flatnonzero((on[3] != off[3]).any(axis=(1, 2))))
    same = on[4] == off[4]
    assert same.all(), "%s: lpj differs in %d entries" % (name, (~same).sum())
    va, vb = engine.acc_views(on[5]), engine.acc_views(off[5])
    for k in ("Fs", "sum_nunique", "sum_sub", "N"):
        assert float(va[k]) == float(vb[k]), (name, k, float(va[k]), float(vb[k]))
    scale = max(1.0, float(np.abs(off[5]).max()))
    assert np.abs(on[5] - off[5]).max() <= 1e-12 * scale, name


@pytest.mark.parametrize("name", list(ep.SPL_FLOW))
def test_every_s_class_through_randflip_selection_and_fused(engine, name):
    """with_spl, one case per S class (ES3C, at most 64 children): evolve_randflip -> vary_kn against oracle.vary_Kn run on
    the device's own lpj values, K^n, lpj and the counters bit for bit; then the fused E-step from the same K^n and seed
    must give that K^n and lpj row bit for bit as well."""
    from oracle import evo_oracle as orc
    N, D, H, S, npar, nch, Mp, seed = ep.SPL_FLOW[name]
    rng = np.random.RandomState(seed)
    p = {"name": name, "model": "sssc", "N": N, "D": D, "H": H, "S": S, "S_perm": 0, "Cmax": npar * nch,
         "Y": rng.normal(size=(N, D)), "theta": ep.es3c_theta(rng, D, H), "ss": ep.make_kn(rng, N, S, H)}
    _configure(engine, p, 1)
    engine.set_option("merge_small_levels", 0)  # (one arithmetic per state in both runs, as in the test above)
    try:
        engine.upload_states(p["ss"])
        engine.lpj_resident()
        engine.stats()  # (the same prefix as _fused_run)
        lpj0 = engine.download_lpj()
        engine.evolve_randflip(npar, nch, seed)
        cand, counts, cl = engine.download_candidates()
        p.update(cand=cand, counts=counts)
        _assert_tie_free(p, lpj0, cl, name)
        want_ss, want_lpj = p["ss"].copy(), lpj0.copy()
        nu = ns = 0
        for n in range(N):
            c = int(counts[n])
            a, b = orc.vary_Kn(lpj0[n].copy(), cl[n, :c].copy(), want_lpj[n], want_ss[n], cand[n, :c], H, S, 0,
                               np.zeros((0, H), dtype=bool), Mp)
            nu += a
            ns += b
        engine.set_estep_counts(0.0, 0.0)
        sums = engine.vary_kn(Mp)
        got_ss, got_lpj = engine.download_states(), engine.download_lpj()
        on = _fused_run(engine, p, 2, npar, nch, Mp, seed, True)
    finally:
        engine.set_option("fused_estep", 0)
        engine.set_option("merge_small_levels", 1)
    assert ns > 0, name
    assert np.array_equal(got_ss, want_ss), "%s: K^n differs in datapoints %s" % (
        name, np.flatnonzero((got_ss != want_ss).any(axis=(1, 2))))
    assert np.array_equal(got_lpj, want_lpj), name
    assert tuple(sums) == (float(nu), float(ns)), (name, sums, nu, ns)
    assert on[0] is True, name + ": the fused kernel did not run"
    assert np.array_equal(on[3], want_ss), "%s (fused): K^n differs in datapoints %s" % (
        name, np.flatnonzero((on[3] != want_ss).any(axis=(1, 2))))
    assert np.array_equal(on[4], want_lpj), name + " (fused)"

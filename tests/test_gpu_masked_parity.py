"""Incomplete data (x_infr with False entries) against the float64 oracle: the masked lpj of both models (resident K^n,
candidate batch, single datapoint), every block of the masked statistics accumulator, y_reconstructed, and the Theta
update with its count of reliable entries.  Problems, their edges and the wrong-reference proofs: _masked_problems.py
and test_masked_problems.py.  Every comparison prints its worst error in units of max(1, |reference|max)."""
import functools

import numpy as np
import pytest

import _masked_problems as mp

pytestmark = pytest.mark.gpu

CMAX = 12  # candidates per datapoint the engine is configured for
ALL = list(mp.PROBLEMS)
WHOLE = [n for n in ALL if n != "es_grid"]  # es_grid: the halves test below
EDGE = ("es_d25", "bsc_d25")
DEFAULTS = {"bsc_stats_wave": 1, "pair_bins": 1, "sssc_precision": 64, "ebsc_f32": 0}


@pytest.fixture(scope="module")
def engine():
    from evo_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


@functools.lru_cache(maxsize=None)
def _reference(name):
    p = mp.make_problem(name)
    return p, mp.oracle(p)


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not want.size:
        return 0.0
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _close(got, want, rtol, what, atol=None):
    """assert_allclose with atol = (atol or rtol) * max(1, |want|max); prints the error it saw first."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print("PARITY %-60s err %.3e  (rtol %.0e)" % (what, _err(got, want), rtol))
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=(rtol if atol is None else atol) * scale, err_msg=what)


def _names(p):
    return mp.ES_NAMES if p["algo"] == "es3c" else mp.BSC_NAMES


def _set_params(engine, p, theta=None):
    th = p["theta"] if theta is None else theta
    if p["algo"] == "es3c":
        return engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    return engine.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))


def _setup(engine, p, Y=None, masks=True):
    """The call order of evo_amd/models/_models.py up to the parameters."""
    engine.configure("sssc" if p["algo"] == "es3c" else "bsc", p["N"], p["D"], p["H"], p["S"], p["S_perm"], min(CMAX, p["S"]))
    engine.upload_data(p["Y0"] if Y is None else Y)
    if masks:
        engine.upload_masks(p["x_infr"], p["x"])
        engine.set_reliable_fraction(p["x_infr"].sum() / float(p["N"]))
    engine.upload_states(p["ss"])
    return _set_params(engine, p)


def _stats(engine, reconstruct=True):
    if reconstruct:
        engine.set_option("reconstruct_in_stats", 1)
    return {k: np.array(v) for k, v in engine.acc_views(engine.stats()).items()}


def _run(engine, p, Y=None):
    """(ljc, lpj, accumulator views, y_hat) of one masked pass."""
    ljc = _setup(engine, p, Y)
    engine.lpj_resident()
    lpj = engine.download_lpj()
    v = _stats(engine)
    return ljc, lpj, v, engine.reconstruct()


def _select(p, y_hat):
    """y_reconstructed from the device's estimate by the reference's rule: the estimate where x is False; EBSC skips a
    datapoint without a reliable entry (_models.py:648-649), ES3C's own loop does not (sssc.py:613-627).  These are the
    rows the M-step's Wp reads (select_rec_kernel), which the Wp block checks; the array a model hands to its caller
    keeps such a datapoint as it is for both models (test_patch_without_reliable_entry_keeps_nan)."""
    miss = ~p["x"]
    if p["algo"] == "ebsc":
        miss = miss & p["x_infr"].any(axis=1)[:, None]
    return np.where(miss, y_hat, p["Y0"])


def _no_clamp(v, what):
    assert (v["reset_isnan"], v["reset_smaller_eps"], v["reset_isinf"]) == (0.0, 0.0, 0.0), what


def _clear(engine):
    if engine.has_masks:
        engine.upload_masks(None)
    engine.set_reliable_fraction(None)


# ---- lpj ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WHOLE)
def test_lpj_statistics_and_reconstruction(engine, name):
    """download_lpj, every named block of the accumulator and y_reconstructed against the oracle."""
    p, o = _reference(name)
    try:
        ljc, lpj, v, y_hat = _run(engine, p)
    finally:
        _clear(engine)
    _close(ljc, o["ljc"], mp.LPJ_RTOL, name + ": ljc")
    _close(lpj, o["lpj"], mp.LPJ_RTOL, name + ": lpj")
    for k in _names(p):
        _close(v[k], o["sums"][k], mp.SUM_RTOL, "%s: %s" % (name, k))
    assert v["N"] == p["N"]
    _no_clamp(v, name)
    _close(_select(p, y_hat), o["y_reconstructed"], mp.SUM_RTOL, name + ": y_reconstructed")
    if p["algo"] == "es3c":  # the masked column sums, said once more without the oracle
        _close(v["y_outer_diag"], (p["Y0"] ** 2).sum(axis=0), mp.BASE_RTOL, name + ": y_outer_diag vs column sums")
    if p["pattern"] == "edge":
        for n in mp.EDGE_EMPTY:  # no reliable entry: the prior alone
            _close(lpj[n], mp.prior_only_lpj(p, n), mp.BASE_RTOL, "%s: prior-only row %d" % (name, n))


@pytest.mark.parametrize("name", ALL)
def test_lpj_candidates(engine, name):
    """The first states of every K^n row sent as a ragged candidate batch."""
    p = mp.make_problem(name)
    if name == "es_grid":
        rows = np.arange(0, p["N"], mp.GRID_STRIDE)
        want = mp.oracle_lpj(mp.rows_of(p, rows))
    else:
        rows, want = np.arange(p["N"]), _reference(name)[1]["lpj"]
    C = min(CMAX, p["S"])
    counts = (1 + (np.arange(p["N"]) * 5) % C).astype(np.int32)
    counts[0], counts[p["N"] - 1] = C, 0
    cand = np.ascontiguousarray(p["ss"][:, :C])
    try:
        _setup(engine, p)
        got = engine.lpj_candidates(cand, counts)
    finally:
        _clear(engine)
    valid = np.arange(C)[None, :] < counts[rows][:, None]
    assert valid.sum() >= 2 * len(rows)  # (equal at C = 3, N = 37: the counts 1, 3, 2 in turn, the first 3, the last 0)
    _close(got[rows][valid], want[:, p["S_perm"]:p["S_perm"] + C][valid], mp.LPJ_RTOL, name + ": candidate lpj")


@pytest.mark.parametrize("name", EDGE)
def test_lpj_single_rows(engine, name):
    """The single-datapoint operator on the complete row, the row with one reliable entry and a row with none; the
    hidden entries are NaN in what it is handed."""
    p, o = _reference(name)
    Yn = mp.hide(p["Y"], p["x_infr"], np.nan)
    try:
        _setup(engine, p)
        for n in (mp.EDGE_COMPLETE, mp.EDGE_SINGLE, mp.EDGE_EMPTY[0]):
            got, flags = engine.lpj_single(Yn[n], p["ss"][n], x_infr=p["x_infr"][n])
            _close(got, o["lpj"][n, p["S_perm"]:], mp.LPJ_RTOL, "%s: lpj_single row %d" % (name, n))
            assert not flags.any(), (name, n, flags)
    finally:
        _clear(engine)


def test_es3c_lpj_single_without_resident_masks(engine):
    """SSSC.log_pseudo_joint hands a row of x_infr to an engine that holds no masks (the per-datapoint operator of a model
    configured for one datapoint): the W^T its per-datapoint Gram blocks read must exist and belong to this Theta."""
    p, o = _reference("es_d65")
    _setup(engine, p, masks=False)
    n = 3
    got, flags = engine.lpj_single(p["Y0"][n], p["ss"][n], x_infr=p["x_infr"][n])
    _close(got, o["lpj"][n], mp.LPJ_RTOL, "es_d65: lpj_single row %d, no resident masks" % n)
    th = dict(p["theta"], W=p["theta"]["W"] * 1.25)  # a second Theta on the same context: W^T follows it
    _set_params(engine, p, th)
    got, _ = engine.lpj_single(p["Y0"][n], p["ss"][n], x_infr=p["x_infr"][n])
    _close(got, mp.oracle_lpj(dict(p, theta=th))[n], mp.LPJ_RTOL, "es_d65: the same after new parameters")
    assert not flags.any()


# ---- hidden values never enter -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["es_d25", "es_d65", "es_h65_wide", "es_keep", "bsc_d25", "bsc_d65", "bsc_perm", "bsc_s300"])
def test_hidden_values_never_enter(engine, name):
    """0, NaN and 1e300 under the mask: bit-identical lpj; the statistics equal up to the order in which atomics add.
    No atomic feeds Fs (a fixed-order reduction of the lpj rows) or, with one block of 256 rows, the squared column sums
    (one add per column onto zero); everything else passes through unsafeAtomicAdd (the E_q rows, the H x H scatter,
    split-K products, the sigma partials)."""
    p, _ = _reference(name)
    runs = []
    try:
        for how in (0.0, np.nan, 1e300):
            _, lpj, v, y_hat = _run(engine, p, mp.hide(p["Y"], p["x_infr"], how))
            _no_clamp(v, (name, how))
            runs.append((lpj, v, _select(p, y_hat)))
    finally:
        _clear(engine)
    exact = ("Fs", "y_outer_diag") if p["N"] <= 256 else ("Fs",)
    for how, (lpj, v, y_rec) in zip(("nan", "1e300"), runs[1:]):
        np.testing.assert_array_equal(lpj, runs[0][0], err_msg="%s: lpj with %s hidden" % (name, how))
        for k in _names(p):
            if k in exact:
                np.testing.assert_array_equal(v[k], runs[0][1][k], err_msg="%s: %s with %s hidden" % (name, k, how))
            else:
                _close(v[k], runs[0][1][k], mp.BASE_RTOL, "%s: %s with %s hidden vs 0 hidden" % (name, k, how))
        _close(y_rec, runs[0][2], mp.BASE_RTOL, "%s: y_reconstructed with %s hidden vs 0 hidden" % (name, how))


# ---- additivity across the grid cap ------------------------------------------------------------------------------------
def test_grid_stride_is_additive(engine):
    """es_grid: N S above the grid cap of the masked launches, so sssc_big_kernel strides; each half stays under it.  The
    whole accumulator is the sum of the halves', the lpj rows are the halves' rows, and every 7th row is the oracle's."""
    p = mp.make_problem("es_grid")
    half = p["N"] // 2
    rows = np.arange(0, p["N"], mp.GRID_STRIDE)
    want = mp.oracle_lpj(mp.rows_of(p, rows))
    parts = []
    try:
        for sl in (slice(0, half), slice(half, p["N"]), slice(None)):
            q = mp.rows_of(p, sl)
            assert (q["N"] * q["S"] < 65536) == (sl != slice(None))
            _, lpj, v, y_hat = _run(engine, q)
            _no_clamp(v, sl)
            parts.append((lpj, v, y_hat))
    finally:
        _clear(engine)
    (la, va, ya), (lb, vb, yb), (lw, vw, yw) = parts
    for label, lpj in (("halves", np.concatenate((la, lb))), ("whole", lw)):
        _close(lpj[rows], want, mp.LPJ_RTOL, "es_grid: lpj of the %s, every 7th row" % label)
    # (not bit for bit: B = Y W of N and of N / 2 rows comes from differently tiled products)
    _close(lw, np.concatenate((la, lb)), mp.BASE_RTOL, "es_grid: lpj, whole vs halves")
    for k in mp.ES_NAMES:
        _close(vw[k], va[k] + vb[k], mp.BASE_RTOL, "es_grid: %s, whole vs sum of halves" % k)
    _close(yw, np.concatenate((ya, yb)), mp.BASE_RTOL, "es_grid: y_hat, whole vs halves")
    assert vw["N"] == p["N"]


# ---- EBSC routes -------------------------------------------------------------------------------------------------------
def test_ebsc_statistics_routes(engine):
    """bsc_d65 through the wave and the classic statistics kernels, pair bins off and forced on."""
    p, o = _reference("bsc_d65")
    out = {}
    try:
        for wave in (1, 0):
            for bins in (0, 2):
                engine.set_option("bsc_stats_wave", wave)
                engine.set_option("pair_bins", bins)
                _, lpj, v, _ = _run(engine, p)
                out[wave, bins] = v
                for k in mp.BSC_NAMES:
                    _close(v[k], o["sums"][k], mp.SUM_RTOL, "bsc_d65 wave %d bins %d: %s" % (wave, bins, k))
                    _close(v[k], out[1, 0][k], mp.BASE_RTOL, "bsc_d65 wave %d bins %d: %s vs wave 1 bins 0" % (wave, bins, k))
    finally:
        engine.set_option("bsc_stats_wave", DEFAULTS["bsc_stats_wave"])
        engine.set_option("pair_bins", DEFAULTS["pair_bins"])
        _clear(engine)


@pytest.mark.parametrize("name", ["bsc_d65", "bsc_keep"])
def test_ebsc_older_reconstruction(engine, name):
    """The step that reuses an older y_reconstructed (bsc.py:186): upload_yrec, no reconstruct_in_stats.  Without
    either the statistics pass refuses."""
    from evo_amd._lib import EvoAmdError
    p, o = _reference(name)
    rng = np.random.RandomState(7)
    y_old = np.where(p["x"], p["Y0"], rng.normal(size=p["Y"].shape))
    want = mp.oracle(p, y_rec_old=y_old)["sums"]
    assert _err(want["Wp"], o["sums"]["Wp"]) > 1e3 * mp.SUM_RTOL  # (the older rows matter)
    try:
        _setup(engine, p)
        engine.lpj_resident()
        with pytest.raises(EvoAmdError, match="needs y_reconstructed"):
            engine.stats()
        engine.upload_yrec(y_old)
        engine.lpj_resident()  # (the refused pass stopped half way)
        v = _stats(engine, reconstruct=False)
    finally:
        _clear(engine)
    for k in mp.BSC_NAMES:
        _close(v[k], want[k], mp.SUM_RTOL, "%s with an older y_reconstructed: %s" % (name, k))


# ---- Theta update ------------------------------------------------------------------------------------------------------
def _theta_keys(p):
    return ("W", "pies", "mus", "Psi", "sigma2") if p["algo"] == "es3c" else ("W", "pi", "sigma")


def _check_theta(p, got, dpar, want, factor, what):
    for k in _theta_keys(p):
        _close(got[k], want[k], factor * mp.THETA_RTOL, "%s: %s" % (what, k), atol=factor * mp.THETA_ATOL)
    sc = mp.new_scalars(p, want)
    for k in sc:  # ljc, sigma / sigma2, pre1 / sigma2_inv ... of the scalar block
        _close(dpar[k], sc[k], factor * mp.THETA_RTOL, "%s: scalar %s" % (what, k), atol=factor * mp.THETA_ATOL)


@pytest.mark.parametrize("name", mp.THETA_PROBLEMS)
def test_theta_update(engine, name):
    """mstep_device(reconstruct=True) with every parameter learned, then without sigma2 / sigma: Theta^new and the scalar
    block against the oracle's update applied to the device's own accumulator (isolates the update kernels) and, ten
    times wider, against the oracle's update of the oracle's sums.  sigma / sigma2 carry the OLD value times the count of
    reliable entries (bsc.py:266-272, sssc.py:747-755)."""
    p, o = _reference(name)
    keys = _theta_keys(p)
    noise = keys[-1]
    get = engine.get_params_sssc if p["algo"] == "es3c" else engine.get_params_bsc
    try:
        _setup(engine, p)
        engine.lpj_resident()
        acc = _stats(engine)
        for to_learn in (keys, keys[:-1]):
            _set_params(engine, p)
            engine.lpj_resident()
            engine.set_option("reconstruct_in_stats", 1)
            tail, dpar = engine.mstep_device(to_learn, reconstruct=True)
            got = get()
            what = "%s learn %s" % (name, "+".join(to_learn))
            _close(dpar["ljc_estep"], o["ljc"], mp.LPJ_RTOL, what + ": ljc of the E-step")
            _close(tail["Fs"], o["sums"]["Fs"], mp.SUM_RTOL, what + ": Fs")
            _close(_select(p, engine.reconstruct()), o["y_reconstructed"], mp.SUM_RTOL, what + ": y_reconstructed")
            _check_theta(p, got, dpar, mp.oracle_update(p, acc, to_learn), 1, what + " vs update of the device sums")
            _check_theta(p, got, dpar, mp.oracle_update(p, o["sums"], to_learn), 10, what + " vs update of the oracle sums")
            if noise not in to_learn:
                assert float(got[noise]) == float(p["theta"][noise]), what
    finally:
        _clear(engine)


@pytest.mark.parametrize("name", mp.TINY)
def test_lazy_theta_update_and_restore(engine, name):
    """mstep_device(theta_to_host=False) on incomplete data: Theta^new against the oracle's update of the device sums, then
    restore_theta_backup brings the E-step's Theta back bit for bit, sigma2 / sigma included, set_params returns the same
    ljc and the masked pass over K^n repeats bit for bit.  es_h2 takes the backup written inside
    sssc_mstep_prepare_kernel (D = 8 H) by H H = 4 threads; a complete-data lazy update of _theta_problems.backup_prelude()
    runs first on the same context, so that the slot of theta_bak the restore reads sigma2 from holds 0.0 and not 1.3
    unless THIS update's backup wrote it (test_theta_problems.py restates the layout)."""
    import _theta_problems as tp
    p, o = _reference(name)
    keys = _theta_keys(p)
    get = engine.get_params_sssc if p["algo"] == "es3c" else engine.get_params_bsc
    assert tp.backup_route(p) == ("in_update" if name == "es_h2" else "side_kernel")
    q = tp.backup_prelude()
    engine.configure("sssc", q["N"], q["D"], q["H"], q["S"], q["S_perm"], min(CMAX, q["S"]))
    engine.upload_data(q["Y"])
    engine.upload_states(q["ss"])
    _set_params(engine, q)
    engine.lpj_resident()
    assert engine.mstep_device(_theta_keys(q), theta_to_host=False)[1]["status"] == 0.0
    try:
        ljc = _setup(engine, p)
        engine.lpj_resident()
        lpj = engine.download_lpj()
        acc = _stats(engine)
        _set_params(engine, p)
        engine.lpj_resident()
        engine.set_option("reconstruct_in_stats", 1)
        tail, dpar = engine.mstep_device(keys, reconstruct=True, theta_to_host=False)
        assert dpar["status"] == 0.0 and dpar["ljc_estep"] == ljc
        _check_theta(p, get(), dpar, mp.oracle_update(p, acc, keys), 1, name + " lazy vs update of the device sums")
        engine.restore_theta_backup()
        back = get()
        for k in keys:
            np.testing.assert_array_equal(back[k], p["theta"][k], err_msg="%s: restored %s" % (name, k))
        assert _set_params(engine, p, back) == ljc
        engine.lpj_resident()
        np.testing.assert_array_equal(engine.download_lpj(), lpj, err_msg=name + ": lpj after the restore")
    finally:
        _clear(engine)


# ---- float32 modes -----------------------------------------------------------------------------------------------------
def test_ebsc_float32_refuses_masks(engine):
    """ebsc_f32 has no masked kernels: evoamd_upload_masks says so."""
    from evo_amd._lib import EvoAmdError
    p = mp.make_problem("bsc_s300")  # (the float32 mode wants H and D in multiples of 4)
    engine.set_option("ebsc_f32", 1)
    try:
        engine.configure("bsc", p["N"], p["D"], p["H"], p["S"], p["S_perm"], CMAX)
        engine.upload_data(p["Y0"])
        with pytest.raises(EvoAmdError, match="incomplete data is not available in the float32 mode"):
            engine.upload_masks(p["x_infr"], p["x"])
    finally:
        engine.set_option("ebsc_f32", DEFAULTS["ebsc_f32"])
        engine.configure("bsc", p["N"], p["D"], p["H"], p["S"], p["S_perm"], CMAX)


def test_es3c_precision_float32_with_masks(engine):
    """ES3C precision = float32 (option "sssc_precision") accepts masks: es_d65 against the oracle in that precision at
    the tolerances of test_es3c_precision_float32 (lpj 2e-6 relative + 1e-6, the sums 3e-6)."""
    p = mp.make_problem("es_d65")
    o = mp.oracle(p, precision=np.float32)
    engine.set_option("sssc_precision", 32)
    try:
        _, lpj, v, _ = _run(engine, p)
    finally:
        engine.set_option("sssc_precision", DEFAULTS["sssc_precision"])
        _clear(engine)
    print("PARITY es_d65 float32: lpj err %.3e" % _err(lpj, o["lpj"]))
    np.testing.assert_allclose(lpj, o["lpj"], rtol=2e-6, atol=1e-6)
    for k in mp.ES_NAMES:
        _close(v[k], np.asarray(o["sums"][k], dtype=np.float64), 3e-6, "es_d65 float32: %s" % k)

"""The device Theta update (evoamd_mstep_device, complete data) against the float64 oracle: every learn set of both
models, the H x H solvers on the moment matrices the update feeds them, the backup and publish routes, the side-stream
mailbox and the float32 mode.  Problems, the branches they reach and the wrong-reference proofs: _theta_problems.py and
test_theta_problems.py.  Every comparison prints its worst error in units of max(1, |reference|max)."""
import time

import numpy as np
import pytest

import _theta_problems as tp

pytestmark = pytest.mark.gpu

CMAX = 12  # candidates per datapoint the engine is configured for
DEFAULTS = {"background_unit": 0, "inverse_spd": 1, "inverse_block": 0, "theta_copy_engine": 0, "mailbox_side_stream": 1,
            "sssc_precision": 64}
SCALARS = {"es3c": ("ljc", "sigma2", "sigma2_inv"), "ebsc": ("ljc", "sigma", "pre1", "pi", "pil_bar")}


@pytest.fixture(scope="module")
def engine():
    from evo_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not want.size:
        return 0.0
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _close(got, want, rtol, what, atol=None):
    """assert_allclose with atol = (atol or rtol) * max(1, |want|max); prints the error it saw first."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print("PARITY %-66s err %.3e  (rtol %.0e)" % (what, _err(got, want), rtol))
    scale = max(1.0, float(np.abs(want).max())) if want.size else 1.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=(rtol if atol is None else atol) * scale, err_msg=what)


def _keys(p):
    return tp.ES_KEYS if p["algo"] == "es3c" else tp.BSC_KEYS


def _set_params(engine, p, theta=None):
    th = p["theta"] if theta is None else theta
    if p["algo"] == "es3c":
        return engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    return engine.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))


def _get(engine, p):
    return engine.get_params_sssc() if p["algo"] == "es3c" else engine.get_params_bsc()


def _setup(engine, p):
    """The call order of evo_amd/models/_models.py up to the parameters (test_gpu_masked_parity._setup without masks)."""
    engine.configure("sssc" if p["algo"] == "es3c" else "bsc", p["N"], p["D"], p["H"], p["S"], p["S_perm"], min(CMAX, p["S"]))
    engine.upload_data(p["Y"])
    engine.upload_states(p["ss"])
    return _set_params(engine, p)


def _first_pass(engine, p):
    """(ljc, lpj, accumulator views) of the pass whose sums every learn set below updates from."""
    ljc = _setup(engine, p)
    engine.lpj_resident()
    lpj = engine.download_lpj()
    acc = {k: np.array(v) for k, v in engine.acc_views(engine.stats()).items()}
    return ljc, lpj, acc


def _update(engine, p, to_learn, **kw):
    """Theta re-installed, the pass over K^n, mstep_device: (tail, scalar block, Theta^new)."""
    _set_params(engine, p)
    engine.lpj_resident()
    tail, dpar = engine.mstep_device(to_learn, **kw)
    return tail, dpar, _get(engine, p)


def _check_theta(p, got, dpar, want, factor, what):
    for k in _keys(p):
        _close(got[k], want[k], factor * tp.THETA_RTOL, "%s: %s" % (what, k), atol=factor * tp.THETA_ATOL)
    sc = tp.new_scalars(p, want)
    for k in SCALARS[p["algo"]]:
        _close(dpar[k], sc[k], factor * tp.THETA_RTOL, "%s: scalar %s" % (what, k), atol=factor * tp.THETA_ATOL)


def _restore(engine, options=DEFAULTS):
    for k in options:
        engine.set_option(k, DEFAULTS[k])


# ---- a, b: every learn set against the oracle; what is not learned does not move ------------------------------------------
@pytest.mark.parametrize("name", list(tp.PROBLEMS))
def test_learn_sets(engine, name):
    """Theta^new and the scalar block of every learn set of the problem against the oracle's update (with check_params'
    clamps) of the device's own accumulator and, up to H = 33 and ten times wider, of the oracle's sums; a parameter outside
    the learn set comes back bit for bit; the empty set changes nothing."""
    from oracle import evo_oracle as orc
    p = tp.make_problem(name)
    o = None if name in tp.LARGE else tp.oracle(name)
    theta, keys = p["theta"], _keys(p)
    try:
        engine.set_option("background_unit", 1 if p["background"] else 0)
        ljc, lpj, acc = _first_pass(engine, p)
        if o is None:  # no second oracle pass on this machine for the large ones: the device's lpj, the oracle's formulas
            ljc_ref, Fs_ref = tp.new_scalars(p, theta)["ljc"], orc.free_energy_sum(lpj)
        else:
            ljc_ref, Fs_ref = o["ljc"], o["sums"]["Fs"]
            _close(lpj, o["lpj"], tp.LPJ_RTOL, name + ": lpj")
        _close(ljc, ljc_ref, tp.LPJ_RTOL, name + ": ljc")
        for ls in tp.learn_sets(name):
            to_learn = tp.LEARN_SETS[p["algo"]][ls]
            what = "%s learn %s" % (name, ls)
            tail, dpar, got = _update(engine, p, to_learn)
            assert dpar["status"] == 0.0, what
            _close(dpar["ljc_estep"], ljc_ref, tp.LPJ_RTOL, what + ": ljc of the E-step")
            _close(tail["Fs"], Fs_ref, tp.SUM_RTOL, what + ": Fs")
            assert tail["N"] == p["N"]
            want = tp.oracle_update(p, acc, to_learn)
            _check_theta(p, got, dpar, want, 1, what + " vs update of the device sums")
            if o is not None:
                _check_theta(p, got, dpar, tp.oracle_update(p, o["sums"], to_learn), 10, what + " vs update of the oracle sums")
            for k in keys:
                if k in to_learn:
                    continue
                np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s is not learned" % (what, k))
                if p["kind"] != "clamp":  # (inside the clamps: test_theta_problems.py)
                    np.testing.assert_array_equal(got[k], theta[k], err_msg="%s: %s is not learned" % (what, k))
            if not to_learn:
                assert dpar["ljc_estep"] == dpar["ljc"] == ljc, what
                sc = tp.new_scalars(p, theta)
                for k in SCALARS[p["algo"]][1:]:
                    if k in theta:
                        assert dpar[k] == float(theta[k]), (what, k)
                    else:  # derived on the host by set_params_*: a rounding of log or of the division
                        np.testing.assert_allclose(dpar[k], sc[k], rtol=1e-15, atol=0, err_msg="%s: %s" % (what, k))
        if p["kind"] == "clamp":
            _check_clamped(p, engine, acc)
    finally:
        _restore(engine, ("background_unit",))


def _check_clamped(p, engine, acc):
    """The clamp problem's values, said without the oracle: latent 0 is in no state, latent 1 in every state."""
    if p["algo"] == "es3c":
        _, _, got = _update(engine, p, ("pies", "mus"))
        assert got["pies"][0] == 5e-5 and got["pies"][1] == 1.0 - 5e-5, got["pies"][:2]
        assert got["mus"][0] == 0.0
        want = p["theta"]["Psi"].copy()
        assert want[0, 0] < 1e-5
        want[0, 0] = 1e-5  # check_params' diagonal floor on the Psi that is not learned
        np.testing.assert_array_equal(got["Psi"], want)
    else:
        _, dpar, got = _update(engine, p, ("pi",))
        assert acc["pies"][0] == 0.0 and abs(acc["pies"][1] - p["N"]) <= 1e-12 * p["N"]
        _close(got["pi"], (acc["pies"] / p["N"]).sum() / p["H"], tp.THETA_RTOL, p["name"] + ": pi from the sums")


# ---- c: solver routes ------------------------------------------------------------------------------------------------------
ROUTES = (("default", {}), ("pivoted", {"inverse_spd": 0}), ("block16", {"inverse_block": 16}), ("block32", {"inverse_block": 32}))


@pytest.mark.parametrize("name", ["es_h130", "es_h257", "bsc_h130"])
def test_solver_routes(engine, name):
    """The "all" learn set through the default SPD elimination, the pivoted one, and the 16- and 32-column steps forced:
    each against the oracle's update of the device sums, and against one another at BASE_RTOL of |reference|max."""
    p = tp.make_problem(name)
    keys = _keys(p)
    # three kernel families per size (one forced block width is the default's: 16 at H = 130, 32 at H = 257)
    assert len({tp.solver(p["H"], o.get("inverse_spd", 1), o.get("inverse_block", 0)) for _, o in ROUTES}) == 3
    out = {}
    try:
        _, _, acc = _first_pass(engine, p)
        want = tp.oracle_update(p, acc, keys)
        for label, opts in ROUTES:
            _restore(engine, ("inverse_spd", "inverse_block"))
            for k, v in opts.items():
                engine.set_option(k, v)
            _, dpar, got = _update(engine, p, keys)
            assert dpar["status"] == 0.0, (name, label)
            _check_theta(p, got, dpar, want, 1, "%s %s vs update of the device sums" % (name, label))
            out[label] = (got, dpar)
    finally:
        _restore(engine, ("inverse_spd", "inverse_block"))
    for label, (got, dpar) in out.items():
        for k in keys:
            _close(got[k], out["default"][0][k], tp.BASE_RTOL, "%s %s vs default: %s" % (name, label, k))
        for k in SCALARS[p["algo"]]:
            _close(dpar[k], out["default"][1][k], tp.BASE_RTOL, "%s %s vs default: scalar %s" % (name, label, k))


# ---- d: publish and backup routes -----------------------------------------------------------------------------------------
def _same(a, b, what):
    """Two device runs of the same arithmetic.  Bit for bit where no atomic takes part: Fs (a fixed-order reduction of the lpj
    rows) and the ljc of the E-step.  Theta^new and the scalar block behind it come from the accumulator, whose E_q rows,
    H x H scatter and split-K products pass through unsafeAtomicAdd in the statistics pass of EVERY run (see
    test_hidden_values_never_enter): the order of those additions is the hardware's, not the route's, so these are held
    at BASE_RTOL, for every pair alike."""
    _close(a, b, tp.BASE_RTOL, what + (" [same bits]" if np.array_equal(a, b) else ""))


IN_UPDATE = ("es_h12", "es_h1", "es_h2", "es_h3", "es_h4")


def _fill_backup(engine):
    """A lazy update of tp.backup_prelude() (es_h2_d17 with sigma2 = 2.7, the side-kernel route): theta_bak, which
    configure keeps, then holds that problem's 58 doubles whatever ran before."""
    q = tp.backup_prelude()
    assert tp.backup_route(q) == "side_kernel"
    _setup(engine, q)
    engine.lpj_resident()
    _, dpar = engine.mstep_device(tp.ES_KEYS, theta_to_host=False)
    assert dpar["status"] == 0.0
    engine.restore_theta_backup()
    assert engine.get_params_sssc()["sigma2"] == 2.7


@pytest.mark.parametrize("name", ["es_h12", "es_d100", "bsc_h12", "es_h1", "es_h2", "es_h2_d17", "es_h3", "es_h4", "bsc_h2"])
def test_publish_and_backup_routes(engine, name):
    """PUBLISH_MAIN (Theta in the mailbox), PUBLISH_FOLDED with the backup (in the update for D <= 8 H, the side kernel
    above, always for EBSC), and both again with option theta_copy_engine (PUBLISH_COPY_ENGINE for the eager call): the
    same Theta^new, scalar block and tail; after every lazy call restore_theta_backup brings the input Theta back bit for
    bit, and the pass over K^n under it repeats the first pass bit for bit.

    The in-update backup is written by the H H live threads of sssc_mstep_prepare_kernel.  While each saved the scalar of
    its own index only, H = 1 kept DP_PRE1 alone and H = 2 the scalars 0 .. 3, so the restore read sigma2 (index 6) from
    a slot of theta_bak that call had not written.  _fill_backup decides what that slot holds (test_theta_problems.py
    restates it): W[8, 1] = -0.0969... of the prelude for es_h1, the prelude's DP_PI = 0.0 for es_h2.  Before the fix the
    restore returned sigma2 = -0.09697344284776688 (es_h1) and 0.0 (es_h2) for the 1.3 installed."""
    p = tp.make_problem(name)
    keys, theta = _keys(p), p["theta"]
    assert tp.backup_route(p) == ("in_update" if name in IN_UPDATE else "side_kernel")
    runs = {}
    try:
        if name in tp.TINY:
            _fill_backup(engine)
        ljc, lpj, acc = _first_pass(engine, p)
        want = tp.oracle_update(p, acc, keys)
        for dma in (0, 1):
            engine.set_option("theta_copy_engine", dma)
            for lazy in (False, True):
                label = "%s%s" % ("lazy" if lazy else "eager", " copy-engine" if dma else "")
                tail, dpar, got = _update(engine, p, keys, theta_to_host=not lazy)
                assert dpar["status"] == 0.0, (name, label)
                _check_theta(p, got, dpar, want, 1, "%s %s vs update of the device sums" % (name, label))
                runs[label] = (tail, dpar, got)
                if not lazy:
                    continue
                engine.restore_theta_backup()
                back = _get(engine, p)
                for k in keys:
                    np.testing.assert_array_equal(back[k], theta[k], err_msg="%s %s: restored %s" % (name, label, k))
                assert _set_params(engine, p, back) == ljc
                engine.lpj_resident()
                np.testing.assert_array_equal(engine.download_lpj(), lpj, err_msg="%s %s: lpj after the restore" % (name, label))
        # a second Theta on the same context: the backup must be this call's, not one that was right the first time
        th2 = tp.second_theta(p)
        assert all(not np.array_equal(th2[k], theta[k]) for k in keys if k != "Psi")
        ljc2 = _set_params(engine, p, th2)
        engine.lpj_resident()
        lpj2 = engine.download_lpj()
        assert ljc2 != ljc and not np.array_equal(lpj2, lpj)
        _, dpar = engine.mstep_device(keys, theta_to_host=False)
        assert dpar["status"] == 0.0 and dpar["ljc_estep"] == ljc2, name
        engine.restore_theta_backup()
        back = _get(engine, p)
        for k in keys:
            np.testing.assert_array_equal(back[k], th2[k], err_msg="%s: restored %s of the second Theta" % (name, k))
        assert _set_params(engine, p, back) == ljc2
        engine.lpj_resident()
        np.testing.assert_array_equal(engine.download_lpj(), lpj2, err_msg="%s: lpj after the second restore" % name)
    finally:
        _restore(engine, ("theta_copy_engine",))
    t0, d0, g0 = runs["eager"]
    for label, (tail, dpar, got) in runs.items():
        assert tail["Fs"] == t0["Fs"] and tail["N"] == t0["N"], (name, label)
        assert dpar["ljc_estep"] == d0["ljc_estep"] == ljc, (name, label)
        for k in keys:
            _same(got[k], g0[k], "%s %s vs eager: %s" % (name, label, k))
        for k in SCALARS[p["algo"]]:
            _same(dpar[k], d0[k], "%s %s vs eager: scalar %s" % (name, label, k))


# ---- e: side-stream mailbox -------------------------------------------------------------------------------------------------
def test_side_stream_mailbox(engine):
    """The smallest N at which an ES3C context with the workload's H = 512 reaches the 8e9 contraction flops from which a
    lazy call publishes its mailbox on the side stream (PUBLISH_SIDE); mailbox_side_stream = 0 folds the header into the
    update's last kernel instead.  No oracle at this size: the two routes against each other."""
    p = tp.make_side_problem()
    assert tp.contraction_flops("es3c", p["N"], p["D"], p["H"]) >= tp.SIDE_FLOPS
    runs = {}
    t = time.perf_counter()
    try:
        ljc = _setup(engine, p)
        for side in (1, 0):
            engine.set_option("mailbox_side_stream", side)
            tail, dpar, got = _update(engine, p, tp.ES_KEYS, theta_to_host=False)
            assert dpar["status"] == 0.0, side
            assert all(np.isfinite(np.asarray(got[k])).all() for k in tp.ES_KEYS), side
            runs[side] = (tail, dpar, got)
    finally:
        _restore(engine, ("mailbox_side_stream",))
    print("side-stream problem N = %d, D = %d, H = %d: %.2f s" % (p["N"], p["D"], p["H"], time.perf_counter() - t))
    (t1, d1, g1), (t0, d0, g0) = runs[1], runs[0]
    for k in ("Fs", "N", "reset_isnan", "reset_smaller_eps", "reset_isinf"):
        assert t1[k] == t0[k], k
    assert d1["ljc_estep"] == d0["ljc_estep"] == ljc
    for k in tp.ES_KEYS:
        _same(g1[k], g0[k], "side stream vs folded: %s" % k)
    for k in SCALARS["es3c"]:
        _same(d1[k], d0[k], "side stream vs folded: scalar %s" % k)


# ---- f: float32 precision ---------------------------------------------------------------------------------------------------
def test_es3c_precision_float32(engine):
    """ES3C precision = float32 (option "sssc_precision"): the update of the sums the device rounded to float32, at the
    tolerance test_es3c_precision_float32 (test_gpu_models.py) holds Theta^new to (2e-4); 1 / sigma2 passes through
    float32 (sssc.py:346-349)."""
    p = tp.make_problem("es_h12")
    engine.set_option("sssc_precision", 32)
    try:
        _, _, acc = _first_pass(engine, p)
        for k in ("xpt_s", "xpt_ss", "xpt_sz", "xpt_szsz", "s_sz_outer", "sz_sz_outer"):
            np.testing.assert_array_equal(acc[k], acc[k].astype(np.float32).astype(np.float64), err_msg=k)
        _, dpar, got = _update(engine, p, tp.ES_KEYS)
    finally:
        _restore(engine, ("sssc_precision",))
    want = tp.oracle_update(p, acc, tp.ES_KEYS)
    for k in tp.ES_KEYS:
        _close(got[k], want[k], 2e-4, "es_h12 float32: %s" % k)
    assert dpar["sigma2"] == float(got["sigma2"])
    assert dpar["sigma2_inv"] == float(np.float32(1.0 / dpar["sigma2"])), (dpar["sigma2_inv"], dpar["sigma2"])

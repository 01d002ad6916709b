"""K^n resized on the GPU: Engine.resize_states / adopt_resized_states (csrc/kernels_resize.hpp) and Model.resize_states
against the NumPy mirror (evo_amd.variational.resize_states_host).

1. kernel against the mirror, exactly (the law has no floating point beyond the keys of given rows: no margin, no undecided
   datapoint), every problem of tests/_resize_problems.py, both models; 2. the digests against digest_kernel's; 3. kept
   states keep their lpj, a shrink's F is the log-sum-exp of the kept entries, a grow's F does not fall; 4. two calls give
   the same bits, a resize without adopt changes nothing; 5. every refusal leaves everything as it was; 6. the Model level;
   7. a round trip; 8. incomplete data; 9. the kernel class.
"""
import numpy as np
import pytest

import _resize_problems as rp
import _sweep_masked_problems as mp
from evo_amd import _lib
from evo_amd._lib import EvoAmdError
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import init_states, resize_states_host

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # (the constant of tests/test_gpu_sweep_states.py)
ALLZERO = {"background": False, "allzero": True, "singletons": False}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model_eng():
    """The Model tests' own engine: Model._prepare keeps per-engine state that the engine-level tests do not maintain."""
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _options_back(eng):
    yield
    eng.set_option("background_unit", 0)


def _set_theta(eng, model, th):
    if model == "sssc":
        eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    else:
        eng.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))


def _configure(eng, p, S):
    eng.set_option("ebsc_f32", 0)
    eng.f32 = False
    eng.set_option("background_unit", 1 if p.background else 0)
    eng.configure(p.model, p.N, p.D, p.H, S, p.S_perm, 4)
    if p.Y is not None:
        eng.upload_data(p.Y)
        _set_theta(eng, p.model, p.theta)


def _install(eng, p, rows=True):
    """The problem's K^n and (rows) its rows resident."""
    _configure(eng, p, p.S)
    eng.upload_states(p.ss)
    if rows:
        eng.upload_lpj(p.lpj)


def _resize_and_adopt(eng, p, S_new):
    src = eng.resize_states(S_new)
    _configure(eng, p, S_new)
    eng.adopt_resized_states()
    return src


def _logsumexp(rows):
    m = rows.max(axis=1)
    return m + np.log(np.exp(rows - m[:, None]).sum(axis=1))


# ---- 1. the kernel against the mirror ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S_new", rp.all_resizes())
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_kernel_equals_mirror(eng, algo, name, S_new):
    p = rp.problem(algo, name)
    want, want_src = rp.mirror(algo, name, S_new)
    _install(eng, p)
    src = _resize_and_adopt(eng, p, S_new)
    got = eng.download_states()
    assert src.dtype == np.int32 and src.shape == want_src.shape and got.shape == want.shape
    bad = [n for n in range(p.N) if not (np.array_equal(got[n], want[n]) and np.array_equal(src[n], want_src[n]))]
    assert not bad, "datapoints that differ from the mirror: %s" % bad[:8]
    assert np.array_equal(eng.download_states_packed(), np.packbits(want, axis=-1))


# ---- 2. / 3. digests, the lpj of kept states, F ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,S_new", [("ragged", 30), ("ragged_perm", 5), ("s200", 70), ("s64", 200), ("large_h", 9),
                                        ("tight", 35), ("handmade", 100)])
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_digests_rows_and_free_energy(eng, algo, name, S_new):
    """The lpj kernels read the digests: the rows of the resized K^n must equal, exactly, those of the same states uploaded
    (upload_states_packed runs digest_kernel).  The rows that rank are the device's own here, so a kept state is evaluated
    twice by the same kernels."""
    p = rp.problem(algo, name)
    _install(eng, p, rows=False)
    eng.lpj_resident()
    old = eng.download_lpj()
    F_before = eng.posterior_scores()["F"]
    want, want_src = resize_states_host(p.ss, old, p.S_perm, S_new, p.background)
    src = _resize_and_adopt(eng, p, S_new)
    assert np.array_equal(src, want_src) and np.array_equal(eng.download_states(), want)
    eng.lpj_resident()
    new = eng.download_lpj()
    F_after = eng.posterior_scores()["F"]
    eng.upload_states_packed(eng.download_states_packed())
    eng.lpj_resident()
    assert not np.isnan(new).any() and np.array_equal(new, eng.download_lpj())
    # kept states keep their lpj
    kept = src >= 0
    old_of_new = np.take_along_axis(old[:, p.S_perm:], np.where(kept, src, 0), axis=1)
    err = np.abs(new[:, p.S_perm:] - old_of_new)[kept] / np.maximum(1.0, np.abs(old_of_new[kept]))
    print("%s %s -> %d: kept rows %.3g" % (algo, name, S_new, err.max()))
    assert err.max() <= RTOL
    if p.S_perm:
        assert np.abs(new[:, 0] - old[:, 0]).max() <= RTOL * np.maximum(1.0, np.abs(old[:, 0])).max()
    if S_new < p.S:
        rows = np.concatenate((old[:, :p.S_perm], old_of_new), axis=1)
        want_F = _logsumexp(rows)
        assert (np.abs(F_after - want_F) <= RTOL * np.maximum(1.0, np.abs(want_F))).all()
    else:
        print("%s %s -> %d: mean F_after - F_before %.4g" % (algo, name, S_new, (F_after - F_before).mean()))
        assert (F_after >= F_before - 1e-12 * np.abs(F_before)).all()


# ---- 4. determinism; a resize without adopt --------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_two_calls_same_bits_and_no_adopt_changes_nothing(eng, algo):
    p = rp.problem(algo, "ragged")
    _install(eng, p)
    packed, lpj, flags = eng.download_states_packed(), eng.download_lpj(), eng.debug_validity()
    scores = eng.posterior_scores()
    a = eng.resize_states(30)
    assert np.array_equal(eng.download_states_packed(), packed) and np.array_equal(eng.download_lpj(), lpj)
    assert eng.debug_validity() == flags
    again = eng.posterior_scores()
    assert all(np.array_equal(scores[k], again[k]) for k in scores)
    b = eng.resize_states(30)
    assert np.array_equal(a, b)
    _configure(eng, p, 30)
    eng.adopt_resized_states()
    first = eng.download_states_packed()
    _install(eng, p)
    c = _resize_and_adopt(eng, p, 30)
    assert np.array_equal(eng.download_states_packed(), first) and np.array_equal(a, c)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _refused(eng, call, match):
    def snapshot():
        return eng.download_states_packed(), eng.download_lpj(), eng.debug_validity()

    before = snapshot()
    with pytest.raises(EvoAmdError, match=match):
        call()
    after = snapshot()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    assert before[2] == after[2], {k: (before[2][k], after[2][k]) for k in before[2] if before[2][k] != after[2][k]}


@pytest.mark.parametrize("algo", rp.ALGOS)
def test_refusals_leave_everything_as_it_was(eng, algo):
    p = rp.problem(algo, "tight")
    _install(eng, p)
    for S_new, match in ((p.S, "nothing to resize"), (0, "must be positive"), (-1, "must be positive"),
                         (1025, "at most 1024"), (rp.TIGHT_REFUSED, "fewer than S_new = 36")):
        _refused(eng, lambda: eng.resize_states(S_new), match)
        _refused(eng, eng.adopt_resized_states, "no resized states")
    # rows that are not those of the resident K^n: K^n uploaded again, no rows since
    eng.upload_states(p.ss)
    _refused(eng, lambda: eng.resize_states(5), "not those of the resident K\\^n")
    eng.lpj_resident()  # ... and a pass makes them so
    eng.resize_states(5)
    # adopt: the geometry differs (still S = 20), then another S; the scratch survives both
    _refused(eng, eng.adopt_resized_states, "the resized states are")
    _configure(eng, p, 7)
    other = np.ascontiguousarray(p.ss[:, :7])
    eng.upload_states(other)
    _refused(eng, eng.adopt_resized_states, "the resized states are")
    _configure(eng, p, 5)
    eng.adopt_resized_states()
    got = eng.download_states()
    assert got.shape == (p.N, 5, p.H)
    _refused(eng, eng.adopt_resized_states, "no resized states")  # an adopt uses the states up
    assert np.array_equal(eng.download_states(), got)
    # a refused resize leaves a waiting result waiting
    _install(eng, p)
    src = eng.resize_states(35)
    _refused(eng, lambda: eng.resize_states(rp.TIGHT_REFUSED), "fewer than S_new = 36")
    _configure(eng, p, 35)
    eng.adopt_resized_states()
    assert np.array_equal(eng.download_states(), rp.mirror(algo, "tight", 35)[0]) and (src[:, p.S:] == -1).all()
    fresh = Engine(0)
    try:
        with pytest.raises(EvoAmdError, match="nothing is resident"):
            fresh.resize_states(5)
    finally:
        fresh.close()


# ---- 6. the Model level --------------------------------------------------------------------------------------------------------
def _model_problem(algo, name, permanent):
    p = rp.problem(algo, name)
    suff = init_states(p.N, p.S, p.H, "fit", "randflip", 3, 2, 1, permanent=permanent)
    assert suff["S_perm"] == p.S_perm
    suff["ss"], suff["lpj"] = p.ss.copy(), p.lpj.copy()
    return p, suff, {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}


@pytest.mark.parametrize("S_new", [5, 30])
@pytest.mark.parametrize("sync_host", [False, True])
@pytest.mark.parametrize("name,permanent", [("ragged", None), ("ragged_perm", ALLZERO)])
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_model_resize_states(model_eng, algo, name, permanent, sync_host, S_new):
    eng = model_eng
    cls = BSC if algo == "ebsc" else SSSC
    p, suff, my_data = _model_problem(algo, name, permanent)
    model = cls(p.D, p.H, p.S, engine=eng, rng="device", sync_host=sync_host, seed=3)
    th = model.check_params(dict(p.theta))
    if not sync_host:  # K^n and its rows resident only
        model.attach_resident_states(suff, my_data, [(0, np.packbits(p.ss, axis=-1))])
        model.E_step_precompute(dict(th), dict(suff), my_data)
        eng.lpj_resident()
        suff["lpj"] = eng.download_lpj()
    old_scores = model.posterior_scores(th, suff, my_data)
    want, want_src = resize_states_host(p.ss, suff["lpj"], p.S_perm, S_new)
    new_model, new_suff, info = model.resize_states(th, suff, my_data, S_new)
    assert type(new_model) is cls and (new_model.H, new_model.S) == (p.H, S_new) and new_model.engine is eng
    assert (new_model.rng, new_model.sync_host, new_model.seed) == ("device", sync_host, 3)
    assert np.array_equal(info["src_slot"], want_src) and info["src_slot"].dtype == np.int32
    assert new_suff["S_perm"] == p.S_perm and new_suff["n_parents"] == suff["n_parents"] and new_suff["Mprime"] <= S_new
    if sync_host:
        ss, lpj = new_suff["ss"], new_suff["lpj"]
    else:
        assert new_suff["ss"] is None and new_suff["lpj"] is None
        ss, lpj = eng.download_states(), eng.download_lpj()
    assert np.array_equal(ss, want) and lpj.shape == (p.N, p.S_perm + S_new)
    assert np.array_equal(info["F_before"], old_scores["F"])
    scores = new_model.posterior_scores(th, new_suff, my_data)
    assert np.array_equal(info["F_after"], scores["F"]) and np.isfinite(scores["F"]).all()
    if S_new > p.S:  # (F_before is from the oracle's rows here: RTOL, not the 1e-12 of a sum)
        assert (info["F_after"] >= info["F_before"] - RTOL * np.abs(info["F_before"])).all()
    # what can follow at once: local search and refinement from the resized K^n, F does not fall
    thc = dict(th)
    new_model.E_step_precompute(thc, dict(new_suff), my_data)  # (for ljc: the precompute stores it in the dict it is given)
    F0 = thc["ljc"] + info["F_after"].mean()
    sw = new_model.sweep_resident_states(th, new_suff, my_data, n_sweeps=1)
    assert sw.n_done == 1 and sw.F[0] >= F0 - 1e-12 * abs(F0)
    res = new_model.refine_resident_states(th, new_suff, my_data, 2)
    assert res.n_done == 2 and res.F[0] >= sw.F[0] - 1e-12 * abs(F0) and res.F[1] >= res.F[0] - 1e-12 * abs(F0)
    base = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in th.items()}
    F_step = new_model.step(base, new_suff, my_data)[0]
    assert np.isfinite(F_step)
    # the old model re-uploads instead of reading the new K^n
    again = model.posterior_scores(th, suff, my_data)
    assert eng.S == p.S and all(np.array_equal(old_scores[k], again[k]) for k in old_scores)


def test_model_resize_background(model_eng):
    """The background unit: Model.resize_states admits it (the sweeps do not)."""
    from _seed_problems import make_data, make_theta
    p = rp.problem("ebsc", "background")
    rng = np.random.RandomState(9)
    theta = make_theta(rng, "ebsc", p.D, p.H)
    Y, _ = make_data(rng, "ebsc", theta, p.N)
    suff = init_states(p.N, p.S, p.H, "fit", "randflip", 3, 2, 1,
                       permanent={"background": True, "allzero": False, "singletons": False})
    suff["ss"], suff["lpj"] = p.ss.copy(), p.lpj.copy()
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = BSC(p.D, p.H, p.S, engine=model_eng, rng="device", sync_host=True, seed=3)
    th = model.check_params(dict(theta))
    new_model, new_suff, info = model.resize_states(th, suff, my_data, 20)
    want, want_src = rp.mirror("ebsc", "background", 20)
    assert np.array_equal(new_suff["ss"], want) and np.array_equal(info["src_slot"], want_src)
    assert np.isfinite(new_model.E_step(th, new_suff, my_data)[0])


# ---- 7. a round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_round_trip(eng, algo):
    p = rp.problem(algo, "ragged")
    _install(eng, p, rows=False)
    eng.lpj_resident()
    rows12 = eng.download_lpj()
    _resize_and_adopt(eng, p, 30)
    eng.lpj_resident()
    rows30 = eng.download_lpj()
    src = _resize_and_adopt(eng, p, 12)
    got = eng.download_states()
    grown, _ = resize_states_host(p.ss, rows12, 0, 30)
    want, want_src = resize_states_host(grown, rows30, 0, 12)
    assert np.array_equal(got, want) and np.array_equal(src, want_src)
    for n in range(p.N):
        top = set(rp.seed_key_order(rows30[n])[:12])
        for j in range(p.S):  # an original state among the 12 best of the grown row is still there
            if j in top:
                assert (got[n] == p.ss[n, j]).all(axis=1).any(), (n, j)


# ---- 8. incomplete data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", rp.ALGOS)
def test_model_resize_incomplete_data(model_eng, algo):
    cls = BSC if algo == "ebsc" else SSSC
    m = mp.problem(algo, "ragged", 0.3)
    suff = init_states(m.N, m.S, m.H, "fit", "randflip", 3, 2, 1)
    suff["ss"], suff["lpj"] = m.ss.copy(), m.lpj.copy()
    my_data = {"y": m.Y.copy(), "x_infr": m.x_infr.copy()}
    model = cls(m.D, m.H, m.S, engine=model_eng, rng="device", sync_host=True, seed=3)
    th = model.check_params(dict(m.theta))
    new_model, new_suff, info = model.resize_states(th, suff, my_data, 30)
    want, want_src = resize_states_host(m.ss, m.lpj, 0, 30)
    assert np.array_equal(new_suff["ss"], want) and np.array_equal(info["src_slot"], want_src)
    want_lpj = mp.rows_of(algo, m.theta, m.Y, m.x_infr, want, 0)
    err = (np.abs(new_suff["lpj"] - want_lpj) / np.maximum(1.0, np.abs(want_lpj))).max()
    print("%s incomplete: lpj against the oracle's masked rows %.3g" % (algo, err))
    assert err <= RTOL


# ---- 9. the kernel class -----------------------------------------------------------------------------------------------------------
def test_kernel_class_is_named(eng):
    assert _lib.KERNEL_IDS_EXTRA["resize"] == 32
    assert eng.lib.evoamd_kernel_name(32) == b"resize"
    p = rp.problem("ebsc", "ragged")
    _install(eng, p)
    eng.timing(["resize"])
    try:
        eng.timing_reset()
        eng.resize_states(5)
        ms, launches = eng.kernel_time_ms("resize")
        assert launches == 1 and ms > 0.0
        assert eng.kernel_time_ms("sweep")[1] == 0
    finally:
        eng.timing(False)

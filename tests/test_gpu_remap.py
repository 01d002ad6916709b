"""The dictionary resized on the GPU: Engine.remap_latents / adopt_remapped_states / latent_map_counts
(csrc/kernels_remap.hpp) and Model.remap_latents / Model.latent_usage.

1. kernel against its NumPy mirror (evo_amd.variational.remap_states_host), bit for bit: K^n through download_states and
   download_states_packed, n_replaced and its sum, for every case of tests/_remap_problems.py and both models;
2. the digests the kernel writes against digest_kernel's (same lpj bits before and after a re-upload of the same rows);
3. two remap calls give the same bits; a remap without adopt changes nothing;
4. adopt with another geometry or a second adopt is refused with K^n unchanged; no stale rows survive an adopt;
5. the LDS cap: the largest admitted S and one above; every refusal leaves K^n, the lpj rows and the flags as they were;
6. Model.remap_latents for both models, device-resident and host-synchronised, incomplete data, the float32 mode;
7. Model.latent_usage against its mirror, planted ties; 8. no buffer outlives the engine.
"""
import ctypes
import functools

import numpy as np
import pytest

import _remap_problems as rp
from _seed_problems import make_data, make_theta
from evo_amd import _lib
from evo_amd._lib import EvoAmdError
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import init_states, latent_usage_host, prune_index, remap_states_host
from oracle import evo_oracle as orc

pytestmark = pytest.mark.gpu

LPJ_RTOL = 1e-9  # (the constant of tests/test_gpu_seed_states.py)
ALLZERO = {"background": False, "allzero": True, "singletons": False}
BACKGROUND = {"background": True, "allzero": False, "singletons": False}
D = 8


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model_eng():
    """The Model tests' own engine: Model._prepare keeps per-engine state that the engine-level tests do not maintain."""
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _mirror(name):
    c = rp.case(name)
    want, n_rep = remap_states_host(c.ss, c.index, c.S_perm, c.background)
    want.setflags(write=False)
    return want, n_rep


def _model_name(algo):
    return "bsc" if algo == "ebsc" else "sssc"


def _set_params(eng, algo, th):
    if algo == "ebsc":
        eng.set_params_bsc(th["W"], th["pi"], th["sigma"])
    else:
        eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], th["sigma2"])


def _configure(eng, algo, c, H, S=None, background=None):
    bg = c.background if background is None else background
    eng.set_option("ebsc_f32", 0)
    eng.f32 = False
    eng.set_option("background_unit", 1 if bg else 0)
    eng.configure(_model_name(algo), c.N, D, H, c.S if S is None else S, c.S_perm, 4)


def _remap_and_adopt(eng, algo, c):
    """Upload the case's K^n at H, remap, configure for H', adopt.  Returns (n_replaced, sum)."""
    _configure(eng, algo, c, c.H)
    eng.upload_states(c.ss)
    n_rep, total = eng.remap_latents(c.index)
    _configure(eng, algo, c, c.H2)
    eng.adopt_remapped_states()
    return n_rep, total


@pytest.fixture(scope="module")
def model_eng2():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def _options_back(eng):
    yield
    eng.set_option("background_unit", 0)  # (the engine-level tests' own engine: the models keep track of theirs)


@pytest.mark.parametrize("name", rp.CASES)
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_kernel_equals_mirror(eng, algo, name):
    c = rp.case(name)
    want, want_rep = _mirror(name)
    n_rep, total = _remap_and_adopt(eng, algo, c)
    got = eng.download_states()
    packed = eng.download_states_packed()
    print("%s %s: mean / max n_replaced %.2f / %d" % (algo, name, n_rep.mean(), n_rep.max()))
    assert n_rep.dtype == np.int32 and np.array_equal(n_rep, want_rep) and total == int(want_rep.sum())
    assert got.shape == want.shape
    bad = [n for n in range(c.N) if not np.array_equal(got[n], want[n])]
    assert not bad, "datapoints that differ from the mirror: %s" % bad[:8]
    assert np.array_equal(packed, np.packbits(want, axis=-1))


@pytest.mark.parametrize("algo,name", [("ebsc", "dense"), ("es3c", "boundary"), ("es3c", "allzero"), ("ebsc", "background"),
                                       ("es3c", "pairs")])
def test_digests_equal_digest_kernel(eng, algo, name):
    """The lpj kernels read the digests: the rows the remap kernel wrote must evaluate exactly like the same rows uploaded
    (upload_states_packed runs digest_kernel)."""
    c = rp.case(name)
    rng = np.random.RandomState(5)
    theta = make_theta(rng, algo, D, c.H2)
    Y, _ = make_data(rng, algo, theta, c.N)
    _remap_and_adopt(eng, algo, c)
    eng.upload_data(Y)
    _set_params(eng, algo, theta)
    eng.lpj_resident()
    before = eng.download_lpj()
    packed = eng.download_states_packed()
    eng.upload_states_packed(packed)
    eng.lpj_resident()
    after = eng.download_lpj()
    assert not np.isnan(before).any()
    assert np.array_equal(before, after)


def test_two_calls_same_bits_and_no_adopt_changes_nothing(eng):
    c = rp.case("small")
    rng = np.random.RandomState(6)
    theta = make_theta(rng, "ebsc", D, c.H)
    Y, _ = make_data(rng, "ebsc", theta, c.N)
    _configure(eng, "ebsc", c, c.H)
    eng.upload_data(Y)
    _set_params(eng, "ebsc", theta)
    eng.upload_states(c.ss)
    eng.lpj_resident()
    lpj, flags = eng.download_lpj(), eng.debug_validity()
    a_rep, a_sum = eng.remap_latents(c.index)
    assert np.array_equal(eng.download_states(), c.ss)  # a remap without adopt leaves K^n alone
    assert np.array_equal(eng.download_lpj(), lpj) and eng.debug_validity() == flags
    b_rep, b_sum = eng.remap_latents(c.index)
    assert np.array_equal(a_rep, b_rep) and a_sum == b_sum
    _configure(eng, "ebsc", c, c.H2)
    eng.adopt_remapped_states()
    first = eng.download_states_packed()
    n_rep, _ = _remap_and_adopt(eng, "ebsc", c)
    assert np.array_equal(eng.download_states_packed(), first) and np.array_equal(n_rep, a_rep)


def test_adopt_refusals_leave_kn_alone(eng):
    c = rp.case("boundary")
    _configure(eng, "ebsc", c, c.H)
    eng.upload_states(c.ss)
    with pytest.raises(EvoAmdError, match="no remapped states"):
        eng.adopt_remapped_states()
    eng.remap_latents(c.index)
    with pytest.raises(EvoAmdError, match="the remapped states are"):  # still configured for H, not H'
        eng.adopt_remapped_states()
    assert np.array_equal(eng.download_states(), c.ss)
    _configure(eng, "ebsc", c, c.H2, S=c.S - 1)  # another S
    other = rp.distinct_states(np.random.RandomState(1), c.N, c.S - 1, c.H2, 0.1)
    eng.upload_states(other)
    with pytest.raises(EvoAmdError, match="the remapped states are"):
        eng.adopt_remapped_states()
    assert np.array_equal(eng.download_states(), other)
    _configure(eng, "ebsc", c, c.H2)  # the scratch survived both configures
    eng.adopt_remapped_states()
    want, _ = _mirror("boundary")
    assert np.array_equal(eng.download_states(), want)
    with pytest.raises(EvoAmdError, match="no remapped states"):  # an adopt uses the states up
        eng.adopt_remapped_states()
    assert np.array_equal(eng.download_states(), want)


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_no_stale_rows_after_adopt(eng, eng2, algo):
    """A permutation needs no configure in between: whatever described the old K^n must be dropped by the adopt itself."""
    c = rp.case("permutation")
    rng = np.random.RandomState(7)
    theta = make_theta(rng, algo, D, c.H)
    Y, _ = make_data(rng, algo, theta, c.N)
    _configure(eng, algo, c, c.H)
    eng.upload_data(Y)
    _set_params(eng, algo, theta)
    eng.upload_states(c.ss)
    eng.lpj_resident()
    old = eng.download_lpj()
    eng.stats()
    eng.posterior_codes(4)
    eng.remap_latents(c.index)
    eng.posterior_codes(4)  # (the remap alone drops nothing)
    kn_gen = eng.debug_validity()["kn_gen"]
    eng.adopt_remapped_states()
    v = eng.debug_validity()
    assert v["kn_gen"] > kn_gen and not v["prefetch_current"] and not v["census_current"] and not v["rows_kn_current"]
    assert not v["kn_lost"]
    with pytest.raises(EvoAmdError):
        eng.posterior_codes(4)
    eng.lpj_resident()
    new = eng.download_lpj()
    assert not np.array_equal(old, new)
    _configure(eng2, algo, c, c.H)  # a fresh context that uploads the same states
    eng2.upload_data(Y)
    _set_params(eng2, algo, theta)
    eng2.upload_states_packed(eng.download_states_packed())
    eng2.lpj_resident()
    assert np.array_equal(new, eng2.download_lpj())


def test_refusals_leave_the_context_alone(eng):
    c = rp.case("cap")
    assert c.S == rp.CAP_S
    rng = np.random.RandomState(8)
    _configure(eng, "ebsc", c, c.H, S=c.S + 1)  # one above the cap
    more = np.concatenate((c.ss, np.zeros((c.N, 1, c.H), dtype=bool)), axis=1)
    more[:, -1, :3] = True
    eng.upload_states(more)
    eng.upload_data(rng.normal(size=(c.N, D)))
    _set_params(eng, "ebsc", make_theta(rng, "ebsc", D, c.H))
    eng.lpj_resident()
    lpj, flags, packed = eng.download_lpj(), eng.debug_validity(), eng.download_states_packed()

    def refused(index, match):
        with pytest.raises(EvoAmdError, match=match):
            eng.remap_latents(index)
        assert np.array_equal(eng.download_states_packed(), packed)
        assert np.array_equal(eng.download_lpj(), lpj) and eng.debug_validity() == flags
        with pytest.raises(EvoAmdError, match="no remapped states"):
            eng.adopt_remapped_states()

    refused(c.index, "the cap at these H, H_new is S = %d" % rp.CAP_S)
    bad = c.index.copy()
    bad[5] = bad[6]
    refused(bad, "duplicate source latent")
    bad = c.index.copy()
    bad[0] = c.H
    refused(bad, "out of range")
    bad[0] = -2
    refused(bad, "out of range")
    refused(np.arange(40, dtype=np.int32), "fewer than S = %d" % (c.S + 1))  # 820 candidates
    eng.set_option("background_unit", 1)  # (an option: the flags are compared within the block)
    flags = eng.debug_validity()
    try:
        refused(c.index[:-1], "the last index must be H - 1")
    finally:
        eng.set_option("background_unit", 0)
    fresh = Engine(0)
    try:
        with pytest.raises(EvoAmdError, match="nothing is resident"):
            fresh.remap_latents(c.index)
    finally:
        fresh.close()


def _oracle_lpj(algo, theta, ss, Y, S_perm, x_infr=None):
    th = {k: v for k, v in theta.items() if k in ("W", "pi", "sigma", "pies", "mus", "Psi", "sigma2")}
    N, S, H = ss.shape
    rows = np.empty((N, S + S_perm))
    Yz = Y if x_infr is None else np.where(x_infr, Y, 0.0)
    if algo == "ebsc":
        cnt = orc.bsc_precompute(th, Y.shape[1], H, x_infr)
        for n in range(N):
            xi = None if x_infr is None else x_infr[n]
            if S_perm:
                rows[n, 0] = orc.bsc_lpj_allzero(th, Yz[n], cnt, xi)[0]
            rows[n, S_perm:] = orc.bsc_lpj(th, ss[n], Yz[n], cnt, xi)
    else:
        cnt = orc.sssc_precompute(th, Y.shape[1], x_infr)
        cache = {}
        for n in range(N):
            xi = None if x_infr is None else x_infr[n]
            if S_perm:
                rows[n, 0] = orc.sssc_lpj_allzero(th, Yz[n], cnt, xi)[0]
            rows[n, S_perm:] = orc.sssc_lpj(th, ss[n], Yz[n], cnt, cache if xi is None else {}, xi)
    return rows


def _rel(a, b):
    return (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()


def _model_problem(algo, name, permanent=None, missing=0.0):
    c = rp.case(name)
    rng = np.random.RandomState(21 if algo == "ebsc" else 22)
    theta = make_theta(rng, algo, D, c.H)
    Y, _ = make_data(rng, algo, theta, c.N)
    x_infr = np.ones_like(Y, dtype=bool)
    if missing:
        x_infr = rng.random_sample(Y.shape) >= missing
        x_infr[:, 0] = True
        Y[~x_infr] = np.nan
    suff = init_states(c.N, c.S, c.H, "fit", "randflip", 6, 1, 1, permanent=permanent)
    assert suff["S_perm"] == c.S_perm
    suff["ss"] = c.ss.copy()
    return c, theta, {"y": Y, "x_infr": x_infr}, suff


@pytest.mark.parametrize("sync_host", [False, True])
@pytest.mark.parametrize("algo,name,permanent", [("ebsc", "boundary", None), ("es3c", "allzero", ALLZERO),
                                                 ("ebsc", "background", BACKGROUND), ("es3c", "prototype", None)])
def test_model_remap_latents(model_eng, model_eng2, algo, name, permanent, sync_host):
    eng, eng2 = model_eng, model_eng2
    cls = BSC if algo == "ebsc" else SSSC
    c, theta, my_data, suff = _model_problem(algo, name, permanent)
    want, want_rep = _mirror(name)
    kw = dict(rng="device", sync_host=sync_host, seed=3)
    model = cls(D, c.H, c.S, engine=eng, **kw)
    th = model.check_params(dict(theta))
    F0 = model.E_step(th, suff, my_data)[0] if sync_host else None  # (the model has worked before it is resized)
    if sync_host:
        suff["ss"][:] = c.ss  # the E-step moved K^n: the case's own again
    else:
        model.attach_resident_states(suff, my_data, [(0, np.packbits(c.ss, axis=-1))])
    new_model, new_theta, new_suff, info = model.remap_latents(th, suff, my_data, c.index, rng=np.random.RandomState(4))
    assert type(new_model) is cls and new_model.H == c.H2 and new_model.S == c.S and new_model.engine is eng
    assert (new_model.rng, new_model.sync_host, new_model.seed) == ("device", sync_host, 3)
    assert np.array_equal(info["index"], c.index) and np.array_equal(info["n_replaced"], want_rep)
    assert info["sum_replaced"] == int(want_rep.sum())
    assert new_theta["W"].shape == (D, c.H2) and new_suff["S_perm"] == c.S_perm and new_suff["incl"].shape[0] == c.S_perm
    assert new_suff["n_parents"] == suff["n_parents"] and new_suff["permanent"] == suff["permanent"]
    if sync_host:
        ss, lpj = new_suff["ss"], new_suff["lpj"]
        assert F0 is not None and np.isfinite(F0)
    else:
        assert new_suff["ss"] is None and new_suff["lpj"] is None
        ss, lpj = eng.download_states(), eng.download_lpj()
    assert np.array_equal(ss, want)
    want_lpj = _oracle_lpj(algo, new_theta, want, my_data["y"], c.S_perm)
    print("%s %s sync_host=%s: lpj against the oracle %.3g" % (algo, name, sync_host, _rel(lpj, want_lpj)))
    assert _rel(lpj, want_lpj) <= LPJ_RTOL
    # what can follow at once
    codes = new_model.encode(new_theta, new_suff, my_data, max_active=8)
    assert codes.idx.shape == (c.N, 8) and codes.idx.max() < c.H2
    scores = new_model.posterior_scores(new_theta, new_suff, my_data)
    assert np.isfinite(scores["F"]).all()
    # one step of the new model = one step of a fresh model of size H' handed the mirror's states and new_theta
    fresh = cls(D, c.H2, c.S, engine=eng2, rng="device", sync_host=True, seed=3)
    f_suff = dict(new_suff)
    f_suff["ss"], f_suff["lpj"] = want.copy(), np.empty((c.N, c.S + c.S_perm))
    base = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in new_theta.items()}
    F_a, _, _, th_a = new_model.step(dict(base), new_suff, my_data)
    F_b, _, _, th_b = fresh.step(dict(base), f_suff, my_data)
    ss_a = new_suff["ss"] if sync_host else eng.download_states()
    assert np.isfinite(F_a) and abs(F_a - F_b) <= LPJ_RTOL * abs(F_b)
    assert np.array_equal(ss_a, f_suff["ss"])
    res = new_model.refine_resident_states(th_a, new_suff, my_data, 2)
    assert res.n_done == 2 and np.isfinite(res.F).all()
    # the old model re-uploads instead of reading the new K^n
    if sync_host:
        F_old = model.E_step(th, suff, my_data)[0]
        assert np.isfinite(F_old) and eng.H == c.H
        assert suff["ss"].shape == (c.N, c.S, c.H)


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_permutation_keeps_the_free_energy(model_eng, algo):
    eng = model_eng
    cls = BSC if algo == "ebsc" else SSSC
    c, theta, my_data, suff = _model_problem(algo, "permutation")
    model = cls(D, c.H, c.S, engine=eng, rng="device", sync_host=True, seed=3)
    th = model.check_params(dict(theta))
    model.E_step(th, suff, my_data)
    before = model.posterior_scores(th, suff, my_data)["F"]
    ss_before = suff["ss"].copy()
    new_model, new_theta, new_suff, info = model.remap_latents(th, suff, my_data, c.index)
    assert info["sum_replaced"] == 0 and np.array_equal(new_suff["ss"], ss_before[:, :, c.index])
    after = new_model.posterior_scores(new_theta, new_suff, my_data)["F"]
    print("%s: F before / after a permutation %.3g" % (algo, _rel(after, before)))
    assert _rel(after, before) <= LPJ_RTOL  # (not bitwise: the order of the sums over latents changes)
    assert abs(new_theta["ljc"] - th["ljc"]) <= 1e-12 * abs(th["ljc"])
    # ... and the inverse permutation restores K^n bit for bit
    back_model, _, back_suff, _ = new_model.remap_latents(new_theta, new_suff, my_data, np.argsort(c.index).astype(np.int32))
    assert np.array_equal(back_suff["ss"], ss_before) and back_model.H == c.H


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_model_remap_incomplete_data(model_eng, algo):
    cls = BSC if algo == "ebsc" else SSSC
    c, theta, my_data, suff = _model_problem(algo, "boundary", missing=0.3)
    want, want_rep = _mirror("boundary")
    model = cls(D, c.H, c.S, engine=model_eng, rng="device", sync_host=True, seed=3)
    th = model.check_params(dict(theta))
    new_model, new_theta, new_suff, info = model.remap_latents(th, suff, my_data, c.index)
    assert np.array_equal(new_suff["ss"], want) and np.array_equal(info["n_replaced"], want_rep)
    want_lpj = _oracle_lpj(algo, new_theta, want, my_data["y"], 0, my_data["x_infr"])
    print("%s incomplete: lpj against the oracle %.3g" % (algo, _rel(new_suff["lpj"], want_lpj)))
    assert _rel(new_suff["lpj"], want_lpj) <= LPJ_RTOL
    my_data["x"] = my_data["x_infr"].copy()
    F = new_model.step(new_theta, new_suff, my_data, do_reconstruction=True)[0]  # (incomplete data: every step reconstructs)
    assert np.isfinite(F)


def test_model_remap_float32(model_eng):
    c, theta, my_data, suff = _model_problem("ebsc", "f32")
    want, want_rep = _mirror("f32")
    assert c.H % 4 == 0 and c.H2 % 4 == 0
    model = BSC(D, c.H, c.S, engine=model_eng, rng="device", sync_host=True, seed=3, dtype=np.float32)
    th = model.check_params(dict(theta))
    new_model, new_theta, new_suff, info = model.remap_latents(th, suff, my_data, c.index)
    assert new_model.dtype == np.float32 and model_eng.f32
    assert np.array_equal(new_suff["ss"], want) and np.array_equal(info["n_replaced"], want_rep)
    want_lpj = _oracle_lpj("ebsc", new_theta, want, my_data["y"], 0)
    err = _rel(new_suff["lpj"], want_lpj)
    print("float32: lpj against the float64 oracle %.3g" % err)
    # float data and B = Y W in float32 (u = 2^-24 = 6e-8), D = 8 products per entry, and the Gram form yy - 2 s.B + s G s
    # cancels to a residual some 50 times smaller than its terms for a well-explained datapoint: 8 * 6e-8 * 50 = 2.4e-5
    assert err <= 1e-4
    assert np.isfinite(new_model.E_step(new_theta, new_suff, my_data)[0])
    try:
        with pytest.raises(EvoAmdError, match="multiples of 4"):  # configure's own rule surfaces for H' = 66
            new_model.remap_latents(new_theta, new_suff, my_data, np.arange(66, dtype=np.int32))
    finally:  # (the failed configure left the context unconfigured: a geometry of its own for whoever comes next)
        model_eng.set_option("ebsc_f32", 0)
        model_eng.f32 = False
        model_eng.configure("bsc", 4, 4, 4, 2)


@pytest.mark.parametrize("sync_host", [False, True])
@pytest.mark.parametrize("algo,name,permanent", [("ebsc", "boundary", None), ("es3c", "allzero", ALLZERO)])
def test_latent_usage(model_eng, algo, name, permanent, sync_host):
    eng = model_eng
    cls = BSC if algo == "ebsc" else SSSC
    c, theta, my_data, suff = _model_problem(algo, name, permanent)
    model = cls(D, c.H, c.S, engine=eng, rng="device", sync_host=True, seed=3)
    th = model.check_params(dict(theta))
    model.E_step(th, suff, my_data)
    if not sync_host:  # the same K^n and lpj, resident only
        model = cls(D, c.H, c.S, engine=eng, rng="device", sync_host=False, seed=3)
        model.attach_resident_states(suff, my_data, [(0, np.packbits(suff["ss"], axis=-1))])
        model.E_step_precompute(dict(th), dict(suff), my_data)
        eng.lpj_resident()
    keys = {k: id(v) for k, v in suff.items()}
    out = model.latent_usage(th, suff, my_data)
    assert {k: id(v) for k, v in suff.items()} == keys  # nothing written into the dicts
    want = latent_usage_host(suff["ss"], suff["lpj"], c.S_perm)
    assert out["N"] == c.N and out["usage"].shape == (c.H,) and out["map_count"].dtype == np.int64
    np.testing.assert_allclose(out["usage"], want["usage"], rtol=1e-8, atol=1e-9)  # (the codes tests' tolerance for E_q[s_h])
    assert np.array_equal(out["map_count"], want["map_count"])
    idx = prune_index(out["usage"], n_keep=c.H - 10)
    assert idx.size == c.H - 10


def test_map_counts_planted_ties(eng):
    c = rp.case("allzero")
    rng = np.random.RandomState(11)
    _configure(eng, "ebsc", c, c.H)
    eng.upload_states(c.ss)
    lpj = rng.normal(size=(c.N, c.S + 1))
    for n in range(c.N):
        a, b = sorted(rng.choice(c.S + 1, 2, replace=False))
        lpj[n, a] = lpj[n, b] = lpj[n].max() + 1.0  # the first of the two wins; column 0 is the all-zero state
    lpj[3, 0] = lpj[3].max()
    eng.upload_lpj(lpj)
    want = latent_usage_host(c.ss, lpj, 1)["map_count"]
    assert np.array_equal(eng.latent_map_counts(), want)
    assert np.array_equal(eng.latent_map_counts(), want)  # the counters start from zero every call
    assert np.array_equal(eng.download_lpj(), lpj)


def _live():
    out = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().evoamd_debug_live_buffers(out))
    return int(out[0]), int(out[1])


def test_no_buffer_outlives_the_engine():
    c = rp.case("shrink")
    before = _live()
    e = Engine(0)
    _remap_and_adopt(e, "es3c", c)
    e.upload_lpj(np.zeros((c.N, c.S)))
    e.latent_map_counts()
    e.remap_latents(np.arange(c.H2, dtype=np.int32)[::-1].copy())  # scratch left waiting
    assert _live()[0] > before[0]
    e.close()
    assert _live() == before

"""Model.sample_posterior / Engine.sample_posterior (csrc/kernels_posterior_sample.hpp) on the GPU.

1. the kernel against its NumPy mirror (evo_amd.models.sample_posterior_counter; references from
   tests/_posterior_sample_problems.py, computed once per shape at T = 70 -- fewer draws are a prefix) on the ten shapes of
   tests/test_gpu_predictive.py: N = 30 / 37 (37 is no multiple of the 4 waves of a workgroup), D = 25 / 64 / 70 / 512,
   H = 10 / 70 (two state words), S = 8, both models, complete and incomplete data, the permanent all-zero state, the
   background unit, noise on / off, fill "missing" / "all", sync_host True / False; T = 1, 5 and 70 (one full pass of 64
   draws and a ragged one; with 8 or 9 slots the lanes of a pass share states).  slot and s bit for bit; z and y rtol 1e-8 /
   atol 1e-9 max(1, max |ref|), the tolerance tests/test_gpu_predictive.py holds this arithmetic to; NaN pattern and info
   equal; a second call returns identical bits;
2. the tie to the existing kernel: the sample mean and variance of 4096 device draws (fill "all") against the device
   predictive_moments of the same inputs, within 6 standard errors (the bounds of tests/test_posterior_sample_host.py);
3. refusals: D = 513, k = 33, float32, "z" for EBSC, outputs that cannot fit the device;
4. the prefix and the shard property on the device, bit for bit;
5. non-interference: step / step with a call in between, encode after it, the device state and the validity flags under
   a fixed Theta, and the live buffers after close.
"""
import ctypes

import numpy as np
import pytest

import _posterior_sample_problems as pp
from _predictive_problems import my_data_of, problem
from evo_amd import _lib
from evo_amd._lib import EvoAmdError, check
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import init_states

pytestmark = pytest.mark.gpu

ARRAYS = ("slot", "s", "z", "y")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _model(eng, algo, D, H, S, sync_host=True, **kw):
    if not sync_host:
        kw.update(rng="device", sync_host=False)
    return (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, **kw)


def _assert_matches(out, ref, T, what):
    assert out["info"] == ref["info"], what
    assert sorted(out) == sorted(ref), what
    for k in ("slot", "s"):
        if k not in ref:
            continue
        want = ref[k][:, :T]
        assert out[k].dtype == want.dtype and out[k].shape == want.shape
        assert np.array_equal(out[k], want), (what, k)
    for k in ("z", "y"):
        if k not in ref:
            continue
        got, want = out[k], ref[k][:, :T]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, k)
        ok = ~np.isnan(want)
        scale = max(1.0, float(np.abs(want[ok]).max()))
        print("%s T = %d: max |%s - ref| = %.3g (max %.3g)" % (what, T, k, np.abs(got[ok] - want[ok]).max(), scale))
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-8, atol=1e-9 * scale, err_msg="%s %s" % (what, k))


def _same_bits(a, b):
    assert sorted(a) == sorted(b) and a["info"] == b["info"]
    for k in a:
        if k != "info":
            assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("T", [1, 5, pp.T_MAX])
@pytest.mark.parametrize("case,noise,sync_host,fill", pp.CASES)
def test_kernel_equals_mirror(eng, case, noise, sync_host, fill, T):
    p = problem(*case)
    model = _model(eng, p.algo, p.D, p.H, p.S, sync_host)
    suff, my_data, theta = pp.suff_of(p), my_data_of(p), dict(p.theta)
    keys = (list(theta), list(suff), list(my_data))
    out = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=pp.SEED, fill=fill, noise=noise)
    assert keys == (list(theta), list(suff), list(my_data))  # nothing written into the three dicts
    assert np.array_equal(suff["ss"], p.ss) and np.array_equal(suff["lpj"], p.lpj)
    assert model.last_sample_seed == pp.SEED
    ref = pp.draws(case, fill, noise)
    assert ref["info"]["n_skipped"] == (1 if p.incomplete else 0)
    _assert_matches(out, ref, T, repr(case))
    if fill == "missing":  # the reliable entries of the datapoints with draws: the datapoint's own y, bit for bit
        rel = np.broadcast_to((p.x_infr & p.x_infr.any(axis=1)[:, None])[:, None, :], out["y"].shape)
        assert np.array_equal(out["y"][rel], np.broadcast_to(p.Y[:, None, :], out["y"].shape)[rel])
    _same_bits(out, model.sample_posterior(theta, suff, my_data, n_samples=T, seed=pp.SEED, fill=fill, noise=noise))


def test_only_the_arrays_asked_for_come_back(eng):
    case, noise, _, fill = pp.CASES[3]
    p = problem(*case)
    model = _model(eng, p.algo, p.D, p.H, p.S)
    ref = pp.draws(case, fill, noise)
    for keep in (("slot",), ("y",), ("z", "s")):
        out = model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), n_samples=5, seed=pp.SEED, keep=keep,
                                     fill=fill, noise=noise)
        assert sorted(out) == sorted(keep + ("info",))
        _assert_matches(out, {k: ref[k] for k in keep + ("info",)}, 5, repr(keep))
    with pytest.raises(EvoAmdError, match="did not keep"):  # z and s were kept last
        a = np.empty((p.N, 5), dtype=np.int32)
        check(eng.lib.evoamd_download_posterior_samples(eng._h, _lib.PSAMP_WHAT["slot"], a.ctypes.data_as(ctypes.c_void_p)))


def test_the_call_has_a_timing_class_of_its_own(eng):
    p = problem("ebsc", 30, 70, 10, True, 0, False)
    model = _model(eng, p.algo, p.D, p.H, p.S)
    model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p))
    assert eng.lib.evoamd_kernel_name(_lib.KERNEL_IDS_EXTRA["posterior_sample"]) == b"posterior_sample"
    eng.timing(["posterior_sample"])
    try:
        eng.timing_reset()
        eng.sample_posterior(3, seed=1, keep=("y",))
        ms, launches = eng.kernel_time_ms("posterior_sample")
        assert launches == 1 and ms > 0.0 and eng.kernel_time_ms("misc")[1] == 0
    finally:
        eng.timing(False)


def test_datapoints_without_draws_are_counted(eng):
    """An indefinite Psi (Lam of every state with latent 4 is not positive definite), lpj rows that are all -inf, hold a
    NaN or +inf, and -- second problem -- a dead latent whose system is singular (the inputs of
    tests/test_gpu_predictive.py::test_singular_system_is_counted): counters, NaN rows and the other datapoints' draws
    are the mirror's."""
    case = ("es3c", 30, 25, 10, False, 1, False)
    p = problem(*case)
    theta = dict(p.theta)
    theta["Psi"] = np.array(theta["Psi"])
    theta["Psi"][4, :] = theta["Psi"][:, 4] = 0.0
    theta["Psi"][4, 4] = -0.05
    lpj = np.array(p.lpj)
    lpj[2] = -np.inf
    lpj[9, 1] = np.nan
    lpj[11, 0] = np.inf
    ref = pp.mirror(p, pp.T_MAX, theta=theta, lpj=lpj)
    assert ref["info"]["n_not_pd"] > 0 and ref["info"]["n_bad_weights"] == 3
    model = _model(eng, "es3c", p.D, p.H, p.S)
    out = model.sample_posterior(dict(theta), pp.suff_of(p, lpj=lpj), my_data_of(p), n_samples=pp.T_MAX, seed=pp.SEED, fill="all")
    _assert_matches(out, ref, pp.T_MAX, "indefinite Psi, bad weights")
    assert (out["slot"][2] == -1).all() and not out["s"][2].any()

    rng = np.random.RandomState(4)
    p = problem("es3c", 30, 25, 10, True, 0, False)
    theta = dict(p.theta)
    theta["Psi"] = np.array(theta["Psi"])
    theta["Psi"][2, :] = theta["Psi"][:, 2] = 0.0
    theta["W"] = np.array(theta["W"])
    ss = np.array(p.ss)
    ss[:, :, 2] = False
    ss[2, 4] = False
    ss[2, 4, [1, 2]] = True
    x_infr = np.array(p.x_infr)
    x_infr[2] = False
    x_infr[2, :3] = True
    theta["W"][:3, [1, 2]] = 0.0
    Y = np.where(x_infr, rng.normal(size=(p.N, p.D)), np.nan)
    lpj = np.array(p.lpj)
    lpj[2, 4] += 3.0  # (drawn within the first draws)
    from evo_amd.models import sample_posterior_counter
    ref = sample_posterior_counter("sssc", theta, ss, lpj, Y, x_infr, n_samples=pp.T_MAX, seed=pp.SEED)
    assert ref["info"] == {"n_singular": 1, "n_skipped": 1, "n_not_pd": 0, "n_bad_weights": 0}
    my_data = {"y": Y, "x_infr": x_infr, "x": x_infr.copy()}
    out = _model(eng, "es3c", p.D, p.H, p.S).sample_posterior(theta, pp.suff_of(p, ss=ss, lpj=lpj), my_data,
                                                              n_samples=pp.T_MAX, seed=pp.SEED)
    _assert_matches(out, ref, pp.T_MAX, "singular")
    assert np.isnan(out["y"][2]).all() and (out["slot"][2] == -1).all()


# ---- 2. the tie to predictive_moments ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_sample_moments_equal_the_predictive_kernel(eng, algo):
    p = problem(algo, 30, 25, 10, False, 1, False)
    model = _model(eng, algo, p.D, p.H, p.S)
    suff, my_data, theta = pp.suff_of(p), my_data_of(p), dict(p.theta)
    mean, var, info = model.predictive_moments(theta, suff, my_data, noise=True)
    out = model.sample_posterior(theta, suff, my_data, n_samples=4096, seed=7, keep=("y",), fill="all", noise=True)
    assert info == {"n_singular": 0, "n_skipped": 0} and not any(out["info"].values())
    zm, zv = pp.moment_bounds(out["y"], mean, var)
    print("%s: mean %.2f, variance %.2f standard errors at most" % (algo, zm, zv))
    assert zm <= 6.0
    assert zv <= 6.0


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_d_above_the_register_limit_is_refused(eng):
    p = problem("ebsc", 30, 512, 10, True, 1, False)
    D = 513
    rng = np.random.RandomState(1)
    model = _model(eng, "ebsc", D, p.H, p.S)
    theta = {"W": rng.normal(size=(D, p.H)), "pi": 0.1, "sigma": np.float64(1.0)}
    my_data = {"y": rng.normal(size=(p.N, D)), "x_infr": np.ones((p.N, D), dtype=bool)}
    with pytest.raises(EvoAmdError, match="D = 513"):
        model.sample_posterior(theta, pp.suff_of(p), my_data)


@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_more_than_32_active_latents_raise(eng, algo):
    case = ("ebsc", 37, 25, 70, False, 1, False) if algo == "ebsc" else ("es3c", 37, 64, 70, True, 0, False)
    p = problem(*case)
    ss = np.array(p.ss)
    assert ss[1, 2].sum() == 32
    ss[1, 2, np.flatnonzero(~ss[1, 2])[0]] = True
    model = _model(eng, algo, p.D, p.H, p.S)
    with pytest.raises(EvoAmdError, match=r"n = 1 .*k = 33"):
        model.sample_posterior(dict(p.theta), pp.suff_of(p, ss=ss), my_data_of(p), n_samples=5, seed=pp.SEED)
    with pytest.raises(EvoAmdError, match="no results"):  # nothing is handed out after the refused call
        a = np.empty((p.N, 5), dtype=np.int32)
        check(eng.lib.evoamd_download_posterior_samples(eng._h, _lib.PSAMP_WHAT["slot"], a.ctypes.data_as(ctypes.c_void_p)))
    # the context serves the next call
    out = model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), n_samples=5, seed=pp.SEED, fill="all")
    _assert_matches(out, pp.draws(case, "all", True), 5, "after the refused call")


def test_float32_mode_is_refused(eng):
    N, D, H, S = 32, 8, 16, 8
    np.random.seed(4)
    Y = np.random.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = BSC(D, H, S, engine=eng, dtype=np.float32)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1)
    with pytest.raises(EvoAmdError, match="float32 mode"):
        model.sample_posterior(theta, suff, my_data)


def test_z_is_refused_for_ebsc_and_oversize_outputs_name_their_bytes(eng):
    p = problem("ebsc", 30, 512, 10, True, 1, False)
    model = _model(eng, "ebsc", p.D, p.H, p.S)
    with pytest.raises(EvoAmdError, match="ES3C output"):
        model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), keep=("slot", "z"))
    model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p))  # (the context holds this shape)
    with pytest.raises(EvoAmdError, match="z is an ES3C output"):
        counters = (ctypes.c_int64 * 4)()
        check(eng.lib.evoamd_posterior_sample(eng._h, 1, 0, 0, _lib.PSAMP_KEEP["z"], 0, 1, counters))
    # 30 x (2^31 - 1) x 512 doubles = 2.6e14 bytes: more than any device holds; refused before anything is launched
    T = 2 ** 31 - 1
    with pytest.raises(EvoAmdError, match="need %d bytes" % (p.N * T * p.D * 8)):
        model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), n_samples=T, keep=("y",))
    out = model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), n_samples=5, seed=pp.SEED)
    assert sorted(out) == ["info", "s", "slot", "y"]  # the default names z for ES3C only
    _assert_matches(out, pp.draws(pp.CASES[9][0], "missing", True), 5, "after the refused calls")


# ---- 4. prefix and shards ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [3, 7])
def test_prefix_and_shards_on_the_device(eng, ci):
    case, noise, _, fill = pp.CASES[ci]
    p = problem(*case)
    model = _model(eng, p.algo, p.D, p.H, p.S)
    kw = dict(seed=pp.SEED, fill=fill, noise=noise)
    full = model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), n_samples=pp.T_MAX, **kw)
    few = model.sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), n_samples=5, **kw)
    assert few["info"] == full["info"]
    for k in ARRAYS:
        if k in full:
            assert np.array_equal(few[k], full[k][:, :5], equal_nan=True), k
    a = 11
    parts = []
    for rows, first in ((slice(0, a), 0), (slice(a, None), a)):
        n = len(range(p.N)[rows])
        suff = init_states(n, p.S, p.H, "fit", "randflip", 4, 1, 1, permanent=dict(p.permanent))
        suff["ss"], suff["lpj"] = np.array(p.ss[rows]), np.array(p.lpj[rows])
        my_data = {k: v[rows].copy() for k, v in my_data_of(p).items()}
        parts.append(_model(eng, p.algo, p.D, p.H, p.S).sample_posterior(dict(p.theta), suff, my_data, n_samples=pp.T_MAX,
                                                                         first_index=first, **kw))
    assert {k: parts[0]["info"][k] + parts[1]["info"][k] for k in full["info"]} == full["info"]
    for k in ARRAYS:
        if k in full:
            assert np.array_equal(np.concatenate((parts[0][k], parts[1][k])), full[k], equal_nan=True), k


# ---- 5. non-interference -----------------------------------------------------------------------------------------------------
def _run_steps(eng, algo, sync_host, with_call):
    N, D, H, S = 45, 10, 48, 16
    rng = np.random.RandomState(5)
    np.random.seed(6)
    Y = rng.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, rng="device", sync_host=sync_host, seed=11)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 6, 1, 1)
    out = []
    F, nu, _, theta = model.step(theta, suff, my_data)
    out.append((F, nu))
    if with_call:
        draws = model.sample_posterior(theta, suff, my_data, n_samples=3, seed=1, fill="all")
        assert np.isfinite(draws["y"]).all() and (draws["slot"] >= 0).all() and not any(draws["info"].values())
    F, nu, _, theta = model.step(theta, suff, my_data)
    out.append((F, nu))
    if with_call:
        model.sample_posterior(theta, suff, my_data, n_samples=3, seed=1)
    codes = model.encode(theta, suff, my_data, max_active=8)
    return out, eng.download_states_packed(), {k: np.array(v) for k, v in theta.items()}, codes


@pytest.mark.parametrize("sync_host", [True, False])
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_steps_and_encode_are_not_disturbed(eng, algo, sync_host):
    """Two steps with a call between them against two steps without, held as in
    tests/test_gpu_predictive.py::test_steps_and_encode_are_not_disturbed (the statistics pass sums through f64 atomics:
    Theta and what is formed under it repeat to 1e-12, K^n, S_nunique and the first step's F bit for bit)."""
    a = _run_steps(eng, algo, sync_host, with_call=False)
    b = _run_steps(eng, algo, sync_host, with_call=True)
    assert a[0][0] == b[0][0], (a[0], b[0])
    assert a[0][1][1] == b[0][1][1]
    np.testing.assert_allclose(a[0][1][0], b[0][1][0], rtol=1e-12)
    assert np.array_equal(a[1], b[1])  # K^n
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        np.testing.assert_allclose(a[2][k], b[2][k], rtol=1e-12, atol=1e-12 * float(np.max(np.abs(a[2][k]))), err_msg=k)
    for f in ("idx", "nnz", "map_slot", "map_state"):
        assert np.array_equal(getattr(a[3], f), getattr(b[3], f)), f
    for f in ("p", "m", "map_q"):
        x, y = getattr(a[3], f), getattr(b[3], f)
        assert (x is None and y is None) or np.allclose(x, y, rtol=1e-10, atol=1e-12), f


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_device_state_and_validity_are_left_as_they_are(eng, algo):
    """Fixed Theta: K^n, lpj, Theta and the codes of the statistics rows read the same bits before and after
    Engine.sample_posterior, and evoamd_debug_validity is unchanged across the call -- but for B_valid where B = Y W had
    to be formed (as every lpj pass forms it), which a second call shows: nothing changes at all."""
    N, D, H, S = 45, 10, 48, 16
    rng = np.random.RandomState(5)
    np.random.seed(6)
    Y = rng.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, rng="device", sync_host=False, seed=11)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 6, 1, 1)
    _, _, _, theta = model.step(theta, suff, my_data)
    codes0 = model.encode(theta, suff, my_data, max_active=8, dense=True)
    lpj0, ss0 = eng.download_lpj(), eng.download_states_packed()
    th0 = eng.get_params_bsc() if algo == "ebsc" else eng.get_params_sssc()
    v0 = eng.debug_validity()
    keep = ("slot", "s", "y") + (("z",) if algo == "es3c" else ())
    first = eng.sample_posterior(4, seed=3, keep=keep, fill="all")
    v1 = eng.debug_validity()
    assert {k: v for k, v in v1.items() if k != "B_valid"} == {k: v for k, v in v0.items() if k != "B_valid"}
    second = eng.sample_posterior(4, seed=3, keep=keep, fill="all")
    assert eng.debug_validity() == v1
    _same_bits(first, second)
    assert np.isfinite(first["y"]).all() and not any(first["info"].values())
    assert np.array_equal(eng.download_lpj(), lpj0) and np.array_equal(eng.download_states_packed(), ss0)
    th1 = eng.get_params_bsc() if algo == "ebsc" else eng.get_params_sssc()
    for k in th0:
        assert np.array_equal(th0[k], th1[k]), k
    codes1 = eng.posterior_codes(8, 0.0)  # the rows of the statistics pass are still the current ones
    third = model.sample_posterior(theta, suff, my_data, n_samples=4, seed=3, fill="all")
    _same_bits(first, third)
    codes2 = model.encode(theta, suff, my_data, max_active=8, dense=True)
    for f in ("idx", "p", "m", "nnz", "map_slot", "map_q", "map_state"):
        for c in (codes1, codes2):
            x, y = getattr(codes0, f), getattr(c, f)
            assert (x is None and y is None) or np.array_equal(x, y), f
    assert np.array_equal(codes0.Es, codes2.Es)


def _live():
    out = (ctypes.c_int64 * 2)()
    check(_lib.load().evoamd_debug_live_buffers(out))
    return int(out[0]), int(out[1])


def test_buffers_are_released_by_configure_and_close():
    before = _live()
    own = Engine(0)
    try:
        p = problem("es3c", 30, 25, 10, False, 1, False)
        _model(own, p.algo, p.D, p.H, p.S).sample_posterior(dict(p.theta), pp.suff_of(p), my_data_of(p), n_samples=5, seed=1)
        held = _live()
        assert held[0] > before[0]
        own.configure("sssc", p.N, p.D, p.H, p.S, 1, 4)  # the same buffers again, but for the samples: those are released
        assert _live()[0] < held[0]
        with pytest.raises(EvoAmdError, match="no results"):
            a = np.empty((p.N, 5), dtype=np.int32)
            check(own.lib.evoamd_download_posterior_samples(own._h, _lib.PSAMP_WHAT["slot"], a.ctypes.data_as(ctypes.c_void_p)))
    finally:
        own.close()
    assert _live() == before

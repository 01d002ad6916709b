"""Model.predictive_moments / Engine.predictive_moments (csrc/kernels_predictive.hpp) on the GPU.

1. the kernel against its NumPy mirror (evo_amd.models.predictive_moments_host; references from
   tests/_predictive_problems.py, computed once per shape) on the smallest shapes at which it can go wrong: N = 30 and 37
   (37 is no multiple of the 4 waves of a workgroup), D = 25 (below one wave), 64, 70 (a ragged second register per lane)
   and 512 (the limit: 8 registers per lane; 513 is refused), H = 10 and 70 (two state words), S = 8, both models, complete
   and incomplete data (with a datapoint without a reliable entry), the permanent all-zero state, the background unit,
   noise on / off, sync_host True / False.  Datapoint 0 holds states of 1, 2, 3, 4, 5, 8, 9 and 12 active latents
   (H = 10: 1 .. 5, 8, 9, 10) and, with S_perm, the all-zero state (k = 0); at H = 70 datapoint 1 holds one of 32 =
   PRED_MAX_K (S = 8 slots do not take all of them in one datapoint).
   Tolerances: mean rtol 1e-8 / atol 1e-9, var rtol 1e-8 / atol 1e-9 max(1, max |var_ref|) -- the tolerances
   tests/test_gpu_models.py holds y_reconstructed to;
2. mean at the missing entries against what Model.reconstruct writes there for the same inputs, and against the
   reference's own numbers (tests/golden/missing_*.npz), same tolerance;
3. a repeated call returns identical bits; k = 33 and float32 are refused; a singular system is counted;
4. non-interference: step / step with a call in between, encode after it, and the device state bit for bit under a
   fixed Theta.
"""
import numpy as np
import pytest

from _predictive_problems import fixture_steps, my_data_of, problem
from evo_amd._lib import EvoAmdError, check
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC, predictive_moments_host
from evo_amd.variational import init_states

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _model(eng, algo, D, H, S, sync_host=True, **kw):
    if not sync_host:
        kw.update(rng="device", sync_host=False)
    return (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, **kw)


def _suff(N, S, H, permanent, ss, lpj):
    suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1, permanent=dict(permanent))
    assert suff["ss"].shape == ss.shape and suff["lpj"].shape == lpj.shape
    suff["ss"], suff["lpj"] = np.array(ss), np.array(lpj)
    return suff


def _assert_close(mean, var, want_mean, want_var, what):
    assert mean.dtype == np.float64 and var.dtype == np.float64 and mean.shape == want_mean.shape == var.shape
    assert np.array_equal(np.isnan(mean), np.isnan(want_mean)) and np.array_equal(np.isnan(var), np.isnan(want_var)), what
    ok = ~np.isnan(want_mean)
    vmax = max(1.0, float(np.abs(want_var[ok]).max()))
    print("%s: max |mean - ref| = %.3g, max |var - ref| = %.3g (max var %.3g)"
          % (what, np.abs(mean[ok] - want_mean[ok]).max(), np.abs(var[ok] - want_var[ok]).max(), vmax))
    np.testing.assert_allclose(mean[ok], want_mean[ok], rtol=1e-8, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(var[ok], want_var[ok], rtol=1e-8, atol=1e-9 * vmax, err_msg=what)


# (algo, N, D, H, incomplete, S_perm, background), noise, sync_host
CASES = [
    (("es3c", 30, 25, 10, False, 1, False), True, True),
    (("es3c", 37, 70, 70, False, 1, False), True, False),
    (("es3c", 37, 64, 70, True, 0, False), False, True),
    (("es3c", 37, 70, 70, True, 1, False), True, True),
    (("es3c", 30, 25, 10, True, 0, True), True, False),
    (("es3c", 30, 512, 10, False, 0, False), False, True),
    (("ebsc", 37, 25, 70, False, 1, False), True, True),
    (("ebsc", 30, 70, 10, True, 0, False), False, True),
    (("ebsc", 37, 64, 10, False, 0, True), True, False),
    (("ebsc", 30, 512, 10, True, 1, False), True, True),
]


@pytest.mark.parametrize("case,noise,sync_host", CASES)
def test_kernel_equals_mirror(eng, case, noise, sync_host):
    p = problem(*case)
    model = _model(eng, p.algo, p.D, p.H, p.S, sync_host)
    suff, my_data, theta = _suff(p.N, p.S, p.H, p.permanent, p.ss, p.lpj), my_data_of(p), dict(p.theta)
    keys = (list(theta), list(suff), list(my_data))
    mean, var, info = model.predictive_moments(theta, suff, my_data, noise=noise)
    assert keys == (list(theta), list(suff), list(my_data))  # nothing written into the three dicts
    assert np.array_equal(suff["ss"], p.ss) and np.array_equal(suff["lpj"], p.lpj)
    assert info == p.info and info["n_skipped"] == (1 if p.incomplete else 0)
    _assert_close(mean, var, p.mean, p.var if noise else p.var0, repr(case))
    ok = ~np.isnan(var)
    s2 = float(p.theta["sigma"] ** 2 if p.algo == "ebsc" else p.theta["sigma2"])
    assert (var[ok] - (s2 if noise else 0.0) >= 0).all()
    # the same call again: identical bits
    mean2, var2, info2 = model.predictive_moments(theta, suff, my_data, noise=noise)
    assert np.array_equal(mean, mean2, equal_nan=True) and np.array_equal(var, var2, equal_nan=True) and info2 == info


def test_d_above_the_register_limit_is_refused(eng):
    p = problem("ebsc", 30, 512, 10, True, 1, False)
    D = 513
    rng = np.random.RandomState(1)
    model = _model(eng, "ebsc", D, p.H, p.S)
    theta = {"W": rng.normal(size=(D, p.H)), "pi": 0.1, "sigma": np.float64(1.0)}
    my_data = {"y": rng.normal(size=(p.N, D)), "x_infr": np.ones((p.N, D), dtype=bool)}
    with pytest.raises(EvoAmdError, match="D = 513"):
        model.predictive_moments(theta, _suff(p.N, p.S, p.H, p.permanent, p.ss, p.lpj), my_data)


@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_mean_equals_reconstruct_and_the_reference(eng, algo):
    """The inputs of the missing_* fixtures: Model.reconstruct (the reference-pinned route through the statistics pass) and
    the fixture's y_reconstructed against the new kernel's mean at the missing entries of datapoints with data."""
    g, steps = fixture_steps(algo)
    N, D, H, S = int(g["N"]), int(g["D"]), int(g["H"]), int(g["S"])
    x_infr = g["x_infr"]
    miss = ~x_infr & x_infr.any(axis=1)[:, None]
    permanent = {"background": False, "allzero": False, "singletons": False}
    for t, theta, ss, lpj, y_rec in steps:
        model = _model(eng, algo, D, H, S)
        my_data = {"y": np.array(g["Y"]), "x_infr": np.array(x_infr), "x": np.array(x_infr)}
        suff = _suff(N, S, H, permanent, ss, lpj)
        mean, var, info = model.predictive_moments(dict(theta), suff, my_data)
        model.reconstruct(my_data, suff, dict(theta))
        rec = np.asarray(my_data["y_reconstructed"])
        print("%s step %d: max |mean - reconstruct| = %.3g, max |mean - fixture| = %.3g"
              % (algo, t, np.abs(mean[miss] - rec[miss]).max(), np.abs(mean[miss] - y_rec[miss]).max()))
        np.testing.assert_allclose(mean[miss], rec[miss], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(mean[miss], y_rec[miss], rtol=1e-8, atol=1e-9)
        want_mean, want_var, want_info = predictive_moments_host("bsc" if algo == "ebsc" else "sssc", theta, ss, lpj, g["Y"], x_infr)
        assert info == want_info
        _assert_close(mean, var, want_mean, want_var, "%s fixture step %d" % (algo, t))


@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_more_than_32_active_latents_raise(eng, algo):
    p = problem(algo, 37, 25 if algo == "ebsc" else 64, 70, False if algo == "ebsc" else True, 1 if algo == "ebsc" else 0, False)
    ss = np.array(p.ss)
    assert ss[1, 2].sum() == 32
    ss[1, 2, np.flatnonzero(~ss[1, 2])[0]] = True
    model = _model(eng, algo, p.D, p.H, p.S)
    with pytest.raises(EvoAmdError, match=r"n = 1 .*k = 33"):
        model.predictive_moments(dict(p.theta), _suff(p.N, p.S, p.H, p.permanent, ss, p.lpj), my_data_of(p))
    with pytest.raises(EvoAmdError, match="no results"):  # nothing is handed out after the refused call
        check(eng.lib.evoamd_download_predictive(eng._h, None, None))
    # the context serves the next call
    mean, var, info = model.predictive_moments(dict(p.theta), _suff(p.N, p.S, p.H, p.permanent, p.ss, p.lpj), my_data_of(p))
    _assert_close(mean, var, p.mean, p.var, "after the refused call")


def test_float32_mode_is_refused(eng):
    N, D, H, S = 32, 8, 16, 8
    np.random.seed(4)
    Y = np.random.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = BSC(D, H, S, engine=eng, dtype=np.float32)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1)
    with pytest.raises(NotImplementedError, match="float32 mode"):
        model.predictive_moments(theta, suff, my_data)


def test_singular_system_is_counted(eng):
    """A dead latent (zero row and column of Psi) in one state of datapoint 2, whose reliable entries see W_A = 0."""
    rng = np.random.RandomState(4)
    H, D, N, S = 10, 25, 30, 8
    p = problem("es3c", N, D, H, True, 0, False)
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
    Y = np.where(x_infr, rng.normal(size=(N, D)), np.nan)
    my_data = {"y": Y, "x_infr": x_infr, "x": x_infr.copy()}
    want_mean, want_var, want_info = predictive_moments_host("sssc", theta, ss, p.lpj, Y, x_infr)
    assert want_info == {"n_singular": 1, "n_skipped": 1}
    model = _model(eng, "es3c", D, H, S)
    mean, var, info = model.predictive_moments(theta, _suff(N, S, H, p.permanent, ss, p.lpj), my_data)
    assert info == want_info and np.isnan(mean[2]).all() and np.isnan(var[2]).all()
    _assert_close(mean, var, want_mean, want_var, "singular")


# ---- 4. non-interference ----------------------------------------------------------------------------------------------------
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
        mean, var, info = model.predictive_moments(theta, suff, my_data)
        assert np.isfinite(mean).all() and (var > 0).all() and info == {"n_singular": 0, "n_skipped": 0}
    F, nu, _, theta = model.step(theta, suff, my_data)
    out.append((F, nu))
    if with_call:
        model.predictive_moments(theta, suff, my_data)
    codes = model.encode(theta, suff, my_data, max_active=8)
    return out, eng.download_states_packed(), {k: np.array(v) for k, v in theta.items()}, codes


@pytest.mark.parametrize("sync_host", [True, False])
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_steps_and_encode_are_not_disturbed(eng, algo, sync_host):
    """Two steps with a call between them against two steps without.  K^n, S_nunique and the first step's F are compared
    bit for bit.  The statistics pass sums through f64 atomics, which are not bit-reproducible run to run (DESIGN section
    4; tests/test_gpu_patches.py::test_merge_between_em_steps_leaves_trajectory): two runs WITHOUT the call already differ
    in the last bits of Theta (observed here: W), so Theta and the second step's F, which is formed under that Theta, are
    held to 1e-12 of their largest entry as there, and the bit-for-bit statement about the device state is made with a
    fixed Theta in test_device_state_is_left_bit_for_bit below."""
    a = _run_steps(eng, algo, sync_host, with_call=False)
    b = _run_steps(eng, algo, sync_host, with_call=True)
    assert a[0][0] == b[0][0], (a[0], b[0])  # F and S_nunique of the first step
    assert a[0][1][1] == b[0][1][1]  # S_nunique of the second
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
def test_device_state_is_left_bit_for_bit(eng, algo):
    """Fixed Theta (deterministic kernels only): K^n, lpj, Theta and the codes of a statistics pass read the same bits
    before and after Engine.predictive_moments, and encode after the Model call returns the codes it returned before."""
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
    mean, var, info = eng.predictive_moments()
    assert np.isfinite(mean).all() and (var > 0).all() and info == {"n_singular": 0, "n_skipped": 0}
    assert np.array_equal(eng.download_lpj(), lpj0) and np.array_equal(eng.download_states_packed(), ss0)
    th1 = eng.get_params_bsc() if algo == "ebsc" else eng.get_params_sssc()
    for k in th0:
        assert np.array_equal(th0[k], th1[k]), k
    codes1 = eng.posterior_codes(8, 0.0)  # the rows of the statistics pass are still the current ones
    mean2, var2, _ = model.predictive_moments(theta, suff, my_data)
    assert np.array_equal(mean, mean2) and np.array_equal(var, var2)
    codes2 = model.encode(theta, suff, my_data, max_active=8, dense=True)
    for f in ("idx", "p", "m", "nnz", "map_slot", "map_q", "map_state"):
        for c in (codes1, codes2):
            x, y = getattr(codes0, f), getattr(c, f)
            assert (x is None and y is None) or np.array_equal(x, y), f
    assert np.array_equal(codes0.Es, codes2.Es)

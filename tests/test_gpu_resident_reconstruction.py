"""The reconstruction kept on the device (Model(resident_reconstruction=True), Engine.reconstruct_resident /
patches_merge_resident, the ResidentReconstruction handle).

The yardstick is the existing path on the SAME device state: after a resident step Engine.reconstruct() still returns
the y_hat of that statistics pass; the five-line host rule of Model._write_reconstruction applied to it is the array the
default path would have stored, and OverlappingPatches.set_and_merge of that array (tests/test_gpu_patches.py ties it to
NumPy bit for bit) is the expected image.  Everything is compared with assert_array_equal (NaN-aware), no tolerance.
Two separate models (flag off / on) are compared bit for bit in K^n, F and the counters, Theta / lpj to the 1e-12 of
test_gpu_patches.py::test_merge_between_em_steps_leaves_trajectory (f64 atomics in the statistics pass): as free
trajectories (test_flag_leaves_trajectory*) and step by step from shared inputs (test_flag_leaves_every_step)."""
import os

import numpy as np
import pytest

from evo_amd._lib import EvoAmdError, check, dptr
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.resident import ResidentReconstruction
from evo_amd.utils.prepost import MultiDimOverlappingPatches, OverlappingPatches, mean_merger, median_merger
from evo_amd.variational import init_states
from test_prepost_host import oracle_extract

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H_LAT, S_ST = 32, 20


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _images():
    return dict(np.load(os.path.join(GOLDEN, "images.npz")))


def _host_rule(my_data, y_hat):
    """Model._write_reconstruction, restated."""
    y_rec = my_data["y"].copy()
    miss = np.logical_not(my_data["x"])
    if not my_data["x_infr"].all():
        miss &= my_data["x_infr"].any(axis=1)[:, None]
    y_rec[miss] = y_hat[miss]
    return y_rec


def _setup(kind, seed=0, block=None):
    """The denoising (house_r04, 5 x 5, x all False) and inpainting (castle_r01, 5 x 5 x 3, x = x_infr) set-ups of
    tests/test_gpu_patches.py.  ``block``: (top, left, size) of a square blanked in every channel (inpainting)."""
    rng = np.random.RandomState(seed)
    if kind == "denoise":
        clean = _images()["house_r04"].astype(np.float64)
        ovp = OverlappingPatches(rng.normal(clean, scale=25), 5, 5, patch_shift=1)
        Y = ovp.get().T
        my_data = {"y": Y, "x_infr": np.logical_not(np.isnan(Y)), "x": np.zeros_like(Y)}
    else:
        clean = _images()["castle_r01"].astype(np.float64)
        incomplete = clean.copy()
        incomplete[rng.random_sample(clean.shape) <= 0.1] = np.nan
        if block is not None:
            t, l, b = block
            incomplete[t:t + b, l:l + b, :] = np.nan
        ovp = MultiDimOverlappingPatches(incomplete, 5, 5, patch_shift=1)
        Y = ovp.get().T
        my_data = {"y": Y, "x_infr": np.logical_not(np.isnan(Y)), "x": np.logical_not(np.isnan(Y))}
    return ovp, my_data


def _model(algo, my_data, seed=0, **kw):
    np.random.seed(seed)
    N, D = my_data["y"].shape
    if algo == "es3c" and not my_data["x_infr"].all():
        kw.setdefault("to_learn", ["W", "pies", "sigma2"])
    model = {"ebsc": BSC, "es3c": SSSC}[algo](D, H_LAT, S_ST, **kw)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S_ST, H_LAT, "fit", "randflip", 10, 1, 1)
    return model, theta, suff


def _check_epoch(model, ovp, my_data):
    """One reconstructing epoch has run in resident mode: handle, both merged images and the materialised array against
    the existing path fed with the y_hat the device still holds."""
    h = my_data["y_reconstructed"]
    assert isinstance(h, ResidentReconstruction) and h.resident and not h.materialised
    assert h.shape == my_data["y"].shape and h.T.shape == my_data["y"].shape[::-1] and h.T.T is h
    got_mean = ovp.set_and_merge(h.T, merge_method=mean_merger)
    got_median = ovp.set_and_merge(h.T, merge_method=median_merger)
    assert not h.materialised  # merging did not bring the N x D array over
    expected = _host_rule(my_data, model.engine.reconstruct())
    want_mean = ovp.set_and_merge(expected.T, merge_method=mean_merger)
    want_median = ovp.set_and_merge(expected.T, merge_method=median_merger)
    np.testing.assert_array_equal(got_mean, want_mean)
    np.testing.assert_array_equal(got_median, want_median)
    got = np.asarray(h)
    assert got.dtype == np.float64 and got.flags.c_contiguous
    np.testing.assert_array_equal(got, expected)
    np.testing.assert_array_equal(np.asarray(h.T), expected.T)
    assert h.materialised and np.asarray(h) is got
    return expected, want_mean, want_median


@pytest.mark.parametrize("kind", ["denoise", "inpaint"])
@pytest.mark.parametrize("device_mstep", [False, True])
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_every_epoch_equals_existing_path(algo, device_mstep, kind):
    ovp, my_data = _setup(kind)
    model, theta, suff = _model(algo, my_data, device_mstep=device_mstep, resident_reconstruction=True)
    for epoch in range(3):
        F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
        assert np.isfinite(F)
        expected, want_mean, _ = _check_epoch(model, ovp, my_data)
        if kind == "inpaint":
            assert not np.isnan(want_mean).any()
        assert not np.array_equal(expected, my_data["y"])  # something was reconstructed


def _two_runs(algo, device_mstep):
    """Flag off / on, same seeds, rng="reference", the inpainting set-up (the M-step reads y_reconstructed, and from the
    second epoch on _prepare meets the handle of the epoch before).  Per epoch: (F, nu, nsub, counters, K^n, arrays)."""
    runs = []
    for flag in (False, True):
        ovp, my_data = _setup("inpaint")
        model, theta, suff = _model(algo, my_data, device_mstep=device_mstep, rng="reference",
                                    resident_reconstruction=flag)
        out = []
        for epoch in range(3):
            F, nu, nsub, theta = model.step(theta, suff, my_data, do_reconstruction=True)
            counters = tuple(suff[k] for k in ("reset_lpj_isnan", "reset_lpj_smaller_eps_lpj", "reset_lpj_isinf"))
            arrays = [np.array(theta["W"], copy=True), np.array(theta["sigma" if algo == "ebsc" else "sigma2"], ndmin=1),
                      np.array(theta["pi" if algo == "ebsc" else "pies"], ndmin=1, dtype=np.float64), suff["lpj"].copy()]
            out.append((F, nu, nsub, counters, suff["ss"].copy(), arrays))
            assert isinstance(my_data["y_reconstructed"], ResidentReconstruction) == flag
        runs.append(out)
    return runs


def _close(x, y):
    # the 1e-12 of test_gpu_patches.py::test_merge_between_em_steps_leaves_trajectory (f64 atomics of the statistics pass)
    np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12 * float(np.max(np.abs(x))))


@pytest.mark.parametrize("device_mstep", [False, True])
def test_flag_leaves_trajectory(device_mstep):
    """K^n, F and the counters equal in every epoch, Theta and lpj to 1e-12.  EBSC: its F is reproducible between two
    runs of the unchanged default path (measured on MI355X, three runs with the flag off, both M-steps: the same bits in
    all three epochs), so the bit comparison is a statement about the flag."""
    for a, b in zip(*_two_runs("ebsc", device_mstep)):
        assert a[0] == b[0] and a[1:4] == b[1:4]
        np.testing.assert_array_equal(a[4], b[4])
        for x, y in zip(a[5], b[5]):
            _close(x, y)


@pytest.mark.parametrize("device_mstep", [False, True])
def test_flag_leaves_trajectory_es3c(device_mstep):
    """ES3C on incomplete data, two free-running models: K^n and the counters equal in every epoch, Theta and lpj to
    1e-12, F bit for bit in epoch 1 -- it is formed before any M-step, from the same Theta^init, K^n and data in both
    runs.  From epoch 2 on F of two free runs is NOT a bit-for-bit yardstick on this path, flag or no flag: the
    statistics pass of ES3C on incomplete data sums its pair moments and the y_hat^2 trace through f64 atomics that no
    option pins ("pair_bins" needs complete data), Theta^new differs in its last bits between two runs of the unchanged
    default path, and F of the next epoch follows it (measured on MI355X, flag off, three runs, epoch 2:
    F = -365.81562568727463 / ...446 / ...463 with the host M-step, ...458 / ...458 / ...446 with the device M-step:
    2-3 ulp).  The bit comparison of F in EVERY epoch is made by test_flag_leaves_every_step below, where both models
    start every epoch from the same Theta and K^n."""
    for epoch, (a, b) in enumerate(zip(*_two_runs("es3c", device_mstep))):
        if epoch == 0:
            assert a[0] == b[0]
        assert a[1:4] == b[1:4]
        np.testing.assert_array_equal(a[4], b[4])
        for x, y in zip(a[5], b[5]):
            _close(x, y)


def _copy_theta(theta):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in theta.items()}


@pytest.mark.parametrize("device_mstep", [False, True])
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_flag_leaves_every_step(algo, device_mstep):
    """Flag off / on, inpainting set-up, rng="reference", three epochs, and in EVERY epoch K^n, F and the counters bit
    for bit, Theta^new and lpj to 1e-12.  So that the atomics of one epoch's M-step cannot leak into the next epoch's F
    (see test_flag_leaves_trajectory_es3c), both models start each epoch from the same inputs: the flag-off model's
    Theta^new and K^n of the epoch before (copies), and the same np.random state.  Each step still runs whole in both
    models -- E-step, statistics pass with the reconstruction, M-step reading y_reconstructed (in resident mode the
    device copy: _prepare meets the handle of the epoch before and uploads nothing) -- only the carry-over is shared."""
    models = []
    for flag in (False, True):
        ovp, my_data = _setup("inpaint")
        model, theta, suff = _model(algo, my_data, device_mstep=device_mstep, rng="reference",
                                    resident_reconstruction=flag)
        models.append([model, my_data, suff])
    carry = theta  # Theta^init: the same numbers in both (same seed)
    for epoch in range(3):
        ss_in, lpj_in = models[0][2]["ss"].copy(), models[0][2]["lpj"].copy()
        rng_state = np.random.get_state()
        out = []
        for model, my_data, suff in models:
            suff["ss"][...] = ss_in
            suff["lpj"][...] = lpj_in
            np.random.set_state(rng_state)
            F, nu, nsub, theta = model.step(_copy_theta(carry), suff, my_data, do_reconstruction=True)
            counters = tuple(suff[k] for k in ("reset_lpj_isnan", "reset_lpj_smaller_eps_lpj", "reset_lpj_isinf"))
            out.append((F, nu, nsub, counters, _copy_theta(theta)))
        a, b = out
        print("epoch %d %s device_mstep=%s: F off %.17g on %.17g" % (epoch + 1, algo, device_mstep, a[0], b[0]))
        assert a[0] == b[0] and a[1:4] == b[1:4]
        np.testing.assert_array_equal(models[0][2]["ss"], models[1][2]["ss"])
        _close(models[0][2]["lpj"], models[1][2]["lpj"])
        for k in ("W", "sigma", "pi") if algo == "ebsc" else ("W", "sigma2", "pies"):
            _close(np.asarray(a[4][k], dtype=np.float64), np.asarray(b[4][k], dtype=np.float64))
        assert isinstance(models[1][1]["y_reconstructed"], ResidentReconstruction)
        assert isinstance(models[0][1]["y_reconstructed"], np.ndarray)
        carry = a[4]


def test_new_mask_object_with_an_old_handle():
    """my_data gets a new x_infr object while it still carries the handle of the epoch before: the upload of the masks
    drops the device's y_reconstructed, which a step WITHOUT reconstruction needs for its M-step (bsc.py:186).  The
    default path uploads the old ndarray; the resident path must fetch the handle before the masks go up and do the
    same.  Same inputs for both steps as in test_flag_leaves_every_step."""
    models = []
    for flag in (False, True):
        ovp, my_data = _setup("inpaint")
        model, theta, suff = _model("ebsc", my_data, rng="reference", resident_reconstruction=flag)
        models.append([model, my_data, suff])
    carry = theta
    for epoch, rec in enumerate((True, False)):
        ss_in, lpj_in = models[0][2]["ss"].copy(), models[0][2]["lpj"].copy()
        rng_state = np.random.get_state()
        out = []
        for model, my_data, suff in models:
            if epoch == 1:
                my_data["x_infr"] = my_data["x_infr"].copy()  # a new array object, the same masks
            suff["ss"][...] = ss_in
            suff["lpj"][...] = lpj_in
            np.random.set_state(rng_state)
            F, nu, nsub, theta = model.step(_copy_theta(carry), suff, my_data, do_reconstruction=rec)
            out.append((F, nu, nsub, _copy_theta(theta)))
        a, b = out
        assert a[:3] == b[:3]
        np.testing.assert_array_equal(models[0][2]["ss"], models[1][2]["ss"])
        for k in ("W", "sigma", "pi"):
            _close(np.asarray(a[3][k], dtype=np.float64), np.asarray(b[3][k], dtype=np.float64))
        carry = a[3]
    h = models[1][1]["y_reconstructed"]
    assert isinstance(h, ResidentReconstruction) and h.materialised
    np.testing.assert_array_equal(np.asarray(h), models[0][1]["y_reconstructed"])


@pytest.mark.parametrize("device_mstep", [False, True])
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_patch_without_reliable_entry_keeps_nan(algo, device_mstep):
    """A blanked 11 x 11 block (patches are 5 x 5): the patches wholly inside it have no reliable entry, the host rule
    keeps their rows as they are (NaN), and the 3 x 3 pixels that only such patches cover have no valid estimate.
    The device holds zeros in those entries of Y; the merge must read NaN there."""
    top, left, b = 20, 10, 11
    ovp, my_data = _setup("inpaint", block=(top, left, b))
    empty = np.logical_not(my_data["x_infr"].any(axis=1))
    assert empty.sum() == (b - 4) ** 2  # checked on the CPU: 49 patches without a reliable entry
    no_estimate = np.zeros(ovp.shape, dtype=bool)
    no_estimate[top + 4:top + b - 4, left + 4:left + b - 4, :] = True  # covered by such patches only
    assert no_estimate.sum() == 27
    model, theta, suff = _model(algo, my_data, device_mstep=device_mstep, resident_reconstruction=True)
    for epoch in range(3):
        F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
        expected, want_mean, want_median = _check_epoch(model, ovp, my_data)
        assert np.isnan(expected[empty]).all()
        np.testing.assert_array_equal(np.isnan(want_mean), no_estimate)
        np.testing.assert_array_equal(np.isnan(want_median), no_estimate)


@pytest.mark.parametrize("masks", ["complete", "incomplete"])
@pytest.mark.parametrize("shape,ph,pw,s", [((23, 19, 3), 3, 7, 2), ((41, 38, 3), 5, 5, 3), ((30, 26), 4, 6, 3),
                                           ((24, 31), 3, 7, 1)])
def test_engine_calls_shift_and_non_square(shape, ph, pw, s, masks):
    """Engine.reconstruct_resident + patches_merge_resident against reconstruct + host rule + patches_merge: patch
    shifts above 1, non-square patches, a keep-mask on complete data (uploaded once, reused), both merge routes."""
    rng = np.random.RandomState(3)
    img = rng.normal(size=shape)
    Y = oracle_extract(img, ph, pw, s)
    N, D = Y.shape
    if masks == "incomplete":
        xi = rng.random_sample(Y.shape) < 0.8
        xi[N // 2] = False
        Y = np.where(xi, Y, np.nan)
        my_data = {"y": Y, "x_infr": xi, "x": xi.copy()}
    else:
        my_data = {"y": Y, "x_infr": np.ones(Y.shape, dtype=bool), "x": rng.random_sample(Y.shape) < 0.3}
    np.random.seed(1)
    model = BSC(D, 12, 8)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, 8, 12, "fit", "randflip", 4, 1, 1)
    e = model.engine
    for it in range(2):
        F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)  # default mode: ndarray
        assert isinstance(my_data["y_reconstructed"], np.ndarray)
        expected = _host_rule(my_data, e.reconstruct())
        np.testing.assert_array_equal(my_data["y_reconstructed"], expected)
        serial = e.reconstruct_resident(my_data["x"])
        for method in ("mean", "median"):
            want = e.patches_merge(expected, shape, ph, pw, s, method)
            np.testing.assert_array_equal(e.patches_merge_resident(shape, ph, pw, s, method, serial=serial), want)
            e.set_option("merge_select_fused", 1)  # the other route: the merge kernels select while they gather
            try:
                np.testing.assert_array_equal(e.patches_merge_resident(shape, ph, pw, s, method), want)
            finally:
                e.set_option("merge_select_fused", 0)
        np.testing.assert_array_equal(e.download_reconstruction(serial), e.reconstruct())
    if masks == "complete":  # x = None: every entry is the estimate
        y_hat = e.reconstruct()
        e.reconstruct_resident(None)
        np.testing.assert_array_equal(e.patches_merge_resident(shape, ph, pw, s, "mean"),
                                      e.patches_merge(y_hat, shape, ph, pw, s, "mean"))


def test_no_n_by_d_array_crosses(monkeypatch):
    ovp, my_data = _setup("inpaint")
    model, theta, suff = _model("ebsc", my_data, device_mstep=True, resident_reconstruction=True)
    F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)

    def forbidden(name):
        def f(*a, **k):
            raise AssertionError("Engine.%s moves an N x D array: not in resident mode" % name)
        return f

    for name in ("reconstruct", "patches_merge", "upload_yrec"):
        monkeypatch.setattr(Engine, name, forbidden(name))
    for epoch in range(2):
        F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
        img = ovp.set_and_merge(my_data["y_reconstructed"].T, merge_method=mean_merger)
        assert img.shape == ovp.shape and not np.isnan(img).any()
        assert not my_data["y_reconstructed"].materialised
    monkeypatch.undo()
    ovp2, my_data2 = _setup("denoise")
    model2, theta2, suff2 = _model("es3c", my_data2, resident_reconstruction=True)
    for name in ("reconstruct", "patches_merge", "upload_yrec"):
        monkeypatch.setattr(Engine, name, forbidden(name))
    F, _, _, theta2 = model2.step(theta2, suff2, my_data2, do_reconstruction=True)
    img = ovp2.set_and_merge(my_data2["y_reconstructed"].T, merge_method=median_merger)
    assert img.shape == ovp2.shape and not np.isnan(img).any()


def test_merge_resident_leaves_em_state_bit_for_bit():
    """As test_gpu_patches.py::test_merge_leaves_em_state_bit_for_bit: lpj of the resident K^n, K^n and Theta before
    and after the merges (deterministic kernels only)."""
    ovp, my_data = _setup("inpaint")
    model, theta, suff = _model("ebsc", my_data, resident_reconstruction=True)
    model.step(theta, suff, my_data, do_reconstruction=True)
    e = model.engine
    h = my_data["y_reconstructed"]
    e.lpj_resident()
    lpj0, ss0, th0 = e.download_lpj(), e.download_states(), e.get_params_bsc()
    imgs = [ovp.set_and_merge(h.T, merge_method=m) for m in (mean_merger, median_merger, mean_merger)]
    np.testing.assert_array_equal(imgs[0], imgs[2])
    e.lpj_resident()
    np.testing.assert_array_equal(e.download_lpj(), lpj0)
    np.testing.assert_array_equal(e.download_states(), ss0)
    th1 = e.get_params_bsc()
    for k in th0:
        np.testing.assert_array_equal(th0[k], th1[k])
    assert h.resident  # lpj passes do not outdate it
    np.testing.assert_array_equal(ovp.set_and_merge(h.T, merge_method=mean_merger), imgs[0])


def test_stale_handle_raises():
    ovp, my_data = _setup("denoise")
    model, theta, suff = _model("ebsc", my_data, resident_reconstruction=True)
    F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
    first = my_data["y_reconstructed"]
    F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
    second = my_data["y_reconstructed"]
    assert second is not first and not first.resident and second.resident
    with pytest.raises(RuntimeError, match="later reconstruction"):
        ovp.set_and_merge(first.T, merge_method=mean_merger)
    with pytest.raises(RuntimeError, match="later reconstruction"):
        np.asarray(first)
    # a step WITHOUT reconstruction runs a statistics pass too: the library refuses, the handle reports it
    F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=False)
    with pytest.raises(RuntimeError, match="outdated"):
        ovp.set_and_merge(second.T, merge_method=median_merger)
    with pytest.raises(RuntimeError, match="outdated"):
        np.asarray(second)
    # read in time: the cached array survives later steps, and merging it takes the host path
    F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
    third = my_data["y_reconstructed"]
    kept = np.asarray(third).copy()
    want = ovp.set_and_merge(kept.T, merge_method=mean_merger)
    F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
    np.testing.assert_array_equal(np.asarray(third), kept)
    np.testing.assert_array_equal(ovp.set_and_merge(third.T, merge_method=mean_merger), want)


def test_library_refuses_without_reconstruction(eng):
    rng = np.random.RandomState(2)
    shape, ph, pw = (20, 18), 4, 4
    Y = oracle_extract(rng.normal(size=shape), ph, pw, 1)
    N, D = Y.shape
    out = np.zeros(shape)
    args = (shape[0], shape[1], 1, ph, pw, 1, 0)
    with pytest.raises(EvoAmdError):  # unconfigured context
        check(eng.lib.evoamd_patches_merge_resident(eng._h, *args, dptr(out)))
    np.random.seed(2)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool), "x": np.zeros_like(Y, dtype=bool)}
    model = BSC(D, 12, 8, engine=eng)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, 8, 12, "fit", "randflip", 4, 1, 1)
    F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)  # default mode: nothing made resident
    with pytest.raises(EvoAmdError, match="no current resident reconstruction"):
        eng.patches_merge_resident(shape, ph, pw, 1, "mean")
    with pytest.raises(EvoAmdError, match="no current resident reconstruction"):
        eng.download_reconstruction()
    assert (out == 0.0).all()
    eng.reconstruct_resident(None)
    img = eng.patches_merge_resident(shape, ph, pw, 1, "mean")
    np.testing.assert_array_equal(img, eng.patches_merge(eng.reconstruct(), shape, ph, pw, 1, "mean"))
    for outdate in ("stats", "params", "data"):
        eng.reconstruct_resident(None)
        if outdate == "stats":
            eng.stats()
        elif outdate == "params":
            eng.set_params_bsc(theta["W"], theta["pi"], theta["sigma"])
            eng.stats()  # (Es rows of the new Theta: the old reconstruction stays outdated)
        else:
            eng.upload_data(Y)
        with pytest.raises(EvoAmdError, match="no current resident reconstruction"):
            eng.patches_merge_resident(shape, ph, pw, 1, "median")
    # method and geometry arguments are checked like evoamd_patches_merge checks them
    eng.reconstruct_resident(None)
    with pytest.raises(EvoAmdError):
        check(eng.lib.evoamd_patches_merge_resident(eng._h, shape[0], shape[1], 1, ph, pw, 1, 2, dptr(out)))
    with pytest.raises(EvoAmdError):
        check(eng.lib.evoamd_patches_merge_resident(eng._h, shape[0], shape[1], 1, ph, pw, 0, 0, dptr(out)))
    with pytest.raises(EvoAmdError, match="patch geometry"):  # another (N, D) than the context's
        check(eng.lib.evoamd_patches_merge_resident(eng._h, shape[0] + 1, shape[1], 1, ph, pw, 1, 0, dptr(out)))


def test_geometry_mismatch_and_float32():
    ovp, my_data = _setup("denoise")
    model, theta, suff = _model("ebsc", my_data, resident_reconstruction=True)
    model.step(theta, suff, my_data, do_reconstruction=True)
    h = my_data["y_reconstructed"]
    other = OverlappingPatches(np.zeros((40, 40)), 5, 5)
    with pytest.raises(ValueError):
        other.set_and_merge(h.T, merge_method=mean_merger)
    with pytest.raises(ValueError):
        model.engine.patches_merge_resident((40, 40), 5, 5, 1, "mean")
    assert h.resident
    # float32 EBSC has no reconstruction; the flag changes nothing about that (D, H multiples of 4: float32 rows)
    rng = np.random.RandomState(0)
    Y32 = rng.normal(size=(256, 24))
    data32 = {"y": Y32, "x_infr": np.ones(Y32.shape, dtype=bool), "x": np.zeros(Y32.shape, dtype=bool)}
    for flag in (False, True):
        m32, th32, suff32 = _model("ebsc", data32, dtype=np.float32, device_mstep=True, resident_reconstruction=flag)
        F, _, _, th32 = m32.step(th32, suff32, data32)  # the mode itself works
        assert np.isfinite(F)
        with pytest.raises(EvoAmdError, match="reconstruction is not available in the float32 mode"):
            m32.step(th32, suff32, data32, do_reconstruction=True)
    e32 = m32.engine
    with pytest.raises(EvoAmdError, match="reconstruction is not available in the float32 mode"):
        e32.reconstruct_resident(None)

"""Overlapping image patches on the GPU (evoamd_patches_extract / evoamd_patches_merge through evo_amd.utils.prepost):
bit parity with the NumPy oracle of tests/test_prepost_host.py, round trips, isolation from the EM state of a configured
context, and the two image workflows of the reference's examples end to end."""
import os

import numpy as np
import pytest

from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.utils.prepost import MultiDimOverlappingPatches, OverlappingPatches, mean_merger, median_merger, psnr
from evo_amd.variational import init_states
from test_prepost_host import oracle_extract, oracle_stack

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _images():
    return dict(np.load(os.path.join(GOLDEN, "images.npz")))


class _quiet:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", RuntimeWarning)

    def __exit__(self, *a):
        return self._w.__exit__(*a)


def _want(Y, shape, ph, pw, s):
    st = oracle_stack(Y, shape, ph, pw, s)
    with _quiet():
        return np.nanmean(st, axis=0), np.nanmedian(st, axis=0)


# (shape, ph, pw, shift): grey and RGB, 1x1 .. 32x32, patch == image, shifts 1..3 with border patches
CASES = [
    ((20, 17), 1, 1, 1),
    ((24, 31), 3, 7, 1),
    ((23, 19, 3), 3, 7, 2),
    ((40, 37), 5, 5, 1),
    ((41, 38, 3), 5, 5, 3),
    ((48, 45), 8, 8, 1),
    ((35, 29, 3), 8, 8, 2),
    ((50, 47), 16, 16, 1),
    ((37, 43, 3), 16, 16, 3),
    ((40, 36), 32, 32, 1),
    ((45, 40), 32, 32, 2),
    ((9, 11, 3), 9, 11, 1),  # patch == image: N = 1
    ((12, 12), 12, 12, 3),
    ((30, 26), 4, 6, 3),  # even and odd estimate counts side by side
]


@pytest.mark.parametrize("nan_frac", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("shape,ph,pw,s", CASES)
def test_parity(eng, shape, ph, pw, s, nan_frac):
    rng = np.random.RandomState(hash((shape, ph, pw, s)) % 2**31)
    img = rng.normal(size=shape)
    img[rng.random_sample(shape) < nan_frac * 0.5] = np.nan  # NaN pixels pass through extract
    ovp = (MultiDimOverlappingPatches if len(shape) == 3 else OverlappingPatches)(img, ph, pw, s, engine=eng)
    Y_T = ovp.get()
    Y = oracle_extract(img, ph, pw, s)
    np.testing.assert_array_equal(Y_T.T, Y)
    assert Y_T.shape == (ph * pw * (shape[2] if len(shape) == 3 else 1), Y.shape[0])
    # merge input: a reconstruction with NaN estimates (some pixels have none at 100 %)
    R = rng.normal(size=Y.shape)
    R[rng.random_sample(Y.shape) < nan_frac] = np.nan
    want_mean, want_median = _want(R, shape, ph, pw, s)
    np.testing.assert_array_equal(ovp.set_and_merge(R.T, merge_method=mean_merger), want_mean)
    np.testing.assert_array_equal(ovp.set_and_merge(R.T, merge_method=median_merger), want_median)
    if nan_frac == 1.0:
        assert np.isnan(want_mean).all()


def test_parity_integer_ties(eng):
    """Few distinct values: many equal estimates, even counts whose two middle values differ and agree."""
    rng = np.random.RandomState(5)
    shape, ph, pw, s = (33, 30, 3), 6, 4, 1
    R = rng.randint(-3, 4, size=(28 * 27, ph * pw * 3)).astype(np.float64)
    R[rng.random_sample(R.shape) < 0.25] = np.nan
    want_mean, want_median = _want(R, shape, ph, pw, s)
    np.testing.assert_array_equal(eng.patches_merge(R, shape, ph, pw, s, "mean"), want_mean)
    np.testing.assert_array_equal(eng.patches_merge(R, shape, ph, pw, s, "median"), want_median)


@pytest.mark.parametrize("nan_frac", [0.0, 0.3])
def test_parity_1024(eng, nan_frac):
    rng = np.random.RandomState(11)
    shape, ph, pw = (1024, 1024), 8, 8
    img = rng.normal(size=shape)
    Y = eng.patches_extract(img, ph, pw, 1)
    np.testing.assert_array_equal(Y, oracle_extract(img, ph, pw, 1))
    Y += rng.normal(scale=0.1, size=Y.shape)
    Y[rng.random_sample(Y.shape) < nan_frac] = np.nan
    want_mean, want_median = _want(Y, shape, ph, pw, 1)
    np.testing.assert_array_equal(eng.patches_merge(Y, shape, ph, pw, 1, "mean"), want_mean)
    np.testing.assert_array_equal(eng.patches_merge(Y, shape, ph, pw, 1, "median"), want_median)


@pytest.mark.parametrize("shape,ph,pw,s", [((64, 48), 8, 8, 1), ((30, 41, 3), 5, 7, 2), ((16, 16), 16, 16, 1)])
def test_round_trip_and_views(eng, shape, ph, pw, s):
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, size=shape).astype(np.uint8)  # integer image: cast to float64
    ovp = (MultiDimOverlappingPatches if len(shape) == 3 else OverlappingPatches)(img, ph, pw, s, engine=eng)
    Y_T = ovp.get()
    for m in (mean_merger, median_merger):
        out = ovp.merge(m)
        assert out.dtype == np.float64 and out.shape == shape
        np.testing.assert_array_equal(out, img)
    # the transposed view (F-ordered (D, N)) and a contiguous copy give the same bytes, twice
    R = Y_T.T + rng.normal(size=Y_T.T.shape)
    R[rng.random_sample(R.shape) < 0.2] = np.nan
    assert R.T.flags.f_contiguous and R.T.T.flags.c_contiguous
    for m in (mean_merger, median_merger):
        a = ovp.set_and_merge(R.T, merge_method=m)
        b = ovp.set_and_merge(np.ascontiguousarray(R.T), merge_method=m)
        c = ovp.set_and_merge(R.T, merge_method=m)
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_invalid_arguments_raise(eng):
    from evo_amd._lib import EvoAmdError, check, dptr
    buf = np.zeros(4096)
    for args in [(4, 4, 1, 5, 2, 1), (4, 4, 1, 2, 5, 1), (4, 4, 1, 2, 2, 0), (40, 40, 1, 33, 32, 1), (0, 4, 1, 1, 1, 1)]:
        with pytest.raises(EvoAmdError):
            check(eng.lib.evoamd_patches_merge(eng._h, dptr(buf), *args, 0, dptr(buf)))
        with pytest.raises(EvoAmdError):
            check(eng.lib.evoamd_patches_extract(eng._h, dptr(buf), *args, dptr(buf)))
    with pytest.raises(EvoAmdError):
        check(eng.lib.evoamd_patches_merge(eng._h, dptr(buf), 4, 4, 1, 2, 2, 1, 2, dptr(buf)))


def _trajectory(eng, Y, merges):
    """Three EBSC EM steps on a shared engine; `merges` runs between the steps (may be None)."""
    N, D = Y.shape
    np.random.seed(7)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = BSC(D, 12, 8, engine=eng)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, 8, 12, "fit", "randflip", 4, 1, 1)
    out = []
    for it in range(3):
        F, nu, nsub, theta = model.step(theta, suff, my_data)
        out.append((F, nu, nsub, suff["ss"].copy(), theta["W"].copy(), float(theta["sigma"]), suff["lpj"].copy()))
        if merges is not None:
            merges()
    return out


def _merges(eng, img, R, rng):
    big = rng.normal(size=(300 * 300, 64))  # grows the patch scratch well past the EM buffers of the context

    def run():
        ovp = OverlappingPatches(img, 4, 4, engine=eng)
        ovp.set_and_merge(R.T, mean_merger)
        ovp.set_and_merge(R.T, median_merger)
        eng.patches_merge(big, (307, 307), 8, 8, 1, "median")
        eng.patches_extract(rng.normal(size=(50, 50, 3)), 5, 5, 1)
    return run


def test_merge_between_em_steps_leaves_trajectory(eng):
    """Merges between EM steps on the model's own engine change nothing.  The statistics pass sums through f64
    atomics, which are not bit-reproducible run to run, so K^n, F and the E-step counters are compared
    bit for bit and Theta / lpj to 1e-12 of their largest entry; the fixed-Theta test below is bit for bit throughout."""
    rng = np.random.RandomState(4)
    img = rng.normal(size=(40, 36))
    Y = oracle_extract(img, 4, 4, 1)
    R = Y + rng.normal(size=Y.shape)
    R[rng.random_sample(R.shape) < 0.3] = np.nan
    ref = _trajectory(eng, Y, None)
    got = _trajectory(eng, Y, _merges(eng, img, R, rng))
    for a, b in zip(ref, got):
        assert a[0] == b[0] and a[1:3] == b[1:3]
        np.testing.assert_array_equal(a[3], b[3])
        for x, y in zip(a[4:], b[4:]):
            # atomics move entries by ulps of the largest one (observed: 5e-16 on an entry of 4e-4, W of scale 0.5)
            np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12 * float(np.max(np.abs(x))))


def test_merge_leaves_em_state_bit_for_bit(eng):
    """Fixed Theta: the resident K^n, Y and Theta of a configured context give the same lpj bits before and after the
    merges (deterministic kernels only)."""
    rng = np.random.RandomState(6)
    img = rng.normal(size=(40, 36))
    Y = oracle_extract(img, 4, 4, 1)
    R = Y + rng.normal(size=Y.shape)
    R[rng.random_sample(R.shape) < 0.3] = np.nan
    _trajectory(eng, Y, None)  # leaves a configured EBSC context with K^n and Theta resident
    eng.lpj_resident()
    lpj0, ss0, th0 = eng.download_lpj(), eng.download_states(), eng.get_params_bsc()
    _merges(eng, img, R, rng)()
    eng.lpj_resident()
    np.testing.assert_array_equal(eng.download_lpj(), lpj0)
    np.testing.assert_array_equal(eng.download_states(), ss0)
    th1 = eng.get_params_bsc()
    for k in th0:
        np.testing.assert_array_equal(th0[k], th1[k])


# ---- end to end: the reference's image workflows ----------------------------------------------------------------------
def _denoise(algo, seed, epochs):
    clean = _images()["house_r04"].astype(np.float64)  # (102, 102)
    rng = np.random.RandomState(seed)
    noisy = rng.normal(clean, scale=25)
    np.random.seed(seed)
    ovp = OverlappingPatches(noisy, 5, 5, patch_shift=1)  # process-wide engine
    Y = ovp.get().T
    N, D = Y.shape
    my_data = {"y": Y, "x_infr": np.logical_not(np.isnan(Y)), "x": np.zeros_like(Y)}
    model = {"ebsc": BSC, "es3c": SSSC}[algo](D, 32, 20)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, 20, 32, "fit", "randflip", 10, 1, 1)
    for e in range(epochs):
        F, _, _, theta = model.step(theta, suff, my_data, e == epochs - 1)
    Y_rec_T = my_data["y_reconstructed"].T
    p_noisy = psnr(clean, noisy)
    return (psnr(clean, ovp.set_and_merge(Y_rec_T, merge_method=mean_merger)) - p_noisy,
            psnr(clean, ovp.set_and_merge(Y_rec_T, merge_method=median_merger)) - p_noisy)


# PSNR gain of the merged reconstruction over the noisy image, dB, 20 epochs.  Observed on MI355X, seeds 0 / 1 / 2
# (mean merge, median merge): EBSC 3.61 3.63 / 3.74 3.73 / 3.76 3.77; ES3C 7.09 7.11 / 7.12 7.25 / 6.94 6.97.
DENOISE_EPOCHS = 20
DENOISE_MIN_GAIN_DB = {"ebsc": 2.5, "es3c": 5.0}


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_denoising_end_to_end(algo):
    g_mean, g_median = _denoise(algo, 0, DENOISE_EPOCHS)
    print("denoise %s: gain mean %.3f dB, median %.3f dB" % (algo, g_mean, g_median))
    assert g_mean > DENOISE_MIN_GAIN_DB[algo] and g_median > DENOISE_MIN_GAIN_DB[algo]


def _inpaint(algo, seed, epochs):
    clean = _images()["castle_r01"].astype(np.float64)  # (48, 32, 3)
    rng = np.random.RandomState(seed)
    incomplete = clean.copy()
    missing = rng.random_sample(clean.shape) <= 0.1
    incomplete[missing] = np.nan
    np.random.seed(seed)
    ovp = MultiDimOverlappingPatches(incomplete, 5, 5, patch_shift=1)
    Y = ovp.get().T
    N, D = Y.shape
    my_data = {"y": Y, "x_infr": np.logical_not(np.isnan(Y)), "x": np.logical_not(np.isnan(Y))}
    kwargs = {"ebsc": {}, "es3c": {"to_learn": ["W", "pies", "sigma2"]}}[algo]
    model = {"ebsc": BSC, "es3c": SSSC}[algo](D, 32, 20, **kwargs)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, 20, 32, "fit", "randflip", 10, 1, 1)
    for e in range(epochs):
        F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
    Y_rec_T = my_data["y_reconstructed"].T
    fill = np.where(missing, np.nanmean(incomplete), clean)
    p_fill = psnr(clean[missing], fill[missing])
    gains = []
    for m in (mean_merger, median_merger):
        img = ovp.set_and_merge(Y_rec_T, merge_method=m)
        assert img.shape == clean.shape and not np.isnan(img).any()  # every pixel had a valid estimate
        gains.append(psnr(clean[missing], img[missing]) - p_fill)
    return tuple(gains)


# PSNR on the missing pixels over filling them with the mean of the observed ones, dB, 20 epochs.  Observed on MI355X,
# seeds 0 / 1 / 2 (mean, median): EBSC 6.68 6.66 / 7.65 7.77 / 6.96 7.05; ES3C 7.50 7.50 / 8.21 8.22 / 8.31 8.27.
INPAINT_EPOCHS = 20
INPAINT_MIN_GAIN_DB = 5.0


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_inpainting_end_to_end(algo):
    g_mean, g_median = _inpaint(algo, 0, INPAINT_EPOCHS)
    print("inpaint %s: gain mean %.3f dB, median %.3f dB" % (algo, g_mean, g_median))
    assert g_mean > INPAINT_MIN_GAIN_DB and g_median > INPAINT_MIN_GAIN_DB

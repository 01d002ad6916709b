"""ResidentDraws / ResidentMoments (evo_amd/resident.py) and image_moments_host without a GPU: the Welford mirror, the
handles' array surface, the ``draws`` argument, one download, the three staleness layers, and how OverlappingPatches and
PrecisionMerger route the handles.  The engine is a stub that records what it is asked."""
import inspect

import numpy as np
import pytest

from evo_amd._lib import EvoAmdError
from evo_amd.resident import DrawFace, ResidentDraws, ResidentMoments
from evo_amd.utils.prepost import (OverlappingPatches, PrecisionMerger, estimate_stack, image_moments_host, mean_merger,
                                   median_merger, patch_geometry, precision_merger)


# ---- image_moments_host -------------------------------------------------------------------------------------------------
def test_moments_of_identical_images_are_their_value_and_exactly_zero():
    img = np.random.RandomState(0).normal(size=(13, 11)) * 1e3
    mean, std = image_moments_host(np.stack([img] * 7))
    assert np.array_equal(mean, img) and (std == 0.0).all() and not np.signbit(std).any()
    mean, std = image_moments_host(img[None])
    assert np.array_equal(mean, img) and (std == 0.0).all()


def test_a_nan_in_one_image_gives_nan_at_that_pixel_only():
    imgs = np.random.RandomState(1).normal(size=(5, 13, 11))
    imgs[2, 4, 7] = np.nan
    imgs[0, 0, 0] = np.nan
    mean, std = image_moments_host(imgs)
    bad = np.zeros((13, 11), dtype=bool)
    bad[4, 7] = bad[0, 0] = True
    assert np.array_equal(np.isnan(mean), bad) and np.array_equal(np.isnan(std), bad)


def test_moments_agree_with_numpy():
    imgs = np.random.RandomState(2).normal(size=(5, 13, 11)) * 3.0 + 100.0
    mean, std = image_moments_host(imgs)
    np.testing.assert_allclose(mean, np.mean(imgs, axis=0), rtol=1e-13, atol=0)
    np.testing.assert_allclose(std, np.std(imgs, axis=0), rtol=1e-13, atol=0)
    with pytest.raises(ValueError):
        image_moments_host(np.zeros((0, 3, 3)))


# ---- a stand-in engine --------------------------------------------------------------------------------------------------
def _host_merge(Y, shape, ph, pw, shift, method):
    stack = estimate_stack(Y, shape[0], shape[1], 1, ph, pw, shift)
    return (mean_merger if method == "mean" else median_merger)(stack, axis=0).reshape(shape)


class StubEngine:
    def __init__(self, y=None, mean=None, var=None):
        self.y, self.mean, self.var = y, mean, var
        self._ps_serial = self._pred_serial = 0
        self.downloads, self.calls = [], []
        self.outdated = False  # the library's own view (a configure released the buffers)

    def sample(self):
        self._ps_serial += 1
        return ResidentDraws(self, self._ps_serial, self.y.shape)

    def moments(self):
        self._pred_serial += 1
        mean = ResidentMoments(self, self._pred_serial, self.mean.shape, "mean")
        return mean, mean.sibling("var")

    def _guard(self, kind, serial):
        if self.outdated or serial != getattr(self, kind):
            raise EvoAmdError("nothing on the device")

    def download_posterior_draws(self, T, serial=None):
        self._guard("_ps_serial", serial)
        self.downloads.append("y")
        return self.y.copy()

    def patches_merge_samples(self, shape, ph, pw, shift=1, method="mean", t0=0, n_draws=1, images=True, moments=False,
                              serial=None):
        if patch_geometry(shape[0], shape[1], 1, ph, pw, shift) != (self.y.shape[0], self.y.shape[2]):
            raise ValueError("geometry")
        self._guard("_ps_serial", serial)
        self.calls.append(("samples", method, t0, n_draws, images, moments))
        imgs = np.stack([_host_merge(self.y[:, t], shape, ph, pw, shift, method) for t in range(t0, t0 + n_draws)])
        m = image_moments_host(imgs) if moments else (None, None)
        return (imgs if images else None), m[0], m[1]

    def download_predictive(self, which, shape=None, serial=None):
        self._guard("_pred_serial", serial)
        self.downloads.append(which)
        return getattr(self, which).copy()

    def patches_merge_predictive(self, shape, ph, pw, shift=1, what=2, serial=None):
        if patch_geometry(shape[0], shape[1], 1, ph, pw, shift) != self.mean.shape:
            raise ValueError("geometry")
        self._guard("_pred_serial", serial)
        self.calls.append(("predictive", what))
        return np.full(shape, float(what))

    def patches_merge(self, Y, shape, ph, pw, shift=1, method="mean", weights=None):
        self.calls.append(("host", method))
        if method == "precision":
            return np.full(shape, -1.0)
        return _host_merge(np.asarray(Y), shape, ph, pw, shift, method)


H, W, PH, PW = 9, 8, 3, 3
N, D = patch_geometry(H, W, 1, PH, PW, 1)
T = 5


def _draws_engine(seed=0):
    y = np.random.RandomState(seed).normal(size=(N, T, D))
    y[0] = np.nan
    return StubEngine(y=y)


def _ovp(engine):
    return OverlappingPatches(np.zeros((H, W)), PH, PW, engine=engine)


# ---- ResidentDraws ------------------------------------------------------------------------------------------------------
def test_draws_array_surface_and_single_download():
    eng = _draws_engine()
    h = eng.sample()
    assert h.shape == (N, T, D) and h.dtype == np.float64 and h.ndim == 3 and len(h) == N
    assert h.resident and not h.materialised and eng.downloads == []
    f = h.draw(2)
    assert isinstance(f, DrawFace) and f.shape == (N, D) and f.T.shape == (D, N) and len(f.T) == D and f.ndim == 2
    assert f.T.T is f and f.T is f.T and h.draw(2) is f and f.T.transposed and not f.transposed
    for t in (-1, T):
        with pytest.raises(ValueError):
            h.draw(t)
    assert eng.downloads == []
    a = np.asarray(h)
    assert np.array_equal(a, eng.y, equal_nan=True) and np.asarray(h) is a and h.materialised
    assert np.array_equal(np.asarray(f.T), eng.y[:, 2].T, equal_nan=True)
    assert eng.downloads == ["y"]


def test_draws_argument_and_device_merges():
    eng = _draws_engine()
    other = StubEngine()  # the engine the patch object was built with: must not be asked
    ovp = _ovp(other)
    h = eng.sample()
    full = h.merge(ovp)
    assert full.shape == (T, H, W) and eng.calls[-1] == ("samples", "mean", 0, T, True, False)
    assert np.array_equal(h.merge(ovp, draws=slice(1, 4)), full[1:4], equal_nan=True)
    assert eng.calls[-1] == ("samples", "mean", 1, 3, True, False)
    assert np.array_equal(h.merge(ovp, draws=3), full[3:4], equal_nan=True)
    assert np.array_equal(h.merge(ovp, draws=slice(None, 2)), full[:2], equal_nan=True)
    h.merge(ovp, median_merger, draws=slice(2, None))
    assert eng.calls[-1] == ("samples", "median", 2, T - 2, True, False)
    for bad in (slice(0, T, 2), slice(0, T + 1), slice(3, 3), slice(-2, None), T, -1):
        with pytest.raises(ValueError):
            h.merge(ovp, draws=bad)
        with pytest.raises(ValueError):
            h.merge_moments(ovp, draws=bad)
    mean, std = h.merge_moments(ovp)
    assert eng.calls[-1] == ("samples", "mean", 0, T, False, True)
    want = image_moments_host(full)
    assert np.array_equal(mean, want[0], equal_nan=True) and np.array_equal(std, want[1], equal_nan=True)
    assert np.isnan(full[:, 0, 0]).all() and np.isnan(mean[0, 0]) and np.isnan(std[0, 0])
    # one draw through OverlappingPatches: merged on the handle's engine, either face
    for arg in (h.draw(2).T, h.draw(2)):
        img = ovp.set_and_merge(arg, merge_method=median_merger)
        assert eng.calls[-1] == ("samples", "median", 2, 1, True, False) and img.shape == (H, W)
    assert np.array_equal(ovp.set_and_merge(h.draw(2).T), full[2], equal_nan=True)
    assert eng.downloads == [] and other.calls == []
    # any other callable takes the host array
    nanmax = lambda stack, axis=0: np.nanmax(np.where(np.isnan(stack), -np.inf, stack), axis=axis)  # noqa: E731
    got = h.merge(ovp, nanmax, draws=1)
    assert np.array_equal(got[0], nanmax(estimate_stack(eng.y[:, 1], H, W, 1, PH, PW, 1)).reshape(H, W))
    assert np.array_equal(ovp.set_and_merge(h.draw(1).T, merge_method=nanmax), got[0])
    assert eng.downloads == ["y"]


def test_wrong_geometry_is_refused():
    eng = _draws_engine()
    h = eng.sample()
    ovp = OverlappingPatches(np.zeros((H, W)), 2, 2, engine=eng)
    for arg in (h.draw(0), h.draw(0).T):
        with pytest.raises(ValueError):
            ovp.set(arg)
    with pytest.raises(ValueError):
        h.merge(ovp)
    with pytest.raises(ValueError):
        h.merge_moments(ovp)
    _ovp(eng).set(h.draw(0))  # the right one is accepted
    assert eng.calls == [] and eng.downloads == []


def test_draws_staleness_three_layers():
    eng = _draws_engine()
    ovp = _ovp(eng)
    first = eng.sample()
    read = np.asarray(first).copy()
    second = eng.sample()
    first._outdate("a later sample_posterior of the same model")
    third = eng.sample()
    second._outdate("a later sample_posterior of the same model")
    # read before it was outdated: the host copy keeps serving; never read: lost, with the cause in the message
    assert np.array_equal(np.asarray(first), read, equal_nan=True) and not first.resident
    n_calls = len(eng.calls)
    img = first.merge(ovp, draws=1)
    assert np.array_equal(img[0], _host_merge(read[:, 1], (H, W), PH, PW, 1, "mean"), equal_nan=True)
    assert eng.calls[n_calls:] == [("host", "mean")]
    assert np.array_equal(ovp.set_and_merge(first.draw(1).T), img[0], equal_nan=True)
    first.merge_moments(ovp)
    for call in (lambda: np.asarray(second), lambda: second.merge(ovp), lambda: second.merge_moments(ovp),
                 lambda: ovp.set_and_merge(second.draw(0).T), lambda: np.asarray(second.draw(0))):
        with pytest.raises(RuntimeError, match="a later sample_posterior of the same model"):
            call()
    # nobody told the handle, but the engine moved on (another model on the same engine): the serial decides
    fourth = eng.sample()
    assert not third.resident
    with pytest.raises(RuntimeError, match="same engine"):
        third.merge(ovp)
    with pytest.raises(RuntimeError):
        np.asarray(third)
    # the library refuses (a configure released the buffers): RuntimeError, not other data
    eng.outdated = True
    with pytest.raises(RuntimeError, match="outdated"):
        fourth.merge(ovp)
    with pytest.raises(RuntimeError, match="outdated"):
        np.asarray(fourth)
    assert eng.downloads == ["y"]


# ---- ResidentMoments ----------------------------------------------------------------------------------------------------
def _moments_engine():
    rng = np.random.RandomState(3)
    return StubEngine(mean=rng.normal(size=(N, D)), var=rng.uniform(0.5, 2.0, size=(N, D)))


def test_moments_handles_route_through_overlapping_patches():
    eng = _moments_engine()
    ovp = _ovp(StubEngine())
    mean, var = eng.moments()
    assert mean.shape == (N, D) and var.T.shape == (D, N) and mean.T.T is mean and var.ndim == 2 and len(var.T) == D
    assert mean.same_call(var) and mean.which == "mean" and var.which == "var"
    merger = precision_merger(var.T)
    assert isinstance(merger, PrecisionMerger) and eng.downloads == []  # built from a handle without materialising it
    assert (ovp.set_and_merge(mean.T, merge_method=merger) == 2.0).all() and eng.calls[-1] == ("predictive", 2)
    assert (ovp.set_and_merge(var.T, merge_method=mean_merger) == 3.0).all()
    assert (ovp.set_and_merge(mean.T, merge_method=mean_merger) == 0.0).all()
    assert (ovp.set_and_merge(mean, merge_method=median_merger) == 1.0).all()
    assert eng.downloads == [] and not mean.materialised
    with pytest.raises(ValueError):
        OverlappingPatches(np.zeros((H, W)), 2, 2, engine=eng).set_and_merge(mean.T, merge_method=merger)


def test_moments_staleness_and_mixed_calls():
    eng = _moments_engine()
    host = StubEngine()
    ovp = _ovp(host)
    mean1, var1 = eng.moments()
    v1 = np.asarray(var1)
    assert eng.downloads == ["var"] and np.asarray(var1.T).shape == (D, N) and np.asarray(var1) is v1
    mean2, var2 = eng.moments()
    mean1._outdate("a later predictive_moments of the same model")
    with pytest.raises(RuntimeError, match="a later predictive_moments of the same model"):
        np.asarray(mean1)  # never read
    assert np.array_equal(np.asarray(var1), eng.var)  # read before: the host copy stays
    # a mean and a var of different calls: no device merge; both become host arrays
    img = ovp.set_and_merge(mean2.T, merge_method=precision_merger(var1.T))
    assert (img == -1.0).all() and host.calls == [("host", "precision")] and eng.calls == []
    assert eng.downloads == ["var", "mean"]
    # the median of var has no device form: host array
    ovp.set_and_merge(var2.T, merge_method=median_merger)
    assert host.calls[-1] == ("host", "median") and eng.downloads == ["var", "mean", "var"]
    eng.outdated = True
    mean3, var3 = eng.moments()
    with pytest.raises(RuntimeError, match="outdated"):
        ovp.set_and_merge(mean3.T, merge_method=precision_merger(var3.T))
    with pytest.raises(RuntimeError, match="outdated"):
        np.asarray(var3)


# ---- the models' keywords -----------------------------------------------------------------------------------------------
def test_models_have_the_resident_keywords():
    from evo_amd.engine import Engine
    from evo_amd.models import BSC, SSSC
    for cls in (BSC, SSSC, Engine):
        for name in ("sample_posterior", "predictive_moments"):
            p = inspect.signature(getattr(cls, name)).parameters
            assert "resident" in p and p["resident"].default is False, (cls, name)

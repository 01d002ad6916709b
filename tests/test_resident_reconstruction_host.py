"""ResidentReconstruction (evo_amd/resident.py) without a GPU: the handle's array surface, the host selection rule of
Model._write_reconstruction applied to the downloaded estimate, one download, staleness, and how OverlappingPatches
routes a handle.  The engine is a stub that records what it is asked."""
import numpy as np
import pytest

from evo_amd._lib import EvoAmdError
from evo_amd.resident import ResidentReconstruction
from evo_amd.utils.prepost import OverlappingPatches, mean_merger, median_merger, patch_geometry


class StubEngine:
    def __init__(self, y_hat):
        self.y_hat = y_hat
        self._rec_serial = 0
        self.downloads = 0
        self.merges = []
        self.outdated = False  # the library's own view (a statistics pass / set_params behind the model's back)

    def reconstruct_resident(self, x=None):
        self._rec_serial += 1
        self.outdated = False
        return self._rec_serial

    def download_reconstruction(self, serial=None):
        if self.outdated or serial != self._rec_serial:
            raise EvoAmdError("no current resident reconstruction")
        self.downloads += 1
        return self.y_hat.copy()

    def patches_merge_resident(self, shape, ph, pw, shift=1, method="mean", serial=None):
        N, D = patch_geometry(shape[0], shape[1], 1, ph, pw, shift)
        if (N, D) != self.y_hat.shape:
            raise ValueError("geometry")
        if self.outdated or serial != self._rec_serial:
            raise EvoAmdError("no current resident reconstruction")
        self.merges.append((tuple(shape), ph, pw, shift, method))
        return np.full(shape, 7.0)

    def patches_merge(self, *a, **k):
        raise AssertionError("the host-array merge must not run for a resident handle")


def _problem(incomplete, seed=0, N=12 * 9, D=16):
    rng = np.random.RandomState(seed)
    y = rng.normal(size=(N, D))
    y_hat = rng.normal(size=(N, D))
    if incomplete:
        x_infr = rng.random_sample((N, D)) < 0.7
        x_infr[3] = False  # a datapoint without a reliable entry: kept as it is, NaN included
        y[~x_infr] = np.nan
        x = x_infr.copy()
    else:
        x_infr = None
        x = rng.random_sample((N, D)) < 0.2
    return y, y_hat, x, x_infr


def _host_rule(y, y_hat, x, x_infr):
    y_rec = y.copy()
    miss = np.logical_not(x)
    if x_infr is not None:
        miss &= x_infr.any(axis=1)[:, None]
    y_rec[miss] = y_hat[miss]
    return y_rec


@pytest.mark.parametrize("incomplete", [False, True])
def test_array_surface_and_single_download(incomplete):
    y, y_hat, x, x_infr = _problem(incomplete)
    eng = StubEngine(y_hat)
    h = ResidentReconstruction(eng, eng.reconstruct_resident(x), y, x, x_infr)
    N, D = y.shape
    assert h.shape == (N, D) and h.T.shape == (D, N) and h.dtype == np.float64 and h.ndim == 2
    assert len(h) == N and len(h.T) == D
    assert h.T.T is h and h.T is h.T and h.T.transposed and not h.transposed
    assert h.resident and not h.materialised and eng.downloads == 0
    want = _host_rule(y, y_hat, x, x_infr)
    np.testing.assert_array_equal(np.asarray(h), want)
    np.testing.assert_array_equal(np.asarray(h.T), want.T)
    np.testing.assert_array_equal(np.array(h.T), want.T)
    assert eng.downloads == 1 and h.materialised and h.T.materialised
    assert np.asarray(h) is np.asarray(h) and np.asarray(h).dtype == np.float64
    if incomplete:
        assert np.isnan(np.asarray(h)[3]).all()  # the datapoint without a reliable entry keeps its NaN
        assert not np.isnan(np.asarray(h)[np.arange(N) != 3]).any()
    assert y is not np.asarray(h) and (np.isnan(y) == np.isnan(_problem(incomplete)[0])).all()  # the data is not edited


def test_stale_unread_handle_raises_and_read_handle_survives():
    y, y_hat, x, x_infr = _problem(False)
    eng = StubEngine(y_hat)
    first = ResidentReconstruction(eng, eng.reconstruct_resident(x), y, x)
    read = np.asarray(first).copy()
    second = ResidentReconstruction(eng, eng.reconstruct_resident(x), y, x)
    first._outdate("a later step")
    third = ResidentReconstruction(eng, eng.reconstruct_resident(x), y, x)
    second._outdate("a later step of the model")
    # read before it was outdated: the cached array stays; never read: lost, with the cause in the message
    np.testing.assert_array_equal(np.asarray(first), read)
    assert not second.resident
    with pytest.raises(RuntimeError, match="a later step of the model"):
        np.asarray(second)
    with pytest.raises(RuntimeError, match="a later step of the model"):
        np.asarray(second.T)
    with pytest.raises(RuntimeError):
        second.merge((15, 12), 4, 4, 1, "mean")
    # nobody told the handle, but the engine moved on (another model on the same engine): the serial decides
    fourth_serial = eng.reconstruct_resident(x)
    assert not third.resident and fourth_serial != third.serial
    with pytest.raises(RuntimeError):
        np.asarray(third)
    # the library refuses (a statistics pass behind the model's back): RuntimeError, not newer data
    fifth = ResidentReconstruction(eng, eng.reconstruct_resident(x), y, x)
    eng.outdated = True
    with pytest.raises(RuntimeError, match="outdated"):
        np.asarray(fifth)
    with pytest.raises(RuntimeError, match="outdated"):
        fifth.merge((15, 12), 4, 4, 1, "mean")
    assert eng.downloads == 1


def test_overlapping_patches_route_a_handle():
    H, W, ph, pw = 14, 11, 3, 3
    N, D = patch_geometry(H, W, 1, ph, pw, 1)
    y, y_hat, x, _ = _problem(False, N=N, D=D)
    eng = StubEngine(y_hat)
    other = StubEngine(y_hat)  # the engine the patch object was built with: must not be asked
    ovp = OverlappingPatches(np.zeros((H, W)), ph, pw, engine=other)
    h = ResidentReconstruction(eng, eng.reconstruct_resident(x), y, x)
    for arg in (h.T, h):
        for merger, name in ((mean_merger, "mean"), (median_merger, "median")):
            img = ovp.set_and_merge(arg, merge_method=merger)
            assert img.shape == (H, W) and (img == 7.0).all()
            assert eng.merges[-1] == ((H, W), ph, pw, 1, name)
    assert eng.downloads == 0 and other.merges == [] and len(eng.merges) == 4
    assert ovp.get() is h.T
    # any other callable: the handle materialises and the host path runs over the estimate stack
    got = ovp.set_and_merge(h.T, merge_method=lambda stack, axis=0: np.nanmax(stack, axis=axis))
    from evo_amd.utils.prepost import estimate_stack
    want = np.nanmax(estimate_stack(_host_rule(y, y_hat, x, None), H, W, 1, ph, pw, 1), axis=0).reshape(H, W)
    np.testing.assert_array_equal(got, want)
    assert eng.downloads == 1


def test_wrong_geometry_raises_value_error():
    y, y_hat, x, _ = _problem(False)  # (108, 16)
    eng = StubEngine(y_hat)
    h = ResidentReconstruction(eng, eng.reconstruct_resident(x), y, x)
    ovp = OverlappingPatches(np.zeros((14, 11)), 3, 3, engine=eng)  # N = 108, D = 9
    for arg in (h, h.T):
        with pytest.raises(ValueError):
            ovp.set(arg)
        with pytest.raises(ValueError):
            ovp.set_and_merge(arg, merge_method=mean_merger)
    with pytest.raises(ValueError):
        ovp.set(np.zeros((16, 108)))  # an array of the wrong shape, as before
    assert eng.merges == [] and eng.downloads == 0


def test_model_keyword_exists_and_defaults_off():
    from evo_amd.models import BSC, SSSC
    for cls in (BSC, SSSC):
        assert cls(8, 4, 3).resident_reconstruction is False
        assert cls(8, 4, 3, resident_reconstruction=True).resident_reconstruction is True

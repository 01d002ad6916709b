"""The precision-weighted patch merge on the GPU (patches_wmean_kernel, Engine.patches_merge(method="precision"),
evo_amd.utils.prepost.precision_merger): bit for bit against its host mirror PrecisionMerger.__call__ -- and through it
against the explicit triple loop of tests/_predictive_problems.py -- on the cases of tests/test_predictive_host.py and one
40 x 50 x 3 image with 8 x 8 patches; a ResidentReconstruction handle as input; the mean and median merges unchanged."""
import numpy as np
import pytest

from _predictive_problems import MERGE_CASES, merge_case
from evo_amd.engine import Engine
from evo_amd.models import BSC
from evo_amd.resident import ResidentReconstruction
from evo_amd.utils.prepost import (MultiDimOverlappingPatches, OverlappingPatches, estimate_stack, mean_merger, median_merger,
                                   patch_geometry, precision_merger)
from evo_amd.variational import init_states

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _mirror(Y, V, H, W, C, ph, pw, shift):
    stack = estimate_stack(Y, H, W, C, ph, pw, shift)
    return precision_merger(V.T).bind(H, W, C, ph, pw, shift)(stack, axis=0)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", list(MERGE_CASES))
def test_engine_equals_mirror_bit_for_bit(eng, name):
    (H, W, C, ph, pw, shift), Y, V, ref = merge_case(name)
    shape = (H, W) if C == 1 else (H, W, C)
    got = eng.patches_merge(Y, shape, ph, pw, shift, method="precision", weights=V)
    want = _mirror(Y, V, H, W, C, ph, pw, shift).reshape(shape)
    assert _same_bits(got, want) and _same_bits(got, ref.reshape(shape))
    assert np.isnan(got[0, 0]).all()  # the pixel without a valid estimate
    # through OverlappingPatches, and the plain merges of the same estimates keep their bits
    ovp = (OverlappingPatches if C == 1 else MultiDimOverlappingPatches)(np.zeros(shape), ph, pw, shift, engine=eng)
    assert _same_bits(ovp.set_and_merge(Y.T, merge_method=precision_merger(V.T)), want)
    stack = estimate_stack(Y, H, W, C, ph, pw, shift)
    assert _same_bits(ovp.set_and_merge(Y.T, merge_method=mean_merger), mean_merger(stack).reshape(shape))
    assert _same_bits(ovp.set_and_merge(Y.T, merge_method=median_merger), median_merger(stack).reshape(shape))
    with pytest.raises(ValueError, match="go together"):
        eng.patches_merge(Y, shape, ph, pw, shift, method="precision")
    with pytest.raises(ValueError, match="weights have shape"):
        eng.patches_merge(Y, shape, ph, pw, shift, method="precision", weights=V[:-1])


def test_larger_image(eng):
    H, W, C, ph, pw, shift = 40, 50, 3, 8, 8, 1
    N, D = patch_geometry(H, W, C, ph, pw, shift)
    rng = np.random.RandomState(2)
    Y = rng.normal(size=(N, D)) * 20 + 100
    V = rng.gamma(2.0, 3.0, size=(N, D))
    Y[rng.random_sample((N, D)) < 0.05] = np.nan
    V[rng.random_sample((N, D)) < 0.05] = 0.0
    V[rng.random_sample((N, D)) < 0.02] = np.nan
    got = eng.patches_merge(Y, (H, W, C), ph, pw, shift, method="precision", weights=V)
    assert _same_bits(got, _mirror(Y, V, H, W, C, ph, pw, shift))
    # equal variances: the mean merge up to the rounding of the weights (exactly with a power of two)
    same = eng.patches_merge(Y, (H, W, C), ph, pw, shift, method="precision", weights=np.full((N, D), 0.25))
    assert _same_bits(same, eng.patches_merge(Y, (H, W, C), ph, pw, shift, method="mean"))


def test_resident_handle_is_materialised(eng):
    """A model with resident_reconstruction: the handle of a reconstructing step goes through rows(); the merged image is
    the one of the array it stands for, and the variances come from the same model."""
    rng = np.random.RandomState(3)
    np.random.seed(3)
    img = rng.normal(size=(12, 14)) * 10 + 50
    ovp = OverlappingPatches(img, 4, 4, patch_shift=1, engine=eng)
    Y = np.ascontiguousarray(ovp.get().T)
    N, D = Y.shape
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool), "x": np.zeros_like(Y, dtype=bool)}
    Hl, S = 8, 6
    model = BSC(D, Hl, S, engine=eng, resident_reconstruction=True)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, Hl, "fit", "randflip", 4, 1, 1)
    _, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
    h = my_data["y_reconstructed"]
    assert isinstance(h, ResidentReconstruction) and not h.materialised
    mean, var, info = model.predictive_moments(theta, suff, my_data)
    assert info == {"n_singular": 0, "n_skipped": 0} and (var > 0).all()
    assert my_data["y_reconstructed"] is h and h.materialised  # fetched before the new parameters outdated the device copy
    got = ovp.set_and_merge(h.T, merge_method=precision_merger(var.T))
    rows = np.asarray(h)
    assert _same_bits(got, ovp.set_and_merge(rows.T, merge_method=precision_merger(var.T)))
    assert _same_bits(got, _mirror(rows, var, 12, 14, 1, 4, 4, 1).reshape(12, 14))
    # the uncertainty map: the mean merge of the variances
    umap = ovp.set_and_merge(var.T, merge_method=mean_merger)
    assert umap.shape == img.shape and (umap > 0).all()

"""Host side of evo_amd.utils.prepost (no GPU): patch geometry, the NumPy extract / stack oracle the GPU tests compare
against, argument checks, psnr and the host fallback of custom merge callables."""
import numpy as np
import pytest

from evo_amd.utils import prepost
from evo_amd.utils.prepost import (MultiDimOverlappingPatches, OverlappingPatches, mean_merger, median_merger,
                                   patch_geometry, patch_tops, psnr)


# ---- NumPy oracle (shared with tests/test_gpu_patches.py) ----------------------------------------------------------
def oracle_extract(img, ph, pw, s):
    """(H, W[, C]) -> (N, D): Y[ir * nc + ic, (dy * pw + dx) * C + c] = img[top_ir + dy, left_ic + dx, c]."""
    img3 = img.reshape(img.shape[0], img.shape[1], -1)
    H, W, C = img3.shape
    tops, lefts = patch_tops(H, ph, s), patch_tops(W, pw, s)
    Y = np.empty((len(tops), len(lefts), ph, pw, C), dtype=np.float64)
    for dy in range(ph):
        for dx in range(pw):
            Y[:, :, dy, dx, :] = img3[tops[:, None] + dy, lefts[None, :] + dx, :]
    return Y.reshape(len(tops) * len(lefts), ph * pw * C)


def oracle_stack(Y, shape, ph, pw, s):
    """(N, D) -> NaN-padded (K, H, W[, C]) stack, each element's estimates in increasing n: grid rows in order, and
    within one grid row the columns in increasing ic (dx descending), each estimate going to the element's next slot."""
    H, W = shape[:2]
    C = shape[2] if len(shape) == 3 else 1
    tops, lefts = patch_tops(H, ph, s), patch_tops(W, pw, s)
    nr, nc = len(tops), len(lefts)
    Y5 = np.asarray(Y, dtype=np.float64).reshape(nr, nc, ph, pw, C)
    K = ph * pw  # upper bound, trimmed below
    stack = np.full((K, H, W, C), np.nan)
    cnt = np.zeros((H, W), dtype=np.int64)
    ys = np.arange(ph)
    for ir in range(nr):
        y = tops[ir] + ys[:, None]  # (ph, 1)
        for dx in range(pw - 1, -1, -1):
            x = lefts[None, :] + dx  # (1, nc)
            k = cnt[y, x]  # (ph, nc)
            stack[k, y, x] = Y5[ir, :, :, dx, :].transpose(1, 0, 2)  # (ph, nc, C)
            cnt[y, x] += 1
    stack = stack[:max(1, int(cnt.max()))]
    return stack if len(shape) == 3 else stack[..., 0]


def test_patch_tops_and_counts():
    assert list(patch_tops(10, 4, 3)) == [0, 3, 6]  # (H - ph) % s == 0: no border patch
    assert list(patch_tops(11, 4, 3)) == [0, 3, 6, 7]  # border patch at H - ph
    assert list(patch_tops(5, 5, 2)) == [0]
    assert list(patch_tops(8, 1, 1)) == list(range(8))
    assert patch_geometry(512, 512, 1, 8, 8, 1) == (505 * 505, 64)
    assert patch_geometry(481, 321, 3, 8, 8, 1) == (474 * 314, 192)
    assert patch_geometry(11, 9, 2, 4, 3, 3) == (4 * 3, 24)  # lefts 0, 3, 6
    for H in range(1, 20):
        for ph in range(1, H + 1):
            for s in range(1, 5):
                t = patch_tops(H, ph, s)
                covered = np.zeros(H, bool)
                for v in t:
                    covered[v:v + ph] = True
                assert t[-1] == H - ph and np.all(np.diff(t) > 0)
                if s <= ph:
                    assert covered.all()  # (a shift above the patch size can leave gaps: such pixels merge to NaN)


def test_oracle_extract_hand_checked():
    img = np.arange(12, dtype=np.float64).reshape(3, 4)
    Y = oracle_extract(img, 2, 2, 1)  # tops 0, 1; lefts 0, 1, 2 -> N = 6
    assert Y.shape == (6, 4)
    assert list(Y[0]) == [0, 1, 4, 5]
    assert list(Y[4]) == [5, 6, 9, 10]  # n = 1 * 3 + 1: top 1, left 1
    assert list(Y[5]) == [6, 7, 10, 11]
    img = np.arange(5 * 3, dtype=np.float64).reshape(5, 3)
    Y = oracle_extract(img, 2, 3, 2)  # tops 0, 2, 3 (border); left 0
    assert list(Y[2]) == [9, 10, 11, 12, 13, 14]
    rgb = np.arange(2 * 2 * 3, dtype=np.float64).reshape(2, 2, 3)
    Y = oracle_extract(rgb, 1, 2, 1)  # d = (dy * pw + dx) * C + c
    assert list(Y[1]) == [6, 7, 8, 9, 10, 11]


def test_oracle_stack_hand_checked():
    img = np.arange(12, dtype=np.float64).reshape(3, 4)
    Y = oracle_extract(img, 2, 2, 1)
    st = oracle_stack(Y, img.shape, 2, 2, 1)
    assert st.shape == (4, 3, 4)
    # pixel (1, 1) is covered by patches n = 0, 1, 3, 4 in that order, always with its own value
    assert list(st[:, 1, 1]) == [5, 5, 5, 5]
    assert np.isnan(st[1:, 0, 0]).all() and st[0, 0, 0] == 0
    # the slots follow increasing n: mark every estimate with its patch index
    Yn = np.repeat(np.arange(6, dtype=np.float64)[:, None], 4, axis=1)
    st = oracle_stack(Yn, img.shape, 2, 2, 1)
    assert list(st[:, 1, 1]) == [0, 1, 3, 4]
    assert list(st[:, 2, 3][:1]) == [5] and np.isnan(st[1:, 2, 3]).all()
    assert list(st[:2, 1, 3]) == [2, 5]
    np.testing.assert_array_equal(mean_merger(oracle_stack(Y, img.shape, 2, 2, 1)), img)


@pytest.mark.parametrize("shape,ph,pw,s", [((7, 9), 3, 2, 1), ((11, 8, 3), 4, 3, 3), ((6, 6), 6, 6, 2),
                                           ((13, 10), 5, 4, 2), ((9, 9, 2), 1, 1, 1)])
def test_module_stack_matches_oracle(shape, ph, pw, s):
    """The module's host fallback builds the same stack as the oracle (slot formula vs running counter)."""
    rng = np.random.RandomState(0)
    img = rng.normal(size=shape)
    Y = oracle_extract(img, ph, pw, s)
    Y[rng.random_sample(Y.shape) < 0.3] = np.nan
    C = shape[2] if len(shape) == 3 else 1
    got = prepost.estimate_stack(Y, shape[0], shape[1], C, ph, pw, s)
    want = oracle_stack(Y, shape, ph, pw, s)
    np.testing.assert_array_equal(got.reshape(want.shape), want)


def test_value_errors():
    img = np.zeros((10, 12))
    with pytest.raises(ValueError):
        OverlappingPatches(np.zeros((10, 12, 3)), 3, 3)
    with pytest.raises(ValueError):
        MultiDimOverlappingPatches(img, 3, 3)
    with pytest.raises(ValueError):
        OverlappingPatches(img, 11, 3)  # ph > H
    with pytest.raises(ValueError):
        OverlappingPatches(img, 3, 13)  # pw > W
    with pytest.raises(ValueError):
        OverlappingPatches(img, 3, 3, patch_shift=0)
    with pytest.raises(ValueError):
        OverlappingPatches(np.zeros((40, 40)), 33, 32)  # ph pw > 1024
    with pytest.raises(ValueError):
        OverlappingPatches(img, 0, 3)
    ovp = OverlappingPatches(img, 3, 4)
    assert (ovp.N, ovp.D) == (8 * 9, 12)
    with pytest.raises(ValueError):
        ovp.set(np.zeros((ovp.N, ovp.D)))  # (N, D) instead of (D, N)
    with pytest.raises(ValueError):
        ovp.set(np.zeros((ovp.D, ovp.N + 1)))
    with pytest.raises(ValueError):
        psnr(np.zeros(3), np.zeros(4))


def test_psnr_formula():
    rng = np.random.RandomState(1)
    t = rng.randint(0, 256, size=(20, 30)).astype(np.uint8)
    r = t + rng.normal(scale=10, size=t.shape)
    want = 10 * np.log10(255.0 ** 2 / np.mean((t.astype(np.float64) - r) ** 2))
    assert psnr(t, r) == pytest.approx(want, rel=1e-15)
    assert psnr(t, r, data_range=1.0) == pytest.approx(want - 20 * np.log10(255.0), rel=1e-12)
    assert psnr(t, t.astype(float) + 1.0) == pytest.approx(20 * np.log10(255.0))


def test_mergers_are_nan_reductions():
    st = np.array([[1.0, np.nan, 3.0], [2.0, np.nan, np.nan], [4.0, np.nan, 5.0], [np.nan, np.nan, 7.0]])
    out = mean_merger(st, axis=0)
    assert out[0] == 7.0 / 3.0 and np.isnan(out[1]) and out[2] == 5.0
    out = median_merger(st, axis=0)
    assert out[0] == 2.0 and np.isnan(out[1]) and out[2] == 5.0


def test_custom_merger_runs_on_host():
    """Any callable other than mean_merger / median_merger gets the NaN-padded stack on the host (no engine is
    touched: the engine argument would fail if it were)."""
    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError("engine used: " + name)

    rng = np.random.RandomState(2)
    img = rng.normal(size=(9, 11, 3))
    ovp = MultiDimOverlappingPatches(img, 3, 4, patch_shift=2, engine=NoEngine())
    Y = oracle_extract(img, 3, 4, 2)
    Y[rng.random_sample(Y.shape) < 0.3] = np.nan
    seen = {}

    def nanmax(stack, axis=0):
        seen["shape"] = stack.shape
        return np.nanmax(stack, axis=axis)

    got = ovp.set_and_merge(Y.T, merge_method=nanmax)
    want = np.nanmax(oracle_stack(Y, img.shape, 3, 4, 2), axis=0)
    np.testing.assert_array_equal(got, want)
    assert got.shape == img.shape and seen["shape"][1:] == img.shape
    grey = rng.randint(0, 256, size=(8, 7)).astype(np.uint8)  # integer images are cast to float64
    ovp = OverlappingPatches(grey, 2, 2, engine=NoEngine())
    assert ovp.image.dtype == np.float64
    got = ovp.set_and_merge(oracle_extract(grey.astype(np.float64), 2, 2, 1).T, merge_method=np.nanmin)
    np.testing.assert_array_equal(got, grey)

"""sample_posterior(resident=True) / predictive_moments(resident=True) on the GPU: the draws and moments stay on the device
and are merged there (evoamd_patches_merge_samples / evoamd_patches_merge_predictive, csrc/kernels_patches.hpp).

Both models, H = 12 latents, S = 10 states (S_perm = 1 once), T = 5 draws.  The data are the patches of a small image of
which about 40 % of the entries are missing; patch 0 has no reliable entry at all (its draws are NaN rows).
  grey    13 x 11, 4 x 4 patches, shift 1: N = 80, D = 16; at most 16 estimates per pixel; pixel (0, 0) is covered by patch 0
          only, so it is NaN in every image;
  colour  9 x 10 x 3, 3 x 3 patches, shift 2: N = 20, D = 27; a ragged last column of patches, C innermost;
  wide    20 x 20, 9 x 9 patches, shift 1: N = 144, D = 81; more than 64 estimates per pixel: the R > 1 median kernel.
Everything is held bit for bit against the default path of the same state and seed: np.asarray of the handle against the
"y" of resident=False, every merged image against Engine.patches_merge of the host slice, the device moments against
image_moments_host of the merged images, the predictive merges against the merges of the downloaded arrays.  One test adds
T = 19 draws and windows of them (a longer recurrence, t0 > 0 with images and moments of one call)."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from _predictive_problems import make_theta
from evo_amd import _lib
from evo_amd._lib import check
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.resident import ResidentDraws, ResidentMoments
from evo_amd.utils.prepost import (MultiDimOverlappingPatches, OverlappingPatches, estimate_stack, image_moments_host,
                                   mean_merger, median_merger, precision_merger)
from evo_amd.variational import init_states

pytestmark = pytest.mark.gpu

HL, S, T, SEED = 12, 10, 5, 424242
GEOM = {"grey": ((13, 11), 4, 4, 1, (80, 16)), "colour": ((9, 10, 3), 3, 3, 2, (20, 27)), "wide": ((20, 20), 9, 9, 1, (144, 81))}
# (geometry, model, S_perm)
CASES = [("grey", "ebsc", 0), ("grey", "es3c", 1), ("colour", "ebsc", 0), ("colour", "es3c", 0), ("wide", "ebsc", 0),
         ("wide", "es3c", 0)]
MERGERS = ((mean_merger, "mean"), (median_merger, "median"))


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _patches_of(eng, image, ph, pw, shift):
    cls = MultiDimOverlappingPatches if image.ndim == 3 else OverlappingPatches
    return cls(image, ph, pw, shift, engine=eng)


@lru_cache(maxsize=None)
def _inputs(geom, algo, S_perm):
    """Image-shaped data (computed once per case; read-only): (Y, x_infr, theta, ss, lpj)."""
    shape, ph, pw, shift, (N, D) = GEOM[geom]
    rng = np.random.RandomState(1000 * len(geom) + 10 * (algo == "ebsc") + S_perm)
    tmp = Engine(0)
    try:
        image = rng.normal(size=shape) * 1.5
        reliable = rng.random_sample(shape) >= 0.4
        Y = _patches_of(tmp, image, ph, pw, shift).get().T.copy()
        x_infr = _patches_of(tmp, reliable.astype(np.float64), ph, pw, shift).get().T > 0.5
    finally:
        tmp.close()
    assert Y.shape == (N, D)
    x_infr[0] = False  # patch 0: no reliable entry at all
    Y[~x_infr] = np.nan
    theta = make_theta(rng, algo, D, HL)
    ss = np.zeros((N, S, HL), dtype=bool)
    for n in range(N):
        seen = set()
        while len(seen) < S:
            seen.add(tuple(sorted(rng.choice(HL, rng.randint(1, 4), replace=False))))
        for s, st in enumerate(sorted(seen)):
            ss[n, s, list(st)] = True
    lpj = rng.normal(size=(N, S_perm + S)) * 1.5 - 40.0
    for a in (Y, x_infr, ss, lpj):
        a.setflags(write=False)
    return Y, x_infr, theta, ss, lpj


def _setup(eng, geom, algo, S_perm):
    shape, ph, pw, shift, (N, D) = GEOM[geom]
    Y, x_infr, theta, ss, lpj = _inputs(geom, algo, S_perm)
    model = (BSC if algo == "ebsc" else SSSC)(D, HL, S, engine=eng)
    suff = init_states(N, S, HL, "fit", "randflip", 4, 1, 1,
                       permanent={"background": False, "allzero": bool(S_perm), "singletons": False})
    assert suff["ss"].shape == ss.shape and suff["lpj"].shape == lpj.shape
    suff["ss"], suff["lpj"] = np.array(ss), np.array(lpj)
    my_data = {"y": np.array(Y), "x_infr": np.array(x_infr), "x": np.array(x_infr)}
    ovp = _patches_of(eng, np.zeros(shape), ph, pw, shift)
    assert (ovp.N, ovp.D) == (N, D)
    return model, dict(theta), suff, my_data, ovp


def _corner(ovp):
    """The pixels that patch 0 alone covers (the next patch starts ``shift`` further)."""
    corner = np.zeros(ovp.shape, dtype=bool)
    corner[:ovp.shift, :ovp.shift] = True
    return corner


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _host_images(eng, y, ovp, name):
    return np.stack([eng.patches_merge(np.ascontiguousarray(y[:, t]), ovp.shape, ovp.ph, ovp.pw, ovp.shift, name)
                     for t in range(y.shape[1])])


def _check_handle(eng, h, y, ovp, what):
    """Laws 2 and 3 of a handle ``h`` against the host array ``y`` of the same draws; the handle is not read before."""
    n = y.shape[1]
    assert isinstance(h, ResidentDraws) and h.shape == y.shape and h.resident and not h.materialised
    for merger, name in MERGERS:
        imgs = h.merge(ovp, merger)
        want = _host_images(eng, y, ovp, name)
        assert imgs.shape == (n,) + ovp.shape
        for t in range(n):
            assert _same(imgs[t], want[t]), (what, name, t)
        assert _same(h.merge(ovp, merger, draws=slice(1, 4)), want[1:4]), (what, name)
        assert _same(h.merge(ovp, merger, draws=n - 1), want[n - 1:]), (what, name)
        assert _same(ovp.set_and_merge(h.draw(2).T, merge_method=merger), want[2]), (what, name)
        mean, std = h.merge_moments(ovp, merger)
        m_host, s_host = image_moments_host(imgs)
        assert _same(mean, m_host) and _same(std, s_host), (what, name)
        mean, std = h.merge_moments(ovp, merger, draws=slice(1, 4))
        m_host, s_host = image_moments_host(imgs[1:4])
        assert _same(mean, m_host) and _same(std, s_host), (what, name)
    assert not h.materialised  # nothing of y was downloaded so far
    return h.merge(ovp), h.merge_moments(ovp)


@pytest.mark.parametrize("geom,algo,S_perm", CASES)
def test_draws_merge_where_they_lie(eng, geom, algo, S_perm):
    model, theta, suff, my_data, ovp = _setup(eng, geom, algo, S_perm)
    x_infr = my_data["x_infr"]
    for fill in ("missing", "all"):
        ref = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED, fill=fill)
        out = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED, fill=fill, resident=True)
        assert sorted(out) == sorted(ref) and out["info"] == ref["info"] and ref["info"]["n_skipped"] == 1
        for k in ref:
            if k not in ("y", "info"):
                assert _same(out[k], ref[k]), k
        y, h = ref["y"], out["y"]
        assert np.isnan(y[0]).all() and not np.isnan(y[1:]).any()
        imgs, (mean, std) = _check_handle(eng, h, y, ovp, (geom, algo, fill))
        # pixel (0, 0) -- with shift 2 the first 2 x 2 pixels -- is covered by patch 0 alone: NaN in every image and in
        # both moments; no other pixel is
        assert np.isnan(imgs[:, 0, 0]).all() and np.isnan(mean[0, 0]).all() and np.isnan(std[0, 0]).all()
        corner = _corner(ovp)
        assert np.array_equal(np.isnan(imgs), np.broadcast_to(corner, imgs.shape))
        assert np.array_equal(np.isnan(mean), corner) and np.array_equal(np.isnan(std), corner)
        if fill == "missing":  # all covering estimates reliable: every draw carries the data there, the spread is exactly 0
            stack = estimate_stack(x_infr.astype(np.float64), ovp.shape[0], ovp.shape[1], ovp.C, ovp.ph, ovp.pw, ovp.shift)
            fixed = (np.nanmin(stack, axis=0) == 1.0).reshape(ovp.shape)
            assert fixed.any() and not fixed.all()
            assert (std[fixed] == 0.0).all() and (std[~corner] > 0.0).any()
        # law 1 last: the download gives the array of the default path, bit for bit, once
        a = np.asarray(h)
        assert _same(a, y) and np.asarray(h) is a and h.materialised


def test_more_draws_and_windows_of_them(eng):
    """T = 19: the recurrence over more draws, windows that start at t0 > 0, images and moments from one call."""
    model, theta, suff, my_data, ovp = _setup(eng, "grey", "es3c", 1)
    ref = model.sample_posterior(theta, suff, my_data, n_samples=19, seed=SEED, fill="all", keep=("y",))
    out = model.sample_posterior(theta, suff, my_data, n_samples=19, seed=SEED, fill="all", keep=("y",), resident=True)
    assert sorted(out) == ["info", "y"]
    h, y = out["y"], ref["y"]
    want = _host_images(eng, y, ovp, "mean")
    assert _same(h.merge(ovp), want)
    assert _same(h.merge(ovp, draws=slice(3, 17)), want[3:17])
    for draws in (None, slice(3, 17), slice(0, 8), slice(2, 11)):
        mean, std = h.merge_moments(ovp, draws=draws)
        m_host, s_host = image_moments_host(want[slice(None) if draws is None else draws])
        assert _same(mean, m_host) and _same(std, s_host), draws
    # images and moments of one call of the library
    imgs, mean, std = eng.patches_merge_samples(ovp.shape, ovp.ph, ovp.pw, ovp.shift, "mean", 0, 19, images=True, moments=True)
    m_host, s_host = image_moments_host(want)
    assert _same(imgs, want) and _same(mean, m_host) and _same(std, s_host)
    assert not h.materialised


@pytest.mark.parametrize("geom,algo,S_perm", CASES)
def test_predictive_moments_merge_where_they_lie(eng, geom, algo, S_perm):
    model, theta, suff, my_data, ovp = _setup(eng, geom, algo, S_perm)
    mean, var, info = model.predictive_moments(theta, suff, my_data)
    mean_h, var_h, info_h = model.predictive_moments(theta, suff, my_data, resident=True)
    assert info_h == info and info["n_skipped"] == 1
    assert isinstance(mean_h, ResidentMoments) and isinstance(var_h, ResidentMoments) and mean_h.shape == mean.shape
    want = ovp.set_and_merge(mean.T, merge_method=precision_merger(var.T))
    assert _same(ovp.set_and_merge(mean_h.T, merge_method=precision_merger(var_h.T)), want)
    assert np.array_equal(np.isnan(want), _corner(ovp))
    assert _same(ovp.set_and_merge(var_h.T, merge_method=mean_merger), ovp.set_and_merge(var.T, merge_method=mean_merger))
    for merger, _ in MERGERS:
        assert _same(ovp.set_and_merge(mean_h.T, merge_method=merger), ovp.set_and_merge(mean.T, merge_method=merger))
    assert not mean_h.materialised and not var_h.materialised  # nothing was downloaded
    # a handle with a host array (or the handles of two calls) takes the host path: same bits
    assert _same(ovp.set_and_merge(mean_h.T, merge_method=precision_merger(var.T)), want)
    assert _same(np.asarray(mean_h), mean) and _same(np.asarray(var_h.T), var.T)


def test_refusals_and_untouched_state(eng):
    model, theta, suff, my_data, ovp = _setup(eng, "grey", "es3c", 1)
    with pytest.raises(ValueError, match="keep"):
        model.sample_posterior(theta, suff, my_data, n_samples=T, keep=("slot", "s"), resident=True)
    ref = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED)
    first = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED, resident=True)["y"]
    other = OverlappingPatches(np.zeros((13, 11)), 3, 3, 1, engine=eng)  # N = 99, D = 9
    with pytest.raises(ValueError):
        first.merge(other)
    with pytest.raises(ValueError):
        other.set(first.draw(0).T)
    with pytest.raises(ValueError):
        eng.patches_merge_samples((13, 11), 3, 3, 1)
    with pytest.raises(ValueError):
        eng.patches_merge_predictive((13, 11), 3, 3, 1)
    for draws in (slice(0, T + 1), slice(0, T, 2), T):
        with pytest.raises(ValueError):
            first.merge(ovp, draws=draws)
    # the library's own refusals (EVOAMD_E_INVALID before anything is launched)
    img = np.empty((T,) + ovp.shape)
    args = (13, 11, 1, 4, 4, 1, 0)
    assert eng.lib.evoamd_patches_merge_samples(eng._h, *args, 0, T, _lib.dptr(img), None, None) == 0
    for rc in (eng.lib.evoamd_patches_merge_samples(eng._h, *args, 0, T + 1, _lib.dptr(img), None, None),
               eng.lib.evoamd_patches_merge_samples(eng._h, *args, -1, 2, _lib.dptr(img), None, None),
               eng.lib.evoamd_patches_merge_samples(eng._h, *args, T, 1, _lib.dptr(img), None, None),
               eng.lib.evoamd_patches_merge_samples(eng._h, *args, 0, 0, _lib.dptr(img), None, None),
               eng.lib.evoamd_patches_merge_samples(eng._h, *args, 0, T, None, None, None),
               eng.lib.evoamd_patches_merge_samples(eng._h, 13, 11, 1, 3, 3, 1, 0, 0, T, _lib.dptr(img), None, None),
               eng.lib.evoamd_patches_merge_samples(eng._h, 13, 11, 1, 4, 4, 1, 2, 0, T, _lib.dptr(img), None, None),
               eng.lib.evoamd_patches_merge_predictive(eng._h, 13, 11, 1, 3, 3, 1, 2, _lib.dptr(img)),
               eng.lib.evoamd_patches_merge_predictive(eng._h, 13, 11, 1, 4, 4, 1, 4, _lib.dptr(img))):
        assert rc != 0 and b"evoamd_patches_merge_" in eng.lib.evoamd_last_error()
    # the EM state and the validity flags across the merges
    eng.lpj_resident()
    lpj0, v0 = eng.download_lpj(), eng.debug_validity()
    imgs = first.merge(ovp)
    first.merge_moments(ovp, median_merger)
    assert eng.debug_validity() == v0
    eng.lpj_resident()
    assert np.array_equal(eng.download_lpj(), lpj0) and eng.debug_validity() == v0
    assert _same(imgs, _host_images(eng, ref["y"], ovp, "mean"))
    # draws made without y: nothing to merge
    model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED, keep=("slot",))
    assert eng.lib.evoamd_patches_merge_samples(eng._h, *args, 0, T, _lib.dptr(img), None, None) != 0
    assert b"did not keep y" in eng.lib.evoamd_last_error()
    # the next call outdates the first, unread handle; the second merges correctly
    y2 = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED + 1, fill="all")["y"]
    second = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED + 1, fill="all", resident=True)["y"]
    for call in (lambda: first.merge(ovp), lambda: np.asarray(first), lambda: ovp.set_and_merge(first.draw(0).T)):
        with pytest.raises(RuntimeError, match="a later sample_posterior"):
            call()
    assert _same(second.merge(ovp), _host_images(eng, y2, ovp, "mean")) and not second.materialised
    third = eng.sample_posterior(T, seed=SEED + 1, keep=("y",), fill="all", resident=True)["y"]  # behind the model's back
    with pytest.raises(RuntimeError, match="same engine"):
        second.merge(ovp)
    assert _same(third.merge(ovp, median_merger), _host_images(eng, y2, ovp, "median"))
    # predictive handles: the next call outdates the unread ones, a configure releases the buffers in the library
    mean1, var1, _ = model.predictive_moments(theta, suff, my_data, resident=True)
    mean2, var2, _ = model.predictive_moments(theta, suff, my_data, resident=True)
    with pytest.raises(RuntimeError, match="a later predictive_moments"):
        ovp.set_and_merge(mean1.T, merge_method=precision_merger(var1.T))
    ovp.set_and_merge(mean2.T, merge_method=precision_merger(var2.T))
    eng.configure("sssc", 80, 16, HL, S, 1, 4)
    assert eng.lib.evoamd_patches_merge_predictive(eng._h, 13, 11, 1, 4, 4, 1, 2, _lib.dptr(img)) != 0
    assert eng.lib.evoamd_patches_merge_samples(eng._h, *args, 0, T, _lib.dptr(img), None, None) != 0
    for call in (lambda: third.merge(ovp), lambda: np.asarray(var2)):
        with pytest.raises(RuntimeError):
            call()


def _live():
    out = (ctypes.c_int64 * 2)()
    check(_lib.load().evoamd_debug_live_buffers(out))
    return int(out[0]), int(out[1])


def test_no_buffer_outlives_its_context():
    _inputs("wide", "es3c", 0)  # (its temporary engine is gone before the count)
    before = _live()
    own = Engine(0)
    try:
        model, theta, suff, my_data, ovp = _setup(own, "wide", "es3c", 0)
        h = model.sample_posterior(theta, suff, my_data, n_samples=T, seed=SEED, resident=True)["y"]
        h.merge(ovp, median_merger)
        h.merge_moments(ovp)
        mean_h, var_h, _ = model.predictive_moments(theta, suff, my_data, resident=True)
        ovp.set_and_merge(mean_h.T, merge_method=precision_merger(var_h.T))
        assert _live()[0] > before[0]
    finally:
        own.close()
    assert _live() == before

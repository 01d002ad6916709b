"""Overlapping image patches: the pre- and post-processing of the reference's image workflows
(examples/image-denoising/main.py, examples/image-inpainting/main.py), which import

    from tvutil.prepost import OverlappingPatches, MultiDimOverlappingPatches, mean_merger, median_merger

With evo_amd that import reads ``from evo_amd.utils.prepost import ...`` and the loops run unchanged.  Extraction and
the two standard merges run as HIP kernels on the GPU (``Engine.patches_extract`` / ``Engine.patches_merge``); any other
merge callable runs on the host over the stack of estimates; ``precision_merger(var.T)`` weights every estimate with the
inverse of its posterior-predictive variance (Model.predictive_moments) and runs on the GPU too.  A model built with ``resident_reconstruction=True`` stores a
``ResidentReconstruction`` handle in my_data["y_reconstructed"]; ``set_and_merge(handle.T, ...)`` merges it on the device.
``sample_posterior(..., resident=True)`` and ``predictive_moments(..., resident=True)`` leave their draws and moments on
the device in the same way (``ResidentDraws`` / ``ResidentMoments``): one draw (``handle.draw(t).T``), the predictive mean
with ``precision_merger(var.T)`` and the uncertainty map ``var.T`` merge where they lie; ``image_moments_host`` is the
NumPy mirror of the pixelwise moments ``ResidentDraws.merge_moments`` forms on the device.

Conventions (ours; tvutil is not a dependency and bit parity with it is not claimed):

- image (H, W) or (H, W, C), cast to float64; NaN marks missing pixels and passes through.
- patch tops 0, s, 2s, ... while <= H - ph, plus H - ph appended if that value was not reached, so every pixel is
  covered while s <= ph; lefts the same with W, pw.
- patch n = ir * nc + ic, row-major over the (top, left) grid; with s = 1, N = (H - ph + 1) (W - pw + 1).
- element d = (dy * pw + dx) * C + c (channel innermost, as in the image's memory); D = ph * pw * C.
- ``get()`` returns the patches as (D, N) -- what the examples transpose into (N, D) data.
- merging: every output element gathers one estimate from each patch that covers it, in increasing n; the stack of
  estimates is (K, H, W[, C]) with NaN padding.  ``mean_merger`` is np.nanmean over it and ``median_merger``
  np.nanmedian (even counts: (lo + hi) / 2); the GPU kernels reproduce both bit for bit.  No valid estimate: NaN.
- limits: ph * pw <= 1024, ph <= H, pw <= W, patch_shift >= 1.
"""
import warnings

import numpy as np

from ..resident import DrawFace, ResidentMoments, ResidentReconstruction

_RESIDENT_ROWS = (ResidentReconstruction, DrawFace, ResidentMoments)  # (N, D) rows on the device, either face

MAX_PATCH_ELEMS = 1024


def mean_merger(stack, axis=0):
    """np.nanmean along ``axis``; all-NaN slices give NaN without a warning."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(stack, axis=axis)


def median_merger(stack, axis=0):
    """np.nanmedian along ``axis``; all-NaN slices give NaN without a warning."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmedian(stack, axis=axis)


class PrecisionMerger:
    """Precision-weighted mean of every element's estimates: out = (sum_k e_k w_k) / (sum_k w_k) with w_k = 1 / v_k, v the
    posterior-predictive variances of the patch entries (Model.predictive_moments), held as ``var_T`` (D, N) like the
    patches.  The sums run over the covering patches in increasing n, multiply and add as separate operations, both from
    0.0; an estimate that is NaN, or whose variance is NaN or <= 0, is skipped; no valid estimate gives NaN.
    ``set_and_merge(mean.T, merge_method=precision_merger(var.T))`` merges on the GPU (Engine.patches_merge with
    method="precision"); calling the object on the (K, H, W[, C]) estimate stack is the host mirror, bit for bit -- it
    builds the stack of the variances with estimate_stack, for which it needs the geometry: ``bind`` (merge() calls it).
    Merging ``var.T`` itself with mean_merger gives the per-pixel uncertainty map (the mean variance of a pixel's
    estimates); the variance of the MERGED image is not that, nor 1 / sum_k w_k: patch estimates are not independent."""

    def __init__(self, var_T):
        # a ResidentMoments handle stays on the device: merge() runs the precision merge there when the estimates are the
        # mean of the same predictive_moments call, and var_T downloads it only for the host paths
        self._src = var_T if isinstance(var_T, ResidentMoments) else np.asarray(var_T, dtype=np.float64)
        if self._src.ndim != 2:
            raise ValueError("precision_merger: var_T must be (D, N) like the patches, got shape %s" % (self._src.shape,))
        self._geom = None

    @property
    def var_T(self):
        """The variances as a (D, N) ndarray (a handle is downloaded on first use)."""
        if isinstance(self._src, ResidentMoments):
            a = self._src.rows()
            return a.T if self._src.transposed else a
        return self._src

    @property
    def resident_var(self):
        """The (N, D) face of the ResidentMoments handle the merger was built from, or None."""
        if not isinstance(self._src, ResidentMoments):
            return None
        return self._src.T if self._src.transposed else self._src

    def bind(self, H, W, C, ph, pw, shift):
        """The patch geometry the variances belong to (ValueError when (D, N) does not fit it)."""
        N, D = patch_geometry(H, W, C, ph, pw, shift)
        if tuple(self._src.shape) != (D, N):
            raise ValueError("precision_merger: variances of shape (D, N) = %s, the patches are %s"
                             % (tuple(self._src.shape), (D, N)))
        self._geom = (int(H), int(W), int(C), int(ph), int(pw), int(shift))
        return self

    def __call__(self, stack, axis=0):
        if self._geom is None:
            raise ValueError("precision_merger: bind(H, W, C, ph, pw, shift) first (OverlappingPatches.merge does)")
        if axis != 0:
            raise ValueError("precision_merger merges along axis 0 of the estimate stack")
        H, W, C = self._geom[:3]
        stack = np.asarray(stack, dtype=np.float64)
        shape = stack.shape[1:]
        est = stack.reshape(stack.shape[0], H, W, C)
        vst = estimate_stack(self.var_T.T, *self._geom)
        num, den = np.zeros((H, W, C)), np.zeros((H, W, C))
        cnt = np.zeros((H, W, C), dtype=np.int64)
        with np.errstate(all="ignore"):
            for k in range(est.shape[0]):  # increasing n: the order of the stack
                ok = ~np.isnan(est[k]) & (vst[k] > 0.0)
                w = 1.0 / np.where(ok, vst[k], 1.0)
                num = np.where(ok, num + np.where(ok, est[k], 0.0) * w, num)
                den = np.where(ok, den + w, den)
                cnt += ok
            out = np.where(cnt > 0, num / den, np.nan)
        return out.reshape(shape)


def precision_merger(var_T):
    """The merge_method of a precision-weighted merge: ``ovp.set_and_merge(mean.T, merge_method=precision_merger(var.T))``
    with (mean, var, _) = model.predictive_moments(...).  See PrecisionMerger."""
    return PrecisionMerger(var_T)


def image_moments_host(images):
    """(mean, std) over axis 0 of a (T, ...) stack of images by Welford's recurrence in draw order, from mean = 0 and
    M2 = 0: delta = x_t - mean, mean += delta / t, M2 += delta (x_t - mean); std = sqrt(M2 / T) (ddof 0, the np.std of T
    merged images).  Sequential over axis 0, multiply and add as separate operations: the NumPy mirror, bit for bit, of
    the moments ResidentDraws.merge_moments forms on the device.  A NaN in any image makes both outputs NaN at that pixel;
    identical images give their own value and exactly 0."""
    images = np.asarray(images, dtype=np.float64)
    if images.ndim < 1 or images.shape[0] < 1:
        raise ValueError("image_moments_host: a stack of at least one image, got shape %s" % (images.shape,))
    mean = np.zeros(images.shape[1:])
    M2 = np.zeros(images.shape[1:])
    with np.errstate(invalid="ignore"):
        for t in range(images.shape[0]):
            delta = images[t] - mean
            mean = mean + delta / float(t + 1)
            M2 = M2 + delta * (images[t] - mean)
        return mean, np.sqrt(M2 / float(images.shape[0]))


def patch_tops(L, p, s):
    """Top rows (or left columns) of the patches along an axis of length L: 0, s, 2s, ... <= L - p, plus L - p."""
    tops = list(range(0, L - p + 1, s))
    if tops[-1] != L - p:
        tops.append(L - p)
    return np.asarray(tops, dtype=np.int64)


def patch_geometry(H, W, C, ph, pw, shift):
    """(N, D) of the patches of an (H, W, C) image; ValueError for arguments outside the limits."""
    H, W, C, ph, pw, shift = (int(v) for v in (H, W, C, ph, pw, shift))
    if min(H, W, C) < 1:
        raise ValueError("image dimensions must be >= 1, got %s" % ((H, W, C),))
    if ph < 1 or pw < 1:
        raise ValueError("patch height and width must be >= 1, got %d x %d" % (ph, pw))
    if ph > H or pw > W:
        raise ValueError("patch %d x %d larger than the image %d x %d" % (ph, pw, H, W))
    if shift < 1:
        raise ValueError("patch_shift must be >= 1, got %d" % shift)
    if ph * pw > MAX_PATCH_ELEMS:
        raise ValueError("patches of %d x %d elements exceed the limit of %d" % (ph, pw, MAX_PATCH_ELEMS))
    N = len(patch_tops(H, ph, shift)) * len(patch_tops(W, pw, shift))
    return N, ph * pw * C


def estimate_stack(Y, H, W, C, ph, pw, shift):
    """Host form of the merge input: the (K, H, W, C) stack of every element's estimates in increasing n, NaN-padded.
    Y is (N, D).  Estimate of element (y, x) from patch (ir, ic) sits in slot (ir - ir0(y)) kc(x) + (ic - ic0(x)),
    where [ir0(y), ..] / [ic0(x), ..] are the first grid rows / columns that cover y / x and kc(x) how many cover x."""
    tops, lefts = patch_tops(H, ph, shift), patch_tops(W, pw, shift)
    nc = len(lefts)

    def cover(L, p, starts):
        ys = np.arange(L)
        lo = np.searchsorted(starts, ys - p + 1, side="left")
        hi = np.searchsorted(starts, ys, side="right") - 1
        return lo, hi - lo + 1

    r0, kr = cover(H, ph, tops)
    c0, kc = cover(W, pw, lefts)
    K = int(kr.max()) * int(kc.max())
    stack = np.full((K, H, W, C), np.nan)
    Y4 = np.asarray(Y, dtype=np.float64).reshape(len(tops), nc, ph, pw, C)
    ir = np.arange(len(tops))[:, None]
    ic = np.arange(nc)[None, :]
    for dy in range(ph):
        y = tops[:, None] + dy
        for dx in range(pw):
            x = lefts[None, :] + dx
            k = (ir - r0[y]) * kc[x] + (ic - c0[x])
            stack[k, y, x] = Y4[:, :, dy, dx]
    return stack


_shared = None


def shared_engine():
    """The process-wide Engine() on default_device(), created on first use."""
    global _shared
    if _shared is None:
        from ..engine import Engine
        _shared = Engine()
    return _shared


class OverlappingPatches:
    """Overlapping patches of a grey (H, W) image (conventions: module docstring)."""

    _ndim = 2

    def __init__(self, image, patch_height, patch_width, patch_shift=1, engine=None):
        image = np.asarray(image)
        if image.ndim != self._ndim:
            raise ValueError("%s takes a %d-D image, got shape %s" % (type(self).__name__, self._ndim, image.shape))
        self.image = image.astype(np.float64)
        self.shape = self.image.shape
        H, W = self.shape[:2]
        self.C = self.shape[2] if self._ndim == 3 else 1
        self.ph, self.pw, self.shift = int(patch_height), int(patch_width), int(patch_shift)
        self.N, self.D = patch_geometry(H, W, self.C, self.ph, self.pw, self.shift)
        self._engine = engine
        self._Y = None  # (N, D) patches: extracted on first use, replaced by set()

    @property
    def engine(self):
        return self._engine if self._engine is not None else shared_engine()

    def _patches(self):
        if self._Y is None:
            self._Y = self.engine.patches_extract(self.image, self.ph, self.pw, self.shift)
        return self._Y

    def get(self):
        """The patches as (D, N) float64 (a transposed view of the (N, D) rows), NaN preserved."""
        return self._patches().T

    def set(self, Y_T):
        """Store new patches, (D, N) like get() returns them, or rows that lie on the device, either face: a
        ResidentReconstruction handle, a draw of a ResidentDraws handle (``handle.draw(t)``), a ResidentMoments handle."""
        if isinstance(Y_T, _RESIDENT_ROWS):
            rows = Y_T.T if Y_T.transposed else Y_T
            if rows.shape != (self.N, self.D):
                raise ValueError("set: the resident rows are (N, D) = %s, the patches are %s"
                                 % (rows.shape, (self.N, self.D)))
            self._Y = rows
            return
        Y_T = np.asarray(Y_T)
        if Y_T.shape != (self.D, self.N):
            raise ValueError("set: expected patches of shape (D, N) = %s, got %s" % ((self.D, self.N), Y_T.shape))
        self._Y = Y_T.T  # (N, D); C-contiguous when Y_T is the transpose of C-ordered rows, passed on without a copy

    def merge(self, merge_method=mean_merger):
        """Image of the input's shape from the current patches.  mean_merger / median_merger run on the GPU; any other
        callable f is applied on the host as f(stack, axis=0) to the NaN-padded (K, H, W[, C]) estimate stack.
        After set() with a ResidentReconstruction handle, mean_merger / median_merger read the reconstruction on the
        HANDLE's engine (the model's context, whichever engine this object was built with) and only the image comes
        back; any other callable, or a handle whose array was read and whose device copy is gone, takes the host array.
        That covers one rank holding all patches: with several ranks gather as before
        (gather_from_processes(my_data["y_reconstructed"]) materialises the handle).
        A draw of a ResidentDraws handle and a ResidentMoments handle merge in the same way on their engine;
        precision_merger(var.T) over mean.T runs there when both are the handles of one predictive_moments call, else
        both are downloaded."""
        Y = self._patches()
        if isinstance(merge_method, PrecisionMerger):
            merge_method.bind(self.shape[0], self.shape[1], self.C, self.ph, self.pw, self.shift)
            if isinstance(Y, ResidentMoments) and merge_method.resident_var is not None:
                img = Y.merge_precision(merge_method.resident_var, self.shape, self.ph, self.pw, self.shift)
                if img is not None:
                    return img
            if isinstance(Y, _RESIDENT_ROWS):
                Y = Y.rows()
            return self.engine.patches_merge(Y, self.shape, self.ph, self.pw, self.shift, "precision",
                                             weights=merge_method.var_T.T)
        gpu_merge = merge_method is mean_merger or merge_method is median_merger
        if isinstance(Y, _RESIDENT_ROWS):
            if gpu_merge:
                img = Y.merge(self.shape, self.ph, self.pw, self.shift, "mean" if merge_method is mean_merger else "median")
                if img is not None:
                    return img
            Y = Y.rows()
        if gpu_merge:
            method = "mean" if merge_method is mean_merger else "median"
            return self.engine.patches_merge(Y, self.shape, self.ph, self.pw, self.shift, method)
        stack = estimate_stack(Y, self.shape[0], self.shape[1], self.C, self.ph, self.pw, self.shift)
        return np.asarray(merge_method(stack, axis=0)).reshape(self.shape)

    def set_and_merge(self, Y_T, merge_method=mean_merger):
        self.set(Y_T)
        return self.merge(merge_method)


def merge_rows(ovp, Y, merge_method=mean_merger):
    """The image ``ovp.set_and_merge(Y.T, merge_method)`` gives for host rows Y (N, D), without replacing ovp's patches."""
    if merge_method is mean_merger or merge_method is median_merger:
        return ovp.engine.patches_merge(Y, ovp.shape, ovp.ph, ovp.pw, ovp.shift,
                                        "mean" if merge_method is mean_merger else "median")
    if isinstance(merge_method, PrecisionMerger):
        merge_method.bind(ovp.shape[0], ovp.shape[1], ovp.C, ovp.ph, ovp.pw, ovp.shift)
        return ovp.engine.patches_merge(Y, ovp.shape, ovp.ph, ovp.pw, ovp.shift, "precision", weights=merge_method.var_T.T)
    stack = estimate_stack(Y, ovp.shape[0], ovp.shape[1], ovp.C, ovp.ph, ovp.pw, ovp.shift)
    return np.asarray(merge_method(stack, axis=0)).reshape(ovp.shape)


class MultiDimOverlappingPatches(OverlappingPatches):
    """Overlapping patches of an (H, W, C) image, e.g. RGB (conventions: module docstring)."""

    _ndim = 3


def psnr(target, reco, data_range=255):
    """10 log10(data_range^2 / mean((target - reco)^2)) in float64: the skimage.metrics.peak_signal_noise_ratio call
    of the reference's examples (eval_fn in their utils.py)."""
    t = np.asarray(target, dtype=np.float64)
    r = np.asarray(reco, dtype=np.float64)
    if t.shape != r.shape:
        raise ValueError("psnr: shapes differ, %s vs %s" % (t.shape, r.shape))
    mse = np.mean((t - r) ** 2, dtype=np.float64)
    return 10.0 * np.log10(float(data_range) ** 2 / mse)

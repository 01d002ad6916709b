"""Handles of results that stay on the device: ResidentReconstruction (below), and -- second half of the module --
ResidentDraws / ResidentMoments, the "y" of ``sample_posterior(resident=True)`` and the mean / var of
``predictive_moments(resident=True)``, which follow the same rules.

ResidentReconstruction: my_data["y_reconstructed"] of a model built with ``resident_reconstruction=True``.

The default path downloads y_hat (N x D) after every reconstructing step, selects on the host and, at a merge, uploads
the N x D array again.  With the flag the selected reconstruction stays on the device
(``Engine.reconstruct_resident``) and my_data["y_reconstructed"] is this handle: ``OverlappingPatches.set_and_merge``
merges it where it lies and only the image comes back; whoever needs the array after all (``np.asarray``,
``gather_from_processes``) gets exactly the ndarray the default path would have stored, downloaded once.

A handle belongs to ONE statistics pass.  The next pass (a later step / E_step / reconstruct), new parameters or new
data outdate the device copy; a handle that was never read then raises RuntimeError naming the cause -- it never
returns the newer reconstruction (the idea of ``LazyTheta``).

Who notices that a handle is outdated -- three layers, each for a case the one before cannot see:
  the handle's ``stale`` cause   the model that made it replaces it (its next step / E_step / reconstruct) and says why;
  the engine's serial number     another model or a direct Engine.reconstruct_resident on the SAME engine made a newer one;
  the library (EVOAMD_E_INVALID) a statistics pass without reconstruction, new parameters or an upload of data / masks
                                 dropped the device copy although nobody made a newer reconstruction."""
import numpy as np


class _Core:
    """What a handle and its transpose share."""

    def __init__(self, engine, serial, y, x, x_infr):
        self.engine, self.serial = engine, serial
        self.y, self.x, self.x_infr = y, x, x_infr  # x_infr: None for complete data
        self.array = None   # the (N, D) ndarray once somebody asked for it
        self.stale = None   # why the device copy is gone (set only while nothing is cached)
        self.faces = [None, None]  # the (N, D) handle and its transpose


class ResidentReconstruction:
    """(N, D) float64, array-like: ``shape``, ``dtype``, ``ndim``, ``len``, ``.T``, ``np.asarray``."""

    dtype = np.dtype(np.float64)
    ndim = 2

    def __init__(self, engine, serial, y, x, x_infr=None, _core=None, _t=False):
        self._c = _Core(engine, serial, y, x, x_infr) if _core is None else _core
        self._t = bool(_t)
        self._c.faces[self._t] = self

    # ---- array-like surface ----------------------------------------------------------------
    @property
    def shape(self):
        N, D = self._c.y.shape
        return (D, N) if self._t else (N, D)

    def __len__(self):
        return self.shape[0]

    @property
    def T(self):
        other = self._c.faces[not self._t]
        return other if other is not None else ResidentReconstruction(None, None, None, None, _core=self._c, _t=not self._t)

    @property
    def transposed(self):
        """True for the (D, N) face."""
        return self._t

    @property
    def engine(self):
        return self._c.engine

    @property
    def serial(self):
        return self._c.serial

    @property
    def materialised(self):
        return self._c.array is not None

    @property
    def resident(self):
        """The device still holds THIS reconstruction as far as the Python layer knows (the library has the last word:
        it refuses a merge or a download once a statistics pass, new parameters or an upload outdated it)."""
        c = self._c
        return c.stale is None and getattr(c.engine, "_rec_serial", None) == c.serial

    def _outdate(self, cause):
        """The model is about to replace the device copy: an unread handle is lost from here on."""
        if self._c.array is None and self._c.stale is None:
            self._c.stale = cause

    def _cause(self):
        return self._c.stale or "a later reconstruction on the same engine"

    def rows(self):
        """The (N, D) ndarray the default path would have stored in my_data["y_reconstructed"] (_models.py:643-665):
        downloaded on first use, cached afterwards."""
        c = self._c
        if c.array is not None:
            return c.array
        if not self.resident:
            raise RuntimeError("this reconstruction was never read and the device copy is outdated by %s; read or merge "
                               "a handle before the next statistics pass" % self._cause())
        try:
            y_hat = c.engine.download_reconstruction(c.serial)
        except RuntimeError as e:  # the library refused: something outside the model outdated it
            raise RuntimeError("the resident reconstruction is outdated (%s)" % e) from e
        y_rec = c.y.copy()
        miss = np.logical_not(c.x)
        if c.x_infr is not None:  # datapoints without a single reliable entry are skipped (_models.py:648-649)
            miss &= c.x_infr.any(axis=1)[:, None]
        y_rec[miss] = y_hat[miss]
        c.array = y_rec
        return y_rec

    def __array__(self, dtype=None, copy=None):
        a = self.rows()
        a = a.T if self._t else a
        if dtype is not None and np.dtype(dtype) != a.dtype:
            return a.astype(dtype)
        return a.copy() if copy else a

    def merge(self, shape, ph, pw, shift, method):
        """Mean / median merge on the handle's engine while the device holds this reconstruction; None when it does not
        but the array was read before (the caller merges ``rows()``); RuntimeError when it is lost."""
        c = self._c
        if self.resident:
            try:  # (a geometry mismatch is a ValueError and passes through)
                return c.engine.patches_merge_resident(shape, ph, pw, shift, method, serial=c.serial)
            except RuntimeError as e:
                if c.array is None:
                    raise RuntimeError("the resident reconstruction is outdated (%s)" % e) from e
                return None
        if c.array is None:
            self.rows()  # raises, naming the cause
        return None

    def __repr__(self):
        state = "cached" if self.materialised else ("resident" if self.resident else "outdated")
        return "ResidentReconstruction(shape=%s, %s)" % (self.shape, state)


# ---- the draws of sample_posterior and the moments of predictive_moments, kept on the device ---------------------------
def _gpu_method(merge_method):
    """"mean" / "median" for the two mergers the merge kernels implement, else None."""
    from .utils.prepost import mean_merger, median_merger
    return "mean" if merge_method is mean_merger else ("median" if merge_method is median_merger else None)


class _ResultCore:
    """What the handles of ONE sample_posterior / predictive_moments call share.  ``kind``: the engine's serial counter
    that names the call ("_ps_serial" / "_pred_serial"); ``arrays``: the host copies once somebody asked for them."""

    def __init__(self, engine, kind, serial, what):
        self.engine, self.kind, self.serial, self.what = engine, kind, serial, what
        self.arrays = {}
        self.stale = None  # why the device copy is gone, once the model that made the handles said so

    @property
    def resident(self):
        return self.stale is None and getattr(self.engine, self.kind, None) == self.serial

    def outdate(self, cause):
        if self.stale is None:
            self.stale = cause

    def cause(self):
        return self.stale or "a later %s on the same engine" % self.what

    def lost(self):
        return RuntimeError("this result of %s was never read and the device copy is outdated by %s; read or merge a "
                            "handle before the next call" % (self.what, self.cause()))

    def fetch(self, name, download):
        """The host array ``name``: downloaded once by ``download()``, cached afterwards; RuntimeError when lost."""
        if name in self.arrays:
            return self.arrays[name]
        if not self.resident:
            raise self.lost()
        try:
            a = download()
        except RuntimeError as e:  # the library refused: something outside the model released the buffers
            raise RuntimeError("the resident result of %s is outdated (%s)" % (self.what, e)) from e
        self.arrays[name] = a
        return a

    def on_device(self, name, run):
        """``run()`` (a merge on the engine) while the device holds the result; None when it does not but the array
        ``name`` was read before (the caller merges the host copy); RuntimeError when it is lost."""
        if self.resident:
            try:  # (a geometry mismatch is a ValueError and passes through)
                return run()
            except RuntimeError as e:
                if name not in self.arrays:
                    raise RuntimeError("the resident result of %s is outdated (%s)" % (self.what, e)) from e
                return None
        if name not in self.arrays:
            raise self.lost()
        return None


class _RowsFace:
    """An (N, D) float64 array-like that lies on the device: ``shape``, ``dtype``, ``ndim``, ``len``, ``.T``, ``np.asarray``;
    what OverlappingPatches.set accepts next to an ndarray.  Subclasses give ``_shape_nd()``, ``rows()``, ``merge()`` and
    ``_twin(t)`` (the other face)."""

    dtype = np.dtype(np.float64)
    ndim = 2
    _t = False

    @property
    def shape(self):
        N, D = self._shape_nd()
        return (D, N) if self._t else (N, D)

    def __len__(self):
        return self.shape[0]

    @property
    def transposed(self):
        """True for the (D, N) face."""
        return self._t

    @property
    def T(self):
        return self._twin(not self._t)

    def __array__(self, dtype=None, copy=None):
        a = self.rows()
        a = a.T if self._t else a
        if dtype is not None and np.dtype(dtype) != a.dtype:
            return a.astype(dtype)
        return a.copy() if copy else a


class ResidentDraws:
    """"y" of ``sample_posterior(..., resident=True)``: (N, T, D) float64, array-like (``shape``, ``dtype``, ``ndim``,
    ``len``, ``np.asarray``).  The draws stay in the context's buffer; ``merge`` / ``merge_moments`` turn them into images
    on the device (Engine.patches_merge_samples) and only the images, or only their pixelwise mean and spread, come back.
    ``np.asarray(handle)`` downloads once and caches exactly the array the default path returns.

    A handle belongs to ONE sample_posterior call.  The next call on the engine outdates an unread handle: its ``merge`` /
    ``np.asarray`` then raise RuntimeError naming the cause; a handle whose array was read keeps working from the host copy.
    Who notices, as for ResidentReconstruction: the model that made the handle (its next sample_posterior), the engine's
    serial number (another model on the same engine), the library (an evoamd_configure released the buffers)."""

    dtype = np.dtype(np.float64)
    ndim = 3

    def __init__(self, engine, serial, shape):
        self._c = _ResultCore(engine, "_ps_serial", serial, "sample_posterior")
        self.shape = tuple(int(v) for v in shape)
        self._faces = {}

    def __len__(self):
        return self.shape[0]

    engine = property(lambda self: self._c.engine)
    serial = property(lambda self: self._c.serial)
    resident = property(lambda self: self._c.resident)
    materialised = property(lambda self: "y" in self._c.arrays)

    def _outdate(self, cause):
        """The model is about to draw again: an unread handle is lost from here on."""
        if not self.materialised:
            self._c.outdate(cause)

    def array(self):
        """The (N, T, D) ndarray of the default path: downloaded on first use, cached afterwards."""
        return self._c.fetch("y", lambda: self._c.engine.download_posterior_draws(self.shape[1], serial=self._c.serial))

    def __array__(self, dtype=None, copy=None):
        a = self.array()
        if dtype is not None and np.dtype(dtype) != a.dtype:
            return a.astype(dtype)
        return a.copy() if copy else a

    def draw(self, t):
        """Draw ``t`` as an (N, D) face (``.T`` gives the (D, N) one): OverlappingPatches.set / set_and_merge accept it, and
        mean_merger / median_merger then merge it on the handle's engine."""
        t = int(t)
        if not 0 <= t < self.shape[1]:
            raise ValueError("draw: t = %d, the handle holds draws 0 .. %d" % (t, self.shape[1] - 1))
        if t not in self._faces:
            self._faces[t] = [DrawFace(self, t, False), None]
        return self._faces[t][0]

    def _range(self, draws):
        """(t0, n) of ``draws``: None (all), a slice with step 1, or an int."""
        T = self.shape[1]
        if draws is None:
            return 0, T
        if isinstance(draws, slice):
            if draws.step not in (None, 1):
                raise ValueError("draws: a slice with step 1, got step %r" % (draws.step,))
            t0 = 0 if draws.start is None else int(draws.start)
            t1 = T if draws.stop is None else int(draws.stop)
        else:
            t0 = int(draws)
            t1 = t0 + 1
        if not 0 <= t0 < t1 <= T:
            raise ValueError("draws %d .. %d asked for, the handle holds draws 0 .. %d" % (t0, t1 - 1, T - 1))
        return t0, t1 - t0

    def _check(self, ovp):
        if (ovp.N, ovp.D) != (self.shape[0], self.shape[2]):
            raise ValueError("the draws are (N, D) = %s per draw, the patches are %s"
                             % ((self.shape[0], self.shape[2]), (ovp.N, ovp.D)))

    def _on_device(self, ovp, method, t0, n, images, moments):
        c = self._c
        return c.on_device("y", lambda: c.engine.patches_merge_samples(ovp.shape, ovp.ph, ovp.pw, ovp.shift, method, t0, n,
                                                                         images=images, moments=moments, serial=c.serial))

    def merge(self, ovp, merge_method=None, draws=None):
        """The merged images of ``draws`` (None: all; a slice with step 1; an int) as a (T', *ovp.shape) ndarray, image t
        what ``ovp.set_and_merge(y[:, t].T, merge_method)`` gives for the host array.  mean_merger (the default) and
        median_merger run on the handle's engine, one launch for all draws; any other callable, or a handle whose array
        was read and whose device copy is gone, takes the host array draw by draw."""
        from .utils.prepost import mean_merger, merge_rows
        merge_method = mean_merger if merge_method is None else merge_method
        t0, n = self._range(draws)
        self._check(ovp)
        method = _gpu_method(merge_method)
        if method is not None:
            got = self._on_device(ovp, method, t0, n, True, False)
            if got is not None:
                return got[0]
        y = self.array()
        return np.stack([merge_rows(ovp, y[:, t], merge_method) for t in range(t0, t0 + n)])

    def merge_moments(self, ovp, merge_method=None, draws=None):
        """(mean_img, std_img): the pixelwise mean and standard deviation (ddof 0) over the merged images of ``draws``,
        the Welford law of evo_amd.utils.prepost.image_moments_host.  With mean_merger / median_merger no image is
        downloaded (the mean merger does not even store them)."""
        from .utils.prepost import image_moments_host, mean_merger
        merge_method = mean_merger if merge_method is None else merge_method
        t0, n = self._range(draws)
        self._check(ovp)
        method = _gpu_method(merge_method)
        if method is not None:
            got = self._on_device(ovp, method, t0, n, False, True)
            if got is not None:
                return got[1], got[2]
        return image_moments_host(self.merge(ovp, merge_method, slice(t0, t0 + n)))

    def __repr__(self):
        state = "cached" if self.materialised else ("resident" if self.resident else "outdated")
        return "ResidentDraws(shape=%s, %s)" % (self.shape, state)


class DrawFace(_RowsFace):
    """One draw of a ResidentDraws handle as (N, D) rows (or, ``.T``, as (D, N))."""

    def __init__(self, draws, t, transposed):
        self.draws, self.t, self._t = draws, t, bool(transposed)

    def _shape_nd(self):
        return self.draws.shape[0], self.draws.shape[2]

    def _twin(self, t):
        faces = self.draws._faces[self.t]
        if faces[t] is None:
            faces[t] = DrawFace(self.draws, self.t, t)
        return faces[t]

    engine = property(lambda self: self.draws.engine)

    def rows(self):
        return self.draws.array()[:, self.t]

    def merge(self, shape, ph, pw, shift, method):
        """Mean / median merge of this draw on the handle's engine; None: merge ``rows()`` (see ResidentReconstruction.merge)."""
        c = self.draws._c
        got = c.on_device("y", lambda: c.engine.patches_merge_samples(shape, ph, pw, shift, method, self.t, 1, images=True,
                                                                        moments=False, serial=c.serial))
        return None if got is None else got[0][0]

    def __repr__(self):
        return "DrawFace(t=%d, shape=%s) of %r" % (self.t, self.shape, self.draws)


class ResidentMoments(_RowsFace):
    """``mean`` / ``var`` of ``predictive_moments(..., resident=True)``: (N, D) float64, array-like like
    ResidentReconstruction.  ``ovp.set_and_merge(mean.T, merge_method=precision_merger(var.T))`` with the two handles of one
    call, ``set_and_merge(var.T, mean_merger)`` and mean / median of ``mean`` merge on the device
    (Engine.patches_merge_predictive); everything else takes the host arrays, each downloaded once.  The next
    predictive_moments on the engine (or a configure) outdates unread handles: RuntimeError naming the cause."""

    def __init__(self, engine, serial, shape, which, _core=None, _t=False, _faces=None):
        self._c = _ResultCore(engine, "_pred_serial", serial, "predictive_moments") if _core is None else _core
        self._nd = tuple(int(v) for v in shape)
        self.which, self._t = which, bool(_t)
        self._pair = [None, None] if _faces is None else _faces
        self._pair[self._t] = self

    def sibling(self, which):
        """The handle of the other moment of the same call."""
        return ResidentMoments(None, None, self._nd, which, _core=self._c)

    def _shape_nd(self):
        return self._nd

    def _twin(self, t):
        if self._pair[t] is None:
            ResidentMoments(None, None, self._nd, self.which, _core=self._c, _t=t, _faces=self._pair)
        return self._pair[t]

    engine = property(lambda self: self._c.engine)
    serial = property(lambda self: self._c.serial)
    resident = property(lambda self: self._c.resident)
    materialised = property(lambda self: self.which in self._c.arrays)

    def _outdate(self, cause):
        """The model is about to form new moments: what was not read of this call is lost from here on."""
        if not ("mean" in self._c.arrays and "var" in self._c.arrays):
            self._c.outdate(cause)

    def same_call(self, other):
        return isinstance(other, ResidentMoments) and other._c is self._c

    def rows(self):
        c = self._c
        return c.fetch(self.which, lambda: c.engine.download_predictive(self.which, self._nd, serial=c.serial))

    def merge(self, shape, ph, pw, shift, method):
        """mean: its mean / median merge; var: its mean merge (the uncertainty map), on the handle's engine.  None: merge
        ``rows()`` (the device copy is gone but the array was read, or the combination has no device form)."""
        what = {("mean", "mean"): 0, ("mean", "median"): 1, ("var", "mean"): 3}.get((self.which, method))
        if what is None:
            return None
        c = self._c
        return c.on_device(self.which, lambda: c.engine.patches_merge_predictive(shape, ph, pw, shift, what, serial=c.serial))

    def merge_precision(self, var, shape, ph, pw, shift):
        """The precision-weighted merge of this mean by ``var`` on the device when both are the handles of one call; None:
        merge the host arrays."""
        if self.which != "mean" or not (self.same_call(var) and var.which == "var"):
            return None
        c = self._c
        if not c.resident and not ("mean" in c.arrays and "var" in c.arrays):
            raise c.lost()
        try:
            return c.on_device("mean", lambda: c.engine.patches_merge_predictive(shape, ph, pw, shift, 2, serial=c.serial))
        except RuntimeError:
            if "var" in c.arrays:
                return None
            raise

    def __repr__(self):
        state = "cached" if self.materialised else ("resident" if self.resident else "outdated")
        return "ResidentMoments(%s, shape=%s, %s)" % (self.which, self.shape, state)

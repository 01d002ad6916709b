"""ResidentReconstruction: my_data["y_reconstructed"] of a model built with ``resident_reconstruction=True``.

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

"""Model base class: the reference's EM driver surface (evo/models/_models.py) over the GPU engine.

Method names, argument order, dict keys and in-place mutation follow the reference
 so a training script written for ``evo.models`` runs unchanged:

    model = BSC(D, H, S)                      # or SSSC(...)
    theta = model.check_params(model.standard_init(my_data))
    my_suff_stat = init_states(N, S, H, "fit", "randflip", 10, 1, 1)
    F, S_nunique, S_sub, theta = model.step(theta, my_suff_stat, my_data)

What changes is where the work happens: the per-datapoint Python loops of the reference
(_models.py:497-538, bsc.py:193-223, sssc.py:510-656) become a handful of kernel launches over all
N datapoints of this rank (see evo_amd/engine.py and csrc/).  Two candidate-generation modes:

``rng="reference"``  candidates are drawn on the host from np.random in the reference's order, so
                     K^n trajectories are bit-identical to the reference for the same seed
                     (exactly for n_generations == 1, where all datapoints are generated first
                     and evaluated in one launch; for more generations the per-datapoint
                     operator is used so the stream stays exact).
``rng="device"``     candidates are generated on the GPU (counter-based generator); statistically
                     equivalent, K^n never leaves the device unless ``sync_host=True``.
"""
import numpy as np

from .. import engine as _engine
from .._lib import EvoAmdError
from ..resident import ResidentReconstruction
from ..utils import parallel
from ..variational import eas
from ..variational.utils import vary_Kn  # noqa: F401  (re-exported like the reference module does)
from ..variational.utils import init_states as _host_init_states

F64_MIN = np.finfo(np.float64).min

_blas_controller = None


class small_blas:
    """Bound the BLAS thread count for the H x H host solves of the Theta update: 1 thread up to
    H = 256, 8 above.  On a many-core GPU host whose process may only use a few CPUs, OpenBLAS
    otherwise starts one thread per *visible* core and the M-step's host part takes longer than
    all the kernels together (measured on the GPU box: 18 ms vs < 1 ms at H = 128, 300 ms at
    H = 512).  No-op when threadpoolctl is not installed."""

    def __init__(self, H):
        self._ctx = None
        global _blas_controller
        try:
            if _blas_controller is None:
                from threadpoolctl import ThreadpoolController
                _blas_controller = ThreadpoolController()
            self._ctx = _blas_controller.limit(limits=1 if H <= 256 else 8, user_api="blas")
        except Exception:  # threadpoolctl missing or no BLAS found: run unrestricted
            self._ctx = None

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False


def _reduce_array(comm, a):
    """Sum a float64 array over ranks with whatever the communicator offers."""
    if comm.size == 1:
        return a
    if hasattr(comm, "allreduce_array"):
        return comm.allreduce_array(a)
    return comm.allreduce(a)  # mpi4py pickle path sums ndarrays element-wise


class LazyTheta(dict):
    """The parameter dict step() hands back when ``lazy_theta=True``: same keys as the reference's, but the arrays
    (W, Psi, mus, pies and what is derived from them) stay on the device until somebody looks at them -- a training
    loop that only carries theta from one step() into the next never moves them over PCIe, a loop that logs W every
    epoch pays one download per epoch.  Scalars (sigma2 / sigma, pi, ljc ...) are always current.  Any read access
    materialises the arrays; passing the object back into step() does not."""

    def __init__(self, scalars, loader):
        super().__init__(scalars)
        self._loader = loader

    def _stale(self, scalars, loader):
        """New Theta on the device: keep the scalars, forget the arrays."""
        dict.clear(self)
        dict.update(self, scalars)
        self._loader = loader

    def _load(self):
        loader, self._loader = self._loader, None
        if loader is not None:
            dict.update(self, loader())

    @property
    def materialised(self):
        return self._loader is None

    def __getitem__(self, key):
        if self._loader is not None and dict.__contains__(self, key):
            return dict.__getitem__(self, key)  # a scalar: current without a download
        self._load()
        return dict.__getitem__(self, key)

    def __contains__(self, key):
        self._load()
        return dict.__contains__(self, key)

    def __iter__(self):
        self._load()
        return dict.__iter__(self)

    def __len__(self):
        self._load()
        return dict.__len__(self)

    def __repr__(self):
        return "LazyTheta(%s)" % ("pending" if self._loader is not None else dict.__repr__(self))

    def get(self, key, default=None):
        self._load()
        return dict.get(self, key, default)

    def keys(self):
        self._load()
        return dict.keys(self)

    def items(self):
        self._load()
        return dict.items(self)

    def values(self):
        self._load()
        return dict.values(self)

    def copy(self):
        self._load()
        return dict(dict.items(self))

    def pop(self, *a):
        self._load()
        return dict.pop(self, *a)

    def __setitem__(self, key, value):
        self._load()
        dict.__setitem__(self, key, value)

    def update(self, *a, **kw):
        self._load()
        dict.update(self, *a, **kw)

    def setdefault(self, key, default=None):
        self._load()
        return dict.setdefault(self, key, default)


class RefineResult:
    """What Model.refine_resident_states returns: ``F``, ``S_nunique``, ``S_sub`` (n_done,) per iteration, ``n_done`` (the
    longest rank's), ``n_done_local`` (this rank's) and ``stopped_early`` (n_done < the iterations asked for)."""
    __slots__ = ("F", "S_nunique", "S_sub", "n_done", "n_done_local", "stopped_early")

    def __init__(self, F, S_nunique, S_sub, n_done, n_done_local, stopped_early):
        self.F, self.S_nunique, self.S_sub = F, S_nunique, S_sub
        self.n_done, self.n_done_local, self.stopped_early = int(n_done), int(n_done_local), bool(stopped_early)

    def __repr__(self):
        return "RefineResult(n_done=%d, stopped_early=%s, F=%s)" % (
            self.n_done, self.stopped_early, self.F[-1] if self.n_done else None)


class SweepResult:
    """What Model.sweep_resident_states returns: ``F``, ``S_nunique``, ``S_sub`` (n_done,) per sweep, ``n_done`` (the
    longest rank's), ``n_done_local`` (this rank's), ``stopped_early`` (n_done < the sweeps asked for) and, per datapoint of
    this rank for the last sweep it ran, ``gain`` (N,), ``best_flip`` int32 (N,) and ``n_capped`` int32 (N,) of the flip
    stage (None with neighbourhood="swap") and ``swap_gain`` (N,), ``best_swap`` int32 (N, 2) and ``n_capped_swap`` int32
    (N,) of the swap stage (None with neighbourhood="flip")."""
    __slots__ = ("F", "S_nunique", "S_sub", "n_done", "n_done_local", "stopped_early", "gain", "best_flip", "n_capped",
                 "swap_gain", "best_swap", "n_capped_swap")

    def __init__(self, F, S_nunique, S_sub, n_done, n_done_local, stopped_early, gain, best_flip, n_capped,
                 swap_gain=None, best_swap=None, n_capped_swap=None):
        self.F, self.S_nunique, self.S_sub = F, S_nunique, S_sub
        self.n_done, self.n_done_local, self.stopped_early = int(n_done), int(n_done_local), bool(stopped_early)
        self.gain, self.best_flip, self.n_capped = gain, best_flip, n_capped
        self.swap_gain, self.best_swap, self.n_capped_swap = swap_gain, best_swap, n_capped_swap

    def __repr__(self):
        return "SweepResult(n_done=%d, stopped_early=%s, F=%s)" % (
            self.n_done, self.stopped_early, self.F[-1] if self.n_done else None)


class Model:
    model_name = None  # "bsc" | "sssc"

    def __init__(self, D, H, S, to_learn=("W", "pi", "sigma"), comm=None, rng="reference", sync_host=True,
                 device=None, engine=None, seed=0, device_mstep=False, dtype=np.float64, lazy_theta=False,
                 resident_reconstruction=False):
        """``D, H, S, to_learn, comm`` as in the reference (_models.py:20-56).  ``comm`` may be an
        mpi4py communicator or one of evo_amd.utils.parallel; None means one rank."""
        if rng not in ("reference", "device"):
            raise ValueError("rng must be 'reference' or 'device'")
        if rng == "reference" and not sync_host:
            raise ValueError("rng='reference' generates candidates on the host and needs sync_host=True")
        self.comm = parallel.SerialComm() if comm is None else comm
        self.to_learn = list(to_learn)
        self.D, self.H, self.S = int(D), int(H), int(S)
        self.rng, self.sync_host, self.seed = rng, bool(sync_host), int(seed)
        # device_mstep: Theta update, clamps and precompute run on the GPU too (csrc/kernels_mstep.hpp);
        # an EM iteration is then ONE stream of kernels with a single host sync.  The H x H solves
        # use Gauss-Jordan instead of LAPACK, so Theta agrees with the host formulas to ~1e-12 but
        # not bit for bit -- keep it off for rng="reference" parity runs.
        self.device_mstep = bool(device_mstep)
        # lazy_theta (device_mstep only): step() returns a LazyTheta whose arrays are downloaded when they are read --
        # the reference's step() returns Theta^new every epoch, which here is 3 MB over PCIe plus a 3 MB host copy per
        # iteration whether or not the caller looks at it.  Off by default: the returned object is then the caller's
        # own dict, mutated in place like the reference does.
        self.lazy_theta = bool(lazy_theta)
        # resident_reconstruction: wherever my_data["y_reconstructed"] is written (step / E_step / reconstruct with
        # do_reconstruction), the selected reconstruction stays on the device and the entry is a ResidentReconstruction
        # handle (evo_amd/resident.py) instead of an N x D ndarray: OverlappingPatches.set_and_merge(handle.T) merges it
        # there and only the image crosses to the host; np.asarray(handle) downloads what the default path stores.
        # Off by default: the reference's loop reads an ndarray every epoch.
        self.resident_reconstruction = bool(resident_reconstruction)
        self._draws_handle = self._moments_handle = None  # the handles of the last resident=True sample_posterior / predictive_moments
        self._rec_handle = None
        # dtype=np.float32 (EBSC only): the data, B = Y W and the E_q[s] rows are kept in float and the two long
        # contractions run on the f32 matrix cores; lpj arithmetic, selection, sums and Theta stay float64.  The reference
        # is float64-only -- this is BASELINE.json configs[4]'s "float32"; agreement with the float64 path ~1e-6 in lpj / F.
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise ValueError("dtype must be float64 or float32")
        if self.dtype == np.float32 and self.model_name != "bsc":
            raise NotImplementedError("float32 mode exists for EBSC (BSC) only")
        self._dev_theta = None   # the dict whose values mirror the parameters resident on the device
        tol = 1e-5
        self.noise_policy = {  # _models.py:47-52
            "W": (-np.inf, +np.inf, False, None),
            "pi": (tol, 1.0 - tol, False, None),
            "sigma": (tol, +np.inf, False, None),
        }
        self.B_max = 0.0
        self.B_max_shft = np.inf
        self.eps_lpj = F64_MIN
        self._engine = engine
        self._device = device
        # Device residency of my_data["y"], the masks and y_reconstructed is keyed on the array OBJECTS: the
        # model keeps a reference to what it uploaded and compares with `is`, so a new array of the same shape
        # (a fresh minibatch / epoch) is always uploaded, whatever address CPython recycles.  In-place edits of
        # an uploaded array are not seen: call invalidate() after them.
        self._y_token = None
        self._x_infr_token = None
        self._incomplete = False
        self._had_masks = False
        self._yrec_token = None
        self._resident = False   # K^n on the device is authoritative (sync_host=False only)
        self._kn_uploads = 0     # how often _prepare() has uploaded my_suff_stat["ss"]
        self._acc = None         # statistics computed by E_step for the M_step of the same step()
        self._n_steps = 0

    # ---- engine plumbing --------------------------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            self._engine = _engine.Engine(self._device)
        return self._engine

    @staticmethod
    def _cmax(my_suff_stat):
        n_par, n_child = my_suff_stat["n_parents"], my_suff_stat["n_children"]
        per_gen = n_par * (n_par - 1) if my_suff_stat["mutation_algorithm"] in (
            eas.cross, eas.cross_randflip, eas.cross_sparseflip) else n_par * n_child
        return max(1, per_gen * my_suff_stat["n_generations"])

    def invalidate(self):
        """Forget what is resident on the device: the next call uploads my_data["y"], the masks,
        y_reconstructed and K^n again.  Needed after IN-PLACE edits of those arrays (the reference re-reads
        my_data every step; here an unchanged array object is taken to hold unchanged data)."""
        self._y_token = self._x_infr_token = self._yrec_token = None
        self._xi_all_token = None
        if self._engine is not None:
            self._engine._keep_token = None  # the keep-mask of reconstruct_resident (my_data["x"], complete data)
        self._resident = False
        self._dev_theta = None

    def _complete(self, my_data):
        """my_data["x_infr"].all(), scanned ONCE per array object (25 M flags at the north-star shape: half a millisecond of
        host time per EM step where the reference's own step re-reads them -- on the critical path between two
        iterations); in-place edits need invalidate(), like everything else that is resident."""
        xi = my_data["x_infr"]
        tok = getattr(self, "_xi_all_token", None)
        if tok is None or tok[0] is not xi:
            self._xi_all_token = (xi, bool(xi.all()))
        return self._xi_all_token[1]

    @staticmethod
    def _same_objects(token, *objs):
        return token is not None and len(token) == len(objs) and all(a is b for a, b in zip(token, objs))

    def attach_resident_states(self, my_suff_stat, my_data, packed_chunks):
        """Hand K^n over bit-packed and in chunks instead of as my_suff_stat["ss"] (bool (N,S,H): 10 GB at the
        north-star shape N=100k, S=200, H=512).  ``packed_chunks`` yields (n0, uint8 (n, S, ceil(H/8))) in
        np.packbits layout.  K^n is then device-resident (sync_host=False); my_suff_stat["ss"] is not read."""
        if self.sync_host:
            raise ValueError("attach_resident_states needs sync_host=False")
        eng = self._prepare(my_suff_stat, my_data, upload_states=False)
        for n0, chunk in packed_chunks:
            eng.upload_states_packed(chunk, n0)
        self._resident = True

    def init_resident_states(self, my_data, parent_selection, mutation_algorithm, no_parents, no_children, no_generations,
                             bitflip_prob=None, Mprime=None, p_init_Kn=None, permanent=None, seed=None, max_rounds=256):
        """``init_states`` for this rank's ``my_data`` with K^n(0) drawn on the device (Engine.init_states): the same law,
        a counter-based stream instead of NumPy's (evo_amd.variational.init_states_counter reproduces it bit for bit for
        ``self.last_init_seed``).  Returns my_suff_stat with init_states' keys, dtypes, assertions and the ``cross`` rule;
        S is the model's.  sync_host=False: K^n stays on the device, "ss" and "lpj" are None (sync_to_host allocates them);
        sync_host=True: "ss" is downloaded once.  ``seed`` None: drawn from np.random (np.random.seed makes runs
        reproducible); rank and world size enter it, so ranks get different streams.  RuntimeError naming the cap when
        a datapoint is not complete after ``max_rounds`` rounds -- shapes with S close to 2 ** H belong to init_states.
        Exact E-steps: S == 2 ** Hv, or S == 2 ** Hv - 1 with the permanent all-zero state (what init_states lays out
        when it is asked for 2 ** Hv states, so the mirror of that case is init_states_counter(N, S + 1, ...), not
        (N, S, ...), which samples); the state table is built on the host and copied to every datapoint."""
        N, H = my_data["y"].shape[0], self.H
        permanent = permanent or {"background": False, "allzero": False, "singletons": False}
        background = bool(permanent["background"])
        Hv = H - 1 if background else H
        S_perm = 0 if background else (1 if (permanent["allzero"] == 1 and permanent["singletons"] == 0) else 0)
        S_arg = self.S + 1 if (S_perm and Hv < 12 and self.S == 2 ** Hv - 1) else self.S
        if Mprime is None:
            Mprime = self.S
        # every key but the two arrays, from the host function itself (no datapoint: no random number is drawn)
        suff = _host_init_states(0, S_arg, H, parent_selection, mutation_algorithm, no_parents, no_children, no_generations,
                                 bitflip_prob, Mprime, p_init_Kn, permanent)
        suff["ss"] = suff["lpj"] = None
        table = None
        if S_arg == 2 ** Hv:
            sm = suff["sm"]
            table = (np.concatenate((sm, np.ones((sm.shape[0], 1), dtype=bool)), axis=1) if background
                     else (sm[1:] if S_perm else sm))
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.last_init_seed = (int(seed) * max(1, self.comm.size) + self.comm.rank) & (2 ** 64 - 1)
        eng = self._prepare(suff, my_data, upload_states=False)
        self._resident = False
        eng.init_states(1.0 / H if p_init_Kn is None else p_init_Kn, self.last_init_seed, max_rounds, table)
        self._resident = True
        if self.sync_host:
            suff["ss"] = eng.download_states()
            suff["lpj"] = np.empty((N, self.S + S_perm))
        return suff

    def seed_resident_states(self, model_params, my_data, parent_selection, mutation_algorithm, no_parents, no_children,
                             no_generations, max_active=None, bitflip_prob=None, Mprime=None, permanent=None,
                             want_path=False, incomplete=False, beam=None):
        """``init_states`` for this rank's ``my_data`` with K^n SEEDED on the device from ``model_params`` and the data
        (Engine.seed_states; evo_amd.variational.seed_states_host is the NumPy mirror): greedy forward selection on the
        model's own lpj, deterministic -- the start for codes, reconstructions, predictive moments or samples from a
        trained Theta, where Bernoulli(1 / H) states would need dozens of E-steps first.  Theta is pushed first.
        ``max_active`` None: min(8, S, H).  Returns my_suff_stat with init_states' keys, dtypes and ``cross`` rule and
        init_resident_states' sync_host behaviour ("ss" / "lpj" None with sync_host=False; with sync_host=True "ss" is
        downloaded once); the lpj rows of the seeded K^n are computed on the device right away (sync_host=True: "lpj"
        holds them), so encode(), predictive_moments() and sample_posterior() can follow without an E-step.
        ``want_path``: self.last_seed_path = (path, lpj_path), else None.  ``incomplete=True`` admits my_data["x_infr"]
        with False entries (inpainting, imputation): the masks go up as for any E-step and every datapoint is seeded on
        its reliable entries alone -- values of y under False, NaN included, never enter.  ValueError for incomplete
        data without ``incomplete=True``, the background unit and a ``max_active`` the law refuses; NotImplementedError
        in the float32 mode.
        ``beam`` None: the greedy law above.  An integer B >= 1: the beam law (Engine.seed_states_beam;
        evo_amd.variational.seed_states_beam_host is its mirror) -- the B best partial states are kept per step and all
        of them expanded, which on correlated dictionaries finds states a single greedy path misses; B = 1 is the greedy
        law bit for bit; self.last_seed_path then holds the path of the last step's best state and the best score of each
        step.  Complete data only: ValueError naming ``beam`` with ``incomplete=True`` or incomplete data, and for a B
        outside [1, min(S // max_active, 16)]."""
        from ..variational.utils import seed_beam_check, seed_quotas
        N, H = my_data["y"].shape[0], self.H
        permanent = permanent or {"background": False, "allzero": False, "singletons": False}
        if permanent["background"]:
            raise ValueError("seed_resident_states: the background unit is not supported")
        if self.dtype == np.float32:
            raise NotImplementedError("seed_resident_states is not available in the float32 mode")
        if beam is not None and (incomplete or not self._complete(my_data)):
            raise ValueError("seed_resident_states: beam is for complete data only (no incomplete=True, no x_infr with "
                             "False entries)")
        if not incomplete and not self._complete(my_data):
            raise ValueError("seed_resident_states: incomplete data (x_infr with False entries) is not supported "
                             "by default: pass incomplete=True")
        if max_active is None:
            max_active = min(8, self.S, H)
        seed_quotas(self.S, H, max_active, self.model_name != "bsc")
        if beam is not None:
            seed_beam_check(self.S, max_active, beam)
        S_perm = 1 if (permanent["allzero"] == 1 and permanent["singletons"] == 0) else 0
        if Mprime is None:
            Mprime = self.S
        # every key but the two arrays, from the host function itself (no datapoint: no random number is drawn)
        suff = _host_init_states(0, self.S, H, parent_selection, mutation_algorithm, no_parents, no_children,
                                 no_generations, bitflip_prob, Mprime, None, permanent)
        suff["ss"] = suff["lpj"] = None
        eng = self._prepare(suff, my_data, upload_states=False)
        # (the precompute stores its derived keys and zeroes the reset counters: on shallow copies here)
        self.E_step_precompute(dict(model_params), dict(suff), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if beam is None:
            self.last_seed_path = eng.seed_states(max_active, want_path=want_path, incomplete=bool(incomplete))
        else:
            self.last_seed_path = eng.seed_states_beam(max_active, beam, want_path=want_path)
        self._resident = True
        eng.lpj_resident()
        if self.sync_host:
            suff["ss"] = eng.download_states()
            suff["lpj"] = eng.download_lpj()
        return suff

    def _prepare(self, my_suff_stat, my_data, upload_states=True):
        """Configure the engine for this rank's shard and make Y / K^n resident."""
        Y = my_data["y"]
        xi = my_data["x_infr"]
        xi_objs = (xi, my_data.get("x"))
        new_masks = not self._same_objects(self._x_infr_token, *xi_objs)
        if new_masks:  # checked once per array object, like the Y upload below
            self._incomplete = not self._complete(my_data)
        yr = my_data.get("y_reconstructed")
        if (isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised
                and (new_masks or not self._same_objects(self._y_token, Y))):
            # the uploads below drop the device copy of an older reconstruction that the M-step may still have to read
            # (bsc.py:186): fetch it first -- the default path holds it as an ndarray and uploads that
            yr.rows()
        reuploaded = False
        N, D = Y.shape
        assert D == self.D
        S_perm = int(my_suff_stat["S_perm"])
        background = bool(my_suff_stat["permanent"]["background"])  # last latent on in every state (utils.py:42-47)
        cmax = self._cmax(my_suff_stat) if "n_parents" in my_suff_stat else 1
        eng = self.engine
        self._background = background  # update_params / the device update pin the unit's prior (bsc.py:259, sssc.py:718)
        if getattr(eng, "_bg_unit", False) != background:  # (only on a change: setting an option drops a prefetched pass)
            eng.set_option("background_unit", 1 if background else 0)
            eng._bg_unit = background
        f32 = self.dtype == np.float32
        if not eng.same_geometry(self.model_name, N, D, self.H, self.S, S_perm, cmax) or eng.f32 != f32:
            eng.set_option("ebsc_f32", 1 if f32 else 0)  # read by configure
            eng.configure(self.model_name, N, D, self.H, self.S, S_perm, cmax)
            eng.f32 = f32
            self._y_token = None
            self._resident = False
        if not self._same_objects(self._y_token, Y):
            eng.upload_data(Y)
            self._y_token = (Y,)
            new_masks = True
        if new_masks:
            reuploaded = True
            if self._incomplete:
                eng.upload_masks(xi, my_data.get("x"))
                self._yrec_token = None
            elif self._had_masks or eng.has_masks:  # this model's own, or another model's on a shared engine
                eng.upload_masks(None)
                eng.upload_data(Y)
            self._had_masks = self._incomplete
            self._x_infr_token = xi_objs
        if self._incomplete and "y_reconstructed" in my_data:
            yr = my_data["y_reconstructed"]
            if not self._same_objects(self._yrec_token, yr):  # an older reconstruction the M-step should read (bsc.py:186)
                current = (isinstance(yr, ResidentReconstruction) and yr.resident and yr.engine is eng
                           and not reuploaded)  # (upload_masks re-allocates the device's y_reconstructed)
                if not current:
                    yr_rows = np.asarray(yr.T if getattr(yr, "transposed", False) else yr)
                    eng.upload_yrec(np.where(np.isnan(yr_rows), 0.0, yr_rows))
                self._yrec_token = (yr,)  # (a current handle: the device holds it already)
        if upload_states and (self.sync_host or not self._resident):
            eng.upload_states(my_suff_stat["ss"])
            self._resident = True
            self._kn_uploads += 1  # the lpj rows on the device no longer belong to this K^n
        return eng

    def _engine_matches(self):
        """True when an engine exists and is configured for this model's (kind, D, H)."""
        e = self._engine
        want = _engine.MODEL_BSC if self.model_name == "bsc" else _engine.MODEL_SSSC
        return e is not None and e.model == want and (e.D, e.H) == (self.D, self.H)

    def sync_to_host(self, my_suff_stat):
        """Copy the device-resident K^n and lpj into the caller's arrays (in place)."""
        my_suff_stat["ss"] = self.engine.download_states(my_suff_stat["ss"])  # (None: allocated -- init_resident_states)
        my_suff_stat["lpj"] = self.engine.download_lpj(my_suff_stat["lpj"])

    # ---- hooks the concrete models provide ---------------------------------------------------
    def _push_params(self, model_params):
        raise NotImplementedError

    def _pull_params(self, dpar):
        """Host copy of the parameters resident on the device + the derived keys of the reference."""
        raise NotImplementedError

    def _scalar_params(self, dpar):
        """The scalar entries of _pull_params(dpar), from the scalar block alone (LazyTheta keeps them current)."""
        raise NotImplementedError

    def E_step_precompute(self, model_params, my_suff_stat, my_data):
        raise NotImplementedError

    def _allzero_lpj(self, model_params, yy):
        raise NotImplementedError

    # ---- reference API -----------------------------------------------------------------------
    def check_params(self, model_params):
        """Clamp Theta into its admissible box on rank 0 and broadcast (_models.py:101-159)."""
        comm = self.comm
        for name, (low, up, absify, low_diag) in self.noise_policy.items():
            v = model_params[name]
            scalar = np.isscalar(v)
            if comm.rank == 0:
                if scalar:
                    if v < low:
                        print("check_params: Reset lower bound of %s" % name)
                        v = low
                    if v >= up:
                        print("check_params: Reset upper bound of %s" % name)
                        v = up
                    if absify:
                        v = np.abs(v)
                    if low_diag is not None and v < low_diag:
                        print("check_params: Reset lower bound of %s (diagonal)" % name)
                        v = low_diag
                else:
                    if (v < low).any():
                        print("check_params: Reset lower bound of %s" % name)
                    if (v >= up).any():
                        print("check_params: Reset upper bound of %s" % name)
                    v = np.minimum(up, np.maximum(low, v))
                    if absify:
                        v = np.abs(v)
                    if low_diag is not None:
                        small = np.diag(v) < low_diag
                        if small.any():
                            print("check_params: Reset lower bound of %s (diagonal)" % name)
                        v[np.diag(small)] = low_diag
            if comm.size > 1:
                v = comm.bcast(v)
            model_params[name] = v
        return model_params

    def _write_reconstruction(self, my_data):
        """my_data["y_reconstructed"] (_models.py:643-665, sssc.py:507,613-627; complete data): a copy of
        y whose entries with my_data["x"] False are the posterior-predictive estimate W E_q[s] (EBSC) /
        W E_q[s o z] (ES3C) under the Theta and K^n of the statistics pass that just ran.
        resident_reconstruction: the same selection on the device, and a handle in place of the array."""
        if self.resident_reconstruction:
            if self._rec_handle is not None:
                self._rec_handle._outdate("a later reconstruction (step / E_step / reconstruct) of the same model")
            serial = self.engine.reconstruct_resident(my_data["x"])
            self._rec_handle = ResidentReconstruction(self.engine, serial, my_data["y"], my_data["x"],
                                                      my_data["x_infr"] if self._incomplete else None)
            my_data["y_reconstructed"] = self._rec_handle
            return
        y_hat = self.engine.reconstruct()
        y_rec = my_data["y"].copy()
        miss = np.logical_not(my_data["x"])
        if self._incomplete:  # datapoints without a single reliable entry are skipped (_models.py:648-649)
            miss &= my_data["x_infr"].any(axis=1)[:, None]
        y_rec[miss] = y_hat[miss]
        my_data["y_reconstructed"] = y_rec

    def _step_device(self, model_params, my_suff_stat, my_data, do_reconstruction=False):
        """EM iteration with the M-step on the device (device_mstep=True)."""
        if self.comm.size > 1 and not getattr(self.comm, "device_reduces", False):
            raise ValueError("device_mstep with several ranks needs an RcclComm (device-side all-reduce)")
        eng = self._prepare(my_suff_stat, my_data)
        if model_params is not self._dev_theta:  # new host Theta: clamp, precompute, upload
            model_params = self.check_params(model_params)
            self.E_step_precompute(model_params, my_suff_stat, my_data)
        self._estep_kernels(eng, model_params, my_suff_stat, my_data)
        self._n_steps += 1
        if self._incomplete and do_reconstruction:
            # y_reconstructed feeds this very M-step's Wp (bsc.py:184-189,211): formed inside the statistics pass
            eng.set_option("reconstruct_in_stats", 1)
        lazy = self.lazy_theta and len(self.to_learn) > 0
        try:
            tail, dpar = eng.mstep_device(self.to_learn, reconstruct=do_reconstruction, theta_to_host=not lazy)
        except _engine.SingularUpdate as e:
            return self._step_device_singular(model_params, my_suff_stat, my_data, do_reconstruction, e.tail, e.dpar)
        if do_reconstruction:
            self._write_reconstruction(my_data)
            if self._incomplete:
                self._yrec_token = (my_data["y_reconstructed"],)  # the device already holds it
        if self.sync_host:
            self.sync_to_host(my_suff_stat)
        my_suff_stat["reset_lpj_isnan"] = int(tail["reset_isnan"])
        my_suff_stat["reset_lpj_smaller_eps_lpj"] = int(tail["reset_smaller_eps"])
        my_suff_stat["reset_lpj_isinf"] = int(tail["reset_isinf"])
        self.last_dpar = dpar
        if lazy:
            scalars = self._scalar_params(dpar)
            loader = (lambda: self._pull_params(self.last_dpar))
            if isinstance(model_params, LazyTheta):
                model_params._stale(scalars, loader)
            else:
                model_params = LazyTheta(scalars, loader)
        else:
            model_params.update(self._pull_params(dpar))
        self._dev_theta = model_params
        self.last_dpar = dpar  # scalar block of the update (engine.Engine.DPAR): n_gt2 / n_gt4 / n_gt8 = overflow census of K^n
        N = tail["N"]
        return dpar["ljc_estep"] + tail["Fs"] / N, tail["sum_nunique"] / N, tail["sum_sub"] / N, model_params

    def _step_device_singular(self, model_params, my_suff_stat, my_data, do_reconstruction, tail, dpar):
        """The device Theta update met an exactly singular H x H system (a latent that never occurs in any
        K^n, N < H ...).  The reference absorbs that case (lstsq / pinv + noise, bsc.py:236-250,
        sssc.py:692-708); so does this path: the E-step results of the failed call stand (``tail``: F term,
        counters); the Theta the E-step ran with -- the host still holds it in ``model_params`` -- goes back
        to the device (the failed update overwrote it), the statistics are summed again from the unchanged
        K^n / lpj, and the reference's host formulas, fallbacks and np.random draws included, give Theta^new."""
        eng = self.engine
        if isinstance(model_params, LazyTheta) and not model_params.materialised:
            # lazy Theta: the host holds no copy of the Theta the E-step ran with, and the loader would download what
            # the failed update left behind.  The library kept the old parameters on the device: bring THOSE back.
            eng.restore_theta_backup()
            model_params._loader = None
            dict.update(model_params, self._pull_params(dpar))  # (E_step_precompute below rewrites the derived keys)
        self.E_step_precompute(model_params, my_suff_stat, my_data)
        if self._incomplete and do_reconstruction:
            eng.set_option("reconstruct_in_stats", 1)
        acc = eng.stats()
        v = dict(eng.acc_views(acc))
        for k in ("Fs", "sum_nunique", "sum_sub", "N", "reset_isnan", "reset_smaller_eps", "reset_isinf"):
            v[k] = tail[k]  # set_params cleared the device-side E-step scalars; the failed call delivered them
        if do_reconstruction:
            self._write_reconstruction(my_data)
            if self._incomplete:
                self._yrec_token = (my_data["y_reconstructed"],)
        if self.sync_host:
            self.sync_to_host(my_suff_stat)
        my_suff_stat["reset_lpj_isnan"] = int(v["reset_isnan"])
        my_suff_stat["reset_lpj_smaller_eps_lpj"] = int(v["reset_smaller_eps"])
        my_suff_stat["reset_lpj_isinf"] = int(v["reset_isinf"])
        N = float(v["N"])
        F = dpar["ljc_estep"] + float(v["Fs"]) / N
        with small_blas(self.H):
            model_params = self.update_params(model_params, v, N)
        self._dev_theta = None  # the next step clamps, precomputes and uploads this host Theta
        return F, float(v["sum_nunique"]) / N, float(v["sum_sub"]) / N, model_params

    def step(self, model_params, my_suff_stat, my_data, do_reconstruction=False):
        """One EM iteration (_models.py:161-203): check_params -> E_step -> M_step."""
        if self.device_mstep:
            return self._step_device(model_params, my_suff_stat, my_data, do_reconstruction)
        model_params = self.check_params(model_params)
        F, S_nunique, S_sub = self.E_step(model_params, my_suff_stat, my_data, _keep_acc=True,
                                          _reconstruct=do_reconstruction)
        if do_reconstruction and not self._incomplete:  # _models.py:193-194: after the E-step, with the Theta it used
            self._write_reconstruction(my_data)
        new_params = (self.M_step(model_params, my_suff_stat, my_data, _from_step=True)
                      if len(self.to_learn) > 0 else model_params)
        self._acc = None
        return F, S_nunique, S_sub, new_params

    def _data_moments(self, my_data):
        """Data mean and mean squared deviation over all ranks (_models.py:240-255, complete data)."""
        Y = my_data["y"]
        N = self.comm.allreduce(Y.shape[0])
        y_mean = _reduce_array(self.comm, np.sum(Y, 0)) / N
        var = _reduce_array(self.comm, np.sum((Y - y_mean) ** 2, 0)) / N
        return y_mean, var, N

    def standard_init(self, my_data, W_init=None, pi_init=None, sigma_init=None):
        """Theta^init for BSC (_models.py:205-283): W = data mean + N(0,(sigma/4)^2) unless given,
        pi = 1/H, sigma = sqrt(mean data variance).  RNG calls as in the reference."""
        D, H = self.D, self.H
        xi = my_data["x_infr"]
        if xi.all():
            y_mean, var, _ = self._data_moments(my_data)
            if sigma_init is None:
                sigma_init = np.sqrt(var.sum() / D)
        else:
            # _models.py:246-267: sums over the reliable entries; the mean divides by my_N (per rank)
            Y = np.where(xi, my_data["y"], 0.0)
            y_mean = self.comm.allreduce(Y.sum(axis=0) / Y.shape[0])
            if sigma_init is None:
                tmp = (np.where(xi, Y - y_mean, 0.0) ** 2).sum(axis=0)
                sigma_init = np.sqrt(self.comm.allreduce(tmp.sum() / xi.sum()))
        assert sigma_init > 0.0
        if type(W_init) is not np.ndarray:
            if W_init == "random_uniform":
                W_init = self.comm.bcast(np.random.random((D, H)))
            elif W_init == "normal":
                W_init = self.comm.bcast(np.random.normal(0, 5, [D, H]))
            elif W_init == "data_mean":
                W_init = np.tile(y_mean[:, None], (1, H))
            else:
                W_init = y_mean[:, None] + self.comm.bcast(np.random.normal(scale=sigma_init / 4.0, size=[D, H]))
        return {"W": W_init, "pi": 1.0 / H if pi_init is None else pi_init, "sigma": sigma_init}

    def generate_data(self, model_params, my_N):
        """s ~ Bernoulli(pi) then generate_from_hidden (_models.py:73-99)."""
        H_gen = model_params["W"].shape[1]
        pies = model_params["pies"] if "pies" in model_params else model_params["pi"]
        s = np.random.random(size=(my_N, H_gen)) <= pies
        return self.generate_from_hidden(model_params, {"s": s})

    def generate_data_device(self, model_params, my_N, seed=None, first_index=0, my_hdata=None,
                             keep=("y", "s", "z", "y_mean")):
        """``generate_data`` on the device (Engine.generate): the same law, a counter-based stream instead of NumPy's
        (evo_amd.models.generate_counter reproduces it for ``self.last_generate_seed``: "s" bit for bit, the real-valued
        outputs to ~1e-13), no loop over the datapoints.  Returns generate_data's dict -- "y", "s" (bool), "y_mean" and, ES3C,
        "z" -- without the keys that ``keep`` does not name.  ``my_hdata={"s": ...}``: the generate_from_hidden form, s is
        taken, not drawn.  Datapoint n is index ``first_index + n`` of the data set, so shards of one seed concatenate to
        the set of a single call.  ``seed`` None: drawn from np.random; rank and world size enter it as in
        init_resident_states.  BSC reads "pi" and "sigma", ES3C "pies", "mus", "Psi" and "sigma2"; ES3C's z is
        s o (mus + F eps) with F F^T = Psi from one eigh per call, which has the reference's law N(mus_A, Psi_AA) on every
        active set and also serves a singular Psi.  Needs no configured engine and leaves a resident run untouched."""
        from .generate import generate_params
        keep = tuple(keep)
        known = ("y", "s", "y_mean") + (("z",) if self.model_name == "sssc" else ())
        for name in keep:
            if name not in ("y", "s", "z", "y_mean"):
                raise ValueError("keep: unknown output %r" % (name,))
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.last_generate_seed = (int(seed) * max(1, self.comm.size) + self.comm.rank) & (2 ** 64 - 1)
        par = generate_params(self.model_name, model_params)
        s = None if my_hdata is None else np.asarray(my_hdata["s"], dtype=np.bool_)
        wanted = [name for name in known if name in keep]
        eng = self.engine
        eng.generate(self.model_name, my_N, self.last_generate_seed, par["Wt"], par["pies"], par["mus"], par["F"],
                     par["sigma"], first_index=first_index, s=s, keep=wanted)
        return {name: eng.download_generated(name) for name in wanted}

    def lpj_reset_check(self, lpj, my_suff_stat):
        """Host mirror of the clamp the kernels apply (_models.py:567-596); used for the permanent
        all-zero column evaluated on the host in free_energy(full=True)."""
        nan_m, low_m, inf_m = np.isnan(lpj), lpj < self.eps_lpj, np.isinf(lpj)
        for key, m in (("reset_lpj_isnan", nan_m), ("reset_lpj_smaller_eps_lpj", low_m), ("reset_lpj_isinf", inf_m)):
            if m.any():
                my_suff_stat[key] = my_suff_stat.get(key, 0) + 1
                break
        lpj[nan_m] = self.eps_lpj
        lpj[low_m] = self.eps_lpj
        lpj[inf_m] = self.B_max
        return lpj

    def log_pseudo_joint(self, model_params, my_suff_stat, my_data):
        """Per-datapoint operator with the reference's calling shape (bsc.py:78-97, sssc.py:241-326):
        reads my_data["this_y"], my_suff_stat["this_states"]; returns lpj (C,).  One small launch
        per call -- for parity tests and multi-generation EA, not for throughput.
        E_step_precompute must have been called with the same ``model_params`` (as in the reference,
        which reads the derived keys it stores)."""
        eng = self.engine
        if not self._engine_matches():
            eng.set_option("ebsc_f32", 0)
            eng.f32 = False
            eng.configure(self.model_name, 1, self.D, self.H, self.S, 0, 1)
            self._y_token = None
            self._resident = False
            self._push_params(model_params)
        states = np.ascontiguousarray(my_suff_stat["this_states"], dtype=bool)
        xi = my_data.get("this_x_infr")
        masked = xi is not None and not np.all(xi)
        this_y = my_data["this_y"]
        out, flags = eng.lpj_single(np.where(xi, this_y, 0.0) if masked else this_y, states, xi if masked else None)
        for key, f in zip(("reset_lpj_isnan", "reset_lpj_smaller_eps_lpj", "reset_lpj_isinf"), flags):
            if f:
                my_suff_stat[key] = my_suff_stat.get(key, 0) + 1
                break
        return out

    def log_pseudo_joint_permanent_states(self, model_params, my_suff_stat, my_data):
        """All-zero permanent state (bsc.py:59-76, sssc.py:224-239)."""
        lpj = np.empty((my_suff_stat["S_perm"],))
        if my_suff_stat["permanent"]["allzero"]:
            xi = my_data.get("this_x_infr")
            y_obs = my_data["this_y"] if xi is None else my_data["this_y"][xi]
            lpj[0] = self._allzero_lpj(model_params, (y_obs ** 2).sum())
        return self.lpj_reset_check(lpj, my_suff_stat)

    # ---- E-step --------------------------------------------------------------------------------
    def _candidates_reference(self, eng, model_params, my_suff_stat, my_data):
        """Host candidate generation in the reference's np.random order, evaluation on the GPU."""
        ss = my_suff_stat["ss"]
        N, S, H = ss.shape
        S_perm = my_suff_stat["S_perm"]
        cmax = eng.Cmax
        cand = np.zeros((N, cmax, H), dtype=bool)
        counts = np.zeros(N, dtype=np.int32)
        lpj_cur = eng.download_lpj()
        if my_suff_stat["n_generations"] == 1:
            for n in range(N):
                new = eas.first_generation_candidates(ss[n], lpj_cur[n, S_perm:], my_suff_stat, model_params["piH"])
                counts[n] = new.shape[0]
                cand[n, :new.shape[0]] = new
            eng.lpj_candidates(cand, counts, want_lpj=False)
            return
        # several generations: generation g+1 needs lpj of generation g before the next datapoint's
        # random numbers are drawn, so evaluate per datapoint to keep the stream exact
        cand_lpj = np.zeros((N, cmax))
        Y = my_data["y"]
        for n in range(N):
            my_data["this_y"] = Y[n]
            my_data["this_x_infr"] = my_data["x_infr"][n]
            my_suff_stat["this_states"] = ss[n]
            my_suff_stat["this_lpj"] = lpj_cur[n, S_perm:]

            def eval_lpj(states):
                my_suff_stat["this_states"] = states
                return self.log_pseudo_joint(model_params, my_suff_stat, my_data)

            new, new_lpj = eas.evolve_states(my_suff_stat, model_params, eval_lpj)
            counts[n] = new.shape[0]
            cand[n, :new.shape[0]] = new
            cand_lpj[n, :new.shape[0]] = new_lpj
        eng.set_candidates(cand, counts, cand_lpj)

    _MUTATION_NAMES = {eas.randflip: "randflip", eas.sparseflip: "sparseflip", eas.cross: "cross",
                       eas.cross_randflip: "cross_randflip", eas.cross_sparseflip: "cross_sparseflip"}

    def _device_seed(self):
        return (self.seed * 1000003 + self._n_steps) * max(1, self.comm.size) + self.comm.rank

    def _estep_kernels(self, eng, model_params, my_suff_stat, my_data):
        """The body of the reference's per-datapoint E-step loop (_models.py:497-538 / sssc.py:510-552) for all datapoints
        of this rank: lpj of K^n -> evolve_states -> lpj of the new states -> vary_Kn.  rng="device" with the examples'
        EA (randflip, one generation) is ONE library call, which runs the fused wave-per-datapoint kernel where the shape
        allows it (csrc/kernels_fused.hpp) and the separate passes otherwise -- same K^n, same lpj bits."""
        mut = my_suff_stat.get("mutation_algorithm")
        if (self.rng == "device" and mut is eas.randflip and my_suff_stat["n_generations"] == 1
                and my_suff_stat["n_children"] <= 8 and my_suff_stat["parent_selection"] in (eas.fitparents, eas.randparents)):
            n_par = min(my_suff_stat["n_parents"], self.S)
            self.last_estep_fused = eng.estep(n_par, my_suff_stat["n_children"], self._device_seed(),
                                              my_suff_stat["parent_selection"] is eas.fitparents, my_suff_stat["Mprime"])
            return
        self.last_estep_fused = False
        eng.lpj_resident()
        if self.rng == "reference":
            self._candidates_reference(eng, model_params, my_suff_stat, my_data)
        else:
            self._candidates_device(eng, my_suff_stat, model_params)
        eng.vary_kn(my_suff_stat["Mprime"], want_sums=False)

    def _candidates_device(self, eng, my_suff_stat, model_params):
        """evolve_states (eas.py:153-313) on the device, every operator and any number of generations."""
        mut = my_suff_stat["mutation_algorithm"]
        if mut not in self._MUTATION_NAMES:
            raise NotImplementedError("rng='device' knows the reference's five mutation operators; got %r" % (mut,))
        fit = my_suff_stat["parent_selection"] is eas.fitparents
        if not fit and my_suff_stat["parent_selection"] is not eas.randparents:
            raise NotImplementedError("rng='device' knows fitparents and randparents")
        seed = self._device_seed()
        n_par = min(my_suff_stat["n_parents"], self.S)
        if mut is eas.randflip and my_suff_stat["n_generations"] == 1 and my_suff_stat["n_children"] <= 8:
            eng.evolve_randflip(n_par, my_suff_stat["n_children"], seed, fit)  # the examples' default: fast path
        else:
            eng.evolve_states(self._MUTATION_NAMES[mut], n_par, my_suff_stat["n_children"], my_suff_stat["n_generations"],
                              seed, fit, float(model_params["piH"]), my_suff_stat["bitflip_prob"])

    def E_step(self, model_params, my_suff_stat, my_data, _keep_acc=False, _reconstruct=False):
        """New variational states, their lpj, K^n update and the free energy (_models.py:453-565).
        Returns (F, S_nunique, S_sub).  my_suff_stat["ss"] / ["lpj"] are updated in place when
        ``sync_host`` (always in rng="reference" mode)."""
        eng = self._prepare(my_suff_stat, my_data)
        self.E_step_precompute(model_params, my_suff_stat, my_data)
        self._estep_kernels(eng, model_params, my_suff_stat, my_data)
        self._n_steps += 1
        if self._incomplete and _reconstruct:
            # incomplete data: y_reconstructed feeds this very M-step's Wp (bsc.py:184-189,211), so the
            # statistics pass forms it between the Es rows and the contraction
            eng.set_option("reconstruct_in_stats", 1)
        acc = eng.stats()
        if self._incomplete and _reconstruct:
            self._write_reconstruction(my_data)
            self._yrec_token = (my_data["y_reconstructed"],)  # the device already holds it
        if not getattr(self.comm, "device_reduces", False):
            acc = _reduce_array(self.comm, acc)
        v = eng.acc_views(acc)
        if self.sync_host:
            self.sync_to_host(my_suff_stat)
        my_suff_stat["reset_lpj_isnan"] = int(v["reset_isnan"])
        my_suff_stat["reset_lpj_smaller_eps_lpj"] = int(v["reset_smaller_eps"])
        my_suff_stat["reset_lpj_isinf"] = int(v["reset_isinf"])
        self._acc = acc if _keep_acc else None
        self.last_acc = acc  # the globally summed packed accumulator of this E-step (engine.acc_views names its blocks)
        N = float(v["N"])
        F = model_params["ljc"] + float(v["Fs"]) / N
        return F, float(v["sum_nunique"]) / N, float(v["sum_sub"]) / N

    def refine_resident_states(self, model_params, my_suff_stat, my_data, n_iterations, patience=None, min_sub=0.0,
                               check_every=8):
        """``n_iterations`` E-steps on K^n while ``model_params`` stays fixed -- the step between seed_resident_states (or a
        trained model meeting new data) and encode / predictive_moments / sample_posterior / posterior_scores -- in ONE
        library call (Engine.refine_states): K^n is evaluated once, then every iteration is children, their lpj and
        selection; no statistics pass, no host wait in between.  The EA is my_suff_stat's, the seeds are those of
        ``n_iterations`` successive E_step calls (same K^n as those, bit for bit), and ``self._n_steps`` advances by
        ``n_iterations`` on every rank whatever was run.  ``patience`` (None: run them all): after every ``check_every``
        iterations the loop ends once the last ``patience`` iterations all swapped at most ``min_sub`` states per
        datapoint of this rank.  Returns a RefineResult: ``F`` (n_done,) = ljc + allreduce(Fs_t) / N after iteration t,
        ``S_nunique`` and ``S_sub`` (n_done,) normalised like E_step's, ``n_done`` and ``stopped_early``.  The loop involves
        no collective: with several ranks each stops on its own (``n_done_local``), and a rank that stopped before the
        longest one enters the sums with its last Fs and zero counts.  sync_host=True: "ss" and "lpj" are downloaded
        once at the end, in place; sync_host=False: only the trace crosses to the host.  The reset counters of
        my_suff_stat stay as they are.  ValueError with rng="reference" (candidates come from the host there);
        NotImplementedError as in E_step for an EA the device does not know."""
        if self.rng == "reference":
            raise ValueError("refine_resident_states needs rng='device': with rng='reference' candidates come from the host")
        T = int(n_iterations)
        if T < 1:
            raise ValueError("refine_resident_states: n_iterations must be positive")
        mut = my_suff_stat["mutation_algorithm"]
        if mut not in self._MUTATION_NAMES:
            raise NotImplementedError("rng='device' knows the reference's five mutation operators; got %r" % (mut,))
        fit = my_suff_stat["parent_selection"] is eas.fitparents
        if not fit and my_suff_stat["parent_selection"] is not eas.randparents:
            raise NotImplementedError("rng='device' knows fitparents and randparents")
        eng = self._prepare(my_suff_stat, my_data)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        seed0, stride = self._device_seed(), max(1, self.comm.size)
        self._n_steps += T
        trace, n_local = eng.refine_states(
            T, self._MUTATION_NAMES[mut], min(my_suff_stat["n_parents"], self.S), my_suff_stat["n_children"],
            my_suff_stat["n_generations"], seed0, stride, fit, float(theta["piH"]), my_suff_stat["bitflip_prob"],
            my_suff_stat["Mprime"], check_every=check_every, patience=0 if patience is None else int(patience),
            min_sub=min_sub)
        # rows of all T iterations: {Fs, new unique, swapped, this rank still ran}; past this rank's end its last Fs
        rows = np.zeros((T, 4))
        rows[:n_local, :3] = trace
        rows[:n_local, 3] = 1.0
        rows[n_local:, 0] = trace[-1, 0]
        rows = _reduce_array(self.comm, rows)
        N = float(self.comm.allreduce(my_data["y"].shape[0]))
        n_done = int(np.count_nonzero(rows[:, 3] > 0.0))
        if self.sync_host:
            self.sync_to_host(my_suff_stat)
        return RefineResult(theta["ljc"] + rows[:n_done, 0] / N, rows[:n_done, 1] / N, rows[:n_done, 2] / N, n_done,
                            n_local, n_done < T)

    def sweep_resident_states(self, model_params, my_suff_stat, my_data, n_sweeps=4, n_parents=1, n_keep=None,
                              stop_when_quiet=True, incomplete=False, neighbourhood="flip"):
        """Local search on K^n while ``model_params`` stays fixed (Engine.sweep_states; csrc/kernels_sweep.hpp has the law,
        evo_amd.variational.sweep_states_host is the NumPy mirror): per sweep every one-flip neighbour of the
        ``n_parents`` best states of each datapoint is scored in the Gram form of the seeding kernel, the ``n_keep`` best
        per parent that K^n does not hold (None: Cmax // n_parents) are evaluated by the model's lpj kernels and go through
        the usual selection.  Deterministic: nothing is drawn, so neither rng="device" nor a known EA is needed and
        ``self._n_steps`` stays.  ``stop_when_quiet``: a rank's loop ends after a sweep that swapped nothing; then
        ``gain`` <= 0 certifies per datapoint that the best state of K^n has no better one-flip neighbour outside K^n.
        Returns a SweepResult: ``F`` (n_done,) = ljc + allreduce(Fs_t) / N after sweep t, ``S_nunique`` and ``S_sub``
        normalised like E_step's, ``n_done``, ``stopped_early`` and this rank's ``gain``, ``best_flip``, ``n_capped`` of its
        last sweep.  The loop involves no collective: ranks stop on their own and enter the sums as in
        refine_resident_states.  sync_host as there.  ``incomplete=True`` admits my_data["x_infr"] with False entries
        (inpainting, imputation): the masks go up as for any E-step and every neighbour is scored on the datapoint's
        reliable entries alone -- values of y under False, NaN included, never enter.  ValueError for the background
        unit and for incomplete data without ``incomplete=True``; NotImplementedError in the float32 mode.
        ``neighbourhood``: "flip" (the above), "swap" or "both" (csrc/kernels_sweep_swap.hpp has the law,
        evo_amd.variational.swap_states_host is the mirror): the swaps of a parent -- one active latent off, one inactive
        latent on, the move that one-flip search cannot make without a loss in between -- are scored too and the
        ``n_keep`` best per parent that K^n does not hold follow the flip rows (``n_keep`` None with "both": Cmax //
        (2 n_parents)).  The result gains ``swap_gain``, ``best_swap`` and ``n_capped_swap``; after a quiet sweep with
        "both", ``gain`` <= 0 and ``swap_gain`` <= 0 certify that the best state has no better one-flip or swap neighbour
        outside K^n.  Swaps on incomplete data are not supported: ValueError for ``incomplete=True`` with a swap
        ``neighbourhood``."""
        T = int(n_sweeps)
        if neighbourhood not in ("flip", "swap", "both"):
            raise ValueError("sweep_resident_states: neighbourhood = %r must be one of 'flip', 'swap', 'both'" % (neighbourhood,))
        if incomplete and neighbourhood != "flip":
            raise ValueError("sweep_resident_states: incomplete=True with neighbourhood=%r: swaps on incomplete data are not "
                             "supported" % (neighbourhood,))
        if T < 1:
            raise ValueError("sweep_resident_states: n_sweeps must be positive")
        if my_suff_stat["permanent"]["background"]:
            raise ValueError("sweep_resident_states: the background unit is not supported")
        if self.dtype == np.float32:
            raise NotImplementedError("sweep_resident_states is not available in the float32 mode")
        if not incomplete and not self._complete(my_data):
            raise ValueError("sweep_resident_states: incomplete data (x_infr with False entries) is not supported "
                             "by default: pass incomplete=True")
        eng = self._prepare(my_suff_stat, my_data)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        P = int(n_parents)
        if neighbourhood == "flip":
            trace, n_local, cert = eng.sweep_states(T, P, eng.Cmax // max(P, 1) if n_keep is None else int(n_keep),
                                                    my_suff_stat["Mprime"], stop_when_quiet=stop_when_quiet,
                                                    incomplete=bool(incomplete))
        else:
            trace, n_local, cert = eng.sweep_states(T, P, None if n_keep is None else int(n_keep), my_suff_stat["Mprime"],
                                                    stop_when_quiet=stop_when_quiet, neighbourhood=neighbourhood)
        # rows of all T sweeps: {Fs, new unique, swapped, this rank still ran}; past this rank's end its last Fs
        rows = np.zeros((T, 4))
        rows[:n_local, :3] = trace
        rows[:n_local, 3] = 1.0
        rows[n_local:, 0] = trace[-1, 0]
        rows = _reduce_array(self.comm, rows)
        N = float(self.comm.allreduce(my_data["y"].shape[0]))
        n_done = int(np.count_nonzero(rows[:, 3] > 0.0))
        if self.sync_host:
            self.sync_to_host(my_suff_stat)
        return SweepResult(theta["ljc"] + rows[:n_done, 0] / N, rows[:n_done, 1] / N, rows[:n_done, 2] / N, n_done,
                           n_local, n_done < T, cert["gain"], cert["best_flip"], cert["n_capped"], cert.get("swap_gain"),
                           cert.get("best_swap"), cert.get("n_capped_swap"))

    def posterior_scores(self, model_params, my_suff_stat, my_data):
        """Per-datapoint scores of this rank's data under ``model_params`` and the caller's K^n / lpj: a dict with the
        (N_loc,) arrays "F" = logsumexp_s lpj_ns (``model_params["ljc"] + F.mean()`` is the rank's free energy; the
        counterpart over K^n of exact_log_likelihood's ll), "entropy" of q_n, "n_eff" = exp(entropy) (the effective
        number of states), "best" (the column of lpj with the row's maximum, the first of equal ones), "k_best" (active
        latents of that state) and "k_mean" = E_q[|s|].  For held-out data and outlier search: a low F_n is a datapoint
        the model explains badly.  One small kernel over the rows on the device (Engine.posterior_scores;
        evo_amd.variational.posterior_scores_host is the NumPy mirror): no pass, no communication, nothing written into
        the three dicts, works with sync_host=False."""
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        out = eng.posterior_scores()
        out["n_eff"] = np.exp(out["entropy"])
        return out

    def _clone_kwargs(self):
        """The constructor arguments, beside (D, H, S), of a model like this one on the same engine."""
        return dict(to_learn=list(self.to_learn), comm=self.comm, rng=self.rng, sync_host=self.sync_host,
                    engine=self.engine, seed=self.seed, device_mstep=self.device_mstep, dtype=self.dtype,
                    lazy_theta=self.lazy_theta, resident_reconstruction=self.resident_reconstruction)

    def remap_latents(self, model_params, my_suff_stat, my_data, index, **new_columns):
        """Resize the dictionary: prune, reorder or grow the latents of a trained model and carry K^n along on the device.
        ``index`` int (H',): entry h' names the source latent that becomes latent h', or -1 for a NEW latent, off in every
        state (evo_amd.variational.prune_index builds one from latent_usage()); with permanent["background"] the last
        entry must be H - 1.  K^n is gathered to the new numbering there (Engine.remap_latents;
        evo_amd.variational.remap_states_host is the NumPy mirror, bit for bit): states that differed only in dropped
        latents collapse, the first stays in its slot and the others are replaced by unused singletons and pairs, so every
        datapoint keeps S distinct states.  Requires Hv' (Hv' + 1) / 2 >= S.  Theta goes through
        evo_amd.models.remap_theta(model_name, model_params, index, **new_columns) (W_new, pies_new, mus_new,
        Psi_diag_new, rng).  Returns (new_model, new_theta, new_suff, info): ``new_model`` is type(self)(D, H', S, ...) with
        this model's settings ON THE SAME ENGINE, prepared (configure, data, masks) with the remapped K^n resident and its
        lpj rows under ``new_theta`` computed, so encode, posterior_scores, refine_resident_states or step can follow at
        once; ``new_suff`` has my_suff_stat's keys re-derived for H' ("ss" / "lpj" None with sync_host=False, downloaded
        once with sync_host=True); ``info`` = {"n_replaced" (N,), "sum_replaced", "index"}.  This model is invalidated
        (its K^n is gone from the device; it uploads again when used).  sync_host=True (or a K^n that is not resident)
        uploads my_suff_stat["ss"] first.  ValueError before the device is touched for an index the law refuses; in the
        float32 mode configure's own H % 4 rule applies to H'.  Several ranks: each remaps its shard, no collective."""
        from ..variational.utils import check_remap_index
        from .remap import remap_theta
        permanent = my_suff_stat["permanent"]
        background = bool(permanent["background"])
        idx = check_remap_index(index, self.H, self.S, background)
        H2 = int(idx.size)
        new_theta = remap_theta(self.model_name, model_params, idx, **new_columns)
        if not self.sync_host and not self._resident and my_suff_stat.get("ss") is None:
            raise ValueError("remap_latents: K^n is neither resident on the device nor in my_suff_stat['ss']")
        eng = self._prepare(my_suff_stat, my_data)
        n_replaced, total = eng.remap_latents(idx)
        new_model = type(self)(self.D, H2, self.S, **self._clone_kwargs())
        new_suff = dict(my_suff_stat)
        derived = _host_init_states(0, self.S, H2, "fit", "randflip", 1, 1, 1, None, None, None, permanent)
        for key in ("incl", "sm", "S_perm"):
            new_suff[key] = derived[key]
        new_suff["ss"] = new_suff["lpj"] = None
        self.invalidate()  # from here on the engine belongs to the new geometry
        neng = new_model._prepare(new_suff, my_data, upload_states=False)
        neng.adopt_remapped_states()
        new_model._resident = True
        new_theta = new_model.check_params(new_theta)
        new_model.E_step_precompute(new_theta, new_suff, my_data)
        neng.lpj_resident()
        if self.sync_host:
            new_suff["ss"] = neng.download_states()
            new_suff["lpj"] = neng.download_lpj()
        return new_model, new_theta, new_suff, {"n_replaced": n_replaced, "sum_replaced": total, "index": idx}

    def resize_states(self, model_params, my_suff_stat, my_data, S_new):
        """Change S, the number of states per datapoint, and carry K^n along on the device (Engine.resize_states;
        csrc/kernels_resize.hpp has the law, evo_amd.variational.resize_states_host is the NumPy mirror, bit for bit).
        Per datapoint, with the slots ranked by their lpj (descending, ties by ascending slot; NaN and +-inf as -inf): a
        SHRINK keeps the ``S_new`` best states in ascending old slot; a GROW keeps every state in place and fills the new
        slots with the one-flip neighbours of the best state in ascending latent, then its two-flip neighbours, skipping
        the empty state and states the datapoint holds (requires Hv (Hv + 1) / 2 - 1 >= S_new).  The rows that rank are
        the caller's: my_suff_stat["lpj"] where K^n is uploaded (sync_host=True, or a K^n that was not resident; None
        there: computed under ``model_params``), else the resident rows of the last E-step, seed or refine.  Returns
        (new_model, new_suff, info): ``new_model`` is type(self)(D, H, S_new, ...) with this model's settings ON THE SAME
        ENGINE, prepared (configure, data, masks) with the resized K^n resident and its lpj rows recomputed under
        ``model_params``, so encode, posterior_scores, sweep_resident_states, refine_resident_states or step can follow
        at once; ``new_suff`` has my_suff_stat's keys re-derived for S_new ("ss" / "lpj" None with sync_host=False,
        downloaded once with sync_host=True; an "Mprime" above S_new becomes S_new); ``info`` = {"src_slot" int32 (N,
        S_new): the old slot of every new slot, -1 for a fill, "F_before", "F_after" (N,): posterior_scores' F per
        datapoint on either side}.  This model is invalidated (its K^n is gone from the device; it uploads again when
        used).  What remap_latents admits -- the background unit, incomplete data, S_perm 0 / 1 -- is admitted here;
        the float32 mode is not: NotImplementedError (its rows rank in float32, where ties differ from the mirror's).
        ValueError before the device is touched for a size the law refuses.  Several ranks: each resizes its shard, no
        collective."""
        from ..variational.utils import check_resize
        permanent = my_suff_stat["permanent"]
        S2 = check_resize(self.S, S_new, self.H, bool(permanent["background"]))
        if self.dtype == np.float32:
            raise NotImplementedError("resize_states is not available in the float32 mode")
        if not self.sync_host and not self._resident and my_suff_stat.get("ss") is None:
            raise ValueError("resize_states: K^n is neither resident on the device nor in my_suff_stat['ss']")
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if self.sync_host or self._kn_uploads != uploads:
            if my_suff_stat.get("lpj") is None:
                eng.lpj_resident()
            else:
                eng.upload_lpj(my_suff_stat["lpj"])
        F_before = eng.posterior_scores()["F"]
        src_slot = eng.resize_states(S2)
        new_model = type(self)(self.D, self.H, S2, **self._clone_kwargs())
        new_suff = dict(my_suff_stat)
        derived = _host_init_states(0, S2, self.H, "fit", "randflip", 1, 1, 1, None, None, None, permanent)
        for key in ("incl", "sm", "S_perm"):
            new_suff[key] = derived[key]
        if new_suff.get("Mprime") is not None:
            new_suff["Mprime"] = min(int(new_suff["Mprime"]), S2)
        new_suff["ss"] = new_suff["lpj"] = None
        self.invalidate()  # from here on the engine belongs to the new geometry
        neng = new_model._prepare(new_suff, my_data, upload_states=False)
        neng.adopt_resized_states()
        new_model._resident = True
        new_model.E_step_precompute(dict(model_params), dict(new_suff), my_data)
        neng.lpj_resident()
        F_after = neng.posterior_scores()["F"]
        if self.sync_host:
            new_suff["ss"] = neng.download_states()
            new_suff["lpj"] = neng.download_lpj()
        return new_model, new_suff, {"src_slot": src_slot, "F_before": F_before, "F_after": F_after}

    def latent_usage(self, model_params, my_suff_stat, my_data):
        """Which latents the data use, over all ranks: {"usage": (H,) = sum_n E_q[s_h] / N -- the column sums one
        statistics pass leaves in its accumulator, all-reduced like it --, "map_count": int64 (H,) = datapoints whose most
        probable state of K^n (the first column of maximal lpj) has latent h on (Engine.latent_map_counts), "N"}.
        evo_amd.variational.latent_usage_host is the NumPy mirror; prune_index turns "usage" into an index for
        remap_latents.  Works with sync_host=False; writes nothing into the three dicts."""
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        # (the precompute stores its derived keys and zeroes the reset counters: on shallow copies here)
        self.E_step_precompute(dict(model_params), dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        if self._incomplete:
            eng.set_option("reconstruct_in_stats", 1)
            self._yrec_token = None  # the pass overwrites the device's y_reconstructed: the next M-step uploads the caller's
        acc = eng.stats()
        if not getattr(self.comm, "device_reduces", False):
            acc = _reduce_array(self.comm, acc)
        v = eng.acc_views(acc)
        N = float(v["N"])
        counts = eng.latent_map_counts()
        if self.comm.size > 1:
            counts = np.rint(_reduce_array(self.comm, counts.astype(np.float64))).astype(np.int64)
        sums = v["pies"] if self.model_name == "bsc" else v["xpt_s"]
        return {"usage": np.array(sums, dtype=np.float64) / N, "map_count": counts, "N": int(N)}

    def _stats_for_mstep(self, model_params, my_suff_stat, my_data, _from_step):
        """Accumulators for the M-step: reuse the ones E_step just produced inside step(), else
        recompute them from the caller's K^n / lpj arrays."""
        if _from_step and self._acc is not None:
            return self._acc
        eng = self._prepare(my_suff_stat, my_data)
        self._push_params(model_params)
        if self.sync_host or not self._resident:
            eng.upload_lpj(my_suff_stat["lpj"])
        acc = eng.stats()
        if not getattr(self.comm, "device_reduces", False):
            acc = _reduce_array(self.comm, acc)
        return acc

    def free_energy(self, my_data, model_params, my_suff_stat, full=True, compute_lpj=True):
        """Free energy of K^n, or the exact log-likelihood over all 2^H states when ``full``
        (_models.py:333-451; H < 12).  The 2^H - 1 non-zero states are ONE shared candidate set
        evaluated against every datapoint in a single launch."""
        permanent = my_suff_stat["permanent"]
        background = bool(permanent["background"])
        Y = my_data["y"]
        N_loc = Y.shape[0]
        N = self.comm.allreduce(N_loc)
        force_zero = full and not permanent["allzero"] and not background  # (_models.py:366-373)
        S_perm = 1 if force_zero else my_suff_stat["S_perm"]
        if full or compute_lpj:
            # a scratch engine geometry is fine here: only Y and Theta are needed
            eng = self._prepare(my_suff_stat, my_data, upload_states=not full)
            self.E_step_precompute(model_params, my_suff_stat, my_data)
        if full:
            sm = my_suff_stat["sm"]
            assert sm is not None
            if background:  # every state of the other H - 1 latents with the unit on; no all-zero state (_models.py:389-390)
                body = eng.lpj_shared(np.concatenate((sm, np.ones((sm.shape[0], 1), dtype=bool)), axis=1))
            else:
                body = eng.lpj_shared(sm[1:, :])
        elif compute_lpj:
            eng.lpj_resident()
            body = eng.download_lpj()[:, my_suff_stat["S_perm"]:]
        else:
            body = my_suff_stat["lpj"][:, my_suff_stat["S_perm"]:]
        if S_perm:
            if full or compute_lpj:
                xi = my_data["x_infr"]
                zero = self._allzero_lpj(model_params, (np.where(xi, Y, 0.0) ** 2).sum(axis=1))  # reliable entries
                zero = np.array([self.lpj_reset_check(np.array([z]), my_suff_stat)[0] for z in zero])
            else:
                zero = my_suff_stat["lpj"][:, 0]
            lpj = np.concatenate((zero[:, None], body), axis=1)
        else:
            lpj = body
        Fs = self.engine.free_energy_sum(lpj)
        return model_params["ljc"] + self.comm.allreduce(Fs) / N

    def exact_log_likelihood(self, my_data, model_params, my_suff_stat, per_datapoint=False, marginals=False,
                             max_H=24, chunk_states=0):
        """The exact log-likelihood over all states, the quantity ``free_energy(full=True)`` returns, without its
        H < 12 cap: no state table is built (``my_suff_stat["sm"]`` is ignored).  The device enumerates the states of
        the Hv = H - background latents that vary in chunks of ``chunk_states`` (0 = automatic), evaluates each chunk
        against every datapoint and folds it into a running log-sum-exp per datapoint (Engine.loglik_exact).  The
        work grows with 2^Hv: more than ``max_H`` (itself at most 32) varying latents raise ValueError before anything
        runs.  Returns L = ljc + allreduce(sum_n ll_n) / N; with ``per_datapoint`` / ``marginals`` set, (L, ll, marg)
        with this rank's ll (N_loc,) = log p(y_n | Theta) - ljc and the exact posterior marginals marg (N_loc, H) =
        E_p[s_h | y_n] -- the ground truth of ``encode(...).p`` -- for the flags set, None otherwise.  Writes nothing
        into the three dicts and leaves K^n and the rest of the EM state on the device as they are."""
        from .exact import MAX_HV
        background = bool(my_suff_stat["permanent"]["background"])
        Hv = self.H - (1 if background else 0)
        if max_H > MAX_HV:
            raise ValueError("exact_log_likelihood: max_H = %d, at most %d latents can be enumerated" % (max_H, MAX_HV))
        if Hv < 1 or Hv > max_H:
            raise ValueError("exact_log_likelihood: %d latents vary, that is 2^%d = %d states per datapoint; "
                             "max_H = %d allows 2^%d (raise max_H to run it anyway)" % (Hv, Hv, 2 ** Hv, max_H, max_H))
        N_loc = my_data["y"].shape[0]
        N = self.comm.allreduce(N_loc)
        eng = self._prepare(my_suff_stat, my_data, upload_states=False)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        Fs, ll, marg = eng.loglik_exact(background, chunk_states, per_datapoint=per_datapoint, marginals=marginals)
        L = theta["ljc"] + self.comm.allreduce(Fs) / N
        if per_datapoint or marginals:
            return L, ll, marg
        return L

    def estimate_log_likelihood(self, model_params, my_suff_stat, my_data, n_samples=256, seed=None, first_index=0,
                                prior_mix=0.25, per_datapoint=False, keep_draws=False):
        """An estimate of the log-likelihood where the 2^H states of exact_log_likelihood cannot be enumerated, and with
        it of the tightness of the bound, log p(y_n) - F_n = KL(q_n || p(s | y_n)).  For every datapoint of this rank
        ``n_samples`` states are drawn on the device from a product of Bernoullis whose means are q_n's own marginals over
        K^n mixed with the prior (``prior_mix`` in (0, 1]: rho_h = (1 - prior_mix) p_h + prior_mix pi_h); a draw that K^n
        holds counts as zero, the others are evaluated by the model's lpj kernels and weighted by 1 / r_n:
        Z^_n = sum_{s in K^n} e^{lpj_ns} + (1 / T) sum_t 1[s_t not in K^n] e^{lpj(s_t)} / r_n(s_t).  The estimate is
        unbiased in the likelihood, ll^_n = log Z^_n >= F_n for every datapoint and seed, and E[ll^_n] <= log p(y_n) - ljc:
        it lies at or above the bound and, in expectation, at or below the truth.  Returns L^ = ljc + allreduce(sum_n
        ll^_n) / N, the convention of exact_log_likelihood; with ``per_datapoint``, (L^, info) with the (N_loc,) arrays
        "ll" (ll^_n without ljc), "F" (the bound: posterior_scores()["F"]), "gap" = ll - F >= 0, "mass_outside" (the share
        of Z^_n from outside K^n), "ess" (the effective number of outside draws, (sum w)^2 / sum w^2: a value near 1 says
        one draw carries the estimate), "n_outside" (int32) and the counters "n_bad_weights" / "n_skipped" of
        sample_posterior: those datapoints have NaN rows and are left out of the sum -- L^ is then over the remaining
        datapoints and divided by their count.  ``keep_draws``: info also carries "s" (bool (N, T, H)), "inside" (bool
        (N, T)), "log_r" and "lpj" ((N, T), lpj NaN where the draw is inside K^n).  The stream is counter-based
        (evo_amd.models.estimate_log_likelihood_counter reproduces it for ``self.last_estimate_seed``: the draws, inside
        and n_outside bit for bit): datapoint n is index ``first_index + n`` of the data set, so shards concatenate to
        the single call, and draw t does not depend on ``n_samples``.  ``seed`` None: drawn from np.random; rank and world
        size enter it as in sample_posterior.  ValueError for n_samples < 1 and prior_mix outside (0, 1]; EvoAmdError for
        the float32 mode, H > 1024, and draws that do not fit the free device memory.  Works with sync_host=False and on
        incomplete data, writes nothing into the three dicts, does no communication besides the final all-reduce and
        leaves K^n, lpj, Theta, y_reconstructed and the statistics rows on the device as they are."""
        if int(n_samples) < 1:
            raise ValueError("estimate_log_likelihood: n_samples must be positive")
        if not 0.0 < float(prior_mix) <= 1.0:
            raise ValueError("estimate_log_likelihood: prior_mix must be in (0, 1]")
        if self.dtype == np.float32:
            raise EvoAmdError("estimate_log_likelihood is not available in the float32 mode")
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.last_estimate_seed = (int(seed) * max(1, self.comm.size) + self.comm.rank) & (2 ** 64 - 1)
        yr = my_data.get("y_reconstructed")
        if isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised:
            yr.rows()  # setting the parameters below drops the device copy of an unread reconstruction: fetch it first
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        total, n_ok, info = eng.loglik_estimate(n_samples, self.last_estimate_seed, first_index, prior_mix, keep_draws)
        total, n_all = _reduce_array(self.comm, np.array([total, float(n_ok)]))  # (the one all-reduce of the call)
        L = theta["ljc"] + total / n_all if n_all else float("nan")
        if per_datapoint or keep_draws:
            return L, info
        return L

    def neighbourhood_bound(self, model_params, my_suff_stat, my_data, n_parents=None, per_datapoint=False,
                            incomplete=False):
        """A deterministic lower bound on the log-likelihood above the free energy: the exact mass of the one-flip
        neighbours of K^n (Engine.neighbour_bound; csrc/kernels_nbound.hpp has the law,
        evo_amd.variational.neighbour_bound_host is the NumPy mirror).  For every datapoint of this rank the ``n_parents``
        best states of K^n (None: all S) are the parents; every state one flip away from a parent that K^n does not hold
        is scored as a flip sweep scores it -- each state once, whichever parents reach it -- and the scores are summed,
        not ranked: F+_n = log(sum_{s in K^n} e^{lpj_ns} + sum_{s in Nb_n} e^{lpj_n(s)}), F_n <= F+_n <= log p(y_n) - ljc.
        No draws, so no variance: where estimate_log_likelihood rests on a single draw (``ess`` near 1), this says how much
        of the mass K^n misses lies one flip away.  It sums one-flip neighbours only; ES3C neighbours above 8 active
        latents (EBSC: 64) are left out and their parents counted in "n_capped".  Returns L+ = ljc + allreduce(sum_n
        F+_n) / count, the convention of estimate_log_likelihood; with ``per_datapoint``, (L+, info) with the (N_loc,)
        arrays "F" (the bound: posterior_scores()["F"]), "F_plus", "gap" = F_plus - F >= 0, "mass_outside" (the share of
        the sum from outside K^n), "n_states" (the neighbours summed), "n_capped", "best_score", "best_parent" (rank) and
        "best_flip" (latent) of the best neighbour (-inf / -1 / -1 without one) and the counter "n_bad_weights": those
        datapoints have NaN rows and are left out of the sum and the count.  ``incomplete=True`` admits my_data["x_infr"]
        with False entries: every neighbour is scored on the datapoint's reliable entries alone, as in
        sweep_resident_states.  ValueError for the background unit, for incomplete data without ``incomplete=True`` and
        for n_parents outside [1, S]; NotImplementedError in the float32 mode.  Works with sync_host=False, writes nothing
        into the three dicts, does no communication besides the final all-reduce and leaves K^n, lpj, Theta,
        y_reconstructed and the statistics rows on the device as they are (the call evaluates the resident rows itself,
        as a sweep does, so the host's lpj is not uploaded)."""
        S = self.S
        P = int(S if n_parents is None else n_parents)
        if my_suff_stat["permanent"]["background"]:
            raise ValueError("neighbourhood_bound: the background unit is not supported")
        if self.dtype == np.float32:
            raise NotImplementedError("neighbourhood_bound is not available in the float32 mode")
        if not 1 <= P <= S:
            raise ValueError("neighbourhood_bound: n_parents = %d must be in [1, S = %d]" % (P, S))
        if not incomplete and not self._complete(my_data):
            raise ValueError("neighbourhood_bound: incomplete data (x_infr with False entries) is not supported by default: "
                             "pass incomplete=True")
        yr = my_data.get("y_reconstructed")
        if isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised:
            yr.rows()  # setting the parameters below drops the device copy of an unread reconstruction: fetch it first
        eng = self._prepare(my_suff_stat, my_data)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        info = eng.neighbour_bound(P, incomplete=bool(incomplete))
        total, n_all = _reduce_array(self.comm, np.array([info.pop("sum"), float(info.pop("count"))]))  # (the one all-reduce)
        L = theta["ljc"] + total / n_all if n_all else float("nan")
        if not per_datapoint:
            return L
        info.pop("M")
        info["n_bad_weights"] = int(np.isnan(info["F"]).sum())
        return L, info

    def ais_log_likelihood(self, model_params, my_suff_stat, my_data, n_chains=16, n_temps=128, betas=None, seed=None,
                           first_index=0, direction="forward", s_start=None, per_datapoint=False, keep_states=False,
                           admit=False, incomplete=False):
        """Annealed importance sampling (Neal 2001): bounds on the log-likelihood that do not depend on K^n, for EBSC
        (incomplete data with ``incomplete=True``, below) (Engine.ais_loglik; csrc/kernels_ais.hpp has the law, evo_amd.models.ais_log_likelihood_counter is
        the NumPy mirror).  Per datapoint ``n_chains`` Gibbs chains walk through the temperatures ``betas`` (a float64
        array of T + 1 values from 0 to 1 that never descends; None: the sigmoid schedule of ``n_temps`` steps,
        evo_amd.models.sigmoid_schedule) between the prior and the posterior, one systematic scan over the latents per
        temperature.  ``direction="forward"``: from a prior draw; the mean of the chains' weights is an unbiased estimate
        of p(y_n), so ll_n is a stochastic LOWER bound (E[ll_n] <= log p(y_n) - ljc).  ``direction="reverse"``: from row n
        of ``s_start`` (bool (N, H)) back to the prior; ll_n is a stochastic UPPER bound (bidirectional Monte Carlo) --
        it is an exact posterior sample only when y_n was generated from this Theta with that s: for synthetic data, the
        "s" that generate_data_device returns.  For any other start the reverse value bounds nothing.  Returns L = ljc +
        allreduce(sum_n ll_n) / N, the convention of estimate_log_likelihood; with ``per_datapoint``, (L, info) with the
        (N_loc,) arrays "ll", "ess" (of the averaged terms: w forward, 1 / w reverse), "log_w_mean", "log_w_min",
        "log_w_max" and "n_flips" (int64, the accepted flips of all chains); ``keep_states`` adds "log_w" (N, C), "final"
        (the chains' last states, uint8, N x C x ceil(H / 8) in np.packbits layout) and "chain_flips" (N, C).  The final
        states of forward chains are approximate posterior samples: ``admit=True`` (forward only) puts those of the first
        min(C, Cmax) chains into the candidate batch in chain order (the all-zero state skipped), evaluates them with
        the model's own lpj kernels and runs the usual selection with my_suff_stat["Mprime"]; info gains "S_sub" (the
        substitutions, normalised like E_step's), "F_before" and "F_after" (N_loc,), and with sync_host K^n and lpj are
        copied back.  Without ``admit`` K^n, lpj, the candidate batch and the statistics rows stay as they are.  The
        stream is counter-based (``self.last_ais_seed``): datapoint n is index ``first_index + n`` of the data set, so
        shards concatenate to the single call, and chain c does not depend on ``n_chains``.  ``seed`` None: drawn from
        np.random; rank and world size enter it as in sample_posterior.  NotImplementedError for ES3C; ValueError for the
        float32 mode, the background unit, incomplete data, H > 1024, n_chains < 1, betas that do not start at 0, end at
        1 or that descend, reverse without an ``s_start`` of shape (N, H) bool, and admit with reverse.  One all-reduce.
        ``incomplete=True`` admits my_data["x_infr"] with False entries, a permission as for seed_resident_states: the
        chains of datapoint n run on its own G(n) = W_o^T W_o over its reliable entries o, a row formed from W and the mask
        when a flip happens (csrc/kernels_ais.hpp, INCOMPLETE DATA; the mirror takes ``x_infr``); values of y under False,
        NaN included, never enter.  A datapoint without a reliable entry is not skipped: its chains are prior draws, log w =
        0, and it stays in the sum and in N, so L = ljc + sum_n ll_n / N with the ljc of incomplete data.  ``admit`` runs
        the masked candidate lpj and selection of every E-step.  With complete data the argument changes nothing; a D
        whose column and list do not fit into LDS beside the rows over H is an EvoAmdError naming D and H."""
        from .ais import AIS_MAX_H, check_betas, sigmoid_schedule
        if self.model_name != "bsc":
            raise NotImplementedError("ais_log_likelihood is for EBSC: ES3C is out of scope (its importance estimate works, "
                                      "and a collapsed Gibbs step would need a bordered k x k system per flip)")
        if self.dtype == np.float32:
            raise ValueError("ais_log_likelihood is not available in the float32 mode")
        if my_suff_stat["permanent"]["background"]:
            raise ValueError("ais_log_likelihood: the background unit is not supported")
        if not incomplete and not self._complete(my_data):
            raise ValueError("ais_log_likelihood: incomplete data (x_infr with False entries) is not supported")
        if self.H > AIS_MAX_H:
            raise ValueError("ais_log_likelihood: H = %d, at most %d latents are supported" % (self.H, AIS_MAX_H))
        C = int(n_chains)
        if C < 1:
            raise ValueError("ais_log_likelihood: n_chains = %d must be positive" % C)
        betas = sigmoid_schedule(n_temps) if betas is None else check_betas(betas)
        if direction not in ("forward", "reverse"):
            raise ValueError("ais_log_likelihood: direction = %r must be 'forward' or 'reverse'" % (direction,))
        reverse = direction == "reverse"
        N = my_data["y"].shape[0]
        if reverse:
            if s_start is None or np.shape(s_start) != (N, self.H) or np.asarray(s_start).dtype != np.bool_:
                raise ValueError("ais_log_likelihood: direction='reverse' needs s_start, a bool array of shape (N, H) = (%d, %d)"
                                 % (N, self.H))
            if admit:
                raise ValueError("ais_log_likelihood: admit=True with direction='reverse': a reverse chain ends at the prior, "
                                 "its final states are no proposals for K^n")
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.last_ais_seed = (int(seed) * max(1, self.comm.size) + self.comm.rank) & (2 ** 64 - 1)
        yr = my_data.get("y_reconstructed")
        if isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised:
            yr.rows()  # setting the parameters below drops the device copy of an unread reconstruction: fetch it first
        eng = self._prepare(my_suff_stat, my_data, upload_states=bool(admit))  # (the chains read no K^n)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        info = eng.ais_loglik(betas, C, self.last_ais_seed, first_index, reverse=reverse, s_start=s_start if reverse else None,
                              keep_states=bool(keep_states), admit=bool(admit),
                              Mprime=my_suff_stat["Mprime"] if admit else 1, incomplete=bool(incomplete))
        red = _reduce_array(self.comm, np.array([info.pop("sum"), float(N), info.pop("S_sub", 0.0)]))  # (the one all-reduce)
        L = theta["ljc"] + red[0] / red[1]
        if admit:
            info.pop("S_nunique")
            info["S_sub"] = red[2] / red[1]
            if self.sync_host:
                self.sync_to_host(my_suff_stat)
        if per_datapoint or keep_states or admit:
            return L, info
        return L

    def ais_posterior(self, model_params, my_suff_stat, my_data, n_chains=16, n_temps=128, n_keep=4, betas=None, seed=None,
                      first_index=0, mean=False, keep_chains=False, incomplete=False, index=None, admit=False):
        """Posterior expectations beyond K^n, for EBSC with H <= 1024 (incomplete data with ``incomplete=True``, below)
        (Engine.ais_posterior;
        csrc/kernels_ais_post.hpp has the law, evo_amd.models.ais_posterior_counter is the NumPy mirror).  encode(...).p,
        reconstruct and predictive_moments are expectations under q_n, the posterior truncated to K^n; here the chains ARE
        the forward chains of ais_log_likelihood (same stream, start and schedule), continued: a chain with its weight is a
        properly weighted sample of the true posterior, the scan at beta_T = 1 is the first of ``n_keep`` >= 1 kept scans,
        and in a kept scan the conditional p(s_h = 1 | the rest) is recorded when latent h is decided (Rao-Blackwell).
        Returns a dict of per-datapoint arrays of this rank: "p" (N, H) = sum_c a_c r_ch with a_c the normalised weights --
        a consistent estimate of E_p[s_h | y_n] -- and "p_se" (N, H), its delta-method standard error (it measures the
        spread over the chains: a mode that no chain visited is not in it; read "ess" beside it); "count" (N) = sum_h
        p_nh; "map_lpj" (N) and "map_state" (uint8 (N, ceil(H / 8)), np.packbits layout), the best state any chain
        visited after a kept scan; "ll", "ess", "log_w_mean", "log_w_min", "log_w_max", "n_flips" as ais_log_likelihood
        (direction="forward", per_datapoint=True) gives them, n_flips with the kept scans.  ``mean=True`` adds "mean" (N,
        D) = p W^T, the posterior mean of W s: the reconstruction that does not go through K^n.  ``keep_chains=True`` adds
        "log_w", "chain_map_lpj" (N, C), "rb" (N, C, H), "chain_map_state" (uint8 (N, C, ceil(H / 8))) and "chain_flips"
        (N, C).  Chain c does not depend on ``n_chains``, shards by ``first_index`` concatenate, two calls give the same
        bits; ``seed`` None: drawn from np.random and left in ``self.last_ais_seed`` (rank and world size enter it as in
        ais_log_likelihood).  Nothing of the EM state is written -- not K^n, lpj, the candidate batch, the statistics rows
        or y_hat -- and there is no collective (``admit``: RESCUE below).  Out of scope: reverse chains, ES3C, resident handles for p / mean,
        second moments, use of the marginals in the M-step.  NotImplementedError for ES3C; ValueError for the float32
        mode, the background unit, incomplete data without ``incomplete=True``, H > 1024, n_chains < 1, n_keep < 1 and
        betas that do not start at 0, end at 1 or that descend.  ``incomplete=True`` admits my_data["x_infr"] with False
        entries as ais_log_likelihood does (the chains on G(n) over the reliable entries; y under False, NaN included,
        never enters); "mean" = p W^T then covers EVERY entry, the missing ones included: the reconstruction of the
        missing entries that does not go through K^n.  A datapoint without a reliable entry has the prior's marginals.

        RESCUE.  ``index``: a 1-d integer array of this rank's datapoints, strictly ascending within [0, N_loc) (ValueError
        naming the first offender otherwise) -- the chains run for these alone, at a cost linear in len(index), and every
        per-datapoint array has len(index) rows in list order; row i is bit for bit row index[i] of the call without
        ``index`` at the same seed (``first_index`` keeps its meaning and is added to index[i]).  An empty list is legal:
        empty arrays, no library call.  ``admit=True`` hands what the chains found to K^n: per listed datapoint the chains'
        best states, ranked by their lpj (ties to the lower chain), without the all-zero state, repeats and states K^n
        holds, at most Cmax of them, become the candidate batch (nothing for the other datapoints); the model's own
        candidate lpj kernels and the usual selection with my_suff_stat["Mprime"] follow (masked with ``incomplete``), as
        for ais_log_likelihood(admit=True), which takes the FINAL states of the FIRST chains unranked.  The result gains
        "F_before", "F_after" (the bound per listed datapoint without ljc), "n_distinct" (distinct non-zero best states),
        "n_new" (those K^n did not hold), "n_proposed" = min(n_new, Cmax), "n_admitted" (the proposed states K^n holds
        afterwards), "map_held_before", "map_held_after" (bool: K^n holds map_state) and "S_sub" (the substitutions,
        all-reduced and normalised like E_step's: the one collective, entered with an empty list too); with sync_host K^n
        and lpj are copied back.  Without ``admit`` the call still writes nothing of the EM state and has no collective.
        The call does not choose the list (Model.posterior_scores gives F per datapoint to choose by), does not repeat
        itself, and a state it admits may be displaced by a later E-step like any other.  Out of scope: ``index`` for
        ais_log_likelihood, ES3C, the float32 mode, the background unit, H > 1024, resident handles for p / mean, choosing
        the list on the device."""
        from .ais import AIS_MAX_H, check_betas, check_index, sigmoid_schedule
        if self.model_name != "bsc":
            raise NotImplementedError("ais_posterior is for EBSC: ES3C is out of scope (a collapsed Gibbs step would need a "
                                      "bordered k x k system per flip)")
        if self.dtype == np.float32:
            raise ValueError("ais_posterior is not available in the float32 mode")
        if my_suff_stat["permanent"]["background"]:
            raise ValueError("ais_posterior: the background unit is not supported")
        if not incomplete and not self._complete(my_data):
            raise ValueError("ais_posterior: incomplete data (x_infr with False entries) is not supported")
        if self.H > AIS_MAX_H:
            raise ValueError("ais_posterior: H = %d, at most %d latents are supported" % (self.H, AIS_MAX_H))
        C, K = int(n_chains), int(n_keep)
        if C < 1:
            raise ValueError("ais_posterior: n_chains = %d must be positive" % C)
        if K < 1:
            raise ValueError("ais_posterior: n_keep = %d must be positive" % K)
        betas = sigmoid_schedule(n_temps) if betas is None else check_betas(betas)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.last_ais_seed = (int(seed) * max(1, self.comm.size) + self.comm.rank) & (2 ** 64 - 1)
        yr = my_data.get("y_reconstructed")
        if isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised:
            yr.rows()  # setting the parameters below drops the device copy of an unread reconstruction: fetch it first
        if index is not None:
            index = check_index(index, my_data["y"].shape[0])
        eng = self._prepare(my_suff_stat, my_data, upload_states=bool(admit))  # (the chains read no K^n)
        theta = dict(model_params)  # (the precompute stores its derived keys and zeroes the reset counters: on copies)
        self.E_step_precompute(theta, dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        info = eng.ais_posterior(betas, C, K, self.last_ais_seed, first_index, mean=bool(mean), keep_chains=bool(keep_chains),
                                 incomplete=bool(incomplete), index=index, admit=bool(admit),
                                 Mprime=my_suff_stat["Mprime"] if admit else 1)
        if admit:
            info.pop("S_nunique")
            red = _reduce_array(self.comm, np.array([info["S_sub"], float(my_data["y"].shape[0])]))  # (the one all-reduce)
            info["S_sub"] = red[0] / red[1]
            if self.sync_host:
                self.sync_to_host(my_suff_stat)
        return info

    def reconstruct(self, my_data, my_suff_stat, model_params):
        """(Re-)estimate the entries with my_data["x"] False from the posterior predictive distribution under
        ``model_params`` and the caller's K^n / lpj; adds my_data["y_reconstructed"] (_models.py:614-665).
        The reference loops over datapoints calling modelmean(); here the statistics pass writes E_q[s]
        (EBSC) / E_q[s o z] (ES3C) per datapoint and ONE f64 MFMA product with W^T gives every estimate."""
        # _prepare() uploads K^n and sets _resident when the device copy was stale (first call, invalidate(), a new
        # geometry): the lpj rows on the device are stale in exactly those cases, so decide BEFORE it runs
        uploads = self._kn_uploads
        eng = self._prepare(my_suff_stat, my_data)
        self.E_step_precompute(model_params, my_suff_stat, my_data)
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        if self._incomplete:
            eng.set_option("reconstruct_in_stats", 1)
        eng.stats()
        self._write_reconstruction(my_data)
        if self._incomplete:
            self._yrec_token = (my_data["y_reconstructed"],)

    def encode(self, model_params, my_suff_stat, my_data, max_active=16, p_min=0.0, dense=False):
        """The code of every datapoint of this rank under ``model_params`` and the caller's K^n / lpj: a
        evo_amd.codes.PosteriorCodes with, per datapoint, the ``max_active`` (1 .. 64) most probable latents among those
        with E_q[s_h] > ``p_min`` -- their posterior marginals E_q[s_h] and, ES3C, posterior means E_q[s_h z_h] -- and the
        most probable state of K^n.  One statistics pass (as in reconstruct()), then the rows it leaves on the device are
        compacted there and only the compact form crosses to the host; ``dense=True`` also brings the dense (N, H) rows
        of the same pass (codes.Es / codes.Ez).  Works with sync_host=False (K^n and lpj are read on the device), does
        no communication and writes nothing into the three dicts."""
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        # (the precompute stores its derived keys and zeroes the reset counters: on shallow copies here)
        self.E_step_precompute(dict(model_params), dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        if self._incomplete:
            eng.set_option("reconstruct_in_stats", 1)
            self._yrec_token = None  # the pass overwrites the device's y_reconstructed: the next M-step uploads the caller's
        eng.stats()
        codes = eng.posterior_codes(max_active, p_min)
        if dense:
            codes.Es, codes.Ez = eng.download_posterior()
        return codes

    def predictive_moments(self, model_params, my_suff_stat, my_data, noise=True, resident=False):
        """The posterior-predictive mean and variance of EVERY entry (n, d) of this rank's data, observed or missing, under
        ``model_params`` and the caller's K^n / lpj: (mean, var, info) with float64 (N_loc, D) arrays.  mean = W E_q[s]
        (EBSC) / W E_q[s o z] (ES3C), what reconstruct() writes at the missing entries; var = the variance of the
        mixture over K^n -- between the states' means plus, ES3C, each state's own w_d^T Lam_s w_d -- plus the noise
        variance (EBSC sigma**2, ES3C sigma2) when ``noise``.  Formed in a centred form on the device
        (Engine.predictive_moments; evo_amd.models.predictive_moments_host is the NumPy mirror): without the noise term
        it is never negative.  A datapoint without a reliable entry (the rows reconstruct() skips) has NaN rows and is
        counted in info["n_skipped"]; one with a singular k x k system has NaN rows and is counted in
        info["n_singular"]; a state with more than 32 active latents raises EvoAmdError naming n and k.  Runs no
        statistics pass, does no communication (per rank), writes nothing into the three dicts, works with
        sync_host=False and leaves K^n, lpj, Theta, y_reconstructed and the statistics rows on the device as they are.
        ``resident=True``: mean and var stay on the device and come back as ResidentMoments handles (array-like; np.asarray
        downloads once): ``ovp.set_and_merge(mean.T, merge_method=precision_merger(var.T))`` and
        ``ovp.set_and_merge(var.T, merge_method=mean_merger)`` merge them there and only the image crosses to the host.
        The handles belong to this call: the next predictive_moments outdates what was not read (RuntimeError)."""
        if self.dtype == np.float32:
            raise NotImplementedError("predictive_moments is not available in the float32 mode")
        if self._moments_handle is not None:
            self._moments_handle._outdate("a later predictive_moments of the same model")
            self._moments_handle = None
        yr = my_data.get("y_reconstructed")
        if isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised:
            yr.rows()  # setting the parameters below drops the device copy of an unread reconstruction: fetch it first
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        # (the precompute stores its derived keys and zeroes the reset counters: on shallow copies here)
        self.E_step_precompute(dict(model_params), dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        mean, var, info = eng.predictive_moments(noise=noise, resident=resident)
        if resident:
            self._moments_handle = mean
        return mean, var, info

    def predictive_log_score(self, model_params, my_suff_stat, my_data, y_true, query=None, noise=True, per_entry=False):
        """The log predictive density of held-out entries and its calibration counterpart, the PIT: (score, info).  Entry
        (n, d) is scored when ``query[n, d]`` (bool (N_loc, D)) is set and ``y_true[n, d]`` (float64 (N_loc, D)) is finite;
        ``query=None`` means ~my_data["x_infr"], the entries the model did not see (ValueError "nothing to score" on
        complete data).  An explicit ``query`` may name reliable entries: that is an IN-SAMPLE score -- the model has
        conditioned on the very value it is asked to predict -- and says nothing about held-out entries.  Values of
        ``y_true`` outside ``query`` are never read (NaN there is fine).  The predictive distribution of an entry is the
        MIXTURE over K^n (and the permanent all-zero state) with the weights q_ns, one Gaussian N(m_ns,d, tau_ns,d) per
        state -- m and v of predictive_moments, tau = v + the noise variance with ``noise`` (score noisy observations) or
        tau = v without (score the clean signal, the denoising case; EBSC has v = 0 everywhere then: ValueError) -- not
        the single Gaussian of predictive_moments' mean and var, which differs from it wherever the states disagree.
        logp = log sum_s q_ns N(y; m, tau), pit = sum_s q_ns Phi((y - m) / sqrt(tau)) (Engine.predictive_score;
        csrc/kernels_predictive_score.hpp has the law, evo_amd.models.predictive_log_score_host is the NumPy mirror;
        pit_summary reads the PIT).  ``score`` is the mean log density per scored entry over all ranks (one all-reduce of
        [sum, count], as estimate_log_likelihood; NaN when nothing was scored).  info holds this rank's "logp_n" (N_loc,)
        -- the sum over the datapoint's scored entries --, "count" (N_loc,) int32, the counters "n_singular", "n_skipped"
        (datapoints with a singular system / without a reliable entry, as in predictive_moments: nothing of them is
        scored), "n_not_queried" (datapoints without a scored entry: not visited at all) and "n_bad_values" (queried
        entries whose y_true is not finite: NaN, left out) and, with ``per_entry``, "logp" and "pit" (N_loc, D), NaN
        outside the scored entries.  It scores entries one by one, not the joint density of a datapoint's held-out
        entries.  The float32 mode raises NotImplementedError; D > 512 and a state with more than 32 active latents in a
        visited datapoint raise as in predictive_moments.  Deterministic (two calls give the same bits), works with
        sync_host=False, writes nothing into the three dicts and leaves K^n, lpj, the candidate batch, Theta,
        y_reconstructed, the statistics rows and the moments of predictive_moments on the device as they are."""
        if self.dtype == np.float32:
            raise NotImplementedError("predictive_log_score is not available in the float32 mode")
        if self.model_name != "sssc" and not noise:
            raise ValueError("predictive_log_score: EBSC without noise has variance 0 at every entry: nothing to score")
        shape = np.shape(my_data["y"])
        if query is None:
            if self._complete(my_data):
                raise ValueError("predictive_log_score: nothing to score (query=None on complete data)")
            query = ~np.asarray(my_data["x_infr"], dtype=bool)
        query = np.asarray(query)
        if query.dtype != np.bool_ or query.shape != shape:
            raise ValueError("predictive_log_score: query must be a bool array of shape %r" % (shape,))
        y_true = np.asarray(y_true)
        if y_true.shape != shape:
            raise ValueError("predictive_log_score: y_true must have the shape %r of my_data[\"y\"], got %r" % (shape, y_true.shape))
        yr = my_data.get("y_reconstructed")
        if isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised:
            yr.rows()  # setting the parameters below drops the device copy of an unread reconstruction: fetch it first
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        # (the precompute stores its derived keys and zeroes the reset counters: on shallow copies here)
        self.E_step_precompute(dict(model_params), dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        info = eng.predictive_score(y_true, query, noise=noise, per_entry=per_entry)
        total, n_all = _reduce_array(self.comm, np.array([info.pop("sum"), float(info.pop("total_count"))]))  # (the one all-reduce)
        return (total / n_all if n_all else float("nan")), info

    _KEEP_ALL = ("slot", "s", "z", "y")  # the default of sample_posterior, told from the same names given by the caller

    def sample_posterior(self, model_params, my_suff_stat, my_data, n_samples=1, seed=None, first_index=0,
                         keep=_KEEP_ALL, fill="missing", noise=True, resident=False):
        """``n_samples`` draws per datapoint of this rank from the variational posterior under ``model_params`` and the
        caller's K^n / lpj: a dict with, for datapoint n and draw t, "slot" (int32 (N, T): the column of lpj drawn with
        probability q_ns), "s" (bool (N, T, H): the drawn state), ES3C "z" (float64 (N, T, H): z_A ~ N(kappa_s, Lam_s) on
        the active set, the Lam and kappa of predictive_moments) and "y" (float64 (N, T, D): W z -- EBSC W s -- plus the
        noise sigma g when ``noise``).  ``fill="missing"``: the reliable entries (x_infr) carry the datapoint's own y and
        only the others the draw (multiple imputation); ``fill="all"``: every entry carries the draw (a posterior-
        predictive replicate).  ``keep`` names the arrays to form: only those are allocated, written and downloaded; the
        default drops "z" for EBSC, which refuses it when asked for by name.  "info" counts the datapoints without draws
        (slot -1, s zero, z and y NaN): "n_skipped" (no reliable entry), "n_bad_weights" (an lpj row with a NaN or +inf,
        or all -inf), "n_singular" / "n_not_pd" (a DRAWN state whose k x k system is singular / whose Lam is not positive
        definite: an indefinite Psi).  The stream is counter-based (evo_amd.models.sample_posterior_counter reproduces it
        for ``self.last_sample_seed``: slot and s bit for bit): datapoint n is index ``first_index + n`` of the data set,
        so shards concatenate to the single call, and draw t does not depend on ``n_samples``.  ``seed`` None: drawn from
        np.random; rank and world size enter it as in generate_data_device.  The float32 mode, D > 512 and a state with
        more than 32 active latents raise (EvoAmdError naming n and k), as do outputs that do not fit into the free device
        memory (naming the bytes).  Runs no statistics pass, does no communication, writes nothing into the three dicts,
        works with sync_host=False and leaves K^n, lpj, Theta, y_reconstructed and the statistics rows on the device as
        they are.  ``resident=True`` (``keep`` must name "y", else ValueError): "y" is not downloaded; the entry is a
        ResidentDraws handle -- ``handle.merge(ovp)`` gives the T merged images, ``handle.merge_moments(ovp)`` their
        pixelwise mean and standard deviation, both formed on the device; np.asarray(handle) is the array of the default
        path.  The handle belongs to this call: the next sample_posterior outdates an unread one (RuntimeError)."""
        default_keep = keep is Model._KEEP_ALL
        keep = tuple(keep)
        for name in keep:
            if name not in ("slot", "s", "z", "y"):
                raise ValueError("keep: unknown output %r" % (name,))
        if self.model_name != "sssc" and "z" in keep:
            if not default_keep:
                raise EvoAmdError("sample_posterior: \"z\" is an ES3C output (EBSC: z = s)")
            keep = tuple(name for name in keep if name != "z")
        if fill not in ("missing", "all"):
            raise ValueError("fill must be 'missing' or 'all'")
        if resident and "y" not in keep:
            raise ValueError("sample_posterior: resident=True keeps the draws \"y\" on the device: keep must name \"y\"")
        if self.dtype == np.float32:
            raise EvoAmdError("sample_posterior is not available in the float32 mode")
        if self._draws_handle is not None:
            self._draws_handle._outdate("a later sample_posterior of the same model")
            self._draws_handle = None
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.last_sample_seed = (int(seed) * max(1, self.comm.size) + self.comm.rank) & (2 ** 64 - 1)
        yr = my_data.get("y_reconstructed")
        if isinstance(yr, ResidentReconstruction) and yr.resident and not yr.materialised:
            yr.rows()  # setting the parameters below drops the device copy of an unread reconstruction: fetch it first
        uploads = self._kn_uploads  # (see reconstruct(): decide before _prepare() runs)
        eng = self._prepare(my_suff_stat, my_data)
        # (the precompute stores its derived keys and zeroes the reset counters: on shallow copies here)
        self.E_step_precompute(dict(model_params), dict(my_suff_stat), my_data)
        if model_params is not self._dev_theta:
            self._dev_theta = None  # the device now holds THIS Theta, not the one a device_mstep step left there
        if self.sync_host or self._kn_uploads != uploads:
            eng.upload_lpj(my_suff_stat["lpj"])
        out = eng.sample_posterior(n_samples, self.last_sample_seed, first_index, keep, fill, noise, resident=resident)
        if resident:
            self._draws_handle = out["y"]
        return out

    def modelmean(self, model_params, this_data, this_suff_stat):
        """Per-datapoint operator of the reference's reconstruct loop: (D_miss, S) means of the entries to be
        reconstructed, one column per state of this_suff_stat["ss"] (bsc.py:279-287, sssc.py:368-405)."""
        raise NotImplementedError

"""Engine: one GPU context of libevo_amd.so, NumPy in / NumPy out.

The engine owns the device-resident copies of the three state bags of the reference
(SURVEY.md 8b): ``my_data["y"]``, ``my_suff_stat["ss"]`` / ``["lpj"]`` (bit-packed K^n), and
``model_params``.  The model classes in ``evo_amd.models`` drive it; ``bench.py`` drives it
directly so that nothing but device work sits in the timed region.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import MODEL_BSC, MODEL_SSSC, EvoAmdError, as_bool_bytes, as_f64, check, dptr, i32ptr, u8ptr


class SingularUpdate(EvoAmdError):
    """evoamd_mstep_device: the H x H system of the Theta update is exactly singular.  The E-step results
    of the same call are valid and ride along (``tail``, ``dpar``) so that the caller can finish the step
    with the reference's host formulas (lstsq / pinv fallbacks, bsc.py:236-250, sssc.py:692-708)."""

    def __init__(self, msg, tail, dpar):
        EvoAmdError.__init__(self, msg)
        self.tail, self.dpar = tail, dpar


def default_device():
    """LOCAL_RANK under torchrun / one process per GPU, else 0."""
    return int(os.environ.get("LOCAL_RANK", "0"))


class Engine:
    def __init__(self, device=None):
        self.lib = _lib.load()
        self.device = default_device() if device is None else int(device)
        h = ctypes.c_void_p()
        check(self.lib.evoamd_ctx_create(self.device, ctypes.byref(h)))
        self._h = h
        self.model = None
        self.N = self.D = self.H = self.S = self.S_perm = self.Cmax = 0
        self.ljc = None
        self.has_masks = False
        self.f32 = False  # EBSC float32 mode of the configured geometry (option "ebsc_f32")
        self.world = 1
        self.rank = 0
        self._configures = 0  # evoamd_configure calls: a keep-mask uploaded for an earlier geometry is gone
        self._keep_token = None  # (x object, geometry, _configures, any(x)) of the keep-mask on the device
        self._rec_serial = 0     # counts reconstruct_resident calls: names the reconstruction the device holds
        self._ps_serial = 0      # counts sample_posterior calls (and configures): names the draws the device holds
        self._pred_serial = 0    # the same for predictive_moments

    # ---- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.evoamd_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib.evoamd_synchronize(self._h))

    def debug_validity(self):
        """The host-side validity state of the context (evoamd_debug_validity): {flag name: bool} for the bits of
        _lib.VALIDITY_BITS and {name: int} for _lib.VALIDITY_WORDS.  No device work."""
        out = (ctypes.c_int64 * 8)()
        check(self.lib.evoamd_debug_validity(self._h, out))
        d = {name: bool((out[0] >> i) & 1) for i, name in enumerate(_lib.VALIDITY_BITS)}
        d.update(zip(_lib.VALIDITY_WORDS, (int(v) for v in out[1:])))
        return d

    def set_option(self, name, value):
        check(self.lib.evoamd_set_option(self._h, name.encode(), int(value)))

    # ---- geometry / uploads --------------------------------------------------------------
    def configure(self, model, N, D, H, S, S_perm=0, Cmax=16):
        m = MODEL_BSC if model in (MODEL_BSC, "bsc", "BSC") else MODEL_SSSC
        check(self.lib.evoamd_configure(self._h, m, int(N), int(D), int(H), int(S), int(S_perm), int(Cmax)))
        self.model = m
        self.N, self.D, self.H, self.S, self.S_perm, self.Cmax = int(N), int(D), int(H), int(S), int(S_perm), int(Cmax)
        self.L = self.S + self.S_perm
        self.has_masks = False  # evoamd_configure drops the masks of the previous geometry
        self._configures += 1
        self._ps_serial += 1    # ... and releases the draws and moments of the previous geometry
        self._pred_serial += 1

    def same_geometry(self, model, N, D, H, S, S_perm, Cmax):
        m = MODEL_BSC if model in (MODEL_BSC, "bsc", "BSC") else MODEL_SSSC
        return (self.model, self.N, self.D, self.H, self.S, self.S_perm, self.Cmax) == (m, N, D, H, S, S_perm, Cmax)

    def upload_data(self, Y):
        Y = as_f64(Y)
        assert Y.shape == (self.N, self.D), (Y.shape, self.N, self.D)
        check(self.lib.evoamd_upload_data(self._h, dptr(Y)))

    def upload_states(self, ss):
        b = as_bool_bytes(ss)
        assert b.shape == (self.N, self.S, self.H), (b.shape, (self.N, self.S, self.H))
        check(self.lib.evoamd_upload_states(self._h, u8ptr(b)))

    def download_states(self, out=None):
        """K^n as bool (N,S,H).  ``out`` may be the caller's my_suff_stat["ss"] (written in place)."""
        if out is None:
            out = np.empty((self.N, self.S, self.H), dtype=np.bool_)
        assert out.shape == (self.N, self.S, self.H) and out.dtype == np.bool_ and out.flags.c_contiguous
        check(self.lib.evoamd_download_states(self._h, u8ptr(out.view(np.uint8))))
        return out

    def upload_states_packed(self, packed, n0=0):
        """K^n rows [n0, n0 + n) as np.packbits(ss, axis=-1) lays them out: uint8 (n, S, ceil(H/8))."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        assert packed.ndim == 3 and packed.shape[1:] == (self.S, (self.H + 7) // 8), packed.shape
        check(self.lib.evoamd_upload_states_packed(self._h, u8ptr(packed), int(n0), packed.shape[0]))

    def download_states_packed(self, n0=0, n=None):
        n = self.N - n0 if n is None else int(n)
        out = np.empty((n, self.S, (self.H + 7) // 8), dtype=np.uint8)
        check(self.lib.evoamd_download_states_packed(self._h, u8ptr(out), int(n0), n))
        return out

    def init_states(self, p_init, seed, max_rounds=256, table=None):
        """K^n(0) drawn on the device with the law of evo_amd.variational.init_states and the counter-based stream of
        evo_amd.variational.init_states_counter (its NumPy mirror, bit for bit); reads S_perm and the "background_unit"
        option of the context.  ``table``: bool (S, H) state table of the exact mode (S == 2 ** Hv), copied to every
        datapoint instead.  EvoAmdError naming the cap when a datapoint is not complete after ``max_rounds`` rounds: K^n
        then counts as not uploaded."""
        tp = None
        if table is not None:
            t = np.ascontiguousarray(table, dtype=np.bool_)
            assert t.shape == (self.S, self.H), (t.shape, (self.S, self.H))
            packed = np.packbits(t, axis=-1)
            tp = u8ptr(packed)
        check(self.lib.evoamd_init_states(self._h, float(p_init), int(seed) & (2 ** 64 - 1), int(max_rounds), tp))

    def _seed_out(self, max_active, want_path):
        """max_active as an int, what a seeding call returns -- (path, lpj_path) or None -- and the two pointers."""
        A = int(max_active)
        if not want_path:
            return A, None, (None, None)
        path = np.empty((self.N, max(A, 1)), dtype=np.int32)
        lpj = np.empty((self.N, max(A, 1)), dtype=np.float64)
        return A, (path, lpj), (i32ptr(path), dptr(lpj))

    def seed_states(self, max_active, want_path=False, incomplete=False):
        """K^n seeded on the device from Theta and the data by greedy forward selection on the model's own lpj
        (evoamd_seed_states; evo_amd.variational.seed_states_host is its NumPy mirror): deterministic, ``max_active``
        steps per datapoint, S distinct states of 1 .. max_active latents in step-major slots.  ``want_path``: returns
        (path int32 (N, max_active), lpj_path (N, max_active)) -- the latent added at each step and its state's lpj --
        else None.  ``incomplete`` permits incomplete data (evoamd_seed_states_ex, EVOAMD_SEED_INCOMPLETE): with masks
        resident (upload_masks) the law runs on each datapoint's reliable entries, its Gram rows formed from W and the
        mask; without masks the flag changes nothing.  EvoAmdError naming the rule, with K^n left as it was, for a
        missing Theta, masks present without ``incomplete``, the background unit, the float32 mode, bsc_direct or a
        ``max_active`` the law refuses."""
        A, out, ptrs = self._seed_out(max_active, want_path)
        if incomplete:
            check(self.lib.evoamd_seed_states_ex(self._h, A, _lib.SEED_INCOMPLETE, *ptrs))
        else:
            check(self.lib.evoamd_seed_states(self._h, A, *ptrs))
        return out

    def seed_states_beam(self, max_active, beam, want_path=False):
        """K^n seeded on the device by a beam of partial states (evoamd_seed_states_beam;
        evo_amd.variational.seed_states_beam_host is its NumPy mirror): the law of seed_states with the ``beam`` best
        partial states kept per step and all of them expanded; ``beam`` = 1 is seed_states bit for bit.  Complete data
        only.  ``want_path``: returns (path int32 (N, max_active), the path of the rank-0 state of the last step, and
        lpj_path (N, max_active), the rank-0 score of each step), else None.  EvoAmdError naming the rule, with K^n left
        as it was, for everything seed_states refuses, resident masks, ``beam`` < 1, > S // max_active or > 16."""
        A, out, ptrs = self._seed_out(max_active, want_path)
        check(self.lib.evoamd_seed_states_beam(self._h, A, int(beam), *ptrs))
        return out

    # ---- samples from the model ------------------------------------------------------------
    def generate(self, model, N, seed, Wt, pies, mus=None, F=None, sigma=1.0, first_index=0, s=None,
                 keep=("s", "z", "y_mean")):
        """N samples drawn on the device (evoamd_generate; evo_amd.models.generate_counter is the NumPy mirror): ``Wt``
        (H, D) = W^T, ``pies`` (H), ES3C ``mus`` (H) and ``F`` (H, H) with F F^T = Psi, ``sigma`` the noise's standard
        deviation.  ``s`` bool (N, H): taken, not drawn.  ``keep``: which outputs besides y stay on the device for
        download_generated.  Needs no configure() and leaves a configured EM state untouched."""
        from .models.generate import pack_words
        sssc = model not in (MODEL_BSC, "bsc", "BSC")
        Wt, pies = as_f64(Wt), as_f64(pies)
        H, D = Wt.shape
        assert pies.shape == (H,), pies.shape
        if sssc:
            mus, F = as_f64(mus), as_f64(F)
            assert mus.shape == (H,) and F.shape == (H, H), (mus.shape, F.shape)
        words = None
        if s is not None:
            assert np.shape(s) == (int(N), H), (np.shape(s), (int(N), H))
            words = pack_words(s)
        bits = 0
        for name in keep:
            if name != "y":
                bits |= _lib.GEN_KEEP[name]
        check(self.lib.evoamd_generate(
            self._h, MODEL_SSSC if sssc else MODEL_BSC, int(N), D, H, int(seed) & (2 ** 64 - 1),
            int(first_index) & (2 ** 64 - 1), dptr(Wt), dptr(pies), dptr(mus) if sssc else None, dptr(F) if sssc else None,
            float(sigma), None if words is None else words.ctypes.data_as(_lib._c_u64p), bits))
        self._gen_shape = (int(N), D, H)

    def download_generated(self, what):
        """One output of the last generate(): "y" / "y_mean" (N, D), "z" (N, H; ES3C), "s" bool (N, H).  EvoAmdError for an
        output that call did not keep."""
        from .models.generate import unpack_words
        N, D, H = getattr(self, "_gen_shape", (1, 1, 1))
        if what == "s":
            out = np.empty((N, (H + 63) // 64), dtype=np.uint64)
        else:
            out = np.empty((N, H if what == "z" else D), dtype=np.float64)
        check(self.lib.evoamd_download_generated(self._h, _lib.GEN_WHAT[what], out.ctypes.data_as(ctypes.c_void_p)))
        return unpack_words(out, H) if what == "s" else out

    def upload_lpj(self, lpj):
        lpj = as_f64(lpj)
        assert lpj.shape == (self.N, self.L)
        check(self.lib.evoamd_upload_lpj(self._h, dptr(lpj)))

    def download_lpj(self, out=None):
        if out is None:
            out = np.empty((self.N, self.L), dtype=np.float64)
        assert out.shape == (self.N, self.L) and out.dtype == np.float64 and out.flags.c_contiguous
        check(self.lib.evoamd_download_lpj(self._h, dptr(out)))
        return out

    # ---- parameters ----------------------------------------------------------------------
    def set_params_bsc(self, W, pi, sigma):
        W = as_f64(W)
        assert W.shape == (self.D, self.H)
        ljc = ctypes.c_double()
        check(self.lib.evoamd_set_params_bsc(self._h, dptr(W), float(pi), float(sigma), ctypes.byref(ljc)))
        self.ljc = ljc.value
        return self.ljc

    def set_params_sssc(self, W, pies, mus, Psi, sigma2):
        W, pies, mus, Psi = as_f64(W), as_f64(pies), as_f64(mus), as_f64(Psi)
        assert W.shape == (self.D, self.H) and pies.shape == (self.H,) and mus.shape == (self.H,)
        assert Psi.shape == (self.H, self.H)
        ljc = ctypes.c_double()
        check(self.lib.evoamd_set_params_sssc(self._h, dptr(W), dptr(pies), dptr(mus), dptr(Psi), float(sigma2),
                                              ctypes.byref(ljc)))
        self.ljc = ljc.value
        return self.ljc

    # ---- E-step --------------------------------------------------------------------------
    def lpj_resident(self):
        check(self.lib.evoamd_lpj_resident(self._h))

    def lpj_candidates(self, cand, counts, want_lpj=True):
        b = as_bool_bytes(cand)
        assert b.shape == (self.N, self.Cmax, self.H), (b.shape, (self.N, self.Cmax, self.H))
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        assert counts.shape == (self.N,)
        out = np.empty((self.N, self.Cmax), dtype=np.float64) if want_lpj else None
        check(self.lib.evoamd_lpj_candidates(self._h, u8ptr(b), i32ptr(counts), self.Cmax,
                                             dptr(out) if want_lpj else None))
        return out

    def set_candidates(self, cand, counts, lpj):
        b = as_bool_bytes(cand)
        assert b.shape == (self.N, self.Cmax, self.H)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        lpj = as_f64(lpj)
        assert lpj.shape == (self.N, self.Cmax)
        check(self.lib.evoamd_set_candidates(self._h, u8ptr(b), i32ptr(counts), self.Cmax, dptr(lpj)))

    def lpj_shared(self, states):
        b = as_bool_bytes(states)
        assert b.ndim == 2 and b.shape[1] == self.H
        out = np.empty((self.N, b.shape[0]), dtype=np.float64)
        check(self.lib.evoamd_lpj_shared(self._h, u8ptr(b), b.shape[0], dptr(out)))
        return out

    def lpj_single(self, y, states, x_infr=None):
        y = as_f64(y)
        b = as_bool_bytes(states)
        assert y.shape == (self.D,) and b.ndim == 2 and b.shape[1] == self.H
        out = np.empty(b.shape[0], dtype=np.float64)
        flags = np.zeros(3, dtype=np.int32)
        if x_infr is None:
            check(self.lib.evoamd_lpj_single(self._h, dptr(y), u8ptr(b), b.shape[0], dptr(out), i32ptr(flags)))
        else:
            m = as_bool_bytes(x_infr)
            assert m.shape == (self.D,)
            check(self.lib.evoamd_lpj_single_masked(self._h, dptr(y), u8ptr(m), u8ptr(b), b.shape[0], dptr(out),
                                                    i32ptr(flags)))
        return out, flags

    def upload_masks(self, x_infr, x=None):
        """EBSC incomplete data: reliable entries x_infr (N, D) and keep-mask x (default x_infr); None clears."""
        if x_infr is None:
            check(self.lib.evoamd_upload_masks(self._h, None, None))
            self.has_masks = False
            return
        self.has_masks = True
        mi = as_bool_bytes(x_infr)
        mx = as_bool_bytes(x_infr if x is None else x)
        assert mi.shape == (self.N, self.D) and mx.shape == (self.N, self.D)
        check(self.lib.evoamd_upload_masks(self._h, u8ptr(mi), u8ptr(mx)))

    def upload_yrec(self, y_rec):
        y_rec = as_f64(y_rec)
        assert y_rec.shape == (self.N, self.D)
        check(self.lib.evoamd_upload_yrec(self._h, dptr(y_rec)))

    def set_reliable_fraction(self, r):
        """Mean reliable entries per datapoint over all ranks (bsc.py:113-118,266-272); None / negative: complete data."""
        check(self.lib.evoamd_set_reliable_fraction(self._h, -1.0 if r is None else float(r)))

    def vary_kn(self, Mprime, want_sums=True):
        sums = np.zeros(2, dtype=np.float64)
        check(self.lib.evoamd_vary_kn(self._h, int(Mprime), dptr(sums) if want_sums else None))
        return sums

    def evolve_randflip(self, n_parents, n_children, seed, fit_parents=True):
        """fitparents / randparents + randflip for one generation on the device (evoamd_evolve_randflip); fills and
        evaluates the candidate batch, slot p * n_children + i = child i of the p-th drawn parent, nothing de-duplicated.
        Counter-based stream (csrc/kernels_evolve.hpp, "THE STREAM"): evo_amd.variational.evolve_randflip_counter is the
        NumPy mirror, bit for bit wherever the float32 race keys of the parent draw are further apart than its margin."""
        check(self.lib.evoamd_evolve_randflip(self._h, int(n_parents), int(n_children), int(seed) & (2 ** 64 - 1),
                                              1 if fit_parents else 0))

    def estep(self, n_parents, n_children, seed, fit_parents, Mprime):
        """lpj of K^n -> randflip children -> their lpj -> vary_Kn in one library call (one fused kernel where the shape
        allows it, else the separate passes; same results).  Returns True when the fused kernel ran."""
        fused = ctypes.c_int(0)
        check(self.lib.evoamd_estep(self._h, int(n_parents), int(n_children), int(seed) & (2 ** 64 - 1),
                                    1 if fit_parents else 0, int(Mprime), ctypes.byref(fused)))
        return bool(fused.value)

    def estep_counters(self):
        """{fused_calls, separate_calls, deferred (datapoints the fused kernel left to its second launch), -} of evoamd_estep."""
        out = (ctypes.c_int64 * 4)()
        check(self.lib.evoamd_estep_counters(self._h, out))
        return dict(zip(("fused_calls", "separate_calls", "deferred", "unused"), [int(v) for v in out]))

    MUTATIONS = {"randflip": 0, "sparseflip": 1, "cross": 2, "cross_randflip": 3, "cross_sparseflip": 4}

    def evolve_states(self, mutation, n_parents, n_children, n_generations, seed, fit_parents=True, sparseness=0.0,
                      bitflip_prob=None):
        """All EA operators / generations on the device (eas.py:153-313); fills and evaluates the candidate batch: the new
        unique states of every generation, np.unique's row order within one.  Counter-based stream
        (csrc/kernels_evolve.hpp, "THE STREAM"): evo_amd.variational.evolve_states_counter is the NumPy mirror, bit for
        bit wherever the float32 race keys of the parent draws are further apart than its margin."""
        check(self.lib.evoamd_evolve_states(self._h, self.MUTATIONS[mutation], 1 if fit_parents else 0, int(n_parents),
                                            int(n_children), int(n_generations), int(seed) & (2 ** 64 - 1),
                                            float(sparseness), float("nan") if bitflip_prob is None else float(bitflip_prob)))

    def refine_states(self, n_iterations, mutation, n_parents, n_children, n_generations, seed0, seed_stride=1,
                      fit_parents=True, sparseness=0.0, bitflip_prob=None, Mprime=None, check_every=8, patience=0,
                      min_sub=0.0):
        """K^n refined at fixed Theta (evoamd_refine_states): one pass over the resident K^n, then ``n_iterations`` x
        (children with seed ``seed0 + t * seed_stride``, their lpj, selection with ``Mprime``, default S) -- what
        lpj_resident() followed by that many evolve_randflip / evolve_states + vary_kn calls compute, bit for bit,
        without a host wait in between and without a statistics pass.  ``patience`` > 0: after every ``check_every``
        iterations the loop ends once the last ``patience`` iterations all swapped at most ``min_sub`` states per
        datapoint.  Returns (trace (n_done, 3), n_done): row t = (Fs, new unique states, swapped states) of iteration t."""
        T = int(n_iterations)
        trace = np.zeros((max(T, 1), 3), dtype=np.float64)
        n_done = ctypes.c_int(0)
        mask = 2 ** 64 - 1
        check(self.lib.evoamd_refine_states(
            self._h, T, self.MUTATIONS[mutation], 1 if fit_parents else 0, int(n_parents), int(n_children),
            int(n_generations), int(seed0) & mask, int(seed_stride) & mask, float(sparseness),
            float("nan") if bitflip_prob is None else float(bitflip_prob), self.S if Mprime is None else int(Mprime),
            int(check_every), int(patience), float(min_sub), dptr(trace), ctypes.byref(n_done)))
        return trace[:n_done.value], n_done.value

    def _sweep_nb(self, neighbourhood, incomplete, score_key, want_scores=False):
        """The flags of an _nb sweep call, the dict it returns -- an array per key of the neighbourhood, the three flip
        keys None with "swap", no swap key with "flip", a "score" key only with ``score_key`` (an array with
        ``want_scores``, else None) -- and the evoamd_sweep_out that points at the arrays."""
        if neighbourhood not in _lib.SWEEP_NEIGHBOURHOODS:
            raise ValueError("sweep: neighbourhood = %r must be one of 'flip', 'swap', 'both'" % (neighbourhood,))
        flags = _lib.SWEEP_NEIGHBOURHOODS[neighbourhood] | (_lib.SWEEP_INCOMPLETE if incomplete else 0)
        N, flips = self.N, neighbourhood != "swap"
        res = {}
        if score_key:
            res["score"] = np.empty((N, self.Cmax), dtype=np.float64) if want_scores else None
        res.update(best_flip=np.empty(N, dtype=np.int32) if flips else None,
                   gain=np.empty(N, dtype=np.float64) if flips else None,
                   n_capped=np.empty(N, dtype=np.int32) if flips else None)
        if neighbourhood != "flip":
            res.update(best_swap=np.empty((N, 2), dtype=np.int32), swap_gain=np.empty(N, dtype=np.float64),
                       n_capped_swap=np.empty(N, dtype=np.int32))
        out = _lib.SweepOut()
        for name, a in res.items():
            if a is not None:
                setattr(out, name, dptr(a) if a.dtype == np.float64 else i32ptr(a))
        return flags, res, out

    def sweep_propose(self, n_parents, n_keep, want_scores=True, incomplete=False, neighbourhood="flip"):
        """One sweep's proposals of the local search on K^n (evoamd_sweep_propose; csrc/kernels_sweep.hpp has the law,
        evo_amd.variational.sweep_states_host is the NumPy mirror): the resident rows are evaluated, every one-flip
        neighbour of the ``n_parents`` best states of each datapoint is scored, the ``n_keep`` best per parent that K^n
        does not hold go to the resident candidate batch and are evaluated by the model's lpj kernels -- vary_kn() or
        download_candidates() can follow.  Returns a dict: "score" (N, Cmax) the score of every emitted row, NaN elsewhere
        (None without ``want_scores``), "best_flip" int32 (N,) and "gain" (N,) of the best state's best scored neighbour
        (-1 / -inf without one; gain <= 0: no better one-flip neighbour outside K^n), "n_capped" int32 (N,).  EvoAmdError
        naming the rule, with the context as it was, without Theta, data or K^n, for incomplete data without
        ``incomplete``, the background unit, the float32 mode, bsc_direct, n_parents outside [1, min(S, 64)], n_keep < 1
        or n_parents * n_keep > Cmax.  ``incomplete`` permits incomplete data (evoamd_sweep_propose_ex,
        EVOAMD_SWEEP_INCOMPLETE): with masks resident (upload_masks) every datapoint's neighbours are scored on its
        reliable entries, its Gram quantities formed from W and the mask (sweep_states_host with ``x_infr``); without masks
        the flag changes nothing.
        ``neighbourhood``: "flip" (the call above), "swap" or "both" (evoamd_sweep_propose_nb; csrc/kernels_sweep_swap.hpp
        has the law, evo_amd.variational.swap_states_host is the mirror): every swap of a parent -- one active latent a off,
        one inactive latent j on -- that K^n does not hold is scored and the ``n_keep`` best per parent are appended behind
        the flip rows ("both": 2 * n_parents * n_keep <= Cmax).  The dict gains "best_swap" int32 (N, 2) = (a, j) of the best
        state's best scored swap or (-1, -1), "swap_gain" (N,) (-inf without one) and "n_capped_swap" int32 (N,), the
        parents above the seeding cap, none of whose swaps is scored; with "swap" the three flip keys are None.  Swaps on
        incomplete data (``incomplete`` or masks resident) are refused.  Every neighbourhood goes through
        evoamd_sweep_propose_nb, which without a swap bit is exactly evoamd_sweep_propose_ex."""
        flags, res, out = self._sweep_nb(neighbourhood, incomplete, True, want_scores)
        check(self.lib.evoamd_sweep_propose_nb(self._h, int(n_parents), int(n_keep), flags, ctypes.byref(out)))
        return res

    def sweep_states(self, n_sweeps, n_parents=1, n_keep=None, Mprime=None, stop_when_quiet=True, incomplete=False,
                     neighbourhood="flip"):
        """``n_sweeps`` x (sweep_propose, selection with ``Mprime``, default S) in one library call (evoamd_sweep_states):
        bit for bit what the separate calls give, the lpj rows stay those of the resident K^n.  ``n_keep`` None: Cmax //
        n_parents.  ``stop_when_quiet``: the loop ends after a sweep that swapped nothing.  Returns (trace (n_done, 3),
        n_done, certificate): row t = (Fs, new unique states, swapped states) of sweep t; the certificate is the dict of
        sweep_propose without "score", for the last sweep run (after a quiet one: the final K^n).  ``incomplete`` as for
        sweep_propose (evoamd_sweep_states_ex).  ``neighbourhood`` as for sweep_propose (evoamd_sweep_states_nb): with
        "both" ``n_keep`` None is Cmax // (2 n_parents), "quiet" means that neither stage's rows swapped anything in, and
        the certificate gains the swap keys."""
        T = int(n_sweeps)
        P = int(n_parents)
        q = self.Cmax // max(P * (2 if neighbourhood == "both" else 1), 1) if n_keep is None else int(n_keep)
        trace = np.zeros((max(T, 1), 3), dtype=np.float64)
        n_done = ctypes.c_int(0)
        flags, res, out = self._sweep_nb(neighbourhood, incomplete, False)
        check(self.lib.evoamd_sweep_states_nb(
            self._h, T, P, q, self.S if Mprime is None else int(Mprime), 1 if stop_when_quiet else 0, flags, dptr(trace),
            ctypes.byref(n_done), ctypes.byref(out)))
        return trace[:n_done.value], n_done.value, res

    def neighbour_bound(self, n_parents, incomplete=False):
        """The neighbourhood bound under the Theta, K^n and data on the device (evoamd_neighbour_bound;
        csrc/kernels_nbound.hpp has the law, evo_amd.variational.neighbour_bound_host is the NumPy mirror): the resident
        rows are evaluated, every one-flip neighbour of the ``n_parents`` best states of each datapoint that K^n does not
        hold is scored as a flip sweep scores it, each state once, and the scores are summed.  Returns a dict of (N,)
        arrays: "F" (the bound of K^n without ljc), "M" (log of the neighbours' summed mass, -inf without one), "F_plus" =
        logaddexp(F, M), "gap" = F_plus - F >= 0, "mass_outside" = exp(M - F_plus), "n_states" and "n_capped" (int32),
        "best_score", "best_parent" and "best_flip" (int32; -inf / -1 / -1 without a scored neighbour), and the scalars
        "sum" (of F_plus over the datapoints with an estimate) and "count" (their number); a datapoint with "bad weights"
        has NaN in the real-valued arrays.  Deterministic; K^n, the candidate batch and the statistics rows are not
        written.  EvoAmdError naming the rule, with the context as it was, without Theta, data or K^n, for incomplete data
        without ``incomplete`` (EVOAMD_NBOUND_INCOMPLETE, a permission as for sweep_propose), the background unit, the
        float32 mode, bsc_direct and n_parents outside [1, S]."""
        N = self.N
        res = {name: np.empty(N, dtype=np.float64) for name in ("F", "M", "best_score")}
        res.update({name: np.empty(N, dtype=np.int32) for name in ("n_states", "n_capped", "best_parent", "best_flip")})
        total = np.zeros(2, dtype=np.float64)
        out = _lib.NboundOut()
        for name, a in res.items():
            setattr(out, name, dptr(a) if a.dtype == np.float64 else i32ptr(a))
        out.sum = dptr(total)
        check(self.lib.evoamd_neighbour_bound(self._h, int(n_parents), _lib.NBOUND_INCOMPLETE if incomplete else 0,
                                              ctypes.byref(out)))
        with np.errstate(invalid="ignore"):
            res["F_plus"] = np.logaddexp(res["F"], res["M"])
            res["gap"] = res["F_plus"] - res["F"]
            res["mass_outside"] = np.exp(res["M"] - res["F_plus"])
        res["sum"], res["count"] = float(total[0]), int(total[1])
        return res

    def ais_loglik(self, betas, n_chains=16, seed=0, first_index=0, reverse=False, s_start=None, keep_states=False,
                   admit=False, Mprime=1, incomplete=False):
        """Annealed importance sampling under the Theta and data on the device (evoamd_ais_loglik; csrc/kernels_ais.hpp
        has the law, evo_amd.models.ais_log_likelihood_counter is the NumPy mirror).  ``betas``: the float64 schedule of
        T + 1 values from 0 to 1.  Returns a dict of (N,) arrays "ll" (forward: a lower bound on log p(y_n) - ljc in
        expectation; ``reverse``: an upper bound, provided row n of ``s_start`` (bool (N, H)) is an exact posterior
        sample), "ess", "log_w_mean", "log_w_min", "log_w_max", "n_flips" (int64) and the scalar "sum" of ll;
        ``keep_states`` adds "log_w" (N, C), "final" (uint8, N x C x ceil(H / 8), np.packbits layout) and "chain_flips"
        (int32 (N, C)); ``admit`` (forward only) runs the final states of the first min(C, Cmax) chains through the
        candidate lpj kernels and the selection with ``Mprime`` and adds "F_before", "F_after" (N,) and the scalars
        "S_nunique" and "S_sub" (sums over the datapoints, as vary_kn).  Without ``admit`` K^n, lpj, the candidate batch
        and the statistics rows are not written.  EvoAmdError naming the rule, before anything is written, for ES3C, the
        float32 mode, the background unit, bsc_direct, masks resident, H > 1024, n_chains < 1, betas that do not start at
        0, end at 1 or that descend, reverse without s_start and admit with reverse.  ``incomplete=True`` is a permission:
        with masks resident the chains run on the datapoint's own G(n) over its reliable entries (the law's INCOMPLETE
        DATA; a D whose column and list do not fit into LDS is refused), without masks it changes nothing."""
        from .models.generate import pack_words
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        if betas.ndim != 1 or betas.size < 2:
            raise ValueError("betas must be a 1-d array of T + 1 >= 2 values")
        N, H, C, T = self.N, self.H, int(n_chains), betas.size - 1
        HW = (H + 63) // 64
        words = None
        if s_start is not None:
            s_start = np.asarray(s_start)
            if s_start.shape != (N, H) or s_start.dtype != np.bool_:
                raise ValueError("s_start must be a bool array of shape (N, H)")
            words = pack_words(s_start)
        res = {name: np.empty(N, dtype=np.float64) for name in ("ll", "ess", "log_w_mean", "log_w_min", "log_w_max")}
        res["n_flips"] = np.empty(N, dtype=np.int64)
        total, sums = np.zeros(1), np.zeros(2)
        out = _lib.AisOut()
        for name in ("ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
            setattr(out, name, dptr(res[name]))
        out.n_flips = res["n_flips"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        out.sum = dptr(total)
        fin = None
        if keep_states and C >= 1:
            res["log_w"] = np.empty((N, C))
            res["chain_flips"] = np.empty((N, C), dtype=np.int32)
            fin = np.empty((N * C, HW), dtype=np.uint64)
            out.log_w, out.chain_flips = dptr(res["log_w"]), i32ptr(res["chain_flips"])
            out.final_words = fin.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        if admit:
            res["F_before"], res["F_after"] = np.empty(N), np.empty(N)
            out.F_before, out.F_after, out.admit_sums = dptr(res["F_before"]), dptr(res["F_after"]), dptr(sums)
        flags = ((_lib.AIS_REVERSE if reverse else 0) | (_lib.AIS_ADMIT if admit else 0)
                 | (_lib.AIS_INCOMPLETE if incomplete else 0))
        check(self.lib.evoamd_ais_loglik(
            self._h, C, T, dptr(betas), int(seed) & (2 ** 64 - 1), int(first_index) & (2 ** 64 - 1), flags,
            None if words is None else words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(Mprime), ctypes.byref(out)))
        if fin is not None:  # the MSB-first words as bytes are the np.packbits layout
            nb = (H + 7) // 8
            res["final"] = np.ascontiguousarray(fin.astype(">u8").view(np.uint8).reshape(N * C, HW * 8)[:, :nb]).reshape(-1)
        if admit:
            res["S_nunique"], res["S_sub"] = float(sums[0]), float(sums[1])
        res["sum"] = float(total[0])
        return res

    def ais_posterior(self, betas, n_chains=16, n_keep=4, seed=0, first_index=0, mean=False, keep_chains=False, block=0,
                      incomplete=False, index=None, admit=False, Mprime=1):
        """Posterior expectations that do not start from K^n, under the Theta and data on the device (evoamd_ais_posterior;
        csrc/kernels_ais_post.hpp has the law, evo_amd.models.ais_posterior_counter is the NumPy mirror): the forward
        chains of ais_loglik, continued by ``n_keep`` - 1 further scans at beta = 1, each chain weighted by its w.
        ``betas``: the float64 schedule of T + 1 values from 0 to 1.  Returns a dict with "p" and "p_se" (N, H: the weighted,
        Rao-Blackwellised marginals E_p[s_h | y_n] and their delta-method standard errors), "count" (N: sum_h p_nh),
        "map_lpj" (N) and "map_state" (uint8 (N, ceil(H / 8)), np.packbits layout: the best state any chain visited after
        a kept scan), and "ll", "ess", "log_w_mean", "log_w_min", "log_w_max", "n_flips" (int64) as ais_loglik gives them
        for forward chains (n_flips counts the kept scans too).  ``mean`` adds "mean" (N, D) = p W^T; ``keep_chains`` adds
        "log_w", "chain_map_lpj" (N, C), "rb" (N, C, H: the chains' averaged conditionals), "chain_map_state" (uint8 (N, C,
        ceil(H / 8))) and "chain_flips" (int32 (N, C)).  ``block``: datapoints per block of the per-chain rows (0: as many
        as 256 MiB hold); the results do not depend on it.  K^n, lpj, the candidate batch, the statistics rows and y_hat
        are not written.  EvoAmdError naming the rule, before anything is written, for ES3C, the float32 mode, the
        background unit, bsc_direct, masks resident, H > 1024, n_chains < 1, n_keep < 1, betas that do not start at 0, end
        at 1 or that descend, and a block above 256 MiB.  ``incomplete=True`` (evoamd_ais_posterior_ex) is a permission:
        with masks resident the chains run on the datapoint's own G(n) over its reliable entries, and "mean" covers every
        entry, the missing ones included; without masks it changes nothing.

        ``index`` (evoamd_ais_posterior_sel): a 1-d integer array of datapoints of this context, strictly ascending within
        [0, N) -- the chains run for these alone and every per-datapoint array has len(index) rows in list order, row i bit
        for bit row index[i] of the call without ``index`` at the same seed (``first_index`` keeps its meaning: the stream
        of row i is that of data set index first_index + index[i]).  ValueError naming the first offender otherwise.  An
        empty list returns empty arrays without a library call.
        ``admit=True``: after the chains, per listed datapoint the chains' best states -- ranked by chain_map_lpj, the
        all-zero state, repeats and states K^n holds dropped, at most Cmax (csrc/kernels_ais_post.hpp, ADMISSION;
        evo_amd.models.ais_admit_candidates_host is the mirror) -- become the candidate batch (count 0 elsewhere), and the
        model's candidate lpj and the selection with ``Mprime`` run as in an E-step.  Adds "F_before", "F_after",
        "n_distinct", "n_new", "n_proposed", "n_admitted" (int32), "map_held_before", "map_held_after" (bool), one row per
        listed datapoint, and the scalars "S_nunique" and "S_sub" (sums over the datapoints, as vary_kn).  Needs K^n on
        the device and Mprime in [1, S].  Out of scope: ``index`` for ais_loglik, ES3C, the float32 mode, the background
        unit, H > 1024, resident handles for p / mean, choosing the list on the device."""
        betas = np.ascontiguousarray(betas, dtype=np.float64)
        if betas.ndim != 1 or betas.size < 2:
            raise ValueError("betas must be a 1-d array of T + 1 >= 2 values")
        N, H, D, C, T = self.N, self.H, self.D, int(n_chains), betas.size - 1
        idx = None
        if index is not None:
            from .models.ais import check_index
            idx = check_index(index, N)
            N = idx.size  # the rows of every output
        HW, nb = (H + 63) // 64, (H + 7) // 8
        u64p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))  # noqa: E731
        res = {"p": np.empty((N, H)), "p_se": np.empty((N, H))}
        res.update({name: np.empty(N) for name in ("count", "map_lpj", "ll", "ess", "log_w_mean", "log_w_min", "log_w_max")})
        res["n_flips"] = np.empty(N, dtype=np.int64)
        out = _lib.AisPostOut()
        for name, a in res.items():
            if a.dtype == np.float64:
                setattr(out, name, dptr(a))
        out.n_flips = res["n_flips"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        map_words = np.empty((N, HW), dtype=np.uint64)
        out.map_state = u64p(map_words)
        if mean:
            res["mean"] = np.empty((N, D))
            out.mean = dptr(res["mean"])
        chain_words = None
        if keep_chains and C >= 1:
            res["log_w"], res["chain_map_lpj"], res["rb"] = np.empty((N, C)), np.empty((N, C)), np.empty((N, C, H))
            res["chain_flips"] = np.empty((N, C), dtype=np.int32)
            chain_words = np.empty((N * C, HW), dtype=np.uint64)
            out.log_w, out.chain_map_lpj, out.rb = dptr(res["log_w"]), dptr(res["chain_map_lpj"]), dptr(res["rb"])
            out.chain_flips, out.chain_map_state = i32ptr(res["chain_flips"]), u64p(chain_words)
        flags = _lib.AIS_INCOMPLETE if incomplete else 0
        if idx is None and not admit:
            check(self.lib.evoamd_ais_posterior_ex(self._h, C, T, int(n_keep), dptr(betas), int(seed) & (2 ** 64 - 1),
                                                   int(first_index) & (2 ** 64 - 1), int(block), flags, ctypes.byref(out)))
        else:
            sel = _lib.AisPostSelOut()
            sel.post = out
            sums = np.zeros(2)
            if admit:
                res["F_before"], res["F_after"] = np.empty(N), np.empty(N)
                sel.F_before, sel.F_after, sel.admit_sums = dptr(res["F_before"]), dptr(res["F_after"]), dptr(sums)
                counts = ("n_distinct", "n_new", "n_proposed", "n_admitted", "map_held_before", "map_held_after")
                for name in counts:
                    res[name] = np.zeros(N, dtype=np.int32)
                    setattr(sel, name, i32ptr(res[name]))
            if idx is None or idx.size:  # (an empty list: empty arrays, no library call)
                check(self.lib.evoamd_ais_posterior_sel(
                    self._h, C, T, int(n_keep), dptr(betas), int(seed) & (2 ** 64 - 1), int(first_index) & (2 ** 64 - 1),
                    int(block), flags | (_lib.AIS_ADMIT if admit else 0),
                    None if idx is None else idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 0 if idx is None else idx.size,
                    int(Mprime), ctypes.byref(sel)))
            if admit:
                for name in ("map_held_before", "map_held_after"):
                    res[name] = res[name].astype(np.bool_)
                res["S_nunique"], res["S_sub"] = float(sums[0]), float(sums[1])
        # the MSB-first words as bytes are the np.packbits layout
        as_bytes = lambda w: np.ascontiguousarray(w.astype(">u8").view(np.uint8).reshape(w.shape[0], HW * 8)[:, :nb])  # noqa: E731
        res["map_state"] = as_bytes(map_words)
        if chain_words is not None:
            res["chain_map_state"] = as_bytes(chain_words).reshape(N, C, nb)
        return res

    def ais_post_admit_probe(self, chain_map_lpj, chain_map_state, index=None):
        """TEST-ONLY (evoamd_ais_post_admit_probe): the emission kernel of ais_posterior(admit=True) alone, on the caller's
        ``chain_map_lpj`` (n, C) and ``chain_map_state`` (bool (n, C, H)) for the rows ``index`` (None: the N datapoints),
        against the resident K^n.  The candidate batch is left installed and evaluated (download_candidates() reads it).
        Returns a dict: "n_distinct", "n_new", "n_proposed" (int32 (n,)), "map_held" (bool (n,)) and "digests" (uint64 (N,
        Cmax), rows below a datapoint's count; None when the context keeps no digests)."""
        from .models.ais import check_index
        from .models.generate import pack_words
        lpj = np.ascontiguousarray(chain_map_lpj, dtype=np.float64)
        st = np.asarray(chain_map_state, dtype=np.bool_)
        idx = None if index is None else check_index(index, self.N)
        n = self.N if idx is None else idx.size
        C = lpj.shape[1]
        assert lpj.shape == (n, C) and st.shape == (n, C, self.H), (lpj.shape, st.shape)
        words = np.ascontiguousarray(pack_words(st.reshape(n * C, self.H)))
        res = {name: np.zeros(n, dtype=np.int32) for name in ("n_distinct", "n_new", "n_proposed", "map_held")}
        dig = np.zeros((self.N, self.Cmax), dtype=np.uint64)
        used = ctypes.c_int(0)
        check(self.lib.evoamd_ais_post_admit_probe(
            self._h, dptr(lpj), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), C,
            None if idx is None else idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 0 if idx is None else idx.size,
            i32ptr(res["n_distinct"]), i32ptr(res["n_new"]), i32ptr(res["n_proposed"]), i32ptr(res["map_held"]),
            dig.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(used)))
        res["map_held"] = res["map_held"].astype(np.bool_)
        res["digests"] = dig if used.value else None
        return res

    SCORES = ("F", "entropy", "best", "k_best", "k_mean")

    def posterior_scores(self, what=SCORES):
        """Per-datapoint scores of the lpj rows and K^n on the device (evoamd_posterior_scores;
        evo_amd.variational.posterior_scores_host is the NumPy mirror): a dict with the (N) arrays ``what`` names --
        "F" = logsumexp_s lpj_ns (the bound per datapoint without ljc), "entropy" of q_n, "best" (int32: the first
        column of lpj with the row's maximum), "k_best" (int32: active latents of that state) and "k_mean" =
        sum_s q_ns |s_s|.  No pass runs; the EM state stays as it is."""
        what = tuple(what)
        for name in what:
            if name not in self.SCORES:
                raise ValueError("posterior_scores: unknown score %r" % (name,))
        out = {name: np.empty(self.N, dtype=np.int32 if name in ("best", "k_best") else np.float64) for name in what}
        ptr = {name: (i32ptr(a) if a.dtype == np.int32 else dptr(a)) for name, a in out.items()}
        check(self.lib.evoamd_posterior_scores(self._h, ptr.get("F"), ptr.get("entropy"), ptr.get("best"),
                                               ptr.get("k_best"), ptr.get("k_mean")))
        return out

    # ---- the dictionary resized (evo_amd.variational.remap_states_host is the NumPy mirror) -------
    def remap_latents(self, index):
        """K^n moved to the latent numbering ``index`` (int (H_new,): source latent or -1 for a new one) on the device
        (evoamd_remap_latents; csrc/kernels_remap.hpp has the law): gathered bits, first occurrences kept in place,
        collapsed slots filled from the enumeration of singletons and pairs.  The result waits in scratch of the context
        for adopt_remapped_states(); the resident K^n, lpj and every flag stay as they are.  Returns (n_replaced int32
        (N,), their sum).  EvoAmdError naming the rule, with the context as it was, for a bad index, a source named twice,
        the background unit not kept last, H_new (H_new + 1) / 2 < S (without the background unit) and an S above the
        LDS cap of the shape."""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        assert idx.ndim == 1 and idx.size >= 1, idx.shape
        n_rep = np.empty(self.N, dtype=np.int32)
        total = ctypes.c_int64(0)
        check(self.lib.evoamd_remap_latents(self._h, i32ptr(idx), idx.size, i32ptr(n_rep), ctypes.byref(total)))
        return n_rep, int(total.value)

    def adopt_remapped_states(self):
        """After configure() for H_new (same N and S): the states remap_latents() left become the resident K^n, as an upload
        of the same rows would make them.  EvoAmdError, with K^n as it was, when the geometry differs from the remap's or
        nothing waits (an adopt uses the states up)."""
        check(self.lib.evoamd_adopt_remapped_states(self._h))

    # ---- K^n resized (evo_amd.variational.resize_states_host is the NumPy mirror) ------------------
    def resize_states(self, S_new):
        """K^n at ``S_new`` states per datapoint, computed on the device from the resident K^n and its lpj rows
        (evoamd_resize_states; csrc/kernels_resize.hpp has the law): a shrink keeps the S_new best states in ascending old
        slot; a grow keeps every state in place and fills the new slots with the one-flip, then two-flip neighbours of the
        best state that the datapoint does not hold.  The result waits in scratch of the context for
        adopt_resized_states(); the resident K^n, lpj and every flag stay as they are.  Returns src_slot int32 (N, S_new):
        the old slot of every new slot, -1 for a fill.  EvoAmdError, with everything as it was, for what the law refuses
        (S_new < 1, S_new = S, above 1024, the bound Hv (Hv + 1) / 2 - 1 >= S_new on a grow, lpj rows that are not those of
        the resident K^n)."""
        S_new = int(S_new)
        src = np.empty((self.N, max(S_new, 1)), dtype=np.int32)
        check(self.lib.evoamd_resize_states(self._h, S_new, i32ptr(src)))
        return src

    def adopt_resized_states(self):
        """After configure() for S_new (same N and H): the states resize_states() left become the resident K^n, as an upload
        of the same rows would make them.  EvoAmdError, with K^n as it was, when the geometry differs from the resize's or
        nothing waits (an adopt uses the states up)."""
        check(self.lib.evoamd_adopt_resized_states(self._h))

    def latent_map_counts(self):
        """int64 (H,): the datapoints whose most probable state of K^n (first column of maximal lpj) has latent h on."""
        out = np.empty(self.H, dtype=np.int64)
        check(self.lib.evoamd_latent_map_counts(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def download_candidates(self):
        """(cand bool (N,Cmax,H), counts (N,), lpj (N,Cmax)) of the resident candidate batch."""
        cand = np.empty((self.N, self.Cmax, self.H), dtype=np.bool_)
        counts = np.empty(self.N, dtype=np.int32)
        lpj = np.empty((self.N, self.Cmax))
        check(self.lib.evoamd_download_candidates(self._h, u8ptr(cand.view(np.uint8)), i32ptr(counts), dptr(lpj)))
        return cand, counts, lpj

    def set_estep_counts(self, sum_nunique, sum_sub):
        check(self.lib.evoamd_set_estep_counts(self._h, float(sum_nunique), float(sum_sub)))

    # ---- statistics ----------------------------------------------------------------------
    def acc_size(self):
        return int(self.lib.evoamd_acc_size(self._h))

    def stats(self):
        """Packed accumulator (already all-reduced over RCCL when a communicator is attached)."""
        acc = np.empty(self.acc_size(), dtype=np.float64)
        check(self.lib.evoamd_stats(self._h, dptr(acc)))
        return acc

    LEARN_BITS = {"W": 1, "pies": 2, "pi": 2, "mus": 4, "sigma2": 8, "sigma": 8, "Psi": 16}
    DPAR = {"pre1": 0, "pil_bar": 1, "sigma2_inv": 2, "ljc": 3, "pi": 4, "sigma": 5, "sigma2": 6, "status": 7,
            "ljc_prev": 8, "n_gt2": 12, "n_gt4": 13, "n_gt8": 14}

    def mstep_device(self, to_learn, reconstruct=False, theta_to_host=True):
        """Statistics + Theta update on the device.  Returns (tail dict, scalar-parameter dict).
        reconstruct: also form the data estimate under the OLD Theta (fetch it with reconstruct()).
        theta_to_host=False: Theta^new is not copied into the host mailbox (get_params_* fetches it on demand)."""
        mask = (32 if reconstruct else 0) | (0 if theta_to_host else 64)
        for name in to_learn:
            mask |= self.LEARN_BITS[name]
        tail = np.zeros(8)
        dpar = np.zeros(16)
        rc = self.lib.evoamd_mstep_device(self._h, mask, dptr(tail), dptr(dpar))
        d = {k: dpar[i] for k, i in self.DPAR.items()}
        # ljc of the Theta the E-step ran with: the update kernels move it to ljc_prev
        d["ljc_estep"] = d["ljc_prev"] if (mask & 31) else d["ljc"]
        if rc == -6 and d["status"] in (1.0, 2.0):  # EVOAMD_E_SINGULAR from the Theta update: exactly singular H x H
            # system, or one so ill-conditioned that the update went non-finite (tail / dpar were delivered)
            raise SingularUpdate(self.lib.evoamd_last_error().decode(), dict(zip(TAIL, tail)), d)
        check(rc)
        return dict(zip(TAIL, tail)), d

    def inverse(self, A, B=None):
        """The M-step's H x H solver: returns (inv(A), inv(B) or None, device milliseconds)."""
        A = np.array(A, dtype=np.float64, order="C")
        assert A.shape == (self.H, self.H)
        Bc = None if B is None else np.array(B, dtype=np.float64, order="C")
        ms = ctypes.c_double()
        check(self.lib.evoamd_inverse(self._h, dptr(A), None if Bc is None else dptr(Bc), self.H, ctypes.byref(ms)))
        return A, Bc, ms.value

    def reconstruct(self):
        """(N, D) posterior-predictive estimate under the Theta / K^n of the last statistics pass."""
        out = np.empty((self.N, self.D))
        check(self.lib.evoamd_reconstruct(self._h, dptr(out)))
        return out

    def gemm_tn(self, A, B, sym_row0=-1):
        """C = A^T B through the statistics pass's f64 MFMA dispatch (A: K x M, B: K x Nc)."""
        A, B = as_f64(A), as_f64(B)
        assert A.shape[0] == B.shape[0]
        C = np.empty((A.shape[1], B.shape[1]))
        check(self.lib.evoamd_gemm_tn(self._h, dptr(A), dptr(B), dptr(C), A.shape[0], A.shape[1], B.shape[1],
                                      int(sym_row0)))
        return C

    def dense_probe(self, op, A, B, C, M, Nc, K, lda, ldb=0, ldc=0, A2=None, lda2=0, side=None, ldct=0, off_a=0, off_b=0,
                    off_c=0, same_operand=False, deterministic=False, sym_row0=-1, c_is_zero=False, accumulate=False,
                    mirror=True, spare=0, diag=False, guard=0):
        """TEST-ONLY (evoamd_dense_probe): one launch of a dense kernel through the launcher the hot path calls.  ``op`` is
        a name of _lib.DENSE_OPS; A, B, A2, C and side are whole padded 1-D buffers (``off`` elements, ``guard`` rows, the
        logical rows, ``guard`` rows, each ``ld`` long; float32 for the operands of the f32 ops and the C of rows_f32).
        Returns (C, side, route): copies of the two output buffers after the call and the launcher's route record as a
        dict (``route`` by its name in _lib.DENSE_ROUTES)."""
        o = _lib.DENSE_OPS.index(op)
        f32 = op in ("tn_f32", "rows_f32")
        ta, tc = (np.float32 if f32 else np.float64), (np.float32 if op == "rows_f32" else np.float64)
        colsum, nn = op.startswith("colsum"), op == "nn"

        def buf(x, dtype, off, rows, ld):
            x = np.ascontiguousarray(x, dtype=dtype)
            assert x.ndim == 1 and x.size == off + (rows + 2 * guard) * ld, (op, x.shape, off, rows, ld, guard)
            return x

        A = buf(A, ta, off_a, M if nn else K, lda)
        B = None if colsum or same_operand else buf(B, ta, off_b, K, ldb)
        A2 = buf(A2, ta, 0, M, lda2) if op == "rows_f32" else None
        C = buf(C, tc, off_c, 1 if colsum else M, ldc).copy()
        if nn and ldct > 0:
            side = buf(side, np.float64, 0, Nc, ldct).copy()
        elif diag:
            side = buf(side, np.float64, 0, M, 1).copy()
        else:
            side = None
        d = _lib.DenseDesc(o, M, Nc, K, lda, ldb, ldc, lda2, ldct, off_a, off_b, off_c, int(same_operand),
                           int(deterministic), int(sym_row0), int(c_is_zero), int(accumulate), int(mirror), int(spare),
                           int(diag), guard)
        r = _lib.DenseRoute()
        vp = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
        check(self.lib.evoamd_dense_probe(self._h, ctypes.byref(d), vp(A), vp(B), vp(A2), vp(C), vp(side), ctypes.byref(r)))
        route = {name: int(getattr(r, name)) for name, _ in _lib.DenseRoute._fields_}
        route["route"] = _lib.DENSE_ROUTES[route["route"]]
        return C, side, route

    def get_params_bsc(self):
        W = np.empty((self.D, self.H))
        pi, sigma = ctypes.c_double(), ctypes.c_double()
        check(self.lib.evoamd_get_params_bsc(self._h, dptr(W), ctypes.byref(pi), ctypes.byref(sigma)))
        return {"W": W, "pi": pi.value, "sigma": np.float64(sigma.value)}

    def get_params_sssc(self):
        W, Psi = np.empty((self.D, self.H)), np.empty((self.H, self.H))
        pies, mus = np.empty(self.H), np.empty(self.H)
        s2 = ctypes.c_double()
        check(self.lib.evoamd_get_params_sssc(self._h, dptr(W), dptr(pies), dptr(mus), dptr(Psi), ctypes.byref(s2)))
        return {"W": W, "pies": pies, "mus": mus, "Psi": Psi, "sigma2": np.float64(s2.value)}

    def restore_theta_backup(self):
        """Re-install the parameters the last E-step ran with (kept on the device by mstep_device(theta_to_host=False))."""
        check(self.lib.evoamd_restore_theta_backup(self._h))

    def free_energy_sum(self, lpj):
        lpj = as_f64(lpj)
        out = ctypes.c_double()
        check(self.lib.evoamd_free_energy(self._h, dptr(lpj), lpj.shape[0], lpj.shape[1], ctypes.byref(out)))
        return out.value

    def loglik_exact(self, background=False, chunk_states=0, per_datapoint=True, marginals=False):
        """Exact log-likelihood terms over all states of the H - background latents that vary (evoamd_loglik_exact; at
        most 32), enumerated on the device in chunks of ``chunk_states`` (0 = automatic) and folded into a running
        log-sum-exp per datapoint.  Returns (Fs, ll, marg): Fs = sum_n ll_n, ll (N) = logsumexp_s lpj_ns when
        ``per_datapoint``, marg (N, H) = E_p[s_h | y_n] when ``marginals``, else None.  Needs data and Theta on the
        device; K^n and everything else of the EM state stay as they are."""
        ll = np.empty(self.N) if per_datapoint else None
        marg = np.empty((self.N, self.H)) if marginals else None
        Fs = ctypes.c_double()
        check(self.lib.evoamd_loglik_exact(self._h, 1 if background else 0, int(chunk_states),
                                           None if ll is None else dptr(ll), None if marg is None else dptr(marg),
                                           ctypes.byref(Fs)))
        return Fs.value, ll, marg

    def acc_views(self, acc):
        return acc_views(acc, self.model, self.D, self.H)

    # ---- RCCL ----------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        lib = _lib.load()
        buf = np.zeros(128, dtype=np.uint8)
        check(lib.evoamd_comm_unique_id(u8ptr(buf)))
        return buf.tobytes()

    def comm_init(self, uid, rank, world):
        buf = np.frombuffer(uid, dtype=np.uint8).copy()
        assert buf.size == 128
        check(self.lib.evoamd_comm_init(self._h, u8ptr(buf), int(rank), int(world)))
        self.rank, self.world = int(rank), int(world)

    def comm_allreduce(self, values, op="sum"):
        a = np.atleast_1d(as_f64(values)).copy()
        check(self.lib.evoamd_comm_allreduce_host(self._h, dptr(a), a.size, 1 if op == "max" else 0))
        return a

    def comm_destroy(self):
        check(self.lib.evoamd_comm_destroy(self._h))
        self.world, self.rank = 1, 0

    # ---- overlapping image patches (evo_amd.utils.prepost) --------------------------------
    def patches_extract(self, img, ph, pw, shift=1):
        """img (H, W) or (H, W, C) -> Y (N, D) float64, the overlapping patches (conventions: evo_amd.utils.prepost)."""
        from .utils.prepost import patch_geometry
        img = as_f64(img)
        H, W, C = _image_hwc(img.shape)
        N, D = patch_geometry(H, W, C, ph, pw, shift)
        Y = np.empty((N, D), dtype=np.float64)
        check(self.lib.evoamd_patches_extract(self._h, dptr(img), H, W, C, int(ph), int(pw), int(shift), dptr(Y)))
        return Y

    def patches_merge(self, Y, shape, ph, pw, shift=1, method="mean", weights=None):
        """Y (N, D) -> image of ``shape`` ((H, W) or (H, W, C)), every element the NaN-skipping mean / median of its
        estimates.  A C-contiguous float64 Y (e.g. the transpose of an F-ordered (D, N) array) is passed without a copy.
        method="precision" with ``weights`` = the (N, D) variances V of the estimates: the precision-weighted mean
        (sum e / v) / (sum 1 / v), estimates that are NaN or whose variance is NaN or <= 0 skipped
        (evo_amd.utils.prepost.PrecisionMerger is the host mirror, bit for bit)."""
        from .utils.prepost import patch_geometry
        H, W, C = _image_hwc(shape)
        N, D = patch_geometry(H, W, C, ph, pw, shift)
        Y = as_f64(Y)
        if Y.shape != (N, D):
            raise ValueError("patches_merge: Y has shape %s, the geometry needs (%d, %d)" % (Y.shape, N, D))
        if (method == "precision") != (weights is not None):
            raise ValueError("patches_merge: method='precision' and weights (the variances) go together")
        if method == "precision":
            V = as_f64(weights)
            if V.shape != (N, D):
                raise ValueError("patches_merge: weights have shape %s, the geometry needs (%d, %d)" % (V.shape, N, D))
            out = np.empty(tuple(shape), dtype=np.float64)
            check(self.lib.evoamd_patches_merge_weighted(self._h, dptr(Y), dptr(V), H, W, C, int(ph), int(pw), int(shift),
                                                         dptr(out)))
            return out
        m = {"mean": 0, "median": 1}[method]
        out = np.empty(tuple(shape), dtype=np.float64)
        check(self.lib.evoamd_patches_merge(self._h, dptr(Y), H, W, C, int(ph), int(pw), int(shift), m, dptr(out)))
        return out

    # ---- the reconstruction kept on the device (evo_amd.models: resident_reconstruction=True) ----------
    def reconstruct_resident(self, x=None):
        """Make the selected reconstruction of the last statistics pass resident (nothing comes to the host): y where it
        is kept, the posterior-predictive estimate elsewhere.  ``x``: the (N, D) keep-mask of complete data (None or all
        False: every entry is estimated), uploaded once per array object; with incomplete data the masks of
        upload_masks are used and ``x`` is not read.  Like every resident array the mask is keyed on the array OBJECT: after
        an in-place edit of ``x`` the device keeps the old mask (while np.asarray of a handle reads the edited one) until
        Model.invalidate() / a new array object.  Returns a serial number: patches_merge_resident /
        download_reconstruction given another one refuse to hand out a newer reconstruction."""
        if x is None or self.has_masks:
            ptr = None
        else:
            tok = self._keep_token
            geom = (self.model, self.N, self.D)
            if tok is not None and tok[0] is x and tok[1] == geom and tok[2] == self._configures:
                ptr = _KEEP_RESIDENT if tok[3] else None
            else:
                mx = as_bool_bytes(x)
                assert mx.shape == (self.N, self.D), (mx.shape, self.N, self.D)
                used = bool(mx.any())
                self._keep_token = (x, geom, self._configures, used)
                ptr = u8ptr(mx) if used else None
        check(self.lib.evoamd_reconstruct_resident(self._h, ptr))
        self._rec_serial += 1
        return self._rec_serial

    def _check_serial(self, serial):
        if serial is not None and serial != self._rec_serial:
            raise EvoAmdError("the resident reconstruction on the device is a newer one (a later reconstruct_resident)")

    def download_reconstruction(self, serial=None):
        """y_hat (N, D) of the resident reconstruction; EvoAmdError once it is outdated."""
        self._check_serial(serial)
        out = np.empty((self.N, self.D))
        check(self.lib.evoamd_download_reconstruction(self._h, dptr(out)))
        return out

    def patches_merge_resident(self, shape, ph, pw, shift=1, method="mean", serial=None):
        """patches_merge over the resident selected reconstruction: only the image crosses to the host.  The geometry must
        give (N, D) of the configured context (ValueError)."""
        from .utils.prepost import patch_geometry
        H, W, C = _image_hwc(shape)
        N, D = patch_geometry(H, W, C, ph, pw, shift)
        if (N, D) != (self.N, self.D):
            raise ValueError("patches_merge_resident: the geometry needs (%d, %d), the resident reconstruction is (%d, %d)"
                             % (N, D, self.N, self.D))
        self._check_serial(serial)
        m = {"mean": 0, "median": 1}[method]
        out = np.empty(tuple(shape), dtype=np.float64)
        check(self.lib.evoamd_patches_merge_resident(self._h, H, W, C, int(ph), int(pw), int(shift), m, dptr(out)))
        return out

    # ---- posterior code readout (evo_amd.codes) ---------------------------------------------
    def posterior_codes(self, max_active=16, p_min=0.0):
        """The codes of the last statistics pass, compacted on the device: a PosteriorCodes with the ``max_active``
        (1 .. 64) most probable latents per datapoint among those with E_q[s_h] > ``p_min`` and the most probable
        state of K^n.  Only the compact arrays cross to the host.  EvoAmdError unless stats() (or a statistics-only
        mstep_device) ran since the last change of Theta, the data or K^n."""
        from .codes import PosteriorCodes
        N, A, sssc = self.N, int(max_active), self.model == MODEL_SSSC
        # (arguments the library refuses get 1-element arrays: it checks them before it writes anything)
        shape = (N, A) if 1 <= A <= 64 else (1, 1)
        idx = np.empty(shape, dtype=np.int32)
        p = np.empty(shape)
        m = np.empty(shape) if sssc else None
        nnz, map_slot = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
        map_q = np.empty(N)
        map_state = np.empty((N, (self.H + 7) // 8), dtype=np.uint8)
        check(self.lib.evoamd_posterior_codes(self._h, A, float(p_min), i32ptr(idx), dptr(p), dptr(m) if sssc else None,
                                              i32ptr(nnz), i32ptr(map_slot), dptr(map_q), u8ptr(map_state)))
        return PosteriorCodes(self.H, idx, p, m, nnz, map_slot, map_q, map_state, p_min=p_min)

    def download_posterior(self):
        """(Es, Ez): the dense (N, H) rows E_q[s_h] and, ES3C, E_q[s_h z_h] (else None) of the last statistics pass --
        what posterior_codes compacts.  Same preconditions."""
        Es = np.empty((self.N, self.H))
        Ez = np.empty((self.N, self.H)) if self.model == MODEL_SSSC else None
        check(self.lib.evoamd_download_posterior(self._h, dptr(Es), None if Ez is None else dptr(Ez)))
        return Es, Ez

    # ---- predictive uncertainty (evo_amd.models.predictive is the NumPy mirror) -----------------
    def predictive_moments(self, noise=True, want_mean=True, want_var=True, resident=False):
        """Posterior-predictive mean and variance of every entry under the Theta, K^n and lpj rows on the device
        (evoamd_predictive_moments; no statistics pass runs and the EM state stays as it is).  Returns (mean, var, info):
        float64 (N, D) arrays (None where not wanted) and info = {"n_singular", "n_skipped"}, the datapoints whose rows are
        NaN because a k x k system is singular / because they have no reliable entry.  EvoAmdError naming n and k for a
        state with more than 32 active latents, and for D > 512; nothing is downloaded then.  ``resident=True``: nothing
        is downloaded at all; mean and var are ResidentMoments handles of the buffers on the device
        (patches_merge_predictive merges them there) until the next call."""
        counters = (ctypes.c_int64 * 2)()
        self._pred_serial += 1  # (before the call: a failed one leaves nothing either)
        check(self.lib.evoamd_predictive_moments(self._h, 1 if noise else 0, counters))
        info = {"n_singular": int(counters[0]), "n_skipped": int(counters[1])}
        if resident:
            from .resident import ResidentMoments
            mean = ResidentMoments(self, self._pred_serial, (self.N, self.D), "mean")
            return (mean if want_mean else None), (mean.sibling("var") if want_var else None), info
        mean = np.empty((self.N, self.D)) if want_mean else None
        var = np.empty((self.N, self.D)) if want_var else None
        check(self.lib.evoamd_download_predictive(self._h, None if mean is None else dptr(mean),
                                                  None if var is None else dptr(var)))
        return mean, var, info

    def predictive_score(self, y_true, query, noise=True, per_entry=False):
        """Log predictive density and PIT of the entries ``query`` (bool (N, D)) names, at the values ``y_true`` (float64
        (N, D), read at the queried entries only), under the mixture over the Theta, K^n and lpj rows on the device
        (evoamd_predictive_score; csrc/kernels_predictive_score.hpp has the law, evo_amd.models.predictive_log_score_host
        is the NumPy mirror).  Returns a dict: "logp_n" (N,) the sum over the datapoint's scored entries, "count" (N,)
        int32, the scalars "sum" and "total_count" (reduced on the device), the counters "n_singular", "n_skipped",
        "n_not_queried" (datapoints without a scored entry: not visited) and "n_bad_values" (queried entries whose y_true
        is not finite) and, with ``per_entry``, "logp" and "pit" (N, D), NaN outside the scored entries.  Deterministic;
        no statistics pass runs and the EM state and the moments of predictive_moments stay as they are.  ValueError for
        wrong shapes; EvoAmdError naming the rule for EBSC without noise, D > 512, the float32 mode, and -- naming n and k
        -- a state with more than 32 active latents in a visited datapoint."""
        y_true = np.ascontiguousarray(y_true, dtype=np.float64)
        query = np.ascontiguousarray(np.asarray(query, dtype=bool).view(np.uint8))
        if y_true.shape != (self.N, self.D) or query.shape != (self.N, self.D):
            raise ValueError("predictive_score: y_true and query must be (N, D) = (%d, %d), got %r and %r"
                             % (self.N, self.D, y_true.shape, query.shape))
        res = {"logp_n": np.empty(self.N, dtype=np.float64), "count": np.empty(self.N, dtype=np.int32)}
        out = _lib.PredScoreOut()
        out.logp_n, out.count = dptr(res["logp_n"]), i32ptr(res["count"])
        if per_entry:
            res["logp"], res["pit"] = np.empty((self.N, self.D)), np.empty((self.N, self.D))
            out.logp, out.pit = dptr(res["logp"]), dptr(res["pit"])
        counters = (ctypes.c_int64 * 4)()
        total = np.zeros(2, dtype=np.float64)
        check(self.lib.evoamd_predictive_score(self._h, dptr(y_true), u8ptr(query), 1 if noise else 0, ctypes.byref(out),
                                               counters, dptr(total)))
        res["sum"], res["total_count"] = float(total[0]), int(total[1])
        for i, name in enumerate(("n_singular", "n_skipped", "n_not_queried", "n_bad_values")):
            res[name] = int(counters[i])
        return res

    def _check_result_serial(self, kind, serial, what):
        if serial is not None and serial != getattr(self, kind):
            raise EvoAmdError("the %s on the device are newer ones (a later call or a configure)" % what)

    def download_predictive(self, which, shape=None, serial=None):
        """The (N, D) "mean" or "var" the last predictive_moments left on the device; EvoAmdError once they are gone."""
        self._check_result_serial("_pred_serial", serial, "predictive moments")
        out = np.empty((self.N, self.D) if shape is None else tuple(shape))
        if out.shape != (self.N, self.D):
            raise EvoAmdError("the predictive moments on the device belong to another geometry")
        check(self.lib.evoamd_download_predictive(self._h, dptr(out) if which == "mean" else None,
                                                  dptr(out) if which == "var" else None))
        return out

    def patches_merge_predictive(self, shape, ph, pw, shift=1, what=2, serial=None):
        """The image merged from the moments the last predictive_moments left on the device (evoamd_patches_merge_predictive):
        ``what`` 0 mean-merge of mean, 1 median-merge of mean, 2 precision-weighted merge of mean by var, 3 mean-merge of
        var.  Only the image crosses to the host.  The geometry must give (N, D) of the moments (ValueError)."""
        from .utils.prepost import patch_geometry
        H, W, C = _image_hwc(shape)
        N, D = patch_geometry(H, W, C, ph, pw, shift)
        if (N, D) != (self.N, self.D):
            raise ValueError("patches_merge_predictive: the geometry needs (%d, %d), the moments are (%d, %d)"
                             % (N, D, self.N, self.D))
        self._check_result_serial("_pred_serial", serial, "predictive moments")
        out = np.empty(tuple(shape), dtype=np.float64)
        check(self.lib.evoamd_patches_merge_predictive(self._h, H, W, C, int(ph), int(pw), int(shift), int(what), dptr(out)))
        return out

    # ---- posterior samples (evo_amd.models.posterior_sample is the NumPy mirror) -----------------
    def sample_posterior(self, n_samples=1, seed=0, first_index=0, keep=("slot", "s", "z", "y"), fill="missing", noise=True,
                         resident=False):
        """``n_samples`` draws per datapoint from the variational posterior under the Theta, K^n and lpj rows on the device
        (evoamd_posterior_sample; no statistics pass runs and the EM state stays as it is).  Returns a dict with the arrays
        ``keep`` names -- "slot" int32 (N, T), "s" bool (N, T, H), "z" float64 (N, T, H; ES3C only), "y" float64 (N, T, D)
        -- and "info" = {"n_singular", "n_skipped", "n_not_pd", "n_bad_weights"}: the datapoints without draws (slot -1,
        s zero, z and y NaN).  Only the arrays named are allocated, written and downloaded.  EvoAmdError naming n and k
        for a state with more than 32 active latents, for D > 512, for "z" with EBSC, and -- naming the bytes -- for
        outputs that do not fit into the free device memory; nothing is downloaded then.  ``resident=True`` (``keep`` must
        name "y"): "y" is not downloaded; the entry is a ResidentDraws handle of the buffer on the device
        (patches_merge_samples merges the draws there) until the next call."""
        from .models.generate import unpack_words
        if fill not in ("missing", "all"):
            raise ValueError("fill must be 'missing' or 'all'")
        keep = tuple(keep)
        bits = 0
        for name in keep:
            if name not in _lib.PSAMP_KEEP:
                raise ValueError("keep: unknown output %r" % (name,))
            bits |= _lib.PSAMP_KEEP[name]
        if resident and "y" not in keep:
            raise ValueError("resident=True keeps the draws \"y\" on the device: keep must name \"y\"")
        T = int(n_samples)
        counters = (ctypes.c_int64 * 4)()
        self._ps_serial += 1  # (before the call: a failed one leaves nothing either)
        check(self.lib.evoamd_posterior_sample(self._h, T, int(seed) & (2 ** 64 - 1), int(first_index) & (2 ** 64 - 1), bits,
                                               1 if fill == "all" else 0, 1 if noise else 0, counters))
        N, D, H = self.N, self.D, self.H
        shapes = {"slot": ((N, T), np.int32), "s": ((N * T, (H + 63) // 64), np.uint64), "z": ((N, T, H), np.float64),
                  "y": ((N, T, D), np.float64)}
        out = {}
        for name in ("slot", "s", "z", "y"):
            if name == "y" and resident and name in keep:
                from .resident import ResidentDraws
                out[name] = ResidentDraws(self, self._ps_serial, (N, T, D))
            elif name in keep:
                a = np.empty(*shapes[name])
                check(self.lib.evoamd_download_posterior_samples(self._h, _lib.PSAMP_WHAT[name], a.ctypes.data_as(ctypes.c_void_p)))
                out[name] = unpack_words(a, H).reshape(N, T, H) if name == "s" else a
        out["info"] = dict(zip(("n_singular", "n_skipped", "n_not_pd", "n_bad_weights"), (int(v) for v in counters)))
        return out

    def download_posterior_draws(self, T, serial=None):
        """The (N, T, D) draws "y" the last sample_posterior left on the device; EvoAmdError once they are gone."""
        self._check_result_serial("_ps_serial", serial, "posterior draws")
        a = np.empty((self.N, int(T), self.D))
        check(self.lib.evoamd_download_posterior_samples(self._h, _lib.PSAMP_WHAT["y"], a.ctypes.data_as(ctypes.c_void_p)))
        return a

    def patches_merge_samples(self, shape, ph, pw, shift=1, method="mean", t0=0, n_draws=1, images=True, moments=False,
                              serial=None):
        """Merge draws t0 .. t0 + n_draws - 1 of the "y" the last sample_posterior left on the device into images
        (evoamd_patches_merge_samples: one launch for all of them).  Returns (imgs, mean, std): imgs (n_draws, *shape)
        when ``images``, mean / std of ``shape`` -- the pixelwise Welford moments over the merged images, ddof 0 -- when
        ``moments``; None for what was not asked for.  Only these arrays cross to the host.  The geometry must give
        (N, D) of the draws (ValueError)."""
        from .utils.prepost import patch_geometry
        H, W, C = _image_hwc(shape)
        N, D = patch_geometry(H, W, C, ph, pw, shift)
        if (N, D) != (self.N, self.D):
            raise ValueError("patches_merge_samples: the geometry needs (%d, %d), the draws are (%d, %d) per draw"
                             % (N, D, self.N, self.D))
        if not (images or moments):
            raise ValueError("patches_merge_samples: ask for the images, the moments or both")
        self._check_result_serial("_ps_serial", serial, "posterior draws")
        m = {"mean": 0, "median": 1}[method]
        imgs = np.empty((int(n_draws),) + tuple(shape)) if images and int(n_draws) >= 1 else None
        mean = np.empty(tuple(shape)) if moments else None
        std = np.empty(tuple(shape)) if moments else None
        check(self.lib.evoamd_patches_merge_samples(self._h, H, W, C, int(ph), int(pw), int(shift), m, int(t0), int(n_draws),
                                                    None if imgs is None else dptr(imgs),
                                                    None if mean is None else dptr(mean), None if std is None else dptr(std)))
        return imgs, mean, std

    # ---- log-likelihood beyond K^n (evo_amd.models.loglik_estimate is the NumPy mirror) -------
    def loglik_estimate(self, n_samples=256, seed=0, first_index=0, prior_mix=0.25, keep_draws=False):
        """The importance-draw estimate of log p(y_n) - ljc per datapoint under the Theta, K^n and lpj rows on the device
        (evoamd_loglik_estimate; csrc/kernels_loglik_estimate.hpp has the law).  Returns (total, n_ok, info): total = the
        sum of ll over the n_ok datapoints that have an estimate, info = the (N,) arrays "ll", "F", "gap",
        "mass_outside", "ess", "n_outside" (int32; NaN / 0 rows for a datapoint without an estimate), the counters
        "n_bad_weights" and "n_skipped" and, with ``keep_draws``, "s" bool (N, T, H), "inside" bool (N, T), "log_r" and
        "lpj" (N, T; lpj NaN where the draw is inside K^n).  K^n, lpj, Theta and the statistics rows stay as they are;
        the resident candidate batch is used up (vary_kn refuses until the next one).  EvoAmdError for the float32 mode,
        H > 1024, S_perm + 2 S > 2048 and, naming the bytes, buffers that do not fit the free device memory."""
        from .models.generate import unpack_words
        T = int(n_samples)
        if T < 1:
            raise ValueError("n_samples must be positive")
        if not 0.0 < float(prior_mix) <= 1.0:
            raise ValueError("prior_mix must be in (0, 1]")
        N, H = self.N, self.H
        info = {name: np.empty(N) for name in ("ll", "F", "mass_outside", "ess")}
        info["n_outside"] = np.empty(N, dtype=np.int32)
        counters = (ctypes.c_int64 * 2)()
        total = ctypes.c_double()
        check(self.lib.evoamd_loglik_estimate(
            self._h, T, int(seed) & (2 ** 64 - 1), int(first_index) & (2 ** 64 - 1), float(prior_mix), 1 if keep_draws else 0,
            dptr(info["ll"]), dptr(info["F"]), dptr(info["mass_outside"]), dptr(info["ess"]), i32ptr(info["n_outside"]),
            counters, ctypes.byref(total)))
        none = np.isnan(info["ll"])
        info["F"][none] = np.nan
        info["n_outside"][none] = 0
        info["gap"] = info["ll"] - info["F"]
        info["n_bad_weights"], info["n_skipped"] = int(counters[0]), int(counters[1])
        if keep_draws:
            shapes = {"s": ((N * T, (H + 63) // 64), np.uint64), "inside": ((N, T), np.uint8),
                      "log_r": ((N, T), np.float64), "lpj": ((N, T), np.float64)}
            for name in ("s", "inside", "log_r", "lpj"):
                a = np.empty(*shapes[name])
                check(self.lib.evoamd_download_loglik_draws(self._h, _lib.LLE_WHAT[name], a.ctypes.data_as(ctypes.c_void_p)))
                info[name] = (unpack_words(a, H).reshape(N, T, H) if name == "s" else
                              a.astype(np.bool_) if name == "inside" else a)
        return total.value, N - int(none.sum()), info

    # ---- timing --------------------------------------------------------------------------
    def timing(self, on=True):
        """on: True (all kernel classes), False, or an iterable of class names (_lib.KERNEL_IDS, _lib.KERNEL_IDS_EXTRA)."""
        if on is True:
            mask = (1 << 64) - 1
        elif not on:
            mask = 0
        else:
            mask = 0
            for name in on:
                mask |= 1 << _lib.kernel_id(name)
        check(self.lib.evoamd_timing_enable64(self._h, mask))

    def timing_reset(self):
        check(self.lib.evoamd_timing_reset(self._h))

    def kernel_time_ms(self, name):
        avg = ctypes.c_double()
        n = ctypes.c_int64()
        check(self.lib.evoamd_kernel_time_ms(self._h, _lib.kernel_id(name), ctypes.byref(avg), ctypes.byref(n)))
        return avg.value, n.value


_KEEP_RESIDENT = ctypes.cast(1, _lib._c_u8p)  # EVOAMD_KEEP_RESIDENT of include/evo_amd.h


def _image_hwc(shape):
    if len(shape) == 2:
        return int(shape[0]), int(shape[1]), 1
    if len(shape) == 3:
        return int(shape[0]), int(shape[1]), int(shape[2])
    raise ValueError("image shape must be (H, W) or (H, W, C), got %s" % (tuple(shape),))


TAIL = ("Fs", "sum_nunique", "sum_sub", "N", "reset_isnan", "reset_smaller_eps", "reset_isinf", "pad")


def acc_layout(model, D, H):
    """Offsets (name -> (start, shape)) of the packed accumulator documented in evo_amd.h."""
    out = {}
    o = 0

    def put(name, shape):
        nonlocal o
        n = int(np.prod(shape)) if shape else 1
        out[name] = (o, shape)
        o += n

    if model in (MODEL_BSC, "bsc", "BSC"):
        put("Wp", (H, D))
        put("Wq", (H, H))
        put("pies", (H,))
        put("sigma", ())
    else:
        put("xpt_s", (H,))
        put("xpt_ss", (H, H))
        put("xpt_sz", (H,))
        put("xpt_szsz", (H, H))
        put("Wp", (D, H))
        put("s_sz_outer", (H, H))
        put("sz_sz_outer", (H, H))
        put("y_outer_diag", (D,))
    for t in TAIL:
        put(t, ())
    out["_size"] = (o, ())
    return out


def acc_size(model, D, H):
    return acc_layout(model, D, H)["_size"][0]


def acc_views(acc, model, D, H):
    """dict name -> view into the packed accumulator (scalars as 0-d views)."""
    lay = acc_layout(model, D, H)
    assert acc.size == lay["_size"][0], (acc.size, lay["_size"][0])
    views = {}
    for name, (start, shape) in lay.items():
        if name == "_size":
            continue
        n = int(np.prod(shape)) if shape else 1
        views[name] = acc[start:start + n].reshape(shape)
    return views

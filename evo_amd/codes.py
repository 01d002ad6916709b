"""Posterior codes: what a sparse-coding run says about each datapoint.

``PosteriorCodes`` holds the compact readout the GPU produces (csrc/kernels_codes.hpp, Engine.posterior_codes,
Model.encode): per datapoint the ``max_active`` most probable latents with their posterior marginals E_q[s_h] and, for
ES3C, posterior means E_q[s_h z_h], plus the most probable state of K^n.  ``codes_from_dense`` is the NumPy mirror of
the kernel: the same selection rule and the same arithmetic for ``map_q``, so the two agree bit for bit on the same
inputs (the project keeps host mirrors of vary_Kn and the evolutionary operators the same way).
"""
import numpy as np

F64_TINY = np.finfo(np.float64).tiny  # eps_pjc_sum of the reference (sssc.py:36): the statistics pass adds it too
MAX_ACTIVE = 64


class PosteriorCodes:
    """idx (N, A) int32, p (N, A), m (N, A) or None (EBSC): the latents with E_q[s_h] > p_min by descending E_q[s_h],
    ties by ascending h, cut to A = max_active; unused slots idx = -1, p = m = 0.  nnz (N,) int32 counts them BEFORE the
    cut (nnz > A: truncated).  map_slot (N,) int32 / map_q (N,) / map_state (N, ceil(H/8)) uint8: index in the lpj row,
    posterior weight and np.packbits bits of the most probable state.  Es / Ez: the dense (N, H) rows of the same pass
    when they were asked for (Model.encode(dense=True)), else None."""

    def __init__(self, H, idx, p, m, nnz, map_slot, map_q, map_state, p_min=0.0, Es=None, Ez=None):
        self.H = int(H)
        self.idx, self.p, self.m, self.nnz = idx, p, m, nnz
        self.map_slot, self.map_q, self.map_state = map_slot, map_q, map_state
        self.p_min = float(p_min)
        self.Es, self.Ez = Es, Ez

    @property
    def max_active(self):
        return self.idx.shape[1]

    @property
    def truncated(self):
        """(N,) bool: the datapoint has more latents above p_min than the code holds."""
        return self.nnz > self.max_active

    def map_states(self):
        """The most probable states as bool (N, H)."""
        return np.unpackbits(self.map_state, axis=-1)[:, :self.H].astype(bool)

    def to_dense(self):
        """(Es, Ez) as (N, H) arrays, zero where the code holds nothing (Ez is None for EBSC)."""
        N = self.idx.shape[0]
        rows, cols = np.nonzero(self.idx >= 0)
        h = self.idx[rows, cols]
        Es = np.zeros((N, self.H))
        Es[rows, h] = self.p[rows, cols]
        Ez = None
        if self.m is not None:
            Ez = np.zeros((N, self.H))
            Ez[rows, h] = self.m[rows, cols]
        return Es, Ez


def codes_exp(x):
    """exp(x) for x <= 0 the way the kernel evaluates it (kernels_codes.hpp: codes_exp): IEEE additions and
    multiplications only, in the same order, so the result has the same bits.  x = k ln2 + r with a two-part ln2,
    degree-13 Taylor polynomial by Horner, scaled by 2^k; 0 below -700 and for NaN."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = x >= -700.0
        xs = np.where(ok, x, 0.0)
        k = np.rint(xs * 1.4426950408889634)
        r = (xs - k * 0.693147180369123816490) - k * 1.90821492927058770002e-10
        q = np.full_like(xs, 1.0 / 6227020800.0)
        for c in (1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
                  1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
            q = q * r + c
        return np.where(ok, np.ldexp(q, k.astype(np.int32)), 0.0)


def _wave_sum(terms):
    """Sum over the last axis in the kernel's order: lane l adds the terms s = l, l + 64, ... in ascending s, the 64
    partial sums meet in an xor butterfly (32, 16, ... 1)."""
    N, L = terms.shape
    pad = np.zeros((N, -(-L // 64) * 64))
    pad[:, :L] = terms
    z = np.zeros((N, 64))
    for j in range(pad.shape[1] // 64):
        z = z + pad[:, 64 * j:64 * (j + 1)]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        z = z + z[:, lanes ^ o]
    return z[:, 0]


def codes_from_dense(Es, Ez, lpj, states, max_active=16, p_min=0.0, S_perm=0):
    """NumPy mirror of posterior_codes_kernel.  Es (N, H); Ez (N, H) or None; lpj (N, S_perm + S); states: K^n as bool
    (N, S, H) or np.packbits bytes (N, S, ceil(H/8)).  Returns a PosteriorCodes (without dense rows)."""
    Es = np.asarray(Es, dtype=np.float64)
    N, H = Es.shape
    A = int(max_active)
    if not 1 <= A <= MAX_ACTIVE:
        raise ValueError("max_active must be in [1, %d]" % MAX_ACTIVE)
    if not p_min >= 0.0:
        raise ValueError("p_min must be >= 0")
    lpj = np.asarray(lpj, dtype=np.float64)
    states = np.asarray(states)
    packed = states if states.dtype == np.uint8 else np.packbits(states.astype(bool), axis=-1)
    assert lpj.shape[0] == N and packed.shape == (N, lpj.shape[1] - S_perm, (H + 7) // 8), (lpj.shape, packed.shape)

    above = Es > p_min
    nnz = above.sum(axis=1).astype(np.int32)
    # descending value, ties by ascending h: a stable sort of -value keeps equal values in index order
    key = np.where(above, -Es, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :A]
    if order.shape[1] < A:
        order = np.concatenate((order, np.zeros((N, A - order.shape[1]), dtype=order.dtype)), axis=1)
    rows = np.arange(N)[:, None]
    used = np.arange(A)[None, :] < np.minimum(nnz, A)[:, None]
    idx = np.where(used, order, -1).astype(np.int32)
    p = np.where(used, Es[rows, order], 0.0)
    m = None if Ez is None else np.where(used, np.asarray(Ez, dtype=np.float64)[rows, order], 0.0)

    map_slot = np.argmax(lpj, axis=1).astype(np.int32)
    shift = 0.0 - lpj.max(axis=1)
    map_q = 1.0 / (_wave_sum(codes_exp(lpj + shift[:, None])) + F64_TINY)
    map_state = np.zeros((N, (H + 7) // 8), dtype=np.uint8)
    in_kn = map_slot >= S_perm
    map_state[in_kn] = packed[np.nonzero(in_kn)[0], map_slot[in_kn] - S_perm]
    return PosteriorCodes(H, idx, p, m, nnz, map_slot, map_q, map_state, p_min=p_min)

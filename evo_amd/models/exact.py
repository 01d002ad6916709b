"""NumPy mirrors of the exact log-likelihood pass (csrc/kernels_exact.hpp, evoamd_loglik_exact): the index -> state map
of the enumeration kernel and the running max / rescale recursion of the fold kernel.  Same recursion, not the same
bits: the device's exp is not NumPy's and the kernel adds a chunk's terms in lane order.

The states of Hv = H - background latents are numbered 0 .. 2^Hv - 1: state g has latent h on iff bit h of g is set.
With the permanent background unit (``background``), latent H - 1 is on in every state.  Without it index 0 is the
all-zero state, whose term is the permanent state's (``zero_lpj``) and not part of any chunk: the index range of the
chunks is 1 .. 2^Hv - 1 then, 0 .. 2^Hv - 1 with the background unit.
"""
import numpy as np

MAX_HV = 32  # EXACT_MAX_HV of the library


def index_range(H, background=False):
    """(first, end) of the state indices the chunks cover."""
    Hv = H - (1 if background else 0)
    return (0 if background else 1), 2 ** Hv


def chunk_bounds(H, background=False, chunk_states=64):
    """The (g0, count) windows the library folds one after the other: [k C, (k + 1) C) cut to index_range()."""
    first, end = index_range(H, background)
    C = int(chunk_states)
    assert C >= 64 and C & (C - 1) == 0, "chunk_states must be a power of two >= 64"
    out = []
    for lo in range(0, end, C):
        g0, g1 = max(lo, first), min(lo + C, end)
        if g1 > g0:
            out.append((g0, g1 - g0))
    return out


def enumerate_chunk(g0, count, H, background=False):
    """bool (count, H): the states of the indices g0 .. g0 + count - 1."""
    Hv = H - (1 if background else 0)
    assert 1 <= Hv <= MAX_HV and g0 >= 0 and g0 + count <= 2 ** Hv
    g = np.arange(g0, g0 + count, dtype=np.uint64)
    states = np.ones((count, H), dtype=bool)  # (the background unit's column stays on)
    for h in range(Hv):
        states[:, h] = (g >> np.uint64(h)) & np.uint64(1)
    return states


def fold_exact(lpj_chunks, state_chunks=None, zero_lpj=None):
    """Running log-sum-exp over chunks of states.  lpj_chunks: iterable of (N, C_k) arrays; state_chunks: the matching
    bool (C_k, H) arrays, or None for no marginals; zero_lpj (N): the all-zero state's term, which seeds the running
    values (m, z) = (zero_lpj, 1) -- without it they start at (-inf, 0).  Per chunk: m' = max(m, chunk max), z and
    a_h are rescaled by exp(m - m') (0 while m is -inf) and the chunk's exp(lpj - m') are added.
    Returns (ll, marg): ll (N) = log z + m, marg (N, H) = a / z (exactly 1 for a latent on in every state) or None."""
    m = z = a = always_on = None
    states_it = iter(state_chunks) if state_chunks is not None else None
    for lpj in lpj_chunks:
        lpj = np.asarray(lpj, dtype=np.float64)
        st = None if states_it is None else np.asarray(next(states_it), dtype=bool)
        if m is None:
            N = lpj.shape[0]
            if zero_lpj is None:
                m, z = np.full(N, -np.inf), np.zeros(N)
            else:
                m, z = np.array(zero_lpj, dtype=np.float64).reshape(N), np.ones(N)
            a = None if st is None else np.zeros((N, st.shape[1]))
            always_on = None if st is None else np.ones(st.shape[1], dtype=bool)
        m_new = np.maximum(m, lpj.max(axis=1))
        with np.errstate(invalid="ignore"):
            scale = np.where(np.isneginf(m), 0.0, np.exp(m - m_new))
        e = np.exp(lpj - m_new[:, None])
        z = z * scale + e.sum(axis=1)
        if a is not None:
            a = a * scale[:, None] + e @ st.astype(np.float64)
            always_on &= st.all(axis=0)
        m = m_new
    assert m is not None, "no chunk"
    ll = np.log(z) + m
    if a is None:
        return ll, None
    marg = a / z[:, None]
    if zero_lpj is None:  # a latent on in every state (the background unit): a_h is z, summed in another order
        marg[:, always_on] = 1.0
    return ll, marg

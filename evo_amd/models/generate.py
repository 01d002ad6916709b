"""Samples from the model with a counter-based stream: the NumPy mirror of evoamd_generate (csrc/kernels_generate.hpp)
and the host-side pieces both share (the factor F of Psi, the word layout of s).

The law is generate_data / generate_from_hidden of the reference (_models.py:73-99, bsc.py:27-57, sssc.py:66-102):

    s_h ~ Bernoulli(pi_h) (u <= pi_h), or s given;   ES3C z_A ~ N(mu_A, Psi_AA), EBSC z = s;   y = W z + sigma g.

The reference factorises Psi_AA per datapoint.  Here z = s o (mu + F eps) with eps ~ N(0, I_H) and ONE matrix F, F F^T = Psi:
the marginal of N(mu, Psi) on the active set A is exactly N(mu_A, Psi_AA), so the law is the reference's for any A.

The stream (rng_u01 and mix64: evo_amd/variational/utils.py, csrc/kernels_evolve.hpp), with i = first_index + n:

    s_h   = rng_u01(seed, i, GEN_PURPOSE + 0, h) <= pi_h
    eps_j = normal number j of purpose GEN_PURPOSE + 1,   g_d = normal number d of purpose GEN_PURPOSE + 2
    normal number k of a purpose: pair p = k >> 1, u1 = rng_u01(.., 2 p), u2 = rng_u01(.., 2 p + 1),
    r = sqrt(-2 log u1), t = 6.283185307179586 u2;  even k: r cos t, odd k: r sin t

The uniforms, and so every bit of s, are the kernel's bit for bit; the normals agree to the last places of log / sin / cos.
The kernel, this mirror and their tests depend on this definition.
"""
import numpy as np

from ..variational.utils import _M64, _mix64

GEN_PURPOSE = 0x47454E0000000000
_TWO_PI = 6.283185307179586
_BLOCK = 1 << 21  # values of one intermediate array: the mirror works through N in blocks of rows, never row by row


def psi_factor(Psi):
    """F (H, H) with F F^T = Psi for a symmetric positive SEMI-definite Psi: F = V sqrt(max(lambda, 0)) from eigh.  Unlike a
    Cholesky factor this exists for a singular Psi; eigenvalues that rounding pushed below zero are clipped."""
    Psi = np.asarray(Psi, dtype=np.float64)
    lam, V = np.linalg.eigh(Psi)
    return np.ascontiguousarray(V * np.sqrt(np.maximum(lam, 0.0)))


def generate_params(model_name, model_params):
    """What evoamd_generate and the mirror read of Theta: W^T (H, D), pies (H), mus / F (ES3C, else None), sigma.
    BSC reads ``pi`` and ``sigma``; ES3C reads ``pies``, ``mus``, ``Psi`` and ``sigma2``."""
    Wt = np.ascontiguousarray(np.asarray(model_params["W"], dtype=np.float64).T)
    H = Wt.shape[0]
    if model_name == "bsc":
        return {"Wt": Wt, "pies": np.full(H, float(model_params["pi"])), "mus": None, "F": None,
                "sigma": float(model_params["sigma"])}
    if model_name != "sssc":
        raise ValueError("model_name must be 'bsc' or 'sssc'")
    pies = np.ascontiguousarray(model_params["pies"], dtype=np.float64)
    mus = np.ascontiguousarray(model_params["mus"], dtype=np.float64)
    assert pies.shape == (H,) and mus.shape == (H,) and np.shape(model_params["Psi"]) == (H, H)
    return {"Wt": Wt, "pies": pies, "mus": mus, "F": psi_factor(model_params["Psi"]),
            "sigma": float(np.sqrt(model_params["sigma2"]))}


def pack_words(s):
    """bool (N, H) -> uint64 (N, ceil(H/64)): latent h in word h // 64 at bit 63 - h % 64 (the device layout of K^n)."""
    s = np.asarray(s, dtype=np.bool_)
    N, H = s.shape
    HW = (H + 63) // 64
    padded = np.zeros((N, HW * 64), dtype=np.bool_)
    padded[:, :H] = s
    return np.ascontiguousarray(np.packbits(padded, axis=-1).view(">u8").astype(np.uint64))


def unpack_words(words, H):
    """The inverse of pack_words: uint64 (N, HW) -> bool (N, H)."""
    b = np.ascontiguousarray(words.astype(">u8")).view(np.uint8)
    return np.unpackbits(b, axis=-1)[:, :H].astype(np.bool_)


def _first_hash(seed, idx):
    """mix64(seed + 0x9e3779b97f4a7c15 (i + 1)) for a uint64 array of data set indices -> (n, 1)."""
    return _mix64(np.uint64(seed) + np.uint64(0x9e3779b97f4a7c15) * (idx + np.uint64(1)))[:, None]


def _u01(x0, purpose, index):
    """rng_u01 behind its first hash: x0 (n, 1), index uint64 (k,) -> float64 (n, k)."""
    salt = np.uint64((purpose * 0xd1b54a32d192ed03 + 0x632be59bd9b4e019) & _M64)
    x = _mix64(x0 ^ (salt + index))
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def _normals(x0, purpose, K):
    """The normal numbers 0 .. K-1 of a purpose -> (n, K)."""
    p = np.arange((K + 1) // 2, dtype=np.uint64)
    r = np.sqrt(-2.0 * np.log(_u01(x0, purpose, np.uint64(2) * p)))
    t = _TWO_PI * _u01(x0, purpose, np.uint64(2) * p + np.uint64(1))
    out = np.empty((x0.shape[0], 2 * p.size))
    out[:, 0::2] = r * np.cos(t)
    out[:, 1::2] = r * np.sin(t)
    return out[:, :K]


def generate_counter(model_name, model_params, N, seed, first_index=0, s=None):
    """The dict Model.generate_data_device returns for stream seed ``seed`` (``model.last_generate_seed``): "y", "s"
    (bool (N, H)), "y_mean" and, ES3C, "z".  ``s`` given: taken, not drawn (generate_from_hidden).  Vectorised over the
    datapoints; needs no GPU."""
    par = generate_params(model_name, model_params)
    Wt, pies, mus, F, sigma = par["Wt"], par["pies"], par["mus"], par["F"], par["sigma"]
    H, D = Wt.shape
    N, seed, first_index = int(N), int(seed) & _M64, int(first_index) & _M64
    sssc = model_name == "sssc"
    if s is not None:
        s = np.asarray(s, dtype=np.bool_)
        assert s.shape == (N, H), (s.shape, (N, H))
    out = {"y": np.empty((N, D)), "s": np.empty((N, H), dtype=np.bool_), "y_mean": np.empty((N, D))}
    if sssc:
        out["z"] = np.empty((N, H))
    hs = np.arange(H, dtype=np.uint64)
    rows = max(1, _BLOCK // max(H, D))
    with np.errstate(over="ignore"):  # the hashes wrap mod 2^64
        for n0 in range(0, N, rows):
            n1 = min(N, n0 + rows)
            x0 = _first_hash(seed, np.uint64(first_index) + np.arange(n0, n1, dtype=np.uint64))
            sb = _u01(x0, GEN_PURPOSE, hs) <= pies if s is None else s[n0:n1]
            out["s"][n0:n1] = sb
            if sssc:
                z = np.where(sb, mus + np.dot(_normals(x0, GEN_PURPOSE + 1, H), F.T), 0.0)
                out["z"][n0:n1] = z
            else:
                z = sb.astype(np.float64)
            y_mean = np.dot(z, Wt)
            out["y_mean"][n0:n1] = y_mean
            out["y"][n0:n1] = y_mean + sigma * _normals(x0, GEN_PURPOSE + 2, D)
    return out

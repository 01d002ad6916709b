"""Annealed importance sampling for EBSC: the NumPy mirror of Model.ais_log_likelihood (csrc/kernels_ais.hpp, which states
the law).  Host only: it never touches the engine.

Per datapoint n (data set index i = first_index + n), chain c < C and temperatures 0 = beta_0 < beta_1 <= ... <= beta_T = 1,
with f_beta(s) = exp(|s| pil_bar + beta l(s)), l(s) = pre1 (yy_n - sum_{a in s} (B_na + c_a)), c_j = B_nj - sum_{i in s} G_ij:

    start     forward: x_0,h = [u01(x0, AIS_PURPOSE + c, h) < pi], an exact draw from f_0 / Z_0, Z_0 = (1 - pi)^-H;
              reverse: x_{T-1} = row n of s_start, the same for every chain
    K_t       one systematic Gibbs scan at beta_t over h ascending (forward) or descending (reverse): Delta = pil_bar +
              (beta_t pre1) (G_hh - 2 c_h) with h off, pil_bar - (beta_t pre1) (G_hh + 2 c_h) with h on, p = 1 / (1 + exp(-Delta)),
              new bit = [u01(x0, AIS_PURPOSE + c, (t + 1) H + h) < p]; on a change c_j -= G_hj (switched on) or += G_hj (off)
    forward   for t = 1 .. T: log w += (beta_t - beta_{t-1}) l(x_{t-1}); for t < T: x_t = K_t(x_{t-1}); one more scan at
              beta_T (uniform block T + 1) gives ``final``
    reverse   for t = T - 1 .. 1: x_{t-1} = K~_t(x_t); log w = sum_t (beta_t - beta_{t-1}) l(x_{t-1}), t = T first; final = x_0
    estimate  a_c = log w_c (forward) / -log w_c (reverse) folded in chain order; forward ll = logsumexp(a) - log C + H
              log1p(exp(pil_bar)) (E[ll] <= log p(y_n) - ljc), reverse ll = -(logsumexp(a) - log C) + H log1p(exp(pil_bar)) (E[ll]
              >= log p(y_n) - ljc IF s_start[n] is an exact posterior sample: y_n generated from this Theta with that s);
              ess = (sum e^a)^2 / sum e^{2 a}

The mirror scans h sequentially; the kernel settles a chunk of 64 latents by ballots, which gives the same decisions.  The
operations are the kernel's in the kernel's order (separate NumPy operations, no fused forms).  ``final``, ``n_flips`` and
the starting draw are bit-level wherever no decision is closer to its uniform than the rounding of B, G and exp (``margin``
says how close the closest was); the real-valued outputs are formula-level.

Incomplete data (``x_infr``, bool (N, D); Model.ais_log_likelihood / ais_posterior with incomplete=True): the same law with
Y zeroed under False (so B_n and yy_n are sums over the reliable entries, and values under False, NaN included, never
enter) and the datapoint's own G(n)_hj = sum over its reliable d, ascending, of (W_dh W_dj) -- each product rounded, then
added, starting from 0.0: a loop over d, which is what the kernel does, so the rows agree bit for bit.  A datapoint without
a reliable entry has G(n) = 0, B = 0, yy = 0: prior draws, log w = 0, ll = H log1p(exp(pil_bar)); it is not skipped.
"""
import numpy as np

from ..variational.utils import _M64, _mix64
from .generate import _first_hash

AIS_PURPOSE = 0x4149530000000000  # "AIS"
AIS_MAX_H = 1024


def sigmoid_schedule(n_temps, delta=4.0):
    """beta_t = (sigma(delta (2 t / T - 1)) - sigma(-delta)) / (sigma(delta) - sigma(-delta)), t = 0 .. T (Grosse et al.), the
    ends set to exactly 0 and 1."""
    T = int(n_temps)
    if T < 1:
        raise ValueError("n_temps must be positive")
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))  # noqa: E731
    t = np.arange(T + 1, dtype=np.float64)
    betas = (sig(delta * (2.0 * t / T - 1.0)) - sig(-delta)) / (sig(delta) - sig(-delta))
    betas[0], betas[-1] = 0.0, 1.0
    return betas


def check_betas(betas):
    """The schedule as a float64 array, or ValueError naming the rule it breaks."""
    b = np.ascontiguousarray(betas, dtype=np.float64)
    if b.ndim != 1 or b.size < 2:
        raise ValueError("ais: betas must be a 1-d array of T + 1 >= 2 values")
    if b[0] != 0.0:
        raise ValueError("ais: betas must start at 0 (betas[0] = %g)" % b[0])
    if b[-1] != 1.0:
        raise ValueError("ais: betas must end at 1 (betas[-1] = %g)" % b[-1])
    if not np.all(b[1:] >= b[:-1]) or not b[1] > 0.0:
        raise ValueError("ais: betas must not descend and must leave 0 at once")
    return b


def ais_scalars(theta):
    """(pre1, pil_bar, pi) of an EBSC Theta, as E_step_precompute forms them."""
    pi, sigma = float(theta["pi"]), float(theta["sigma"])
    return -1.0 / 2.0 / sigma / sigma, float(np.log(pi / (1.0 - pi))), pi


def ais_conditional(pre1, pil_bar, c_h, G_hh, on, beta):
    """p(s_h = 1 | the other latents) under f_beta, from c_h = B_nh - sum_{i in s} G_ih of the CURRENT state (h included
    when it is on).  Scalars, or arrays over chains for c_h and on."""
    bp = beta * pre1
    two_c = 2.0 * np.asarray(c_h, dtype=np.float64)
    t_on = bp * (G_hh + two_c)
    t_off = bp * (G_hh - two_c)
    delta = np.where(on, pil_bar - t_on, pil_bar + t_off)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-delta))


def _ell(pre1, yy, Bn, c, s):
    """l(s) for every chain: s bool (C, H), c (C, H); the sum runs over the active a in ascending order."""
    total = np.zeros(s.shape[0])
    for a in np.flatnonzero(s.any(axis=0)):
        total = np.where(s[:, a], total + (Bn[a] + c[:, a]), total)
    return pre1 * (yy - total)


def _mask_data(Y, x_infr):
    """(Y with zeros under False, the mask as bool (N, D)), or (Y, None) for complete data."""
    if x_infr is None:
        return Y, None
    mask = np.asarray(x_infr)
    if mask.shape != Y.shape or mask.dtype != np.bool_:
        raise ValueError("ais: x_infr must be a bool array of the shape of Y")
    return np.where(mask, Y, 0.0), mask


def _datapoint_gram(W, G, Gd, o):
    """(diagonal, row getter) of the G that the chains of one datapoint read.  ``o`` None (complete data): G itself.  Else
    o lists the reliable d in ascending order and G(n)_hj = sum_{d in o} (W_dh W_dj), each product rounded, then added,
    starting from 0.0 -- a loop over d.  A row is formed when a chain first asks for it and kept for the datapoint."""
    if o is None:
        return Gd, lambda h: G[h]
    H = W.shape[1]
    gd = np.zeros(H)
    for d in o:
        gd = gd + W[d] * W[d]
    rows = {}

    def row(h):
        if h not in rows:
            r = np.zeros(H)
            for d in o:
                r = r + W[d, h] * W[d]
            rows[h] = r
        return rows[h]
    return gd, row


def _u01_chains(x0, C, index):
    """u01(x0, AIS_PURPOSE + c, index) for c < C: x0 (1, 1), index uint64 (k,) -> float64 (C, k)."""
    salt = np.array([((AIS_PURPOSE + c) * 0xd1b54a32d192ed03 + 0x632be59bd9b4e019) & _M64 for c in range(C)], dtype=np.uint64)
    x = _mix64(x0[0, 0] ^ (salt[:, None] + index[None, :]))
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def _fold(a):
    """(logsumexp, ess) of a_0, a_1, ... folded in order, the maximum rescaled when it grows."""
    m, z, q = -np.inf, 0.0, 0.0
    for t in a:
        if t > m:
            r = np.exp(m - t)
            z = z * r + 1.0
            q = q * (r * r) + 1.0
            m = t
        else:
            e = np.exp(t - m)
            z = z + e
            q = q + e * e
    return m + np.log(z), z * z / q


def ais_log_likelihood_counter(theta, Y, n_chains=16, n_temps=128, betas=None, seed=0, first_index=0, direction="forward",
                               s_start=None, B=None, G=None, x_infr=None):
    """What Model.ais_log_likelihood returns in ``info`` with per_datapoint=True and keep_states=True, for stream seed
    ``seed`` (``model.last_ais_seed``): the (N,) arrays "ll", "ess", "log_w_mean", "log_w_min", "log_w_max", "n_flips"
    (int64), "log_w" (N, C), "final" (uint8, N x C x ceil(H / 8), np.packbits layout), and beside them "final_bool" (N, C,
    H), "start" (the starting states, bool (N, C, H)), "margin" (N, C) = the minimum over all decisions of the chain of
    |u - p| (the starting draw: |u - pi|) and "sum" = the sum of ll.  ``theta``: an EBSC Theta with "W" (D, H), "pi",
    "sigma"; ``Y`` (N, D) complete data; ``B`` / ``G``: Y W and W^T W when the caller has them (else formed here).
    ``x_infr`` (bool (N, D)): incomplete data -- Y is used with zeros under False and the chains of datapoint n read its own
    G(n) over its reliable entries (the module's docstring); ``G`` is then not read."""
    if direction not in ("forward", "reverse"):
        raise ValueError("ais: direction must be 'forward' or 'reverse'")
    rev = direction == "reverse"
    C = int(n_chains)
    if C < 1:
        raise ValueError("ais: n_chains must be positive")
    betas = sigmoid_schedule(n_temps) if betas is None else check_betas(betas)
    T = betas.size - 1
    W = np.asarray(theta["W"], dtype=np.float64)
    Y, mask = _mask_data(np.asarray(Y, dtype=np.float64), x_infr)
    N, H = Y.shape[0], W.shape[1]
    if H > AIS_MAX_H:
        raise ValueError("ais: H = %d, at most %d latents are supported" % (H, AIS_MAX_H))
    if rev:
        if s_start is None or np.shape(s_start) != (N, H) or np.asarray(s_start).dtype != np.bool_:
            raise ValueError("ais: direction='reverse' needs s_start, a bool array of shape (N, H)")
        s_start = np.asarray(s_start)
    pre1, pilb, pi = ais_scalars(theta)
    B = np.dot(Y, W) if B is None else np.asarray(B, dtype=np.float64)
    if mask is not None:
        G = Gd = None  # (every datapoint has its own)
    else:
        G = np.dot(W.T, W) if G is None else np.asarray(G, dtype=np.float64)
        Gd = np.diag(G).copy()
    yy = (Y * Y).sum(axis=1)
    seed, first_index = int(seed) & _M64, int(first_index) & _M64
    hs = np.arange(H, dtype=np.uint64)
    out = {"log_w": np.empty((N, C)), "final_bool": np.zeros((N, C, H), dtype=bool), "start": np.zeros((N, C, H), dtype=bool),
           "margin": np.full((N, C), np.inf), "n_flips": np.zeros(N, dtype=np.int64)}
    for name in ("ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
        out[name] = np.empty(N)
    chain_flips = np.zeros((N, C), dtype=np.int64)
    lz0 = H * np.log1p(np.exp(pilb))

    def scan(s, c, beta, u, order, flips, margin, gd, row):
        """One scan of all chains in place: s bool (C, H), c (C, H), u (C, H); flips and margin (C,) are updated; gd, row:
        the diagonal and the rows of the datapoint's G (_datapoint_gram)."""
        for h in order:
            on = s[:, h].copy()
            p = ais_conditional(pre1, pilb, c[:, h], gd[h], on, beta)
            np.minimum(margin, np.abs(u[:, h] - p), out=margin)
            nb = u[:, h] < p
            up, down = nb & ~on, on & ~nb
            if up.any():
                c[up] = c[up] - row(h)     # (one subtraction per j)
            if down.any():
                c[down] = c[down] + row(h)
            s[:, h] = nb
            flips += up | down

    fwd, bwd = range(H), range(H - 1, -1, -1)
    with np.errstate(over="ignore"):  # the hashes wrap mod 2^64
        for n in range(N):
            x0 = _first_hash(seed, np.array([(first_index + n) & _M64], dtype=np.uint64))
            block = lambda b: _u01_chains(x0, C, np.uint64(b * H) + hs)  # noqa: E731  (uniform block b: indices b H .. b H + H - 1)
            margin = np.full(C, np.inf)
            flips = np.zeros(C, dtype=np.int64)
            if rev:
                s = np.repeat(s_start[n][None, :], C, axis=0)
            else:
                u = block(0)
                s = u < pi
                margin = np.abs(u - pi).min(axis=1)
            out["start"][n] = s
            gd, row = _datapoint_gram(W, G, Gd, None if mask is None else np.flatnonzero(mask[n]))
            c = np.repeat(B[n][None, :], C, axis=0)
            for i in np.flatnonzero(s.any(axis=0)):
                c[s[:, i]] = c[s[:, i]] - row(i)
            if not rev:
                lw = np.zeros(C)
                for t in range(1, T + 1):  # (the scan of t = T gives ``final``)
                    lw = lw + (betas[t] - betas[t - 1]) * _ell(pre1, yy[n], B[n], c, s)
                    scan(s, c, betas[t], block(t + 1), fwd, flips, margin, gd, row)
            else:
                lw = (betas[T] - betas[T - 1]) * _ell(pre1, yy[n], B[n], c, s)
                for t in range(T - 1, 0, -1):
                    scan(s, c, betas[t], block(t + 1), bwd, flips, margin, gd, row)
                    lw = lw + (betas[t] - betas[t - 1]) * _ell(pre1, yy[n], B[n], c, s)
            out["log_w"][n] = lw
            out["final_bool"][n] = s
            out["margin"][n] = margin
            chain_flips[n] = flips
            lse, ess = _fold(-lw if rev else lw)
            lse = lse - np.log(float(C))
            out["ll"][n] = (-lse if rev else lse) + lz0
            out["ess"][n] = ess
            total = 0.0
            for v in lw:
                total = total + v
            out["log_w_mean"][n] = total / float(C)
            out["log_w_min"][n], out["log_w_max"][n] = lw.min(), lw.max()
    out["n_flips"] = chain_flips.sum(axis=1)
    out["chain_flips"] = chain_flips
    out["final"] = np.packbits(out["final_bool"], axis=-1).reshape(-1)
    out["sum"] = float(np.sum(out["ll"]))
    return out


def check_index(index, N):
    """The list of Model.ais_posterior(index=...): a 1-d integer array, strictly ascending within [0, N) -> int64, C-contiguous.
    ValueError naming the first offender."""
    idx = np.asarray(index)
    if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
        raise ValueError("ais_posterior: index must be a 1-d integer array")
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    for i, v in enumerate(idx):
        if v < 0 or v >= N:
            raise ValueError("ais_posterior: index[%d] = %d is outside [0, N = %d)" % (i, v, N))
        if i and v == idx[i - 1]:
            raise ValueError("ais_posterior: index[%d] = %d is repeated" % (i, v))
        if i and v < idx[i - 1]:
            raise ValueError("ais_posterior: index[%d] = %d descends (after %d): the list is ascending" % (i, v, idx[i - 1]))
    return idx


def ais_posterior_counter(theta, Y, n_chains=16, n_temps=128, n_keep=4, betas=None, seed=0, first_index=0, mean=False, B=None,
                          G=None, x_infr=None, index=None):
    """The NumPy mirror of Model.ais_posterior (csrc/kernels_ais_post.hpp states the law): the forward chains of
    ais_log_likelihood_counter, continued.  The scan at beta_T = 1 (uniform block T + 1) is the first KEPT scan; kept scans
    2 .. ``n_keep`` follow at beta = 1 with the uniform blocks T + 2, T + 3, ...; none of them enters w.  In every kept scan
    the conditional p = 1 / (1 + exp(-Delta)) from the current c_h is added to R_c[h] at the moment latent h is decided,
    whether or not the bit changes; r_ch = R_c[h] / n_keep.  After each kept scan lpj(x) = |x| pil_bar + l(x); a chain keeps
    its best visited state, a strictly greater value replaces it.  Per datapoint, with lse = logsumexp(log w) folded in chain
    order (``_fold``) and a_c = exp(log w_c - lse):

        p[n, h]     = sum_c a_c r_ch                       (chain order)
        p_se[n, h]  = sqrt(sum_c (a_c (r_ch - p_nh))^2)    the delta-method error of a self-normalised estimate
        count[n]    = sum_h p_nh                           (h ascending)
        map_lpj / map_state: the best over the chains, ties to the lowest chain; map_state in np.packbits layout

    Returns these with "ll", "ess", "log_w_mean", "log_w_min", "log_w_max", "n_flips" (int64; the kept scans included) as
    ais_log_likelihood_counter forms them, the per-chain "log_w" (N, C), "rb" (N, C, H), "chain_map_lpj" (N, C),
    "chain_map_state" (uint8 (N, C, ceil(H / 8))), "chain_flips" (N, C), beside them "chain_map_bool" (N, C, H), "map_bool"
    (N, H), "first_bool" and "first_flips" (the state and the flips after the first kept scan: ``final_bool`` and
    ``chain_flips`` of ais_log_likelihood_counter), "margin" (N, C; every decision of the chain, the kept scans included)
    and, with ``mean``, "mean" (N, D) = p W^T.  ``x_infr`` (bool (N, D)): incomplete data, as ais_log_likelihood_counter takes
    it; "mean" then covers every entry, the missing ones included.  ``index``: the listed datapoints of
    Model.ais_posterior(index=...) -- only these rows of ``Y`` are walked, each with the stream of data set index first_index
    + index[i], and every array has len(index) rows in list order."""
    C, K = int(n_chains), int(n_keep)
    if C < 1:
        raise ValueError("ais_posterior: n_chains must be positive")
    if K < 1:
        raise ValueError("ais_posterior: n_keep must be positive")
    betas = sigmoid_schedule(n_temps) if betas is None else check_betas(betas)
    T = betas.size - 1
    W = np.asarray(theta["W"], dtype=np.float64)
    Y, mask = _mask_data(np.asarray(Y, dtype=np.float64), x_infr)
    H = W.shape[1]
    if H > AIS_MAX_H:
        raise ValueError("ais_posterior: H = %d, at most %d latents are supported" % (H, AIS_MAX_H))
    pre1, pilb, pi = ais_scalars(theta)
    B = np.dot(Y, W) if B is None else np.asarray(B, dtype=np.float64)
    if mask is not None:
        G = Gd = None  # (every datapoint has its own)
    else:
        G = np.dot(W.T, W) if G is None else np.asarray(G, dtype=np.float64)
        Gd = np.diag(G).copy()
    yy = (Y * Y).sum(axis=1)
    src = np.arange(Y.shape[0], dtype=np.int64) if index is None else check_index(index, Y.shape[0])
    Y, B, yy = Y[src], B[src], yy[src]  # (a row of B = Y W and of yy depends on its own datapoint alone)
    if mask is not None:
        mask = mask[src]
    N = src.size
    seed, first_index = int(seed) & _M64, int(first_index) & _M64
    hs = np.arange(H, dtype=np.uint64)
    out = {"log_w": np.empty((N, C)), "rb": np.empty((N, C, H)), "chain_map_lpj": np.empty((N, C)),
           "chain_map_bool": np.zeros((N, C, H), dtype=bool), "first_bool": np.zeros((N, C, H), dtype=bool),
           "margin": np.empty((N, C)), "p": np.empty((N, H)), "p_se": np.empty((N, H)), "count": np.empty(N),
           "map_lpj": np.empty(N), "map_bool": np.zeros((N, H), dtype=bool)}
    for name in ("ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
        out[name] = np.empty(N)
    chain_flips = np.zeros((N, C), dtype=np.int64)
    first_flips = np.zeros((N, C), dtype=np.int64)
    lz0 = H * np.log1p(np.exp(pilb))

    def scan(s, c, beta, u, flips, margin, R, gd, row):
        """One ascending scan of all chains in place; R (C, H) or None: where the conditionals are added; gd, row: the
        diagonal and the rows of the datapoint's G (_datapoint_gram)."""
        for h in range(H):
            on = s[:, h].copy()
            p = ais_conditional(pre1, pilb, c[:, h], gd[h], on, beta)
            if R is not None:
                R[:, h] = R[:, h] + p
            np.minimum(margin, np.abs(u[:, h] - p), out=margin)
            nb = u[:, h] < p
            up, down = nb & ~on, on & ~nb
            if up.any():
                c[up] = c[up] - row(h)
            if down.any():
                c[down] = c[down] + row(h)
            s[:, h] = nb
            flips += up | down

    with np.errstate(over="ignore"):  # the hashes wrap mod 2^64
        for n in range(N):
            x0 = _first_hash(seed, np.array([(first_index + int(src[n])) & _M64], dtype=np.uint64))
            block = lambda b: _u01_chains(x0, C, np.uint64(b * H) + hs)  # noqa: E731
            flips = np.zeros(C, dtype=np.int64)
            u = block(0)
            s = u < pi
            margin = np.abs(u - pi).min(axis=1)
            gd, row = _datapoint_gram(W, G, Gd, None if mask is None else np.flatnonzero(mask[n]))
            c = np.repeat(B[n][None, :], C, axis=0)
            for i in np.flatnonzero(s.any(axis=0)):
                c[s[:, i]] = c[s[:, i]] - row(i)
            lw = np.zeros(C)
            R = np.zeros((C, H))
            best = np.full(C, -np.inf)
            best_s = np.zeros((C, H), dtype=bool)
            for t in range(1, T + K):
                if t <= T:
                    lw = lw + (betas[t] - betas[t - 1]) * _ell(pre1, yy[n], B[n], c, s)
                kept = t >= T
                scan(s, c, betas[min(t, T)], block(t + 1), flips, margin, R if kept else None, gd, row)
                if kept:
                    lpj = s.sum(axis=1).astype(np.float64) * pilb + _ell(pre1, yy[n], B[n], c, s)
                    better = lpj > best  # (strictly: the earliest scan wins ties)
                    best = np.where(better, lpj, best)
                    best_s[better] = s[better]
                if t == T:
                    out["first_bool"][n] = s
                    first_flips[n] = flips
            r = R / float(K)
            out["log_w"][n], out["rb"][n], out["margin"][n] = lw, r, margin
            out["chain_map_lpj"][n], out["chain_map_bool"][n] = best, best_s
            chain_flips[n] = flips
            lse, ess = _fold(lw)
            out["ll"][n] = (lse - np.log(float(C))) + lz0
            out["ess"][n] = ess
            total = 0.0
            for v in lw:
                total = total + v
            out["log_w_mean"][n] = total / float(C)
            out["log_w_min"][n], out["log_w_max"][n] = lw.min(), lw.max()
            a = np.exp(lw - lse)
            p = np.zeros(H)
            for ch in range(C):
                p = p + a[ch] * r[ch]
            q = np.zeros(H)
            for ch in range(C):
                d = a[ch] * (r[ch] - p)
                q = q + d * d
            out["p"][n], out["p_se"][n] = p, np.sqrt(q)
            cnt = 0.0
            for v in p:
                cnt = cnt + v
            out["count"][n] = cnt
            top = 0
            for ch in range(1, C):
                if best[ch] > best[top]:
                    top = ch
            out["map_lpj"][n], out["map_bool"][n] = best[top], best_s[top]
    out["n_flips"] = chain_flips.sum(axis=1)
    out["chain_flips"], out["first_flips"] = chain_flips, first_flips
    out["chain_map_state"] = np.packbits(out["chain_map_bool"], axis=-1)
    out["map_state"] = np.packbits(out["map_bool"], axis=-1)
    if mean:
        out["mean"] = np.dot(out["p"], W.T)
    return out


def state_digest(state):
    """The digest the device keeps beside a packed state (csrc/common.hpp): bits 0 .. 7 the number of active latents
    (saturated at 255), bits 8 + 14 j .. 8 + 14 j + 13 the j-th active latent in ascending order, j < 4."""
    on = np.flatnonzero(np.asarray(state, dtype=bool))
    d = min(len(on), 255)
    for j, h in enumerate(on[:4]):
        d |= int(h) << (8 + 14 * j)
    return d


def ais_admit_candidates_host(chain_map_lpj, chain_map_state, kn_states, Cmax):
    """The NumPy mirror of the emission of Model.ais_posterior(admit=True) for ONE datapoint (csrc/kernels_ais_post.hpp,
    ADMISSION, states the law).  ``chain_map_lpj`` (C,), ``chain_map_state`` bool (C, H): the chains' best states;
    ``kn_states`` bool (S, H): K^n of the datapoint.  A chain whose lpj is not finite is left out of the walk and of every
    count.  The others rank by lpj descending, ties by ascending chain; in that order a state is dropped when it is
    all-zero, when it equals the state of a chain ranked before it, or when K^n holds it; the first ``Cmax`` of the rest
    are the candidates.  Returns (candidates bool (k, H) in order, counts) with counts = {"n_distinct": the states that are
    not all-zero and repeat no state ranked before them, "n_new": those of them K^n does not hold, "n_proposed": k =
    min(n_new, Cmax), "map_held": whether K^n holds map_state, the best state of the fold (chain 0 when its lpj is NaN,
    else the first chain with the greatest lpj that is not NaN), "chains": the chain of every candidate}."""
    lpj = np.asarray(chain_map_lpj, dtype=np.float64)
    st = np.asarray(chain_map_state, dtype=bool)
    kn = np.asarray(kn_states, dtype=bool).reshape(-1, st.shape[1])
    key = lambda row: np.packbits(row).tobytes()  # noqa: E731
    held = {key(row) for row in kn}
    order = sorted((c for c in range(len(lpj)) if np.isfinite(lpj[c])), key=lambda c: (-lpj[c], c))
    seen, new = set(), []
    n_distinct = 0
    for c in order:
        k = key(st[c])
        if not st[c].any() or k in seen:
            continue
        seen.add(k)
        n_distinct += 1
        if k not in held:
            new.append(c)
    top = 0
    if not np.isnan(lpj[0]):
        for c in range(1, len(lpj)):
            if lpj[c] > lpj[top]:
                top = c
    taken = new[:int(Cmax)]
    counts = {"n_distinct": n_distinct, "n_new": len(new), "n_proposed": len(taken), "map_held": key(st[top]) in held,
              "chains": taken}
    return st[taken].reshape(len(taken), st.shape[1]), counts

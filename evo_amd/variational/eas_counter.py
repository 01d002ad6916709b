"""NumPy mirror of the device EA (csrc/kernels_evolve.hpp: evolve_randflip_kernel, evolve_general_kernel).

The law is evolve_states' (eas.py), the random numbers come from the counter-based stream rng_u01(seed, n, purpose,
index) that the header of kernels_evolve.hpp documents under "THE STREAM".  Everything below is written from that law on
bool rows: duplicates are found by comparing rows, row order is np.unique's.  For a given (seed, n) the kernels must
return these candidates bit for bit, with one reservation:

The parent draw ranks exponential race keys -log(u) / p that the kernels compute in float32.  The mirror computes the
same key in float64 from the same float32-rounded inputs and reports, per datapoint and generation, the MARGIN: the
smallest relative gap (b - a) / b between neighbours a < b among the first P + 1 sorted keys (exactly equal keys -- the
zero-fitness sentinel, or u = 1 -- are resolved by the lowest index on both sides and do not count).  A datapoint whose
margin is below RACE_TAU is undecided from that generation on: the float32 order may differ.  The sparseflip operator
has two float64 transcendental steps; a draw that falls within SPARSE_INT_TOL of an integer (geometric skip) or within
SPARSE_CMP_RTOL of p1 (comparison) marks its datapoint undecided in the same way.
"""
from itertools import combinations

import numpy as np

from .eas import row_keys
from .utils import _M64, _mix64

MUTATIONS = ("randflip", "sparseflip", "cross", "cross_randflip", "cross_sparseflip")

# The device key passes through at most six float32 steps (two conversions, the base-2 logarithm, its scaling by ln 2, a
# reciprocal and a multiplication), each within 1 ULP = 2^-23 relative: within 6 * 2^-23 < 2^-20 of the float64 key.
# RACE_TAU takes a factor 4 over that.  Never tuned from what a device returned.
RACE_TAU = 2.0 ** -18
SPARSE_INT_TOL = 1e-9
SPARSE_CMP_RTOL = 1e-12

_FLT_MIN = np.float32(1.17549435e-38)
_KEY_ZERO_FIT = float(np.float32(1e30))   # p <= 0: taken last
_KEY_CLAMP = float(np.float32(3.0e38))
_EPS = 1e-100


def rng_u01(seed, n, purpose, index):
    """The stream: uniform double in (0, 1) of (seed, datapoint n, purpose, index); n, purpose and index broadcast."""
    seed = int(seed) & _M64
    n = np.atleast_1d(np.asarray(n)).astype(np.uint64)
    purpose = np.atleast_1d(np.asarray(purpose)).astype(np.uint64)
    index = np.atleast_1d(np.asarray(index)).astype(np.uint64)
    with np.errstate(over="ignore"):
        x0 = _mix64(np.uint64(seed) + np.uint64(0x9e3779b97f4a7c15) * (n + np.uint64(1)))
        x = _mix64(x0 ^ (purpose * np.uint64(0xd1b54a32d192ed03) + index + np.uint64(0x632be59bd9b4e019)))
    return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def rng_bits(seed, n, purpose, index):
    """One draw as the exact integer rng_u01 * 2^54 (= 2 (x >> 11) + 1 below 2^52), a Python int: what a test pins."""
    u = float(rng_u01(seed, n, purpose, index).ravel()[0])
    return int(u * 18014398509481984.0)


# ---- parents: exponential races ------------------------------------------------------------------------------------------
def fitness(lpj, fit_parents):
    """p of fitparents (eas.py:139) along the last axis, unnormalised; all ones for randparents."""
    lpj = np.asarray(lpj, dtype=np.float64)
    if not fit_parents:
        return np.ones_like(lpj)
    return lpj - 2.0 * np.minimum(lpj.min(axis=-1, keepdims=True), 0.0)


def race_keys(u, p):
    """key = -log(u) / p in float64 from the float32-rounded inputs of the kernels."""
    uf = np.maximum(np.asarray(u, dtype=np.float64).astype(np.float32), _FLT_MIN)
    e = -np.log(uf.astype(np.float64))
    e = np.where(uf == np.float32(1.0), 0.0, e)
    p32 = np.asarray(p, dtype=np.float64).astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.fmin(e / p32, _KEY_CLAMP)
    return np.where(np.asarray(p) > 0.0, k, _KEY_ZERO_FIT)


def draw_parents(keys, P):
    """The P smallest keys along the last axis in draw order (equal keys: lowest index first) and the margin."""
    order = np.argsort(keys, axis=-1, kind="stable")
    top = np.take_along_axis(keys, order[..., :P + 1], axis=-1)
    a, b = top[..., :-1], top[..., 1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(b > a, (b - a) / b, np.inf)
    margin = gap.min(axis=-1) if gap.shape[-1] else np.full(keys.shape[:-1], np.inf)
    return order[..., :P], margin


# ---- randflip picks --------------------------------------------------------------------------------------------------------
def flip_picks(u, Hd):
    """u (..., T): the T distinct flip positions of one parent.  Pick t takes r = int(u_t (Hd - t)), clamped to
    Hd - t - 1, and lands on the r-th position that the earlier picks left unused."""
    u = np.asarray(u, dtype=np.float64)
    T = u.shape[-1]
    picks = np.empty(u.shape, dtype=np.int64)
    for t in range(T):
        r = np.minimum((u[..., t] * float(Hd - t)).astype(np.int64), Hd - t - 1)
        for q in np.moveaxis(np.sort(picks[..., :t], axis=-1), -1, 0):  # ascending: skip every used position <= r
            r = r + (q <= r)
        picks[..., t] = r
    return picks


def _check(states, lpj, S_perm):
    states = np.asarray(states, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    N, S, H = states.shape
    assert lpj.shape == (N, S_perm + S), (lpj.shape, (N, S_perm + S))
    return states, lpj[:, S_perm:], N, S, H


# ---- the fast kernel -------------------------------------------------------------------------------------------------------
def evolve_randflip_counter(states, lpj, S_perm, n_parents, n_children, seed, fit_parents, background=False):
    """evoamd_evolve_randflip for K^n ``states`` bool (N, S, H) and the lpj rows (N, S_perm + S): returns (cand bool
    (N, n_parents * n_children, H), counts (N,), info).  Slot p * n_children + i holds child i of the p-th drawn parent;
    nothing is de-duplicated.  info: "parents" (N, P) K^n slots in draw order, "flips" (N, P, n_children), "margin"
    (N, 1)."""
    states, lpj, N, S, H = _check(states, lpj, S_perm)
    Hd = H - 1 if background else H
    P, C = int(n_parents), int(n_children)
    n = np.arange(N)
    keys = race_keys(rng_u01(seed, n[:, None], 1, np.arange(S)[None, :]), fitness(lpj, fit_parents))
    parents, margin = draw_parents(keys, P)
    u = rng_u01(seed, n[:, None, None], 2 + np.arange(P)[None, :, None], np.arange(C)[None, None, :])
    flips = flip_picks(u, Hd)
    cand = np.repeat(states[n[:, None], parents], C, axis=1)  # (N, P * C, H)
    cand[n[:, None], np.arange(P * C)[None, :], flips.reshape(N, P * C)] ^= True
    return cand, np.full(N, P * C, dtype=np.int32), {"parents": parents, "flips": flips, "margin": margin[:, None]}


# ---- the general kernel ----------------------------------------------------------------------------------------------------
def sparse_probabilities(Hd, s_abs, sparseness, p_bf):
    """(p0, p1) of sparseflip (eas.py:75-83, same operation order) for parents with s_abs active latents."""
    Hd = float(Hd)
    s_abs = np.asarray(s_abs, dtype=np.float64)
    with np.errstate(all="ignore"):
        alpha = (Hd - s_abs) * ((Hd * p_bf) - (sparseness - s_abs)) / ((sparseness - s_abs + Hd * p_bf) * s_abs + _EPS)
        p0 = (Hd * p_bf) / (Hd + (alpha - 1.0) * s_abs + _EPS)
    return p0, alpha * p0


def _sparseflip(kids, Hd, seed, n, purposes, sparseness, p_bf):
    """Sparse flips of the rows ``kids`` (K, H) over the latents < Hd, every position judged against the row as it
    comes in.  Returns (children, undecided)."""
    K = kids.shape[0]
    orig = kids[:, :Hd]
    p0, p1 = sparse_probabilities(Hd, orig.sum(axis=1), sparseness, p_bf)
    # 1-bits: one uniform each at index 1 + latent
    u = rng_u01(seed, n, purposes[:, None], 1 + np.arange(Hd)[None, :])
    flip = orig & (u < p1[:, None])
    close = orig & (np.abs(u - p1[:, None]) <= SPARSE_CMP_RTOL * np.maximum(np.abs(p1[:, None]), u))
    undecided = bool(close.any())
    # 0-bits: geometric skipping with p0; draw t at index 1 + Hd + t
    every = ~(p0 < 1.0)
    with np.errstate(all="ignore"):
        l1p = np.where(every, -1.0, np.log1p(-np.where(every, 0.5, p0)))
    pos = np.full(K, -1, dtype=np.int64)
    live = p0 > 0.0
    t = 0
    while live.any():
        k = np.flatnonzero(live)
        with np.errstate(all="ignore"):
            q = np.log(rng_u01(seed, n, purposes[k], 1 + Hd + t)) / l1p[k]
        step = np.where(every[k], 0.0, np.floor(q))
        close = ~every[k] & (np.abs(q - np.rint(q)) <= SPARSE_INT_TOL) & (pos[k] + 1 + step <= Hd)
        undecided = undecided or bool(close.any())
        pos[k] += 1 + np.minimum(step, float(Hd)).astype(np.int64)
        t += 1
        live[k[pos[k] >= Hd]] = False
        k = k[pos[k] < Hd]
        flip[k, pos[k]] |= ~orig[k, pos[k]]
    out = kids.copy()
    out[:, :Hd] ^= flip
    return out, undecided


def _children(pool, parents, mutation, Hd, C, seed, n, gsalt, sparseness, p_bf, background):
    """The raw children of one generation of one datapoint, in the kernel's child order, and what was drawn."""
    P = parents.size
    par = pool[parents]
    detail = {}
    if not mutation.startswith("cross"):
        kids = np.repeat(par, C, axis=0)
        if mutation == "randflip":
            flips = flip_picks(rng_u01(seed, n, gsalt + 8 + 1024 + np.arange(P)[:, None], np.arange(C)[None, :]), Hd)
            kids[np.arange(P * C), flips.ravel()] ^= True
            detail["flips"] = flips
    else:
        pairs = list(combinations(range(P), 2))
        kids = np.empty((2 * len(pairs), par.shape[1]), dtype=bool)
        cuts = np.empty(len(pairs), dtype=np.int64)
        for t, (ia, ib) in enumerate(pairs):
            cp = min(1 + int(float(rng_u01(seed, n, gsalt + 8 + 4096 + t, 0)[0]) * (Hd - 1)), Hd - 1)  # randint(1, Hd)
            kids[2 * t] = np.concatenate((par[ia, :cp], par[ib, cp:]))
            kids[2 * t + 1] = np.concatenate((par[ib, :cp], par[ia, cp:]))
            cuts[t] = cp
        detail["cuts"] = cuts
        if background:
            kids[:, Hd:] = True
    K = kids.shape[0]
    purposes = gsalt + 16 + np.arange(K)
    undecided = False
    if mutation == "cross_randflip" and K:
        flips = np.minimum((rng_u01(seed, n, purposes, 0) * float(Hd)).astype(np.int64), Hd - 1)
        kids[np.arange(K), flips] ^= True
        detail["flips"] = flips
    if mutation in ("sparseflip", "cross_sparseflip") and K:
        kids, undecided = _sparseflip(kids, Hd, seed, n, purposes, sparseness, p_bf)
    return kids, undecided, detail


def _packed(rows):
    return np.packbits(rows, axis=1)


def _new_and_unique(known, kids):
    """(the children that equal no row of ``known`` and no earlier child, in np.unique's row order; the positions u >= 1
    of ``known`` that a child equals, ascending)."""
    if kids.shape[0] == 0:
        return kids, np.zeros(0, dtype=np.int64)
    pk, pn = _packed(kids), _packed(known)
    eq_known = (pk[:, None, :] == pn[None, :, :]).all(axis=2)   # (K, U)
    eq_kids = (pk[:, None, :] == pk[None, :, :]).all(axis=2)    # (K, K)
    earlier = np.tril(eq_kids, -1).any(axis=1)
    keep = ~eq_known.any(axis=1) & ~earlier
    hit = np.flatnonzero(eq_known.any(axis=0))
    fresh = kids[keep]
    if fresh.shape[0]:
        _, first = np.unique(row_keys(fresh), return_index=True)
        fresh = fresh[first]
    return fresh, hit[hit >= 1]


def evolve_states_counter(states, lpj, S_perm, mutation, n_parents, n_children, n_generations, seed, fit_parents,
                          sparseness, bitflip_prob, cand_lpj, background=False):
    """evoamd_evolve_states for K^n ``states`` bool (N, S, H) and the lpj rows (N, S_perm + S): returns (cand bool
    (N, Cmax, H) with Cmax = children per generation x n_generations, counts int32 (N,), info).  ``cand_lpj(n, slot0,
    new_states) -> lpj`` is called after every generation of datapoint n with the states just appended at slots slot0..;
    the next pool needs their values.  info: "margin" (N, G) of the parent draw of each generation (inf: nothing to
    decide), "sparse_undecided" bool (N, G), "gen_counts" int (N, G + 1) -- candidates before each generation and at the
    end --, and "draws": per datapoint a list with one dict per generation that ran -- "pool_u" positions in [incl; K^n;
    candidates] of the pool entries, "parents" pool indices in draw order, "flips" / "cuts" where the operator draws
    them, "raw" the children before de-duplication."""
    assert mutation in MUTATIONS, mutation
    states, lpj, N, S, H = _check(states, lpj, S_perm)
    Hd = H - 1 if background else H
    P0, C, G = int(n_parents), int(n_children), int(n_generations)
    crossing = mutation.startswith("cross")
    per_gen = P0 * (P0 - 1) if crossing else P0 * C
    cand = np.zeros((N, per_gen * G, H), dtype=bool)
    counts = np.zeros(N, dtype=np.int32)
    margin = np.full((N, G), np.inf)
    sparse_und = np.zeros((N, G), dtype=bool)
    gen_counts = np.zeros((N, G + 1), dtype=np.int64)
    draws = []
    incl = np.zeros((S_perm, H), dtype=bool)
    for n in range(N):
        known = np.concatenate((incl, states[n]), axis=0)  # [incl; K^n; candidates]
        known_lpj = lpj[n].copy()                          # of known[S_perm:]
        pool, pool_l, pool_u = states[n], known_lpj, S_perm + np.arange(S)
        cnt = 0
        mine = []
        for g in range(G):
            gen_counts[n, g] = cnt
            if pool.shape[0] == 0:
                break
            gsalt = (g + 1) << 32
            P = min(pool.shape[0], P0)
            keys = race_keys(rng_u01(seed, n, gsalt + 1, np.arange(pool.shape[0])), fitness(pool_l, fit_parents))
            parents, margin[n, g] = draw_parents(keys, P)
            kids, sparse_und[n, g], detail = _children(pool, parents, mutation, Hd, C, seed, n, gsalt, sparseness,
                                                       bitflip_prob, background)
            detail.update(pool_u=pool_u, parents=parents, raw=kids)
            mine.append(detail)
            fresh, hit = _new_and_unique(known, kids)
            fresh_l = np.zeros(0)
            if fresh.shape[0]:
                cand[n, cnt:cnt + fresh.shape[0]] = fresh
                fresh_l = np.asarray(cand_lpj(n, cnt, fresh), dtype=np.float64)
            # next pool (eas.py:278-293): the new states, then the known states a child met, with lpj_unique[u - 1]
            pool = np.concatenate((fresh, known[hit]), axis=0)
            pool_l = np.concatenate((fresh_l, known_lpj[hit - 1]))
            pool_u = np.concatenate((S_perm + S + cnt + np.arange(fresh.shape[0]), hit))
            known = np.concatenate((known, fresh), axis=0)
            known_lpj = np.concatenate((known_lpj, fresh_l))
            cnt += fresh.shape[0]
        gen_counts[n, len(mine):] = cnt
        counts[n] = cnt
        draws.append(mine)
    return cand, counts, {"margin": margin, "sparse_undecided": sparse_und, "gen_counts": gen_counts, "draws": draws}


def undecided(info, tau=RACE_TAU):
    """bool (N, G): datapoint n is undecided in generation g or an earlier one (margin below ``tau``, or a sparseflip
    draw too close to call)."""
    bad = info["margin"] < tau
    if "sparse_undecided" in info:
        bad = bad | info["sparse_undecided"]
    return np.logical_or.accumulate(bad, axis=1)

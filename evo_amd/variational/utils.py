"""K^n initialisation and host-side selection with the reference's signatures
(evo/variational/utils.py).  The accelerated E-step uses the device kernel
(csrc/kernels_common.hpp: vary_kn_kernel); ``vary_Kn`` here is the same rule on NumPy arrays for
callers that drive the per-datapoint API."""
from itertools import combinations

import numpy as np

from .eas import (cross, cross_randflip, cross_sparseflip, fitparents, randflip, randparents, row_keys,
                  sparseflip)
from ..utils.parallel import pprint

PARENT_SELECTION = {"fit": fitparents, "rand": randparents}
MUTATION = {"randflip": randflip, "sparseflip": sparseflip, "cross": cross,
            "cross_randflip": cross_randflip, "cross_sparseflip": cross_sparseflip}


def enumerate_states(H):
    """All 2^H binary states ordered by |s|, then by combination order (variational/utils.py:58-67)."""
    rows = [np.fromiter(c, dtype=np.intp, count=g) for g in range(H + 1) for c in combinations(range(H), g)]
    sm = np.zeros((len(rows), H), dtype=bool)
    for i, on in enumerate(rows):
        sm[i, on] = True
    return sm


def _unique_after(blocks, n_before):
    """Rows of concat(blocks) that are first occurrences located at index >= n_before, in
    lexicographic order (what np.unique(..., return_index=True) yields in the reference)."""
    both = np.concatenate(blocks, axis=0)
    _, first = np.unique(row_keys(both), return_index=True)
    return both[first[first >= n_before]]


def init_states(N, S, H, parent_selection, mutation_algorithm, no_parents, no_children, no_generations,
                bitflip_prob=None, Mprime=None, p_init_Kn=None, permanent=None):
    """Build ``my_suff_stat`` (variational/utils.py:19-228): S unique Bernoulli(p_init_Kn) states per
    datapoint (RNG: np.random.random((S,H)) per round, rounds repeated until S unique rows exist)
    plus the EA hyper-parameters.  Keys and dtypes are the reference's.

    ``permanent["background"]`` (:42-47, :96-98, :140-141): the last latent is a background unit, on in every state --
    the draws and the state table ``sm`` cover the other H - 1 latents, and there is no permanent all-zero state
    whatever ``allzero`` says.  ``S == 2 ** H_`` (H_ = latents that vary; < 12) means exact E-steps (:55, :71-88): K^n is
    the whole state table for every datapoint and no random number is drawn (with the permanent all-zero state the
    table's other 2^H - 1 rows: K^n then has one row fewer than S, as in the reference)."""
    permanent = permanent or {"background": False, "allzero": False, "singletons": False}
    background = bool(permanent["background"])
    Hv = H - 1 if background else H
    S_perm = 0 if background else (1 if (permanent["allzero"] == 1 and permanent["singletons"] == 0) else 0)
    incl = np.zeros((S_perm, Hv), dtype=bool)
    sm = enumerate_states(Hv) if Hv < 12 else None
    if S == 2 ** Hv:
        assert Hv < 12, "Exact E-steps too expensive for H={})".format(Hv)
        pprint("Computing exact E-steps")
        if background:
            table = np.concatenate((sm, np.ones((sm.shape[0], 1), dtype=bool)), axis=1)
            lpj = np.empty((N, 2 ** Hv))
        else:
            table = (sm[1:] if S_perm else sm).copy()
            lpj = np.empty((N, S + S_perm))
        ss = np.tile(table[None], (N, 1, 1))
    else:
        p0 = 1.0 / H if p_init_Kn is None else p_init_Kn
        lpj = np.empty((N, S + S_perm))
        ss = np.empty((N, S, H), dtype=bool)
        if background:
            ss[:, :, -1] = True
        for n in range(N):
            have = _unique_after([incl, np.random.random(size=(S, Hv)) < p0], S_perm)
            while have.shape[0] < S:
                more = np.random.random(size=(S, Hv)) < p0
                have = np.concatenate((have, _unique_after([incl, have, more], S_perm + have.shape[0])), axis=0)
            ss[n, :, :Hv] = have[:S]
    if background:
        incl = np.zeros((S_perm, H), dtype=bool)
    if "cross" in mutation_algorithm:
        no_children = no_parents - 1
        pprint("Setting no_children to pre-determined value `no_parents - 1` ({}) when using crossover".format(
            no_parents - 1))
    assert no_parents <= S
    if Mprime is None:
        Mprime = S
    assert Mprime <= S
    return {
        "ss": ss, "lpj": lpj, "permanent": permanent, "incl": incl, "S_perm": S_perm, "sm": sm,
        "n_parents": no_parents, "n_children": no_children, "n_generations": no_generations,
        "parent_selection": PARENT_SELECTION[parent_selection],
        "mutation_algorithm": MUTATION[mutation_algorithm],
        "bitflip_prob": bitflip_prob, "Mprime": Mprime,
    }


def vary_Kn(lpj_old, lpj_new, lpj, states, states_new, H, S, S_perm, incl, Mprime, unification=True,
            reject_worse=True):
    """Selection step (variational/utils.py:231-337) on host arrays, in place.

    Same rule as the device kernel: drop candidates equal to a permanent state, to a member of
    K^n or to an earlier candidate; with M' = min(#kept, Mprime) the j-th best kept candidate
    replaces the j-th worst old state while it is strictly better (j = 1..M').  For tie-free
    inputs this is exactly the reference's argpartition / argsort construction; for exact ties
    NumPy's order is unspecified and the rule here is "no swap on equality, lowest index first".
    Returns (#new unique, #swapped).  ``unification=False`` keeps the reference's set-replacement
    behaviour (variational/utils.py:325-335)."""
    kept = _unique_after_idx([incl, states, states_new], S + S_perm)
    if not unification:
        if reject_worse and (lpj_new.sum() < lpj_old.sum()):
            lpj[:] = lpj_old
            return 0, 0
        lpj[:] = lpj_new
        states[:, :] = states_new
        return kept.size, kept.size
    cand = states_new[kept]
    cand_lpj = lpj_new[kept]
    m = min(cand_lpj.size, Mprime)
    best_new = np.argsort(-cand_lpj, kind="stable")[:m]
    worst_old = np.argsort(lpj_old, kind="stable")[:m]
    n_sub = 0
    for j in range(m):
        if not cand_lpj[best_new[j]] > lpj_old[worst_old[j]]:
            break
        states[worst_old[j]] = cand[best_new[j]]
        lpj_old[worst_old[j]] = cand_lpj[best_new[j]]
        n_sub += 1
    lpj[:] = lpj_old
    return kept.size, n_sub


def _unique_after_idx(blocks, n_before):
    both = np.concatenate(blocks, axis=0)
    _, first = np.unique(row_keys(both), return_index=True)
    return first[first >= n_before] - n_before


# ---- K^n(0) with a counter-based stream: the NumPy mirror of evoamd_init_states (csrc/kernels_init.hpp) ----------------
#
# The law is init_states' above.  The stream: the bit of (datapoint n, round r, candidate s, latent h) is
#     rng_u01(seed, n, INIT_PURPOSE + r, s * Hv + h) < p0
# with the device EA's generator (csrc/kernels_evolve.hpp),
#     mix64(x):  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31   (mod 2^64)
#     rng_u01(seed, n, purpose, index) = ((x >> 11) + 0.5) * 2^-53   with
#     x = mix64(mix64(seed + 0x9e3779b97f4a7c15 * (n + 1)) ^ (purpose * 0xd1b54a32d192ed03 + index + 0x632be59bd9b4e019))
# -- integer hashing, one exact integer -> double conversion, one IEEE addition and a multiplication by a power of two, so
# the kernel and this file agree bit for bit.  The kernel, this mirror and their tests depend on this definition.
INIT_PURPOSE = 0x494E495400000000
_M64 = (1 << 64) - 1


def _mix64(x):
    """mix64 on a Python int (exact) or on a uint64 array (wraps mod 2^64)."""
    if isinstance(x, np.ndarray):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & _M64
    return x ^ (x >> 31)


def counter_draw(seed, S, Hv, p0):
    """draw(n, r) -> bool (S, Hv): the candidates of round r of datapoint n under the stream above."""
    seed = int(seed) & _M64
    index = np.arange(S * Hv, dtype=np.uint64).reshape(S, Hv)  # s * Hv + h

    def draw(n, r):
        x0 = _mix64((seed + 0x9e3779b97f4a7c15 * (int(n) + 1)) & _M64)
        salt = ((INIT_PURPOSE + int(r)) * 0xd1b54a32d192ed03 + 0x632be59bd9b4e019) & _M64
        x = _mix64(np.uint64(x0) ^ (np.uint64(salt) + index))
        return ((x >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0) < p0

    return draw


def assemble_states(N, S, H, draw, permanent=None, max_rounds=256):
    """The law of init_states with the candidates of (datapoint n, round r) taken from ``draw(n, r) -> bool (S, Hv)``:
    bool (N, S, H) -- in the exact mode (S == 2 ** Hv) the state table for every datapoint, S - S_perm rows, and ``draw`` is
    never called.  RuntimeError naming the cap when a datapoint holds fewer than S states after ``max_rounds`` rounds
    (the reference loops without bound; shapes with S close to 2 ** Hv need hundreds of rounds and belong to
    init_states)."""
    permanent = permanent or {"background": False, "allzero": False, "singletons": False}
    background = bool(permanent["background"])
    Hv = H - 1 if background else H
    S_perm = 0 if background else (1 if (permanent["allzero"] == 1 and permanent["singletons"] == 0) else 0)
    incl = np.zeros((S_perm, Hv), dtype=bool)
    if S == 2 ** Hv:
        assert Hv < 12, "Exact E-steps too expensive for H={})".format(Hv)
        sm = enumerate_states(Hv)
        if background:
            table = np.concatenate((sm, np.ones((sm.shape[0], 1), dtype=bool)), axis=1)
        else:
            table = sm[1:] if S_perm else sm
        return np.tile(table[None], (N, 1, 1))
    ss = np.empty((N, S, H), dtype=bool)
    if background:
        ss[:, :, -1] = True
    for n in range(N):
        have = _unique_after([incl, draw(n, 0)], S_perm)
        r = 1
        while have.shape[0] < S:
            if r >= max_rounds:
                raise RuntimeError("init_states_counter: datapoint %d holds %d of S = %d distinct states after max_rounds = %d "
                                   "rounds (the round cap)" % (n, have.shape[0], S, max_rounds))
            have = np.concatenate((have, _unique_after([incl, have, draw(n, r)], S_perm + have.shape[0])), axis=0)
            r += 1
        ss[n, :, :Hv] = have[:S]
    return ss


def init_states_counter(N, S, H, seed, p_init_Kn=None, permanent=None, max_rounds=256):
    """my_suff_stat["ss"] as evoamd_init_states / Model.init_resident_states draw it for ``seed``: init_states' law, the
    counter-based stream documented above (not NumPy's Mersenne-Twister stream).  ``S`` is init_states' argument: a
    model of 2 ** Hv - 1 states with the permanent all-zero state runs exact E-steps (Model.init_resident_states copies
    the state table), which is ``S = 2 ** Hv`` here, as it is for init_states; ``S = 2 ** Hv - 1`` here SAMPLES the
    2 ** Hv - 1 non-zero states, as init_states does (hundreds of rounds)."""
    background = bool(permanent["background"]) if permanent else False
    Hv = H - 1 if background else H
    p0 = 1.0 / H if p_init_Kn is None else p_init_Kn
    return assemble_states(N, S, H, counter_draw(seed, S, Hv, p0), permanent, max_rounds)

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


# ---- K^n seeded from Theta and the data: the NumPy mirror of evoamd_seed_states (csrc/kernels_seed.hpp) ------------------
#
# Greedy forward selection on the model's own lpj (without ljc, without the lpj_reset_check clamp).  Per datapoint, with
# A = max_active steps, A_0 = {} and quotas q_t = S // A + (t <= S % A): step t scores every latent j outside A_{t-1} with
# lpj(A_{t-1} + {j}), ranks by descending score (ties: ascending j; a score that is not finite, or an ES3C det T that is not
# positive, is -inf), writes the q_t best states to the next q_t slots in rank order and keeps the best as A_t.
SEED_MAX_ACTIVE = {"bsc": 64, "sssc": 8}


def seed_quotas(S, Hv, max_active, sssc):
    """The quotas q_1 .. q_A of the seeding law; ValueError naming the rule for a ``max_active`` the law refuses."""
    A, cap = int(max_active), SEED_MAX_ACTIVE["sssc" if sssc else "bsc"]
    if A < 1 or A > S or A > Hv or A > cap:
        raise ValueError("seed_states: max_active = %d must be in [1, min(S = %d, Hv = %d, %d)] (%s)"
                         % (A, S, Hv, cap, "ES3C: at most 8" if sssc else "EBSC: at most 64"))
    q = [S // A + (1 if t <= S % A else 0) for t in range(1, A + 1)]
    for t, qt in enumerate(q, start=1):
        if qt > Hv - (t - 1):
            raise ValueError("seed_states: the quota q_%d = %d exceeds the Hv - (t - 1) = %d latents left at step %d "
                             "(S = %d, max_active = %d)" % (t, qt, Hv - (t - 1), t, S, A))
    return q


def _seed_scores_sssc(G, Psi, mus, pil_bar, s2inv, b_n, yy_n, active, cand):
    """ES3C lpj of active + [j] for every j of ``cand`` (the quantities of models/predictive.py: state_posterior_es3c)."""
    k = len(active) + 1
    idx = np.empty((len(cand), k), dtype=np.intp)
    idx[:, :k - 1] = active
    idx[:, k - 1] = cand
    Gb = G[idx[:, :, None], idx[:, None, :]]
    Pb = Psi[idx[:, :, None], idx[:, None, :]]
    mu, b = mus[idx], b_n[idx]
    v = b - np.einsum("cij,cj->ci", Gb, mu)
    rr = yy_n - (mu * (b + v)).sum(axis=1)
    T = np.eye(k)[None] + Pb @ Gb * s2inv
    rhs = np.einsum("cij,cj->ci", Pb, v)
    sign, logdet = np.linalg.slogdet(T)
    try:
        x = np.linalg.solve(T, rhs[:, :, None])[:, :, 0]
    except np.linalg.LinAlgError:  # an exactly singular system among them: one by one
        x = np.full_like(rhs, np.nan)
        for c in range(len(cand)):
            try:
                x[c] = np.linalg.solve(T[c], rhs[c])
            except np.linalg.LinAlgError:
                pass
    with np.errstate(invalid="ignore", over="ignore"):
        lpj = pil_bar[idx].sum(axis=1) - 0.5 * (logdet + rr * s2inv - (v * x).sum(axis=1) * s2inv * s2inv)
    return np.where((sign > 0) & np.isfinite(lpj), lpj, -np.inf)


def _seed_gap(a, b):
    if not (np.isfinite(a) and np.isfinite(b)):
        return np.inf  # -inf ranks last and among themselves by j: nothing a rounding error decides
    return (a - b) / max(1.0, abs(a))


def seed_states_host(model, theta, Y, S, max_active, S_perm=0, x_infr=None):
    """K^n as evoamd_seed_states / Model.seed_resident_states lay it out.  ``model``: "bsc" or "sssc"; ``theta``: W, pi,
    sigma (EBSC) or W, pies, mus, Psi, sigma2 (ES3C); ``Y`` (N, D) complete data; ``S`` varying states per datapoint (the
    permanent all-zero state of ``S_perm`` = 1 is not among them and is never produced).  Returns (states, path,
    lpj_path, margin): states bool (N, S, H); path int32 (N, A), the latent added at each step; lpj_path (N, A), the
    winner's score; margin (N,), the smallest relative gap (a - b) / max(1, |a|) over the steps of a datapoint between
    the winner and the runner-up and between rank q_t - 1 and rank q_t -- a datapoint whose margin is far above the
    rounding error of the scores is decided the same way by any correct implementation.
    ``x_infr`` bool (N, D), incomplete data: datapoint n is scored on its reliable entries o = x_infr[n] alone --
    G(n) = W_o^T W_o, B_n = y_o^T W_o, yy_n = |y_o|^2 (the lpj of the reference's W[this_x_infr, :] branches); entries of Y
    under False are never read as numbers (NaN included); a datapoint without a reliable entry is scored by the prior
    alone.  None: complete data."""
    sssc = model not in ("bsc", "BSC", "ebsc")
    assert S_perm in (0, 1)
    W = np.asarray(theta["W"], dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    (D, H), N = W.shape, Y.shape[0]
    assert Y.shape == (N, D)
    A = int(max_active)
    quotas = seed_quotas(int(S), H, A, sssc)
    if x_infr is None:
        G, B, yy = W.T @ W, Y @ W, (Y * Y).sum(axis=1)
    else:
        x_infr = np.asarray(x_infr, dtype=bool)
        assert x_infr.shape == (N, D)
        Y = np.where(x_infr, Y, 0.0)
        G, B, yy = None, Y @ W, (Y * Y).sum(axis=1)
    if sssc:
        mus, Psi = np.asarray(theta["mus"], dtype=np.float64), np.asarray(theta["Psi"], dtype=np.float64)
        pies = np.asarray(theta["pies"], dtype=np.float64)
        pil_bar, s2inv = np.log(pies / (1.0 - pies)), 1.0 / float(theta["sigma2"])
    else:
        pi, sigma = float(theta["pi"]), float(theta["sigma"])
        pre1, pil_bar = -1.0 / 2.0 / sigma / sigma, np.log(pi / (1.0 - pi))
        Gd = None if G is None else np.diag(G).copy()
    states = np.zeros((N, S, H), dtype=bool)
    path = np.zeros((N, A), dtype=np.int32)
    lpj_path = np.zeros((N, A))
    margin = np.full(N, np.inf)
    masked = x_infr is not None
    for n in range(N):
        if masked:  # the datapoint's own Gram matrix, from the reliable rows of W
            Wo = W[x_infr[n]]
            G = Wo.T @ Wo
            Gd = np.diag(G).copy()
        active, free = [], np.ones(H, dtype=bool)
        c, base, slot = B[n].copy(), (0.0 if sssc else pre1 * yy[n]), 0
        for t, q in enumerate(quotas, start=1):
            cand = np.flatnonzero(free)
            if sssc:
                score = _seed_scores_sssc(G, Psi, mus, pil_bar, s2inv, B[n], yy[n], active, cand)
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    score = base + pil_bar + pre1 * (Gd[cand] - 2.0 * c[cand])
                score = np.where(np.isfinite(score), score, -np.inf)
            order = np.lexsort((cand, -score))  # descending score, ties (and the -inf ones) by ascending j
            ranked, sc = cand[order], score[order]
            if len(sc) > 1:
                margin[n] = min(margin[n], _seed_gap(sc[0], sc[1]))
            if q < len(sc):
                margin[n] = min(margin[n], _seed_gap(sc[q - 1], sc[q]))
            for r in range(q):
                states[n, slot + r, active] = True
                states[n, slot + r, ranked[r]] = True
            jw = int(ranked[0])
            path[n, t - 1], lpj_path[n, t - 1] = jw, sc[0]
            active.append(jw)
            free[jw] = False
            c -= G[jw]
            base = sc[0]
            slot += q
    return states, path, lpj_path, margin


# ---- beam seeding: the NumPy mirror of evoamd_seed_states_beam (csrc/kernels_seed_beam.hpp has the law) --------------------
SEED_BEAM_MAX = 16


def seed_beam_check(S, max_active, beam):
    """ValueError naming ``beam`` unless 1 <= beam <= min(S // max_active, SEED_BEAM_MAX) (every beam member is a stored
    state)."""
    B, top = int(beam), int(S) // int(max_active)
    if B < 1 or B > top or B > SEED_BEAM_MAX:
        raise ValueError("seed_states: beam = %d must be in [1, min(S // max_active = %d, %d)]" % (B, top, SEED_BEAM_MAX))
    return B


def seed_states_beam_host(model, theta, Y, S, max_active, beam, S_perm=0):
    """K^n as evoamd_seed_states_beam / Model.seed_resident_states(beam=B) lay it out: the law of seed_states_host with the
    ``beam`` = B best partial states kept per step (rank order) and all of them expanded.  A member carries its path, and
    its candidates P_r + {j} are scored in the arithmetic of that path (EBSC: c = B_n - G_{w_1} - ... in path order and
    score = lpj(P_r) + pil_bar + pre1 (G_jj - 2 c_j) with lpj(P_r) the score the member was ranked with; ES3C: the system in
    path order).  A candidate whose set an earlier parent reaches as well is absent (a test on the sets, never on scores);
    all candidates of a step are ranked by descending score, ties by ascending parent rank, then ascending j; the q_t best
    fill the step's slots in rank order and the first B of them are the next beam.  B = 1 is seed_states_host exactly.
    Complete data only.  Returns (states bool (N, S, H), lpj (N, S) the score every slot was ranked with, path int32 (N, A)
    the path of the rank-0 state of the last step, lpj_path (N, A) the rank-0 score of each step, margin (N,)): margin is
    the smallest relative gap (_seed_gap) between any two adjacent ranks among the first max(q_t, B) + 1 ranked candidates,
    over the steps -- everything that decides the output."""
    sssc = model not in ("bsc", "BSC", "ebsc")
    assert S_perm in (0, 1)
    W = np.asarray(theta["W"], dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    (D, H), N = W.shape, Y.shape[0]
    assert Y.shape == (N, D)
    A = int(max_active)
    quotas = seed_quotas(int(S), H, A, sssc)
    nB = seed_beam_check(S, A, beam)
    G, Bm, yy = W.T @ W, Y @ W, (Y * Y).sum(axis=1)
    if sssc:
        mus, Psi = np.asarray(theta["mus"], dtype=np.float64), np.asarray(theta["Psi"], dtype=np.float64)
        pies = np.asarray(theta["pies"], dtype=np.float64)
        pil_bar, s2inv = np.log(pies / (1.0 - pies)), 1.0 / float(theta["sigma2"])
    else:
        pi, sigma = float(theta["pi"]), float(theta["sigma"])
        pre1, pil_bar = -1.0 / 2.0 / sigma / sigma, np.log(pi / (1.0 - pi))
        Gd = np.diag(G).copy()
    states = np.zeros((N, S, H), dtype=bool)
    lpj = np.zeros((N, S))
    path = np.zeros((N, A), dtype=np.int32)
    lpj_path = np.zeros((N, A))
    margin = np.full(N, np.inf)
    for n in range(N):
        # a member: (path, score, c) with c = B_n minus the rows of G of its path, in path order (EBSC)
        members = [([], 0.0 if sssc else pre1 * yy[n], None if sssc else Bm[n].copy())]
        slot = 0
        for t, q in enumerate(quotas, start=1):
            sc_all, par_all, j_all = [], [], []
            sets = [frozenset(m[0]) for m in members]
            for r, (pth, base, c) in enumerate(members):
                free = np.ones(H, dtype=bool)
                free[pth] = False
                for r2 in range(r):  # the sets an earlier parent reaches
                    extra = sets[r2] - sets[r]
                    if len(extra) == 1:
                        free[next(iter(extra))] = False
                cand = np.flatnonzero(free)
                if sssc:
                    score = _seed_scores_sssc(G, Psi, mus, pil_bar, s2inv, Bm[n], yy[n], pth, cand)
                else:
                    with np.errstate(invalid="ignore", over="ignore"):
                        score = base + pil_bar + pre1 * (Gd[cand] - 2.0 * c[cand])
                    score = np.where(np.isfinite(score), score, -np.inf)
                sc_all.append(score)
                par_all.append(np.full(len(cand), r))
                j_all.append(cand)
            sc_all, par_all, j_all = np.concatenate(sc_all), np.concatenate(par_all), np.concatenate(j_all)
            order = np.lexsort((j_all, par_all, -sc_all))  # descending score, then parent rank, then j
            sc, par, jj = sc_all[order], par_all[order], j_all[order]
            for i in range(min(max(q, nB), len(sc) - 1)):
                margin[n] = min(margin[n], _seed_gap(sc[i], sc[i + 1]))
            for r in range(q):
                states[n, slot + r, members[par[r]][0]] = True
                states[n, slot + r, jj[r]] = True
                lpj[n, slot + r] = sc[r]
            lpj_path[n, t - 1] = sc[0]
            if t == A:
                path[n] = members[par[0]][0] + [int(jj[0])]
            members = [(members[par[i]][0] + [int(jj[i])], sc[i], None if sssc else members[par[i]][2] - G[jj[i]])
                       for i in range(min(nB, q))]
            slot += q
    return states, lpj, path, lpj_path, margin


# ---- local search on K^n: the NumPy mirror of one sweep's proposals (csrc/kernels_sweep.hpp has the law) -----------------
def sweep_states_host(model, theta, Y, ss, lpj, S_perm, n_parents, n_keep, x_infr=None):
    """One sweep's proposals as evoamd_sweep_propose emits them.  ``ss`` bool (N, S, H) and ``lpj`` (N, S_perm + S) are
    taken as given, so the choice of the parents (the ``n_parents`` = P varying states with the largest lpj, ties by
    ascending slot) is exact.  Every one-flip neighbour of a parent is scored with the model's lpj (no ljc, no clamp) unless
    it is the all-zero state, K^n holds it, or it has more than SEED_MAX_ACTIVE latents; per parent the ``n_keep`` = q best
    (descending score, ties by ascending latent; scores that are not finite are never proposed) are emitted parent-major,
    then by rank.  Returns (cand bool (N, P q, H), counts int32 (N,), scores (N, P q) -- NaN beyond counts --, best_flip
    int32 (N,), gain (N,), n_capped int32 (N,), margin (N,)): best_flip / gain describe the best scored neighbour of parent
    0 (-1 / -inf without one; gain NaN when an ES3C parent 0 above 8 latents has no score of its own), n_capped counts the
    parents that lost a neighbour to the cap, margin is the smallest relative gap (a - b) / max(1, |a|) between
    consecutive chosen ranks and between rank q - 1 and rank q over the datapoint's parents.
    ``x_infr`` bool (N, D), incomplete data: datapoint n is scored on its reliable entries o = x_infr[n] alone, as in
    seed_states_host -- G(n) = W_o^T W_o, B_n = y_o^T W_o, yy_n = |y_o|^2; entries of Y under False are never read as
    numbers (NaN included) and a datapoint without a reliable entry is scored by the prior alone.  ``lpj`` is then the
    masked lpj of ``ss``.  None: complete data."""
    fs = _FlipScores(model, theta, Y, ss, lpj, S_perm, x_infr)
    N, S, H = fs.N, fs.S, fs.H
    P, q = int(n_parents), int(n_keep)
    if not (1 <= P <= min(S, 64)) or q < 1:
        raise ValueError("sweep_states: n_parents = %d must be in [1, min(S = %d, 64)] and n_keep = %d positive" % (P, S, q))
    cand = np.zeros((N, P * q, H), dtype=bool)
    counts = np.zeros(N, dtype=np.int32)
    scores = np.full((N, P * q), np.nan)
    best_flip = np.full(N, -1, dtype=np.int32)
    gain = np.full(N, -np.inf)
    n_capped = np.zeros(N, dtype=np.int32)
    margin = np.full(N, np.inf)
    for n in range(N):
        for r, slot in enumerate(fs.parents(n)[:P]):
            p = fs.ss[n, slot]
            sc, lost, base = fs.neighbours(n, p)
            n_capped[n] += lost
            js = np.flatnonzero(np.isfinite(sc))
            order = np.lexsort((js, -sc[js]))
            ranked, rs = js[order], sc[js][order]
            k = min(q, len(ranked))
            for i in range(k):
                if i + 1 < len(rs):
                    margin[n] = min(margin[n], _seed_gap(rs[i], rs[i + 1]))
                at = counts[n] + i
                cand[n, at] = p
                cand[n, at, ranked[i]] = ~p[ranked[i]]
                scores[n, at] = rs[i]
            counts[n] += k
            if r == 0 and k:
                best_flip[n], gain[n] = ranked[0], rs[0] - base
    return cand, counts, scores, best_flip, gain, n_capped, margin


class _FlipScores:
    """What sweep_states_host and neighbour_bound_host share (the flip law of csrc/kernels_sweep.hpp): the parents of a
    datapoint and the score of every one-flip neighbour of a parent."""

    def __init__(self, model, theta, Y, ss, lpj, S_perm, x_infr=None):
        self.sssc = model not in ("bsc", "BSC", "ebsc")
        assert S_perm in (0, 1)
        self.S_perm = S_perm
        W = self.W = np.asarray(theta["W"], dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        self.masked = x_infr is not None
        if self.masked:
            self.x_infr = np.asarray(x_infr, dtype=bool)
            assert self.x_infr.shape == Y.shape
            Y = np.where(self.x_infr, Y, 0.0)
        self.ss = np.asarray(ss, dtype=bool)
        self.lpj = np.asarray(lpj, dtype=np.float64)
        (D, self.H), (self.N, self.S) = W.shape, self.ss.shape[:2]
        assert Y.shape == (self.N, D) and self.ss.shape == (self.N, self.S, self.H)
        assert self.lpj.shape == (self.N, S_perm + self.S)
        self.cap = SEED_MAX_ACTIVE["sssc" if self.sssc else "bsc"]
        self.G, self.B, self.yy = W.T @ W, Y @ W, (Y * Y).sum(axis=1)
        self.Gd = np.diag(self.G).copy()
        self.n_G = None  # masked: the datapoint whose Gram matrix G is
        if self.sssc:
            self.mus, self.Psi = np.asarray(theta["mus"], dtype=np.float64), np.asarray(theta["Psi"], dtype=np.float64)
            pies = np.asarray(theta["pies"], dtype=np.float64)
            self.pil_bar, self.s2inv = np.log(pies / (1.0 - pies)), 1.0 / float(theta["sigma2"])
        else:
            pi, sigma = float(theta["pi"]), float(theta["sigma"])
            self.pre1, self.pil_bar = -1.0 / 2.0 / sigma / sigma, np.log(pi / (1.0 - pi))

    def _gram(self, n):
        if self.masked and self.n_G != n:  # the datapoint's own Gram matrix, from the reliable rows of W
            Wo = self.W[self.x_infr[n]]
            self.G = Wo.T @ Wo
            self.Gd = np.diag(self.G).copy()
            self.n_G = n

    def _state_lpj(self, n, act):
        if len(act) == 0:
            return -0.5 * self.yy[n] * self.s2inv
        return float(_seed_scores_sssc(self.G, self.Psi, self.mus, self.pil_bar, self.s2inv, self.B[n], self.yy[n],
                                       list(act[:-1]), np.array(act[-1:]))[0])

    def parents(self, n):
        """The S varying slots of datapoint n by descending lpj, ties by ascending slot."""
        row = np.where(np.isfinite(self.lpj[n, self.S_perm:]), self.lpj[n, self.S_perm:], -np.inf) + 0.0
        return np.lexsort((np.arange(self.S), -row))

    def neighbours(self, n, p):
        """(sc, lost, base) of the parent ``p`` (bool (H,)) of datapoint n: sc (H,) the score of p with bit j flipped, -inf
        where that state is all-zero, held by K^n, above the cap or has no finite score; lost: a neighbour went to the
        cap; base: the score of p itself (ES3C above the cap: NaN)."""
        self._gram(n)
        G, B, yy, cap, H = self.G, self.B, self.yy, self.cap, self.H
        act = np.flatnonzero(p)
        m = len(act)
        diff = self.ss[n] ^ p
        one = diff.sum(axis=1) == 1
        held = np.zeros(H, dtype=bool)
        held[np.argmax(diff[one], axis=1)] = True
        size = np.where(p, m - 1, m + 1)
        live = (size > 0) & ~held
        lost = live & (size > cap)
        live &= ~lost
        sc = np.full(H, -np.inf)
        if self.sssc:
            base = self._state_lpj(n, act) if m <= cap else np.nan
            add = np.flatnonzero(live & ~p)
            if len(add):
                sc[add] = _seed_scores_sssc(G, self.Psi, self.mus, self.pil_bar, self.s2inv, B[n], yy[n], list(act), add)
            for j in np.flatnonzero(live & p):
                sc[j] = self._state_lpj(n, act[act != j])
        else:
            pre1, pil_bar = self.pre1, self.pil_bar
            c = B[n] - G[act].sum(axis=0)
            base = pre1 * (yy[n] - (B[n, act] + c[act]).sum()) + m * pil_bar
            with np.errstate(invalid="ignore", over="ignore"):
                both = np.where(p, base - pil_bar + pre1 * (self.Gd + 2.0 * c), base + pil_bar + pre1 * (self.Gd - 2.0 * c))
            sc[live] = both[live]
        sc[~np.isfinite(sc)] = -np.inf
        return sc, bool(lost.any()), base


# ---- the neighbourhood bound: the NumPy mirror of evoamd_neighbour_bound (csrc/kernels_nbound.hpp has the law) --------------
def neighbour_bound_host(model, theta, Y, ss, lpj, S_perm, n_parents, x_infr=None):
    """The exact mass of the one-flip neighbours of K^n as evoamd_neighbour_bound sums it, written from the law on bool rows.
    ``ss`` bool (N, S, H) and ``lpj`` (N, S_perm + S) are taken as given; the parents are the ``n_parents`` = P (1 <= P <= S)
    varying states with the largest lpj, ties by ascending slot, and the scores are those of sweep_states_host.  A
    neighbour -- parent r with bit j flipped -- is absent when it is (a) the all-zero state, (b) held by K^n, (c) above
    SEED_MAX_ACTIVE latents (``n_capped`` counts the parents that lost one so), (d) owned by an earlier parent: some r' < r is
    two flips from parent r and j is one of the two differing bits; or when its score is not finite.  Returns a dict of
    (N,) arrays: "F" = logsumexp of the lpj row, "M" = log sum exp of the present scores (-inf without one), "F_plus" =
    logaddexp(F, M), "gap", "mass_outside" = exp(M - F_plus), "n_states", "n_capped" (int32), "best_score", "best_parent"
    (rank) and "best_flip" (int32) of the largest present score, ties by ascending rank, then latent (-inf / -1 / -1
    without one), and "margin", the relative gap (a - b) / max(1, |a|) between the two largest present scores (inf with
    fewer than two).  A row with a NaN or +inf, or all -inf ("bad weights"): NaN in the real-valued arrays, 0 / -1 in the
    others.  ``x_infr`` as for sweep_states_host."""
    fs = _FlipScores(model, theta, Y, ss, lpj, S_perm, x_infr)
    N, S, H = fs.N, fs.S, fs.H
    P = int(n_parents)
    if not 1 <= P <= S:
        raise ValueError("neighbour_bound: n_parents = %d must be in [1, S = %d]" % (P, S))
    out = {name: np.full(N, np.nan) for name in ("F", "M", "F_plus", "gap", "mass_outside")}
    out["best_score"] = np.full(N, -np.inf)
    out["margin"] = np.full(N, np.inf)
    for name in ("n_states", "n_capped"):
        out[name] = np.zeros(N, dtype=np.int32)
    for name in ("best_parent", "best_flip"):
        out[name] = np.full(N, -1, dtype=np.int32)
    for n in range(N):
        row = fs.lpj[n]
        if np.isnan(row).any() or (row == np.inf).any() or not (row > -np.inf).any():
            continue  # bad weights
        mx = row.max()
        F = mx + np.log(np.exp(row - mx).sum())
        parents = fs.parents(n)[:P]
        present = []  # (score, r, j)
        for r, slot in enumerate(parents):
            p = fs.ss[n, slot]
            sc, lost, _ = fs.neighbours(n, p)
            out["n_capped"][n] += lost
            for r2 in range(r):  # (d)
                d = np.flatnonzero(fs.ss[n, parents[r2]] ^ p)
                if len(d) == 2:
                    sc[d] = -np.inf
            present += [(sc[j], r, j) for j in np.flatnonzero(np.isfinite(sc))]
        out["F"][n] = F
        out["n_states"][n] = len(present)
        M = -np.inf
        if present:
            v = np.array([t[0] for t in present])
            M = v.max() + np.log(np.exp(v - v.max()).sum())
            present.sort(key=lambda t: (-t[0], t[1], t[2]))
            out["best_score"][n], out["best_parent"][n], out["best_flip"][n] = present[0]
            if len(present) > 1:
                out["margin"][n] = _seed_gap(present[0][0], present[1][0])
        out["M"][n] = M
        out["F_plus"][n] = np.logaddexp(F, M)
        out["gap"][n] = out["F_plus"][n] - F
        out["mass_outside"][n] = np.exp(M - out["F_plus"][n])
    return out


# ---- local search on K^n, the swap neighbourhood: the NumPy mirror of the swap stage (csrc/kernels_sweep_swap.hpp has the law)
def swap_states_host(model, theta, Y, ss, lpj, S_perm, n_parents, n_keep):
    """One sweep's swap proposals as evoamd_sweep_propose_nb emits them with EVOAMD_SWEEP_SWAP | EVOAMD_SWEEP_NO_FLIP (with
    both stages on they follow the rows of sweep_states_host).  ``ss`` bool (N, S, H) and ``lpj`` (N, S_perm + S) are taken
    as given; the parents are those of sweep_states_host.  Every swap of a parent p -- a in p switched off, j not in p
    switched on -- is scored with the model's lpj (no ljc, no clamp) unless K^n holds that state; a parent above
    SEED_MAX_ACTIVE latents has none of its swaps scored and counts in n_capped_swap, an empty parent has no swaps.  Per
    parent the ``n_keep`` = q best (descending score, ties by ascending a, then ascending j; scores that are not finite are
    never proposed) are emitted parent-major, then by rank.  Complete data only.  Returns (cand bool (N, P q, H), counts
    int32 (N,), scores (N, P q) -- NaN beyond counts --, best_swap int32 (N, 2), swap_gain (N,), n_capped_swap int32 (N,),
    margin (N,)): best_swap / swap_gain describe the best scored swap of parent 0 ((-1, -1) / -inf without one), margin is
    the smallest relative gap (a - b) / max(1, |a|) between consecutive chosen ranks and between rank q - 1 and rank q
    over the datapoint's parents, as in sweep_states_host."""
    sssc = model not in ("bsc", "BSC", "ebsc")
    assert S_perm in (0, 1)
    W = np.asarray(theta["W"], dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    ss = np.asarray(ss, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    (D, H), (N, S) = W.shape, ss.shape[:2]
    assert Y.shape == (N, D) and ss.shape == (N, S, H) and lpj.shape == (N, S_perm + S)
    P, q = int(n_parents), int(n_keep)
    if not (1 <= P <= min(S, 64)) or q < 1:
        raise ValueError("swap_states: n_parents = %d must be in [1, min(S = %d, 64)] and n_keep = %d positive" % (P, S, q))
    cap = SEED_MAX_ACTIVE["sssc" if sssc else "bsc"]
    G, B, yy = W.T @ W, Y @ W, (Y * Y).sum(axis=1)
    if sssc:
        mus, Psi = np.asarray(theta["mus"], dtype=np.float64), np.asarray(theta["Psi"], dtype=np.float64)
        pies = np.asarray(theta["pies"], dtype=np.float64)
        pil_bar, s2inv = np.log(pies / (1.0 - pies)), 1.0 / float(theta["sigma2"])
    else:
        pi, sigma = float(theta["pi"]), float(theta["sigma"])
        pre1, pil_bar = -1.0 / 2.0 / sigma / sigma, np.log(pi / (1.0 - pi))
        Gd = np.diag(G).copy()
    cand = np.zeros((N, P * q, H), dtype=bool)
    counts = np.zeros(N, dtype=np.int32)
    scores = np.full((N, P * q), np.nan)
    best_swap = np.full((N, 2), -1, dtype=np.int32)
    swap_gain = np.full(N, -np.inf)
    n_capped_swap = np.zeros(N, dtype=np.int32)
    margin = np.full(N, np.inf)
    for n in range(N):
        row = np.where(np.isfinite(lpj[n, S_perm:]), lpj[n, S_perm:], -np.inf) + 0.0
        parents = np.lexsort((np.arange(S), -row))[:P]
        for r, slot in enumerate(parents):
            p = ss[n, slot]
            act = np.flatnonzero(p)
            m = len(act)
            if m > cap:
                n_capped_swap[n] += 1
                continue
            if m == 0:
                continue
            # (b) the swaps K^n holds: two differing bits, one in p and one outside
            diff = ss[n] ^ p
            two = (diff.sum(axis=1) == 2) & ((diff & p).sum(axis=1) == 1)
            held = np.zeros((H, H), dtype=bool)
            held[np.argmax(diff[two] & p, axis=1), np.argmax(diff[two] & ~p, axis=1)] = True
            free = np.flatnonzero(~p)
            if sssc:
                base = float(_seed_scores_sssc(G, Psi, mus, pil_bar, s2inv, B[n], yy[n], list(act[:-1]), act[-1:])[0])
            else:
                c = B[n] - G[act].sum(axis=0)
                base = pre1 * (yy[n] - (B[n, act] + c[act]).sum()) + m * pil_bar
            sa, sj, sc = [], [], []
            for a in act:  # ascending a, then ascending j
                js = free[~held[a, free]]
                if len(js) == 0:
                    continue
                if sssc:
                    s = _seed_scores_sssc(G, Psi, mus, pil_bar, s2inv, B[n], yy[n], list(act[act != a]), js)
                else:
                    with np.errstate(invalid="ignore", over="ignore"):
                        base_a = base - pil_bar + pre1 * (Gd[a] + 2.0 * c[a])
                        caj = c[js] + G[a, js]
                        s = base_a + pil_bar + pre1 * (Gd[js] - 2.0 * caj)
                ok = np.isfinite(s)
                sa.append(np.full(ok.sum(), a)), sj.append(js[ok]), sc.append(s[ok])
            if not sc:
                continue
            sa, sj, sc = np.concatenate(sa), np.concatenate(sj), np.concatenate(sc)
            order = np.lexsort((sj, sa, -sc))
            sa, sj, rs = sa[order], sj[order], sc[order]
            k = min(q, len(rs))
            for i in range(k):
                if i + 1 < len(rs):
                    margin[n] = min(margin[n], _seed_gap(rs[i], rs[i + 1]))
                at = counts[n] + i
                cand[n, at] = p
                cand[n, at, sa[i]] = False
                cand[n, at, sj[i]] = True
                scores[n, at] = rs[i]
            counts[n] += k
            if r == 0 and k:
                best_swap[n], swap_gain[n] = (sa[0], sj[0]), rs[0] - base
    return cand, counts, scores, best_swap, swap_gain, n_capped_swap, margin


def posterior_scores_host(lpj, ss=None, S_perm=0):
    """NumPy mirror of Engine.posterior_scores (csrc/kernels_refine.hpp): ``lpj`` (N, L) with L = S_perm + S columns,
    ``ss`` bool (N, S, H) the states of columns S_perm .. L - 1 (columns below S_perm are the permanent all-zero
    state).  With m = max_s lpj_ns, d_s = lpj_ns - m, w_s = exp(d_s), z = sum_s w_s it returns a dict with "F" = m +
    log z, "entropy" = log z - sum_s w_s d_s / z (a weight that underflowed to 0 contributes 0), "best" (int32: the
    first column with lpj_ns == m) and, when ``ss`` is given, "k_best" (int32: active latents of that state) and
    "k_mean" = sum_s q_ns |s_s|."""
    lpj = np.asarray(lpj, dtype=np.float64)
    N, L = lpj.shape
    m = lpj.max(axis=1)
    d = lpj - m[:, None]
    w = np.exp(d)
    z = w.sum(axis=1)
    wd = np.zeros_like(w)
    np.multiply(w, d, out=wd, where=w > 0.0)
    out = {"F": m + np.log(z), "entropy": np.log(z) - wd.sum(axis=1) / z,
           "best": np.argmax(lpj == m[:, None], axis=1).astype(np.int32)}
    if ss is not None:
        ss = np.asarray(ss, dtype=bool)
        assert ss.shape[:2] == (N, L - S_perm), (ss.shape, (N, L - S_perm))
        k = np.concatenate((np.zeros((N, S_perm), dtype=np.int64), ss.sum(axis=2)), axis=1)
        out["k_best"] = k[np.arange(N), out["best"]].astype(np.int32)
        out["k_mean"] = (w * k).sum(axis=1) / z
    return out


# ---- the dictionary resized: the NumPy mirror of evoamd_remap_latents (csrc/kernels_remap.hpp) -----------------------------
#
# index: int (H',); an entry >= 0 names a source latent in [0, H), each at most once; -1 marks a NEW latent, off in every
# state.  Hv' = H' - 1 with the background unit (the last entry is then H - 1), else H'.  Per datapoint: gather t_j[h'] =
# s_j[index[h']] (0 for -1); slot j is KEPT iff t_j differs from every t_i with i < j and, with S_perm = 1, is not all-zero;
# the other slots, in ascending order, each take the next state of the enumeration {0}, {1}, .. {Hv' - 1}, {0,1}, {0,2}, ..
# {0,Hv'-1}, {1,2}, .. (each with the background bit) that equals no kept state of the datapoint.  Hv' (Hv' + 1) / 2 >= S
# guarantees that the enumeration does not run out.
REMAP_MAX_H = 1 << 14  # DIG_MAX_H of csrc/common.hpp


def check_remap_index(index, H, S, background=False):
    """``index`` as a validated int32 array; ValueError naming the rule otherwise."""
    idx = np.asarray(index)
    if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("remap: index must be a one-dimensional integer array with at least one entry")
    idx = idx.astype(np.int32)
    H2 = idx.size
    if H2 > REMAP_MAX_H:
        raise ValueError("remap: H' = %d exceeds %d" % (H2, REMAP_MAX_H))
    bad = np.flatnonzero((idx < -1) | (idx >= H))
    if bad.size:
        raise ValueError("remap: index[%d] = %d is out of range (-1 or a source latent in [0, %d))"
                         % (bad[0], idx[bad[0]], H))
    src = idx[idx >= 0]
    uniq, cnt = np.unique(src, return_counts=True)
    if (cnt > 1).any():
        raise ValueError("remap: duplicate source latent %d" % uniq[cnt > 1][0])
    if background:
        if idx[-1] == -1:
            raise ValueError("remap: a new latent (-1) cannot take the background unit's place: the last index must be "
                             "H - 1 = %d" % (H - 1))
        if idx[-1] != H - 1:
            raise ValueError("remap: the background unit is not last: the last index must be H - 1 = %d (it is %d)"
                             % (H - 1, idx[-1]))
    Hv2 = H2 - (1 if background else 0)
    if Hv2 * (Hv2 + 1) // 2 < S:
        raise ValueError("remap: Hv' (Hv' + 1) / 2 = %d fill candidates are fewer than S = %d states (Hv' = %d): such "
                         "shapes belong to init_states" % (Hv2 * (Hv2 + 1) // 2, S, Hv2))
    return idx


def _remap_enumeration(Hv2, H2, background):
    for a in range(Hv2):
        row = np.zeros(H2, dtype=bool)
        row[a] = True
        if background:
            row[-1] = True
        yield row
    for a in range(Hv2):
        for b in range(a + 1, Hv2):
            row = np.zeros(H2, dtype=bool)
            row[a] = row[b] = True
            if background:
                row[-1] = True
            yield row


def remap_states_host(ss, index, S_perm=0, background=False):
    """K^n in the latent numbering ``index`` as evoamd_remap_latents / Model.remap_latents lay it out: ``ss`` bool
    (N, S, H) -> (ss_new bool (N, S, H'), n_replaced int32 (N,)).  Host only; ValueError for an index the law refuses."""
    ss = np.asarray(ss, dtype=bool)
    N, S, H = ss.shape
    idx = check_remap_index(index, H, S, background)
    H2 = idx.size
    Hv2 = H2 - (1 if background else 0)
    out = np.zeros((N, S, H2), dtype=bool)
    src = idx >= 0
    out[:, :, src] = ss[:, :, idx[src]]
    n_replaced = np.zeros(N, dtype=np.int32)
    for n in range(N):
        kept, dup = set(), []
        for j in range(S):
            key = out[n, j].tobytes()
            if key in kept or (S_perm and not out[n, j].any()):
                dup.append(j)
            else:
                kept.add(key)
        if dup:
            fills = _remap_enumeration(Hv2, H2, background)
            for j in dup:
                row = next(fills)
                while row.tobytes() in kept:
                    row = next(fills)
                out[n, j] = row
            n_replaced[n] = len(dup)
    return out, n_replaced


# ---- K^n resized: the NumPy mirror of evoamd_resize_states (csrc/kernels_resize.hpp) ------------------------------------------
#
# Per datapoint, from the S varying slots of K^n and the lpj row (the permanent all-zero column of S_perm = 1 is not a slot);
# Hv = H - background.  Slot j has key seed_key(lpj[n, S_perm + j]): NaN and +-inf rank as -inf, -0 equals +0; rank order is
# descending key, then ascending slot.  Shrink (S' < S): the kept slots are the first S' in rank order, written in ascending
# old slot; src_slot[n, j'] is the old slot of new slot j'.  Grow (S' > S): slots 0 .. S - 1 in place, src_slot[n, j] = j; b =
# the best varying state (rank 0), e_c = candidate c of the enumeration {0}, .. {Hv - 1}, {0,1}, {0,2}, .. {Hv-2, Hv-1}; the
# candidate fill f_c = b XOR e_c is skipped when it has no varying latent on or equals a state the datapoint holds; slots S,
# S + 1, .. take the unskipped f_c in ascending c, src_slot -1.  Bound: Hv (Hv + 1) / 2 - 1 >= S'.
RESIZE_MAX_S = 1024  # RESIZE_MAX_S of csrc/kernels_resize.hpp


def check_resize(S, S_new, H, background=False):
    """``S_new`` as an int the law admits for a K^n of S states of H latents; ValueError naming the rule otherwise."""
    S_new = int(S_new)
    if S_new < 1:
        raise ValueError("resize: S_new = %d must be positive" % S_new)
    if S_new == S:
        raise ValueError("resize: S_new = %d is the S of K^n: nothing to resize" % S_new)
    if S_new > RESIZE_MAX_S or S > RESIZE_MAX_S:
        raise ValueError("resize: S = %d -> S_new = %d: at most %d states per datapoint are supported" % (S, S_new, RESIZE_MAX_S))
    if H > REMAP_MAX_H:
        raise ValueError("resize: H = %d exceeds %d" % (H, REMAP_MAX_H))
    Hv = H - (1 if background else 0)
    if S_new > S and Hv * (Hv + 1) // 2 - 1 < S_new:
        raise ValueError("resize: Hv (Hv + 1) / 2 - 1 = %d neighbours of the best state are fewer than S_new = %d states "
                         "(Hv = %d)" % (Hv * (Hv + 1) // 2 - 1, S_new, Hv))
    return S_new


def _resize_enumeration(Hv):
    for a in range(Hv):
        yield (a,)
    for a in range(Hv):
        for b in range(a + 1, Hv):
            yield (a, b)


def resize_states_host(ss, lpj, S_perm, S_new, background=False):
    """K^n at ``S_new`` states per datapoint as evoamd_resize_states / Model.resize_states lay it out: ``ss`` bool (N, S, H),
    ``lpj`` (N, S_perm + S) -> (states bool (N, S_new, H), src_slot int32 (N, S_new)).  Host only; ValueError for a size the
    law refuses."""
    ss = np.asarray(ss, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    N, S, H = ss.shape
    assert S_perm in (0, 1) and lpj.shape == (N, S_perm + S), (lpj.shape, (N, S_perm + S))
    S2 = check_resize(S, S_new, H, background)
    Hv = H - (1 if background else 0)
    out = np.zeros((N, S2, H), dtype=bool)
    src = np.full((N, S2), -1, dtype=np.int32)
    for n in range(N):
        row = np.where(np.isfinite(lpj[n, S_perm:]), lpj[n, S_perm:], -np.inf) + 0.0  # the order of seed_key
        order = np.lexsort((np.arange(S), -row))
        if S2 < S:
            kept = np.sort(order[:S2])
            out[n], src[n] = ss[n, kept], kept
            continue
        out[n, :S], src[n, :S] = ss[n], np.arange(S)
        b = ss[n, order[0]]
        held = {s.tobytes() for s in ss[n]}
        at = S
        for e in _resize_enumeration(Hv):
            if at == S2:
                break
            f = b.copy()
            f[list(e)] ^= True
            if not f[:Hv].any() or f.tobytes() in held:
                continue
            out[n, at] = f
            at += 1
        assert at == S2  # (the bound)
    return out, src


def latent_usage_host(ss, lpj, S_perm=0):
    """NumPy mirror of Model.latent_usage on one rank: {"usage": (H,) = sum_n E_q[s_h] / N with q_ns = exp(lpj_ns - max) /
    (sum_s exp(lpj_ns - max) + tiny) as the statistics pass forms it, "map_count": int64 (H,) = datapoints whose first
    column of maximal lpj is a state with latent h on, "N"}.  ``lpj`` (N, S_perm + S); columns below S_perm are the
    permanent all-zero state."""
    ss = np.asarray(ss, dtype=bool)
    lpj = np.asarray(lpj, dtype=np.float64)
    N, S, H = ss.shape
    assert lpj.shape == (N, S + S_perm), (lpj.shape, (N, S + S_perm))
    m = lpj.max(axis=1)
    w = np.exp(lpj - m[:, None])
    q = w[:, S_perm:] / (w.sum(axis=1) + np.finfo(np.float64).tiny)[:, None]
    Es = np.einsum("ns,nsh->nh", q, ss)
    best = np.argmax(lpj == m[:, None], axis=1)
    in_kn = best >= S_perm
    rows = np.flatnonzero(in_kn)
    counts = ss[rows, best[rows] - S_perm].sum(axis=0).astype(np.int64) if rows.size else np.zeros(H, dtype=np.int64)
    return {"usage": Es.sum(axis=0) / N, "map_count": counts, "N": N}


def prune_index(usage, keep_min=None, n_keep=None, n_new=0, background=False):
    """An ``index`` for remap_latents from a per-latent usage (Model.latent_usage()["usage"]): the latents with usage >=
    ``keep_min`` or, with ``n_keep``, the n_keep most used ones (ties: the lower latent), in ascending order; then
    ``n_new`` entries -1; with ``background`` the last latent is kept whatever its usage and stays last, behind the new
    ones.  Exactly one of ``keep_min`` / ``n_keep``."""
    usage = np.asarray(usage, dtype=np.float64)
    if usage.ndim != 1 or (keep_min is None) == (n_keep is None):
        raise ValueError("prune_index: a one-dimensional usage and exactly one of keep_min / n_keep")
    H = usage.size
    Hv = H - 1 if background else H
    if keep_min is not None:
        kept = np.flatnonzero(usage[:Hv] >= keep_min)
    else:
        if not 0 <= int(n_keep) <= Hv:
            raise ValueError("prune_index: n_keep = %d must be in [0, %d]" % (n_keep, Hv))
        kept = np.sort(np.argsort(-usage[:Hv], kind="stable")[:int(n_keep)])
    parts = [kept.astype(np.int32), np.full(int(n_new), -1, dtype=np.int32)]
    if background:
        parts.append(np.array([H - 1], dtype=np.int32))
    return np.concatenate(parts)

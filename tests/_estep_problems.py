"""Synthetic E-step problems for test_gpu_estep_paths.py (and their CPU checks in test_estep_problems.py).

A selection problem is a K^n of S distinct states per datapoint, its lpj row, and a ragged candidate batch (cand, counts,
cand_lpj), with the awkward inputs of vary_kn_kernel planted on purpose (duplicates in the last lane block or across the
64-candidate boundary, digest collisions, saturated counts, the all-zero candidate, latents on word boundaries).  Problems
"with data" also carry Y and a well-conditioned Theta; their lpj values come from the float64 oracle in the GPU module.

Restated from the source, so that a test can say which kernel instantiation or route a case reaches: the SPL / CPL ladder
of with_spl / with_cpl, the eligibility rule of bsc_lpj_gram2_kernel, the digest layout of common.hpp, the LDS plan of the
fused E-step, and the documented selection rule of vary_kn_kernel (ties included)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evo_amd", "csrc")

# common.hpp
DIG_IDX_BITS = 14
DIG_MAX_H = 1 << DIG_IDX_BITS
DIG_SLOTS = 4
# kernels_common.hpp
VK_MAX_S_PER_LANE = 16
VK_MAX_C_PER_LANE = 4
# evo_amd.hip (launch_bsc_lpj): LDS of the gram2 kernel's B rows; (FUSED_LDS_MAX): LDS limit of one workgroup of the fused kernel
GRAM2_LDS_MAX = 40 * 1024
FUSED_LDS_MAX = 150 * 1024
SSSC_KCAP = 64


# ---- restatements --------------------------------------------------------------------------------------------------
def vk_instantiation(S, Cmax):
    """with_spl / with_cpl: the <SPL, CPL> of vary_kn_kernel that a geometry launches."""
    spl = 1 if S <= 64 else 2 if S <= 128 else 4 if S <= 256 else 8 if S <= 512 else 16
    return spl, (1 if Cmax <= 64 else 4)


def uses_digests(H, state_digest):
    """Digests exist for H <= DIG_MAX_H (evoamd_configure) and are read when the option "state_digest" is on."""
    return bool(state_digest) and H <= DIG_MAX_H


def gram2_eligible(H, C, state_digest=1, bsc_direct=0):
    """launch_bsc_lpj for a candidate batch (tag 1, complete data, not shared): bsc_lpj_gram2_kernel needs H even, a word
    count it is instantiated for or digests, and (512 / C + 2) B rows of H doubles in 40 KB of LDS."""
    if bsc_direct:
        return False
    HW = (H + 63) // 64
    hw_ok = HW in (1, 2, 4, 8, 16)
    lds = (512 // C + 2) * H * 8
    return (hw_ok or uses_digests(H, state_digest)) and H % 2 == 0 and lds <= GRAM2_LDS_MAX


def digest(state):
    """make_digest (common.hpp) of one bool state: bits 0..7 = active latents saturated at 255, bits 8 + 14 j ... = the
    j-th active latent (ascending), j < DIG_SLOTS.  Python int (u64)."""
    idx = np.flatnonzero(state)
    assert state.shape[0] <= DIG_MAX_H
    d = min(idx.size, 255)
    for j, h in enumerate(idx[:DIG_SLOTS]):
        d |= int(h) << (8 + DIG_IDX_BITS * j)
    return d


def fused_lds_wave_bytes(SPL, kc_big):
    """kernels_fused.hpp: dynamic LDS per wave of sssc_estep_fused_kernel."""
    b = SPL * 64 * 8 * 2 + 64 * 8 * 3 + 64 * 2 * 2 + 64 * 4 * 3 + 32 * 4 + (16 * 8 + 16) * 4
    b += (4 * kc_big * kc_big + 5 * kc_big) * 8 + ((kc_big * 4 + 7) // 8) * 8
    return (b + 15) // 16 * 16


def fused_launch_plan(S, H):
    """estep_plan: per stage (waves per workgroup, kc_big, LDS bytes, halvings of W, kc_big shrinks)."""
    SPL = vk_instantiation(S, 1)[0]
    tab = 4 * H * 8
    out = []
    for stage in (0, 1):
        W = 4 if stage == 0 else 1
        kc = 16 if stage == 0 else SSSC_KCAP
        lds_of = lambda w: (tab if stage == 0 else 0) + w * fused_lds_wave_bytes(SPL, kc)
        shrinks = halvings = 0
        while stage == 1 and lds_of(1) > FUSED_LDS_MAX and kc > 16:
            kc -= 4
            shrinks += 1
        while W > 1 and lds_of(W) > FUSED_LDS_MAX:
            W >>= 1
            halvings += 1
        out.append({"W": W, "kc_big": kc, "lds": lds_of(W), "halvings": halvings, "shrinks": shrinks})
    return out


def select_rule(old, old_lpj, cand, cand_lpj, cnt, Mprime, S_perm, cand_tie="low", strict=True):
    """The documented rule of vary_kn_kernel (kernels_common.hpp) for one datapoint: candidate c survives iff no equal row
    precedes it in [all-zero state if S_perm; K^n; cand[0:c]]; M = min(#survivors, Mprime); survivors ranked by
    descending value, old states by ascending value, the lower index first among equal values; swap j happens iff the
    j-th best candidate is strictly greater than the j-th worst old state, and the first failure ends the swaps.
    cand_tie="high" / strict=False are the two wrong variants the tie cases must tell apart.
    Returns (states, lpj, n_unique, n_sub) with fresh arrays."""
    S, H = old.shape
    seen = {old[s].tobytes() for s in range(S)}
    if S_perm:
        seen.add(np.zeros(H, dtype=bool).tobytes())
    kept = []
    for c in range(cnt):
        key = cand[c].tobytes()
        if key not in seen:
            kept.append(c)
        seen.add(key)
    M = min(len(kept), Mprime)
    tie = (lambda c: c) if cand_tie == "low" else (lambda c: -c)
    best = sorted(kept, key=lambda c: (-cand_lpj[c], tie(c)))
    worst = sorted(range(S), key=lambda s: (old_lpj[s], s))
    states, lpj = old.copy(), old_lpj.copy()
    g = 0
    for j in range(M):
        better = cand_lpj[best[j]] > old_lpj[worst[j]] if strict else cand_lpj[best[j]] >= old_lpj[worst[j]]
        if not better:
            break
        states[worst[j]] = cand[best[j]]
        lpj[worst[j]] = cand_lpj[best[j]]
        g += 1
    return states, lpj, len(kept), g


def survivors(p, n):
    """Indices of the candidates of datapoint n that survive de-duplication (select_rule's first step)."""
    S, H = p["S"], p["H"]
    seen = {p["ss"][n, s].tobytes() for s in range(S)}
    if p["S_perm"]:
        seen.add(np.zeros(H, dtype=bool).tobytes())
    out = []
    for c in range(int(p["counts"][n])):
        key = p["cand"][n, c].tobytes()
        if key not in seen:
            out.append(c)
        seen.add(key)
    return out


# ---- selection problems --------------------------------------------------------------------------------------------
# name -> (model, N, D, H, S, S_perm, Cmax, data, seed).  Together: every <SPL, CPL> x S_perm; every case runs with
# state_digest 1 and 0 (H = 16385 has no digests: the word path either way).
SELECTION = {
    "s1c1p0": ("bsc", 7, 9, 64, 64, 0, 64, True, 101),
    "s1c1p1": ("sssc", 3, 8, 40, 40, 1, 20, True, 102),
    "s1c4p0": ("bsc", 1, 4, 130, 33, 0, 200, False, 103),
    "s1c4p1": ("bsc", 7, 9, 65, 64, 1, 130, True, 104),
    "s2c1p0": ("sssc", 7, 8, 64, 100, 0, 40, True, 105),
    "s2c1p1": ("bsc", 3, 4, 16384, 65, 1, 64, False, 106),   # digests: latent 16383 in the last 14-bit slot value
    "s2c4p0": ("bsc", 3, 4, 200, 128, 0, 100, False, 107),
    "s2c4p0_h16385": ("bsc", 3, 4, 16385, 128, 0, 100, False, 121),  # no digests: the word path at HW = 257
    "s2c4p1": ("bsc", 7, 9, 128, 128, 1, 256, True, 108),
    "s4c1p0": ("bsc", 7, 9, 512, 256, 0, 64, True, 109),       # states above 255 latents: saturated counts
    "s4c1p1": ("bsc", 1, 4, 63, 129, 1, 1, False, 110),
    "s4c4p0": ("sssc", 3, 8, 64, 200, 0, 100, True, 111),
    "s4c4p1": ("bsc", 3, 4, 1000, 256, 1, 65, False, 112),
    "s8c1p0": ("bsc", 7, 9, 100, 257, 0, 16, True, 113),
    "s8c1p1": ("bsc", 3, 4, 64, 512, 1, 64, False, 114),
    "s8c4p0": ("bsc", 3, 4, 200, 400, 0, 256, False, 115),
    "s8c4p1": ("sssc", 3, 8, 64, 300, 1, 80, True, 116),
    "s16c1p0": ("bsc", 3, 4, 64, 1024, 0, 64, False, 117),
    "s16c1p1": ("bsc", 7, 9, 70, 600, 1, 40, True, 118),
    "s16c4p0": ("sssc", 3, 8, 64, 1024, 0, 256, True, 119),
    "s16c4p1": ("bsc", 3, 4, 129, 1024, 1, 200, False, 120),
}
# tie cases: small integer lpj values, so that candidates tie with each other and with old states
TIES = {
    "ties_s1": ("bsc", 7, 4, 40, 64, 0, 64, False, 201),
    "ties_s4c4": ("bsc", 3, 4, 64, 200, 1, 150, False, 202),
    "ties_s16": ("bsc", 3, 4, 96, 700, 0, 100, False, 203),
}
PROBLEMS = dict(SELECTION, **TIES)


def mprimes(S):
    return sorted({1, max(1, S // 3), S})


def _rand_state(rng, H, kmax=6):
    k = int(rng.randint(0, min(H, kmax) + 1))
    st = np.zeros(H, dtype=bool)
    st[rng.choice(H, k, replace=False)] = True
    return st


def _fresh(rng, H, seen, kmax=6, tries=1000):
    for _ in range(tries):
        st = _rand_state(rng, H, kmax)
        if st.tobytes() not in seen:
            return st
    raise AssertionError("no fresh state")


def _with(H, idx):
    st = np.zeros(H, dtype=bool)
    st[np.asarray(idx, dtype=np.int64)] = True
    return st


def _collision_partner(rng, st, H):
    """A state with the same active-latent count and the same first four latents as `st` (k >= 5), different beyond."""
    idx = np.flatnonzero(st)
    k = idx.size
    assert k >= DIG_SLOTS + 1
    head = idx[:DIG_SLOTS]
    free = np.setdiff1d(np.arange(head[-1] + 1, H), idx)
    tail = np.sort(rng.choice(free, k - DIG_SLOTS, replace=False)) if free.size >= k - DIG_SLOTS else None
    if tail is None or np.array_equal(tail, idx[DIG_SLOTS:]):
        return None
    return _with(H, np.concatenate([head, tail]))


def make_problem(name):
    """Selection problem `name`.  plants: list of (kind, n, info) of what was planted where."""
    model, N, D, H, S, S_perm, Cmax, data, seed = PROBLEMS[name]
    rng = np.random.RandomState(seed)
    ties = name in TIES
    kmax = 6 if H >= 16 else max(1, H // 3)
    ss = np.zeros((N, S, H), dtype=bool)
    cand = np.zeros((N, Cmax, H), dtype=bool)
    counts = rng.randint(0, Cmax + 1, size=N).astype(np.int32)
    counts[0] = Cmax  # a full row, an empty row and a single candidate wherever N allows it
    if N > 1:
        counts[1] = 0
    if N > 2:
        counts[2] = 1
    if N > 3:
        counts[N - 1] = max(2, counts[N - 1])
    plants = []
    for n in range(N):
        seen = set() if not S_perm else {np.zeros(H, dtype=bool).tobytes()}
        row = []
        # planted old states first: word-boundary latents, and dense states for the collision / saturation plants
        special = [_with(H, [h for h in (0, 63, 64, H - 1) if h < H])]
        if H > 128:
            special.append(_with(H, [127, 128, H - 2]))
        if H >= 512 and n % 2 == 0:
            sat = _with(H, np.concatenate([[1, 2, 3, 5], 6 + np.sort(rng.choice(H - 6, 296, replace=False))]))
            special.append(sat)  # 300 latents
        if H >= 9:
            special.append(_with(H, np.sort(rng.choice(H, 5 + n % 3, replace=False))))  # k = 5..7: collision base
        for st in special:
            if st.tobytes() not in seen and len(row) < S:
                row.append(st)
                seen.add(st.tobytes())
        while len(row) < S:
            st = _fresh(rng, H, seen, kmax)
            row.append(st)
            seen.add(st.tobytes())
        row = np.array(row)
        # move the planted ones to random places (one of them into the last lane block)
        perm = rng.permutation(S)
        last0 = 64 * ((S - 1) // 64)  # the last lane block that holds states
        if S > last0 + 1:
            j = int(rng.randint(last0, S))
            i0 = int(np.flatnonzero(perm == 0)[0])
            perm[i0], perm[j] = perm[j], perm[i0]
        inv = np.empty(S, dtype=np.int64)
        inv[perm] = np.arange(S)
        ss[n] = row[inv]
        # candidates
        cnt = int(counts[n])
        cseen = set(seen)
        crow = []
        kinds = []
        if cnt:
            big_s = int(rng.randint(last0, S))
            want = [("dup_old_last_block", ss[n, big_s].copy(), big_s)]
            # (S_perm = 0: a duplicate or a fresh state, whichever K^n makes it)
            want.append(("zero_cand", np.zeros(H, dtype=bool), None))
            dense = sorted((s for s in range(S) if ss[n, s].sum() >= DIG_SLOTS + 1), key=lambda s: -ss[n, s].sum())
            for s in dense[:2]:
                if ss[n, s].sum() > 255:  # 20 latents fewer, still above 255: the saturated digests agree
                    kind, partner = "sat255_old", _with(H, np.flatnonzero(ss[n, s])[:-20])
                else:
                    kind, partner = "dig_collision_old", _collision_partner(rng, ss[n, s], H)
                if partner is not None and partner.tobytes() not in cseen:
                    want.append((kind, partner, s))
            bnd = _with(H, [h for h in (63, 64, H - 1) if h < H] + ([1] if H > 65 else []))
            want.append(("boundary_latents", bnd, None))
            for kind, st, info in want:
                if len(crow) >= cnt:
                    break
                if kind in ("dup_old_last_block", "zero_cand") or st.tobytes() not in cseen:
                    crow.append(st)
                    kinds.append((kind, info))
                    cseen.add(st.tobytes())
            # a fresh dense candidate and its collision partner among the candidates (k >= 5)
            if H >= 9 and len(crow) + 2 <= cnt:
                a = _with(H, np.sort(rng.choice(H, 5 + int(rng.randint(0, 3)), replace=False)))
                while a.tobytes() in cseen:
                    a = _with(H, np.sort(rng.choice(H, 5 + int(rng.randint(0, 3)), replace=False)))
                b = _collision_partner(rng, a, H)
                if b is not None and b.tobytes() not in cseen and b.tobytes() != a.tobytes():
                    crow += [a, b]
                    kinds += [("dense_cand", None), ("dig_collision_cand", len(crow) - 2)]
                    cseen |= {a.tobytes(), b.tobytes()}
            while len(crow) < cnt:
                r = rng.random_sample()
                if r < 0.08 and crow:  # an ordinary duplicate of an earlier candidate
                    c0 = int(rng.randint(len(crow)))
                    crow.append(crow[c0].copy())
                    kinds.append(("dup_cand", c0))
                elif r < 0.14:
                    s0 = int(rng.randint(S))
                    crow.append(ss[n, s0].copy())
                    kinds.append(("dup_old", s0))
                else:
                    st = _fresh(rng, H, cseen, kmax)
                    crow.append(st)
                    kinds.append(("fresh", None))
                    cseen.add(st.tobytes())
            # c >= 64 repeats c < 64 (the lane block boundary of the candidates)
            if cnt > 64:
                c_hi = int(rng.randint(64, cnt))
                c_lo = int(rng.randint(0, 64))
                crow[c_hi] = crow[c_lo].copy()
                kinds[c_hi] = ("dup_cand_cross64", c_lo)
                for j in range(c_hi + 1, len(crow)):  # later copies of the old crow[c_hi] follow it
                    if kinds[j] == ("dup_cand", c_hi):
                        crow[j] = crow[c_hi].copy()
            crow = np.array(crow)[:cnt]
            cand[n, :cnt] = crow
            for c, (kind, info) in enumerate(kinds[:cnt]):
                if kind not in ("fresh", "dense_cand"):
                    plants.append((kind, n, (c, info)))
    # one row whose candidates are all duplicates (the last datapoint, where N > 3)
    n_all = N - 1
    cnt = int(counts[n_all]) if N > 3 else 0
    if cnt:
        for c in range(cnt):
            cand[n_all, c] = ss[n_all, int(rng.randint(S))] if c == 0 or rng.random_sample() < 0.5 else cand[n_all, c - 1]
        plants = [pl for pl in plants if pl[1] != n_all]
        plants.append(("all_dup_row", n_all, (cnt, None)))
    p = {"name": name, "model": model, "N": N, "D": D, "H": H, "S": S, "S_perm": S_perm, "Cmax": Cmax, "data": data,
         "ss": ss, "cand": cand, "counts": counts, "plants": plants, "ties": ties}
    # values: synthetic (tie-free continuous values, or small integers for the tie cases); data problems get theirs from
    # the oracle (oracle_lpj)
    L = S + S_perm
    if ties:
        p["lpj"] = rng.randint(-6, 3, size=(N, L)).astype(np.float64)
        p["cand_lpj"] = rng.randint(-5, 5, size=(N, Cmax)).astype(np.float64)
    else:
        p["lpj"] = rng.normal(size=(N, L)) * 5.0 - 40.0
        p["cand_lpj"] = rng.normal(size=(N, Cmax)) * 5.0 - 37.0
        for n in range(N):  # a duplicate carries the value of the state it repeats (as an lpj evaluation would)
            for c in range(int(counts[n])):
                st = cand[n, c]
                hit = np.flatnonzero((ss[n] == st).all(axis=1))
                if hit.size:
                    p["cand_lpj"][n, c] = p["lpj"][n, S_perm + hit[0]]
                    continue
                prev = np.flatnonzero((cand[n, :c] == st).all(axis=1))
                if prev.size:
                    p["cand_lpj"][n, c] = p["cand_lpj"][n, prev[0]]
        # planted non-duplicates rank first (so that they are accepted whenever they survive)
        top = p["lpj"].max() + 1.0
        for kind, n, (c, _) in p["plants"]:
            if kind in ("zero_cand", "dig_collision_old", "dig_collision_cand", "sat255_old", "boundary_latents"):
                p["cand_lpj"][n, c] = top + rng.random_sample()
        p["cand_lpj"][np.arange(Cmax)[None, :] >= counts[:, None]] = 0.0
    if data:
        Y = rng.normal(size=(N, D))
        if model == "sssc":
            A = rng.normal(size=(H, 3)) * 0.2
            p["theta"] = {"W": rng.normal(size=(D, H)) * 0.4, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H),
                          "Psi": np.eye(H) + A @ A.T, "sigma2": np.float64(1.3)}
        else:
            p["theta"] = {"W": rng.normal(size=(D, H)) * 0.5, "pi": np.float64(0.15), "sigma": np.float64(2.0)}
        p["Y"] = Y
    return p


def oracle_lpj(p, states, n0=0):
    """float64 oracle lpj of `states` (n, C, H) of datapoints n0, n0 + 1, ... under problem p's Theta and data: (n, C)."""
    from oracle import evo_oracle as orc
    th = dict(p["theta"])
    N = states.shape[0]
    out = np.empty(states.shape[:2])
    if p["model"] == "sssc":
        orc.sssc_precompute(th, p["D"])
        cache = {}
        for n in range(N):
            out[n] = orc.sssc_lpj(th, states[n], p["Y"][n0 + n], orc.new_counters(), cache)
    else:
        cnt = orc.bsc_precompute(th, p["D"], p["H"])
        for n in range(N):
            out[n] = orc.bsc_lpj(th, states[n], p["Y"][n0 + n], cnt)
    return out


def oracle_allzero(p):
    from oracle import evo_oracle as orc
    th = dict(p["theta"])
    if p["model"] == "sssc":
        orc.sssc_precompute(th, p["D"])
        return np.array([orc.sssc_lpj_allzero(th, y, orc.new_counters())[0] for y in p["Y"]])
    cnt = orc.bsc_precompute(th, p["D"], p["H"])
    return np.array([orc.bsc_lpj_allzero(th, y, cnt)[0] for y in p["Y"]])


def attach_oracle_values(p):
    """Data problems: lpj of K^n (+ the all-zero column) and of the candidates from the float64 oracle."""
    N, S_perm = p["N"], p["S_perm"]
    lpj = np.empty((N, p["S"] + S_perm))
    if S_perm:
        lpj[:, 0] = oracle_allzero(p)
    lpj[:, S_perm:] = oracle_lpj(p, p["ss"])
    cl = np.zeros((N, p["Cmax"]))
    for n in range(N):
        c = int(p["counts"][n])
        if c:
            cl[n, :c] = oracle_lpj(p, p["cand"][n:n + 1, :c], n)[0]
    p["lpj"], p["cand_lpj"] = lpj, cl
    return p


def oracle_select(p, Mprime, lpj=None, cand_lpj=None):
    """oracle.vary_Kn per datapoint: (states, lpj row, n_unique sum, n_sub sum)."""
    from oracle import evo_oracle as orc
    lpj = p["lpj"] if lpj is None else lpj
    cand_lpj = p["cand_lpj"] if cand_lpj is None else cand_lpj
    N, S, H, S_perm = p["N"], p["S"], p["H"], p["S_perm"]
    states = p["ss"].copy()
    out = lpj.copy()
    incl = np.zeros((S_perm, H), dtype=bool)
    nu = ns = 0
    for n in range(N):
        c = int(p["counts"][n])
        a, b = orc.vary_Kn(lpj[n, S_perm:].copy(), cand_lpj[n, :c].copy(), out[n, S_perm:], states[n], p["cand"][n, :c],
                           H, S, S_perm, incl, Mprime)
        nu += a
        ns += b
    return states, out, nu, ns


# ---- candidate lpj problems (evoamd_lpj_candidates) ----------------------------------------------------------------
# name -> (model, N, D, H, Cmax, options, seed, k list (ES3C) or None).  EBSC: the route each one takes is asserted from
# gram2_eligible in the CPU module.
CAND_LPJ = {
    "bsc_h_odd": ("bsc", 9, 10, 63, 12, {}, 301, None),
    "bsc_hw3_nodigest": ("bsc", 9, 10, 160, 24, {"state_digest": 0}, 302, None),
    "bsc_hw3_digest": ("bsc", 9, 10, 160, 24, {}, 303, None),
    "bsc_c1_h10": ("bsc", 33, 7, 10, 1, {}, 304, None),
    "bsc_c1_h8": ("bsc", 33, 7, 8, 1, {}, 305, None),
    "bsc_direct": ("bsc", 9, 10, 64, 12, {"bsc_direct": 1}, 306, None),
    "es_mixed_k": ("sssc", 5, 12, 96, 12, {}, 307, (0, 1, 2, 3, 4, 5, 8, 9, 64, 65)),
    "es_mixed_k_nodigest": ("sssc", 5, 12, 96, 12, {"state_digest": 0}, 308, (0, 1, 2, 3, 4, 5, 8, 9, 64, 65)),
    # the lower edge: H = 1 (odd: the plain EBSC kernel; ES3C: no pair of latents exists, the pair table is one dummy
    # entry), H = 2 (the Gram kernel's smallest H; one pair), H = 3 on the word path
    "bsc_h1": ("bsc", 9, 3, 1, 2, {}, 309, None),
    "bsc_h2": ("bsc", 9, 3, 2, 4, {}, 310, None),
    "es_h1": ("sssc", 9, 3, 1, 2, {}, 311, (0, 1)),
    "es_h2": ("sssc", 9, 3, 2, 4, {}, 312, (0, 1, 2)),
    "es_h3_nodigest": ("sssc", 9, 3, 3, 4, {"state_digest": 0}, 313, (0, 1, 2, 3)),
}


def make_cand_problem(name):
    model, N, D, H, Cmax, opts, seed, ks = CAND_LPJ[name]
    rng = np.random.RandomState(seed)
    counts = rng.randint(1, Cmax + 1, size=N).astype(np.int32)
    counts[0] = Cmax
    cand = np.zeros((N, Cmax, H), dtype=bool)
    for n in range(N):
        for c in range(Cmax):  # entries at c >= counts[n] hold states too: the kernel must not care
            k = ks[(c + n) % len(ks)] if ks else int(rng.randint(0, min(H, 8) + 1))
            cand[n, c, rng.choice(H, k, replace=False)] = True
    Y = rng.normal(size=(N, D))
    if model == "sssc":
        A = rng.normal(size=(H, 3)) * 0.2
        theta = {"W": rng.normal(size=(D, H)) * 0.4, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H),
                 "Psi": np.eye(H) + A @ A.T, "sigma2": np.float64(1.3)}
    else:
        theta = {"W": rng.normal(size=(D, H)) * 0.5, "pi": np.float64(0.15), "sigma": np.float64(2.0)}
    return {"name": name, "model": model, "N": N, "D": D, "H": H, "S": 4, "S_perm": 0, "Cmax": Cmax, "opts": opts,
            "cand": cand, "counts": counts, "Y": Y, "theta": theta, "ss": np.zeros((N, 4, H), dtype=bool)}


# ---- device flow and fused E-step -----------------------------------------------------------------------------------
# evolve_randflip with n_parents x n_children > 64 (the <., 4> instantiation in the real flow): (N, D, H, S, parents,
# children, Mprime, seed), EBSC with data
DEVICE_FLOW = {
    "flow_s257": (5, 10, 64, 257, 10, 8, 40, 401),
    "flow_s513": (5, 10, 72, 513, 12, 7, 513, 402),
    "flow_s1024": (3, 10, 64, 1024, 40, 2, 1, 403),
}
# fused against separate (ES3C): (N, D, H, S, parents, children, Mprime, dense, seed).  dense: S / 8 states of 16 latents
# in every other datapoint and random parents, so that children of 17 latents send datapoints to the second launch
# (kc_big = SSSC_KCAP)
FUSED = {
    "fused_s65": (31, 12, 64, 65, 8, 8, 65, False, 501),
    "fused_s65_dense": (31, 12, 64, 65, 64, 1, 10, True, 502),
    "fused_s257": (15, 12, 64, 257, 8, 8, 20, False, 503),
    "fused_s513": (7, 12, 64, 513, 8, 8, 513, False, 504),
    "fused_s1024": (7, 12, 64, 1024, 16, 4, 64, False, 505),
    "fused_s1024_dense": (7, 12, 64, 1024, 64, 1, 64, True, 506),
}
# every S class of with_spl (S <= 64, 65-128, 129-256, 257-512, 513-1024) through the randflip kernel, the selection and
# the fused kernel (ES3C, at most 64 children): (N, D, H, S, parents, children, Mprime, seed).  H = 12 gives enough
# distinct states for S = 520; a wrong template argument in the dispatch shows at these sizes, larger ones add nothing
SPL_FLOW = {
    "spl_s4": (8, 6, 12, 4, 2, 2, 4, 601),
    "spl_s72": (8, 6, 12, 72, 4, 4, 24, 602),
    "spl_s136": (8, 6, 12, 136, 8, 4, 136, 603),
    "spl_s264": (8, 6, 12, 264, 8, 8, 88, 604),
    "spl_s520": (8, 6, 12, 520, 8, 8, 173, 605),
}


def make_kn(rng, N, S, H, dense_every=0, kmax=6):
    """N rows of S distinct states of 0..kmax latents; with dense_every, every dense_every-th datapoint also holds
    max(2, S / 8) states of 16 latents."""
    ss = np.zeros((N, S, H), dtype=bool)
    for n in range(N):
        seen = set()
        s = 0
        while s < S:
            k = 16 if (dense_every and n % dense_every == 0 and s < max(2, S // 8)) else int(rng.randint(0, kmax + 1))
            st = np.zeros(H, dtype=bool)
            st[rng.choice(H, k, replace=False)] = True
            if st.tobytes() in seen:
                continue
            seen.add(st.tobytes())
            ss[n, s] = st
            s += 1
    return ss


def es3c_theta(rng, D, H):
    A = rng.normal(size=(H, 3)) * 0.2
    return {"W": rng.normal(size=(D, H)) * 0.4, "pies": rng.uniform(0.05, 0.2, H), "mus": rng.normal(size=H),
            "Psi": np.eye(H) + A @ A.T, "sigma2": np.float64(1.3)}


def bsc_theta(rng, D, H):
    return {"W": rng.normal(size=(D, H)) * 0.5, "pi": np.float64(0.1), "sigma": np.float64(2.0)}

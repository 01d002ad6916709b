"""Problems for the device EA's stream parity (test_gpu_evolve_parity.py) and for the host checks of its NumPy mirror
(test_evolve_counter_host.py): the case tables, K^n with the awkward rows planted, the lpj rows that steer the parent
draw, Theta and data, and the mirror's result per case (computed once, shared).

Every case has N = 256 distinct datapoints.  K^n holds S distinct random states per datapoint; from H = 16 on a pair of
rows per datapoint has six active latents and shares its first four (the digests of the two agree: the word comparison
decides), and further rows have five to seven.  The lpj row is uploaded, not computed, so that generation 0 depends on
no device lpj: by datapoint index mod 4 it is all negative, positive with two exact 0s (states of fitness zero: taken
last, the lower slot first), one value repeated, or a mixture of both signs with repeated values."""
import functools
from collections import namedtuple

import numpy as np

import _estep_problems as ep

N = 256
D = 4

Fast = namedtuple("Fast", "H S S_perm bg n_parents n_children fit model")
# the cases of the randflip kernel: (H, S, S_perm, bg, n_parents, n_children, fit)
FAST = {
    "h7_all_positions": Fast(7, 8, 0, 0, 3, 7, 1, "bsc"),          # every position is picked; the clamp of r
    "h64_lane_block": Fast(64, 64, 0, 0, 8, 8, 1, "bsc"),          # one full lane block
    "h64_lane_block_es3c": Fast(64, 64, 0, 0, 8, 8, 1, "sssc"),    # the kernel also clears the overflow lists
    "h65_72_children": Fast(65, 65, 1, 0, 9, 8, 1, "bsc"),         # 72 children; SPL 2; a word boundary
    "h65_bg_domain64": Fast(65, 12, 0, 1, 4, 2, 0, "bsc"),         # a domain of exactly 64 latents
    "h130_spl4": Fast(130, 129, 0, 0, 16, 4, 1, "bsc"),
    "h200_spl8": Fast(200, 300, 0, 0, 16, 2, 1, "bsc"),
    "h128_spl16_64_parents": Fast(128, 1024, 0, 0, 64, 1, 0, "bsc"),  # n_parents at its limit
    "h520_hw9": Fast(520, 20, 0, 0, 5, 3, 1, "bsc"),               # past the loop that keeps eight words in flight
    "h1": Fast(1, 2, 0, 0, 1, 1, 1, "bsc"),                        # one latent: every flip is the same one; S = 2^H
    "h2": Fast(2, 3, 0, 0, 2, 2, 1, "sssc"),                       # n_children = H: both positions of either parent
}

General = namedtuple("General", "H S S_perm bg mutation n_parents n_children n_gen fit sparseness p_bf Cmax zero_parent")
OPERATORS = ("randflip", "sparseflip", "cross", "cross_randflip", "cross_sparseflip")


def _general_cases():
    g = {}
    for i, op in enumerate(OPERATORS):
        # collisions all the time, pools smaller than n_parents, empty pools; S_perm alternates over the operators
        g["%s_h5" % op] = General(5, 4, i % 2, 0, op, 3, 2, 3, 1, 1.0, 0.15, None, False)
        g["%s_h64" % op] = General(64, 20, 0, 0, op, 4, 2, 2, 1, 2.5, 0.05, None, False)
        g["%s_h65" % op] = General(65, 65, 1, 0, op, 5, 2, 2, i % 2, 2.5, 0.05, None, False)
        g["%s_h130" % op] = General(130, 12, 0, 0, op, 4, 3, 3, 1, 3.0, 0.03, None, False)
    # the lower edge: H = 2 (randint(1, H) of the crossover has one value; S = 2^H - 1, so at most one state is new),
    # H = 3 and, for randflip, H = 1 with S = 2^H (every child is the other known state, or a duplicate: counts stay 0).
    # sparseflip: (sparseness, p_bf) = (1.0, 0.25) at H = 2 and (1.5, 0.25) at H = 3 keep p0 and p1 of every parent with
    # 0 < |s| < H inside (0, 1) (test_evolve_counter_host.py evaluates the mirror's formula)
    for i, op in enumerate(OPERATORS):
        g["%s_h2" % op] = General(2, 3, 0, 0, op, 2, 1, 2, 1, 1.0, 0.25, None, False)
        g["%s_h3" % op] = General(3, 5, i % 2, 0, op, 3, 2, 2, 1, 1.5, 0.25, None, False)
    g["randflip_h1"] = General(1, 2, 0, 0, "randflip", 1, 1, 1, 1, 0.0, 0.0, None, False)
    g["randflip_h65_bg"] = General(65, 16, 0, 1, "randflip", 4, 8, 2, 1, 0.0, 0.0, None, False)
    g["cross_sparseflip_h65_bg"] = General(65, 16, 0, 1, "cross_sparseflip", 4, 1, 2, 1, 2.5, 0.05, None, False)
    g["cross_p9_72_children"] = General(64, 12, 0, 0, "cross", 9, 1, 1, 1, 0.0, 0.0, None, False)
    g["cross_randflip_p16_240_children"] = General(130, 20, 1, 0, "cross_randflip", 16, 1, 1, 1, 0.0, 0.0, 256, False)
    g["randflip_s1024"] = General(64, 1024, 0, 0, "randflip", 8, 2, 2, 1, 0.0, 0.0, None, False)
    g["sparseflip_h520"] = General(520, 10, 0, 0, "sparseflip", 4, 2, 2, 1, 3.0, 0.01, None, False)
    g["cross_sparseflip_h520"] = General(520, 10, 1, 0, "cross_sparseflip", 4, 1, 2, 0, 3.0, 0.01, None, False)
    g["sparseflip_p0_ge_1"] = General(64, 6, 0, 0, "sparseflip", 6, 1, 2, 1, 2.5, 2.0, None, True)   # every 0 flips
    g["sparseflip_p0_le_0"] = General(64, 6, 0, 0, "sparseflip", 4, 2, 3, 1, 2.5, 0.0, None, True)   # no 0 flips
    # a parent of 6 = sparseness + H p_bf latents sits on the pole of alpha: p0 ~ 1e-103, p1 = 7 / 12, a skip beyond 1e100
    g["sparseflip_alpha_pole"] = General(70, 8, 0, 0, "sparseflip", 4, 2, 2, 0, 2.5, 0.05, None, False)
    g["sparseflip_zero_parent"] = General(70, 4, 0, 0, "sparseflip", 4, 3, 2, 0, 2.5, 0.05, None, True)
    return g


GENERAL = _general_cases()
CASES = dict(FAST, **GENERAL)
TINY = tuple(sorted(k for k, v in CASES.items() if v.H <= 3))  # added later: seeds of their own, the others keep theirs


def per_generation(c):
    if c.mutation.startswith("cross"):
        return c.n_parents * (c.n_parents - 1)
    return c.n_parents * c.n_children


def cmax(name):
    c = CASES[name]
    if name in FAST:
        return c.n_parents * c.n_children
    return c.Cmax or per_generation(c) * c.n_gen


def seed_of(name):
    if name in TINY:
        return 2000 + TINY.index(name)
    return 1000 + sorted(k for k in CASES if k not in TINY).index(name)


# ---- K^n ---------------------------------------------------------------------------------------------------------------
def _random_rows(rng, M, Hd, kmax, nonzero):
    k = rng.randint(1 if nonzero else 0, kmax + 1, size=M)
    pos = rng.randint(0, Hd, size=(M, kmax))
    rows = np.zeros((M, Hd), dtype=bool)
    for j in range(kmax):  # (a position drawn twice: one latent fewer)
        m = j < k
        rows[np.flatnonzero(m), pos[m, j]] = True
    return rows


def _distinct(rows):
    key = np.packbits(rows, axis=1)
    return np.unique(key.view(np.dtype((np.void, key.shape[1]))).ravel()).size == rows.shape[0]


def make_kn(rng, S, H, S_perm, bg, zero_parent=False):
    """K^n of every datapoint: bool (N, S, H)."""
    Hd = H - 1 if bg else H
    ss = np.zeros((N, S, H), dtype=bool)
    nonzero = bool(S_perm)  # (the permanent all-zero state is no member of K^n)
    small = Hd <= 12
    if small:
        table = np.array([[(i >> (Hd - 1 - h)) & 1 for h in range(Hd)] for i in range(2 ** Hd)], dtype=bool)
        assert S <= table.shape[0] - (1 if nonzero else 0)  # (S = 2^Hd: the whole table, the all-zero state included)
    kmax = min(6, max(1, Hd // 3))
    for n in range(N):
        if small:
            pick = rng.permutation(np.arange(1 if nonzero else 0, table.shape[0]))[:S]
            rows = table[pick]
        else:
            rows = _random_rows(rng, 2 * S + 64, Hd, kmax, nonzero)
            _, first = np.unique(_row_keys(rows), return_index=True)
            rows = rows[np.sort(first)][:S]
            assert rows.shape[0] == S
            if Hd >= 16 and S >= 6:  # a pair with equal digests, and rows of five to seven latents
                base = rows
                for _ in range(20):
                    rows = base.copy()
                    head = np.sort(rng.choice(Hd // 2, 4, replace=False))
                    tails = rng.permutation(np.arange(Hd // 2, Hd))
                    slots = rng.choice(S, 4, replace=False)
                    rows[slots[0]] = ep._with(Hd, np.concatenate((head, tails[:2])))
                    rows[slots[1]] = ep._with(Hd, np.concatenate((head, tails[2:4])))
                    rows[slots[2]] = ep._with(Hd, rng.choice(Hd, 5, replace=False))
                    rows[slots[3]] = ep._with(Hd, rng.choice(Hd, 7, replace=False))
                    if _distinct(rows):
                        break
                else:
                    raise AssertionError("no distinct planted rows")
        if zero_parent and rows.any(axis=1).all():  # a parent of no active latent
            rows[0] = False
        ss[n, :, :Hd] = rows
    if bg:
        ss[:, :, H - 1] = True
    return ss


def _row_keys(rows):
    packed = np.ascontiguousarray(np.packbits(rows, axis=1))
    return packed.view(np.dtype((np.void, packed.shape[1]))).ravel()


def make_lpj(rng, S, S_perm):
    """The uploaded lpj rows (N, S_perm + S)."""
    L = S + S_perm
    lpj = np.empty((N, L))
    for n in range(N):
        kind = n % 4
        if kind == 0:    # all negative
            row = -40.0 + 5.0 * rng.normal(size=L)
            row = np.minimum(row, -0.5)
        elif kind == 1:  # positive with exact 0s: fitness zero, taken last, the lower slot first
            row = 0.5 + 3.0 * np.abs(rng.normal(size=L))
            row[S_perm + rng.choice(S, min(2, S - 1), replace=False)] = 0.0
        elif kind == 2:  # one value for all
            row = np.full(L, -7.25)
        else:            # both signs, values repeated
            row = np.round(4.0 * rng.normal(size=L)) * 0.5
        lpj[n] = row
    return lpj


@functools.lru_cache(maxsize=None)
def make_problem(name):
    c = CASES[name]
    rng = np.random.RandomState(seed_of(name))
    model = getattr(c, "model", "bsc")
    p = {"name": name, "case": c, "model": model, "N": N, "D": D, "H": c.H, "S": c.S, "S_perm": c.S_perm, "bg": c.bg,
         "Cmax": cmax(name), "seed": 77000 + seed_of(name)}
    p["ss"] = make_kn(rng, c.S, c.H, c.S_perm, c.bg, getattr(c, "zero_parent", False))
    p["lpj"] = make_lpj(rng, c.S, c.S_perm)
    p["Y"] = rng.normal(size=(N, D))
    p["theta"] = ep.es3c_theta(rng, D, c.H) if model == "sssc" else ep.bsc_theta(rng, D, c.H)
    for n in range(0, N, 37):
        assert _distinct(p["ss"][n]), (name, n)
    return p


def oracle_lpj(p, states, n):
    """float64 oracle lpj of ``states`` (C, H) of datapoint n."""
    return ep.oracle_lpj(p, states[None], n)[0]


def run_mirror(p, cand_lpj=None):
    """The mirror's (cand, counts, info) of problem p; ``cand_lpj`` as evolve_states_counter takes it (default: the
    float64 oracle)."""
    from evo_amd.variational import eas_counter as ec
    c = p["case"]
    if p["name"] in FAST:
        return ec.evolve_randflip_counter(p["ss"], p["lpj"], c.S_perm, c.n_parents, c.n_children, p["seed"], bool(c.fit),
                                          background=bool(c.bg))
    if cand_lpj is None:
        def cand_lpj(n, slot0, new_states):
            return oracle_lpj(p, new_states, n)
    return ec.evolve_states_counter(p["ss"], p["lpj"], c.S_perm, c.mutation, c.n_parents, c.n_children, c.n_gen, p["seed"],
                                    bool(c.fit), c.sparseness, c.p_bf, cand_lpj, background=bool(c.bg))

"""Problems for the dictionary-resize tests (tests/test_remap_host.py, tests/test_gpu_remap.py): K^n with S distinct states
per datapoint, built so that states collapse under the index of the case, the index itself and an independent brute
force of the remap law on bool rows (sets of tuples of active latents; evo_amd.variational.remap_states_host is the
mirror under test).  A case is computed once and handed out read-only."""
from functools import lru_cache
from itertools import combinations

import numpy as np

N_DEFAULT = 37  # no multiple of the waves per workgroup


class RemapCase:
    pass


def distinct_states(rng, N, S, H, p_on, S_perm=0, background=False):
    """bool (N, S, H): S distinct Bernoulli(p_on) states per datapoint (never all-zero with S_perm = 1)."""
    Hv = H - 1 if background else H
    ss = np.zeros((N, S, H), dtype=bool)
    for n in range(N):
        seen = []
        keys = set()
        while len(seen) < S:
            row = np.zeros(H, dtype=bool)
            row[:Hv] = rng.random_sample(Hv) < p_on
            if background:
                row[-1] = True
            if S_perm and not row.any():
                continue
            if row.tobytes() not in keys:
                keys.add(row.tobytes())
                seen.append(row)
        ss[n] = np.array(seen)
    return ss


def plant(rng, ss, dropped, max_plant, S_perm=0):
    """In place: up to ``max_plant`` slots per datapoint become a copy of another slot with one dropped latent flipped (they
    collapse under the index), wherever the result is new to the datapoint."""
    N, S, H = ss.shape
    dropped = np.asarray(dropped)
    for n in range(N):
        for _ in range(rng.randint(0, max_plant + 1)):
            a, b = rng.choice(S, 2, replace=False)
            row = ss[n, a].copy()
            d = dropped[rng.randint(len(dropped))]
            row[d] = ~row[d]
            if (S_perm and not row.any()) or any((ss[n, j] == row).all() for j in range(S)):
                continue
            ss[n, b] = row


def brute_force(ss, index, S_perm, background):
    """The remap law restated on tuples of active latents.  Returns (ss_new, n_replaced, kept (N, S) bool)."""
    N, S, H = ss.shape
    index = [int(v) for v in index]
    H2 = len(index)
    Hv2 = H2 - 1 if background else H2
    enum = [(a,) for a in range(Hv2)] + list(combinations(range(Hv2), 2))
    if background:
        enum = [t + (H2 - 1,) for t in enum]
    out = np.zeros((N, S, H2), dtype=bool)
    kept = np.zeros((N, S), dtype=bool)
    n_rep = np.zeros(N, dtype=np.int32)
    for n in range(N):
        gathered = [tuple(h2 for h2, h in enumerate(index) if h >= 0 and ss[n, j, h]) for j in range(S)]
        for j, t in enumerate(gathered):
            kept[n, j] = t not in gathered[:j] and not (S_perm and len(t) == 0)
        have = {t for j, t in enumerate(gathered) if kept[n, j]}
        pos = 0
        for j, t in enumerate(gathered):
            if not kept[n, j]:
                while enum[pos] in have:
                    pos += 1
                t = enum[pos]
                pos += 1
                n_rep[n] += 1
            out[n, j, list(t)] = True
    return out, n_rep, kept


def _index_drop(rng, H, drop, n_new=0, shuffle=True, background=False):
    Hv = H - 1 if background else H
    keep = np.array([h for h in range(Hv) if h not in set(drop)], dtype=np.int32)
    idx = np.concatenate((keep, np.full(n_new, -1, dtype=np.int32)))
    if shuffle:
        idx = idx[rng.permutation(idx.size)]
    if background:
        idx = np.concatenate((idx, np.array([H - 1], dtype=np.int32)))
    return idx.astype(np.int32)


def _build(name):
    c = RemapCase()
    c.name, c.N, c.S_perm, c.background = name, N_DEFAULT, 0, False
    rng = np.random.RandomState(sum(map(ord, name)))
    if name == "boundary":      # H 70 -> 66: dropped latents on both sides of bit 63 / 64, HW 2 -> 2
        c.H, c.S, drop = 70, 40, [61, 63, 64, 66]
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.06)
        plant(rng, c.ss, drop, 3)
        c.index = _index_drop(rng, c.H, drop)
    elif name == "prototype":   # 70 -> 68: a random permutation with four latents dropped and two new
        c.H, c.S, drop = 70, 40, [5, 33, 63, 69]
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.05)
        plant(rng, c.ss, drop, 3)
        c.index = _index_drop(rng, c.H, drop, n_new=2)
    elif name == "shrink":      # H 130 -> 60: HW 3 -> 1
        c.H, c.S = 130, 40
        drop = [int(h) for h in rng.choice(c.H, 70, replace=False)]
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.03)
        plant(rng, c.ss, drop, 3)
        c.index = _index_drop(rng, c.H, drop)
    elif name == "grow":        # H 64 -> 70 with six new latents: HW 1 -> 2
        c.H, c.S = 64, 40
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.06)
        c.index = _index_drop(rng, c.H, [], n_new=6)
    elif name == "permutation":  # nothing collapses: n_replaced = 0
        c.H, c.S = 70, 40
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.06)
        c.index = rng.permutation(c.H).astype(np.int32)
    elif name == "pairs":       # H 8 -> 6, S = 18 of 21 fill candidates: fills run past the six singletons into the pairs
        c.H, c.S = 8, 18
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.3)
        plant(rng, c.ss, [6, 7], 4)
        c.index = np.arange(6, dtype=np.int32)
    elif name == "small":       # H 12 -> 10, S = 30: many replacements per datapoint
        c.H, c.S, drop = 12, 30, [1, 4, 7, 10]
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.3)
        c.index = _index_drop(rng, c.H, drop, n_new=2)
    elif name == "allzero":     # S_perm = 1: states of dropped latents only gather to the permanent all-zero state
        c.H, c.S, c.S_perm, drop = 70, 40, 1, [2, 40, 63, 64, 69]
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.05, S_perm=1)
        for n in range(c.N):
            for j, d in zip(rng.choice(c.S, rng.randint(1, 4), replace=False), rng.permutation(drop)):
                row = np.zeros(c.H, dtype=bool)
                row[d] = True
                if not any((c.ss[n, i] == row).all() for i in range(c.S)):
                    c.ss[n, j] = row
        plant(rng, c.ss, drop, 2, S_perm=1)
        c.index = _index_drop(rng, c.H, drop)
    elif name == "background":  # the background unit stays last and on; fills carry its bit
        c.H, c.S, c.background, drop = 70, 40, True, [0, 31, 63, 64]
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.05, background=True)
        plant(rng, c.ss, drop, 4)
        c.index = _index_drop(rng, c.H, drop, n_new=1, background=True)
    elif name == "dense":       # 5 .. 9 active latents: equal digests (count and first four latents) with different words
        c.H, c.S, drop = 130, 40, [3, 64, 100, 129]
        c.ss = np.zeros((c.N, c.S, c.H), dtype=bool)
        kept_lat = np.array([h for h in range(c.H) if h not in drop])
        for n in range(c.N):
            keys, rows = set(), []
            head = np.sort(rng.choice(kept_lat[kept_lat < 60], 4, replace=False))  # the digest's four slots, shared
            while len(rows) < c.S:
                k = rng.randint(5, 10)
                tail = rng.choice(kept_lat[kept_lat >= 60], k - 4, replace=False)
                row = np.zeros(c.H, dtype=bool)
                row[head] = True
                row[tail] = True
                if row.tobytes() not in keys:
                    keys.add(row.tobytes())
                    rows.append(row)
            c.ss[n] = np.array(rows)
        plant(rng, c.ss, drop, 4)
        c.index = _index_drop(rng, c.H, drop, shuffle=False)  # ascending: the shared head stays the digest's four slots
    elif name == "f32":         # EBSC float32 mode: H and H' multiples of 4
        c.H, c.S, drop = 72, 40, [61, 63, 64, 66]
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.06)
        plant(rng, c.ss, drop, 3)
        c.index = _index_drop(rng, c.H, drop)
    elif name == "cap":         # the largest S whose LDS slice fits at H 640 -> 576 (10 + 9 + 1 words per state)
        c.N, c.H, c.S, drop = 3, 640, 945, list(range(0, 640, 10))
        c.ss = distinct_states(rng, c.N, c.S, c.H, 0.01)
        plant(rng, c.ss, drop, 5)
        c.index = _index_drop(rng, c.H, drop, shuffle=False)
    else:
        raise KeyError(name)
    c.H2 = int(c.index.size)
    for n in range(c.N):
        assert len({r.tobytes() for r in c.ss[n]}) == c.S
    c.want, c.n_replaced, c.kept = brute_force(c.ss, c.index, c.S_perm, c.background)
    for a in (c.ss, c.index, c.want, c.n_replaced, c.kept):
        a.setflags(write=False)
    return c


CASES = ("boundary", "prototype", "shrink", "grow", "permutation", "pairs", "small", "allzero", "background", "dense", "f32", "cap")
# LDS cap of evoamd_remap_latents: 150 KiB = 256 ceil(H'/64) bytes of index + 8 S (ceil(H/64) + ceil(H'/64) + 1) per wave
CAP_S = (150 * 1024 // 8 - 32 * 9) // (10 + 9 + 1)
assert CAP_S == 945


@lru_cache(maxsize=None)
def case(name):
    return _build(name)

"""The NumPy mirror of the device EA (evo_amd.variational.eas_counter) against the reference's law, without a GPU.

The mirror is what test_gpu_evolve_parity.py holds the kernels to bit for bit, so it has to be right on its own account:
the laws that test_gpu_evolve.py checks on the device are checked here on the mirror (1-2 x 10^4 runs, the same 5 sigma
band and chi-square slack: fixed seeds, deterministic outcome), the returned-set law of several generations is compared
with oracle.evolve_states on np.random, every case of the parity tables keeps the invariants of evolve_states and its
share of undecided datapoints under the cap, and a few values of the stream are pinned as integers."""
import functools
import itertools
import warnings

import numpy as np
import pytest

import _evolve_problems as vp
from evo_amd.variational import eas_counter as ec
from evo_amd.variational import evolve_randflip_counter, evolve_states_counter

Z_MAX = 5.0
UNDECIDED_CAP = 0.02


def _z(count, n, prob):
    count, prob = np.asarray(count, dtype=float), np.asarray(prob, dtype=float)
    return (count - n * prob) / np.sqrt(np.maximum(n * prob * (1.0 - prob), 1e-300))


def _chi2_ok(obs, exp, slack=1.6):
    obs, exp = np.asarray(obs, float), np.asarray(exp, float)
    df = len(obs) - 1
    stat = ((obs - exp) ** 2 / exp).sum()
    assert stat < slack * df + 5 * np.sqrt(2.0 * df), (stat, df)


def _inclusion_probs(p, n_draw):
    """Exact inclusion probabilities of successive sampling without replacement (np.random.choice(..., replace=False,
    p=p))."""
    inc = np.zeros(len(p))
    for seq in itertools.permutations(range(len(p)), n_draw):
        pr, rest = 1.0, 1.0
        for i in seq:
            pr *= p[i] / rest
            rest -= p[i]
        inc[list(seq)] += pr
    return inc


def _tiled(states, lpj, N):
    return np.tile(states[None], (N, 1, 1)), np.tile(np.asarray(lpj, dtype=float)[None], (N, 1))


def _no_lpj(n, slot0, new_states):
    return np.zeros(new_states.shape[0])


# ---- the stream ------------------------------------------------------------------------------------------------------------
def _u01_int(seed, n, purpose, index):
    """rng_u01 on Python integers, straight from the definition in csrc/kernels_evolve.hpp."""
    M = (1 << 64) - 1

    def mix(x):
        x ^= x >> 30
        x = (x * 0xbf58476d1ce4e5b9) & M
        x ^= x >> 27
        x = (x * 0x94d049bb133111eb) & M
        return x ^ (x >> 31)

    x = mix((seed + 0x9e3779b97f4a7c15 * (n + 1)) & M)
    x = mix(x ^ ((purpose * 0xd1b54a32d192ed03 + index + 0x632be59bd9b4e019) & M))
    return (float(x >> 11) + 0.5) * (1.0 / 9007199254740992.0)


PINNED = [  # (seed, n, purpose, index) -> rng_u01 * 2^54
    ((0, 0, 0, 0), 1166817572498717),
    ((1234, 7, 1, 63), 9604932571280908),
    ((77001, 255, 2 + 8, 7), 11151370011309036),
    ((2 ** 64 - 1, 10 ** 6, (3 << 32) + 16 + 239, 1 + 520 + 3), 8950705362584129),
    ((555, 3, (1 << 32) + 8 + 4096 + 5, 0), 10946048634069616),
]


def test_stream_values_are_pinned():
    for args, want in PINNED:
        assert ec.rng_bits(*args) == want, (args, ec.rng_bits(*args))
        assert float(ec.rng_u01(*args)[0]) == _u01_int(*args)
    # broadcasting draws what the single calls draw
    n, pu, ix = np.arange(5)[:, None, None], (1 << 32) + np.arange(3)[None, :, None], np.arange(70)[None, None, :]
    u = ec.rng_u01(99, n, pu, ix)
    assert u.shape == (5, 3, 70) and np.all((u > 0.0) & (u < 1.0))
    for a, b, c in [(0, 0, 0), (4, 2, 69), (2, 1, 64)]:
        assert u[a, b, c] == _u01_int(99, a, (1 << 32) + b, c)


def test_race_keys_and_margin():
    """The float64 key of the float32-rounded inputs; the sentinels; ties go to the lowest index; the margin is the
    smallest relative gap among the first P + 1 keys, equal keys left out."""
    u = np.array([0.5, 0.25, 1.0 - 2.0 ** -30, 1e-300, 0.5])
    p = np.array([2.0, 1.0, 3.0, 1.0, 0.0])
    k = ec.race_keys(u, p)
    assert k[0] == np.log(2.0) / 2.0 and k[1] == np.log(4.0)
    assert k[2] == 0.0                                     # float32(u) = 1
    assert k[3] == -np.log(float(np.float32(1.17549435e-38)))  # u clamped at FLT_MIN
    assert k[4] == float(np.float32(1e30))                 # p <= 0
    assert ec.race_keys(np.array([0.5]), np.array([1e-60]))[0] == float(np.float32(3.0e38))  # float32(p) = 0: clamped
    keys = np.array([3.0, 1.0, 1.0, 2.0, 1e30, 1e30])
    order, margin = ec.draw_parents(keys, 3)
    assert order.tolist() == [1, 2, 3] and margin == (3.0 - 2.0) / 3.0   # (1, 1) is no gap; 2 | 3 is the P-th | (P+1)-th
    order, margin = ec.draw_parents(keys, 5)
    assert order.tolist() == [1, 2, 3, 0, 4] and margin == (3.0 - 2.0) / 3.0
    assert ec.draw_parents(np.array([1.0]), 1)[1] == np.inf
    assert ec.fitness(np.array([-3.0, -1.0]), True).tolist() == [3.0, 5.0]      # eas.py:139
    assert ec.fitness(np.array([3.0, 1.0]), True).tolist() == [3.0, 1.0]
    assert ec.fitness(np.array([3.0, 1.0]), False).tolist() == [1.0, 1.0]


def test_flip_picks_are_the_rth_unused_positions():
    rng = np.random.RandomState(0)
    for Hd, T in [(7, 7), (64, 8), (5, 2)]:
        u = rng.random_sample((200, T))
        u[0] = 1.0 - 2.0 ** -53   # the clamp of r
        u[1] = 2.0 ** -53
        got = ec.flip_picks(u, Hd)
        for row_u, row in zip(u, got):
            unused = list(range(Hd))
            for t in range(T):
                r = min(int(row_u[t] * (Hd - t)), Hd - t - 1)
                assert row[t] == unused.pop(r)


# ---- the laws of the operators -----------------------------------------------------------------------------------------------
def _distant_states(S, H):
    states = np.zeros((S, H), dtype=bool)
    for j in range(S):
        states[j, 4 * j:4 * j + 3] = True  # pairwise Hamming distance 6: a child names its parent and its flip
    return states


LPJ8 = np.array([-1.0, -9.5, -2.25, -12.0, -5.0, -3.5, -10.0, -7.0])


def test_fast_kernel_parent_and_flip_law():
    """fitparents + randflip of the fast kernel's stream: first parent ~ p, inclusion = successive sampling, no parent
    twice, flips uniform over H and distinct per parent; the children are the parents with those flips."""
    H, S, P, C, N = 32, 8, 3, 4, 20000
    states = _distant_states(S, H)
    ss, lpj = _tiled(states, LPJ8, N)
    f = LPJ8 - 2 * min(LPJ8.min(), 0.0)
    p = f / f.sum()
    assert p.max() / p.min() > 1.3
    cand, counts, info = evolve_randflip_counter(ss, lpj, 0, P, C, 1234, True)
    assert np.all(counts == P * C) and cand.shape == (N, P * C, H)
    par, flips = info["parents"], info["flips"]
    _chi2_ok(np.bincount(par[:, 0], minlength=S), N * p)
    cnt = np.array([(par == j).any(axis=1).sum() for j in range(S)])
    assert np.abs(_z(cnt, N, _inclusion_probs(p, P))).max() < Z_MAX
    srt = np.sort(par, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1])
    _chi2_ok(np.bincount(flips.ravel(), minlength=H), np.full(H, flips.size / H))
    fs = np.sort(flips, axis=2)
    assert np.all(fs[:, :, 1:] != fs[:, :, :-1])
    want = np.repeat(states[par], C, axis=1)
    want[np.arange(N)[:, None], np.arange(P * C)[None, :], flips.reshape(N, -1)] ^= True
    assert np.array_equal(cand, want)
    # randparents: uniform inclusion; S_perm only moves the lpj row; the background unit is never flipped
    ss1 = ss.copy()
    ss1[:, :, H - 1] = True
    cand, counts, info = evolve_randflip_counter(ss1, np.concatenate((lpj[:, :1], lpj), axis=1), 1, P, C, 99, False,
                                                 background=True)
    cnt = np.array([(info["parents"] == j).any(axis=1).sum() for j in range(S)])
    assert np.abs(_z(cnt, N, np.full(S, P / S))).max() < Z_MAX
    assert info["flips"].max() == H - 2 and cand[:, :, H - 1].all()
    _chi2_ok(np.bincount(info["flips"].ravel(), minlength=H - 1), np.full(H - 1, info["flips"].size / (H - 1.0)))


def test_general_kernel_parent_and_flip_law():
    """The same laws for generation 0 of the general kernel's stream (other purposes, de-duplicated sorted output)."""
    H, S, P, C, N = 32, 8, 3, 4, 5000
    states = _distant_states(S, H)
    ss, lpj = _tiled(states, LPJ8, N)
    f = LPJ8 - 2 * min(LPJ8.min(), 0.0)
    p = f / f.sum()
    cand, counts, info = evolve_states_counter(ss, lpj, 0, "randflip", P, C, 1, 4321, True, 0.0, None, _no_lpj)
    assert np.all(counts == P * C)  # distant parents, distinct flips: nothing collides
    par = np.array([d[0]["parents"] for d in info["draws"]])
    flips = np.array([d[0]["flips"] for d in info["draws"]])
    _chi2_ok(np.bincount(par[:, 0], minlength=S), N * p)
    cnt = np.array([(par == j).any(axis=1).sum() for j in range(S)])
    assert np.abs(_z(cnt, N, _inclusion_probs(p, P))).max() < Z_MAX
    _chi2_ok(np.bincount(flips.ravel(), minlength=H), np.full(H, flips.size / H))
    fs = np.sort(flips, axis=2)
    assert np.all(fs[:, :, 1:] != fs[:, :, :-1])
    for n in range(0, N, 50):  # the batch is the sorted set of the raw children
        raw = info["draws"][n][0]["raw"]
        want = np.repeat(states[par[n]], C, axis=0)
        want[np.arange(P * C), flips[n].ravel()] ^= True
        assert np.array_equal(raw, want)
        rows = sorted(bytes(np.packbits(r)) for r in raw)
        assert [bytes(np.packbits(r)) for r in cand[n, :counts[n]]] == rows


def test_cross_law():
    """cross: both tail exchanges of every pair of combinations(range(P), 2) at a cut uniform on 1 .. H-1;
    cross_randflip: one more uniform flip per child."""
    H, S, P, N = 24, 4, 4, 2500
    rng = np.random.RandomState(3)
    states = rng.random_sample((S, H)) < 0.5
    ss, lpj = _tiled(states, np.array([-3.0, -4.0, -5.0, -6.0]), N)
    for mutation in ("cross", "cross_randflip"):
        cand, counts, info = evolve_states_counter(ss, lpj, 0, mutation, P, 1, 1, 31, False, 0.0, None, _no_lpj)
        cuts = np.array([d[0]["cuts"] for d in info["draws"]])
        assert cuts.shape == (N, 6) and cuts.min() == 1 and cuts.max() == H - 1
        _chi2_ok(np.bincount(cuts.ravel(), minlength=H)[1:], np.full(H - 1, cuts.size / (H - 1.0)))
        for n in range(0, N, 25):
            d = info["draws"][n][0]
            par = states[d["parents"]]
            want = []
            for t, (a, b) in enumerate(itertools.combinations(range(P), 2)):
                cp = d["cuts"][t]
                want += [np.concatenate((par[a, :cp], par[b, cp:])), np.concatenate((par[b, :cp], par[a, cp:]))]
            want = np.array(want)
            if mutation == "cross_randflip":
                want[np.arange(12), d["flips"]] ^= True
            assert np.array_equal(d["raw"], want)
        if mutation == "cross_randflip":
            flips = np.array([d[0]["flips"] for d in info["draws"]])
            _chi2_ok(np.bincount(flips.ravel(), minlength=H), np.full(H, flips.size / H))


@pytest.mark.parametrize("k", [0, 1, 3, 7])
def test_sparseflip_law(k):
    """sparseflip (eas.py:46-100): a 0 flips with p_0, a 1 with p_1 = alpha p_0, independently (k = 0: a parent of no
    active latent), and the oracle's operator on np.random obeys the same law."""
    from oracle import evo_oracle as orc
    H, N, C = 40, 3000, 4
    sparseness, p_bf = 2.5, 0.08
    parent = np.zeros((1, H), dtype=bool)
    parent[0, [3, 11, 12, 20, 29, 30, 38][:k]] = True
    s_abs, eps = float(k), 1e-100
    alpha = (H - s_abs) * ((H * p_bf) - (sparseness - s_abs)) / ((sparseness - s_abs + H * p_bf) * s_abs + eps)
    p0 = (H * p_bf) / (H + (alpha - 1.0) * s_abs + eps)
    pbit = np.clip(np.where(parent[0], alpha * p0, p0), 0.0, 1.0)
    np.random.seed(3)
    kids = orc.sparseflip(np.repeat(parent, 12000, axis=0), 1, sparseness, p_bf)
    assert np.abs(_z((kids ^ parent).sum(axis=0), 12000, pbit)).max() < Z_MAX
    ss, lpj = _tiled(parent, np.array([-5.0]), N)
    cand, counts, info = evolve_states_counter(ss, lpj, 0, "sparseflip", 1, C, 1, 2024 + k, False, sparseness, p_bf, _no_lpj)
    assert not info["sparse_undecided"].any()
    fl = np.concatenate([d[0]["raw"] for d in info["draws"]]) ^ parent
    assert np.abs(_z(fl.sum(axis=0), N * C, pbit)).max() < Z_MAX
    z0 = np.flatnonzero(~parent[0])[:2]   # independence of two zero bits
    assert abs(_z((fl[:, z0[0]] & fl[:, z0[1]]).sum(), N * C, pbit[z0[0]] * pbit[z0[1]])) < Z_MAX
    # the batch: the distinct children that differ from the parent
    for n in range(0, N, 100):
        rows = {bytes(np.packbits(r)) for r in info["draws"][n][0]["raw"]} - {bytes(np.packbits(parent[0]))}
        assert [bytes(np.packbits(r)) for r in cand[n, :counts[n]]] == sorted(rows)


def test_sparseflip_edges():
    """p_0 >= 1 flips every 0, p_0 <= 0 none, and every position is judged against the state before any flip."""
    H = 64
    parent = np.zeros((1, 1, H), dtype=bool)
    lpj = np.array([[-5.0]])
    cand, counts, _ = evolve_states_counter(parent, lpj, 0, "sparseflip", 1, 1, 1, 5, True, 2.5, 2.0, _no_lpj)
    assert counts[0] == 1 and cand[0, 0].all()
    cand, counts, _ = evolve_states_counter(parent, lpj, 0, "sparseflip", 1, 1, 1, 5, True, 2.5, 0.0, _no_lpj)
    assert counts[0] == 0
    parent[0, 0, [1, 2, 3]] = True  # p_bf = 2: p_0 >= 1 and p_1 >= 1, the child is the complement
    cand, counts, _ = evolve_states_counter(parent, lpj, 0, "sparseflip", 1, 1, 1, 5, True, 2.5, 2.0, _no_lpj)
    assert counts[0] == 1 and np.array_equal(cand[0, 0], ~parent[0, 0])


def _oracle_runs(states, lpj, ea, piH, eval_lpj, n_runs, seed):
    from oracle import evo_oracle as orc
    np.random.seed(seed)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(n_runs):
            st, _ = orc.evolve_states(states.copy(), lpj.copy(), ea, piH, eval_lpj)
            out.append(frozenset(tuple(np.flatnonzero(r)) for r in st))
    return out


@pytest.mark.parametrize("mutation,S_perm,n_gen,n_par,n_child", [
    ("randflip", 1, 3, 2, 2), ("sparseflip", 0, 2, 3, 2), ("cross_randflip", 0, 2, 3, 2), ("cross_sparseflip", 1, 2, 3, 2)])
def test_generations_match_oracle_law(mutation, S_perm, n_gen, n_par, n_child):
    """n_generations > 1 with the next-generation pools of eas.py:278-293 on H = 5, where children collide
    with known states all the time: which state is returned how often and how many states a run returns, mirror against
    oracle.evolve_states on np.random (two samples)."""
    from oracle import evo_oracle as orc
    H, S, D, N, n_or = 5, 4, 6, 10000, 3000
    rng = np.random.RandomState(11)
    all_states = np.array(list(itertools.product([False, True], repeat=H)))[1:]
    states = all_states[rng.permutation(len(all_states))[:S]]
    crossing = "cross" in mutation
    if crossing:
        n_child = n_par - 1
    per_gen = n_par * (n_par - 1) if crossing else n_par * n_child
    rng = np.random.RandomState(21)
    W, y = rng.normal(size=(D, H)), rng.normal(size=D)
    theta = {"W": W, "pi": 0.2, "sigma": 1.3}
    orc.bsc_precompute(theta, D, H)
    cnt = orc.new_counters()
    lpj = orc.bsc_lpj(theta, states, y, cnt)
    lpj_perm = orc.bsc_lpj_allzero(theta, y, cnt)[:S_perm]
    ea = {"permanent": {"background": False, "allzero": S_perm == 1, "singletons": False},
          "incl": np.zeros((S_perm, H), dtype=bool), "n_parents": n_par, "n_children": n_child, "n_generations": n_gen,
          "parent_selection": orc.fitparents, "mutation_algorithm": orc.MUTATION[mutation], "bitflip_prob": 0.15}
    runs = _oracle_runs(states, lpj, ea, theta["piH"], lambda st: orc.bsc_lpj(theta, st, y, cnt), n_or, 7)
    table = {}  # (every datapoint is the same: the lpj of a state is looked up)

    def cand_lpj(n, slot0, new):
        out = np.empty(new.shape[0])
        for i, r in enumerate(new):
            key = r.tobytes()
            if key not in table:
                table[key] = orc.bsc_lpj(theta, r[None], y, cnt)[0]
            out[i] = table[key]
        return out

    ss, rows = _tiled(states, np.concatenate((np.ravel(lpj_perm), lpj)), N)
    cand, counts, info = evolve_states_counter(ss, rows, S_perm, mutation, n_par, n_child, n_gen, 555, True, theta["piH"],
                                               0.15, cand_lpj)
    assert cand.shape[1] == per_gen * n_gen
    code = (cand * (1 << np.arange(H))[None, None, :]).sum(axis=2)
    valid = np.arange(cand.shape[1])[None, :] < counts[:, None]
    for st in all_states.tolist() + [[False] * H]:
        key = tuple(np.flatnonzero(st))
        c_or = sum(1 for r in runs if key in r)
        c_mi = int(((code == sum(1 << h for h in key)) & valid).any(axis=1).sum())
        pool = (c_or + c_mi) / float(n_or + N)
        if pool in (0.0, 1.0):
            assert c_or / n_or == c_mi / N
            continue
        z = (c_mi / N - c_or / n_or) / np.sqrt(pool * (1 - pool) * (1.0 / N + 1.0 / n_or))
        assert abs(z) < Z_MAX, (key, c_mi / N, c_or / n_or, z)
    sizes_or = np.bincount([len(r) for r in runs], minlength=per_gen * n_gen + 1) / n_or
    sizes_mi = np.bincount(counts, minlength=per_gen * n_gen + 1) / N
    for a, b in zip(sizes_mi, sizes_or):
        pool = (a * N + b * n_or) / (N + n_or)
        if 0.0 < pool < 1.0:
            assert abs(a - b) / np.sqrt(pool * (1 - pool) * (1.0 / N + 1.0 / n_or)) < Z_MAX, (sizes_mi, sizes_or)


# ---- the lower edge of the latent space ----------------------------------------------------------------------------------------
def test_tiny_cases_are_in_the_tables():
    assert vp.FAST["h1"] == vp.Fast(1, 2, 0, 0, 1, 1, 1, "bsc") and vp.FAST["h2"] == vp.Fast(2, 3, 0, 0, 2, 2, 1, "sssc")
    for i, op in enumerate(vp.OPERATORS):
        c = vp.GENERAL["%s_h2" % op]
        assert (c.H, c.S, c.S_perm, c.n_parents, c.n_children, c.n_gen) == (2, 3, 0, 2, 1, 2), op
        c = vp.GENERAL["%s_h3" % op]
        assert (c.H, c.S, c.S_perm) == (3, 5, i % 2) and c.S_perm == vp.GENERAL["%s_h5" % op].S_perm, op
    c = vp.GENERAL["randflip_h1"]
    assert (c.H, c.S, c.mutation) == (1, 2, "randflip")
    assert set(vp.TINY) == {"h1", "h2", "randflip_h1"} | {"%s_h%d" % (op, H) for op in vp.OPERATORS for H in (2, 3)}
    # the cases that were there before keep their seeds
    assert vp.seed_of("cross_h130") == 1000 and vp.seed_of("sparseflip_zero_parent") == 1000 + len(vp.CASES) - len(vp.TINY) - 1
    assert len({vp.seed_of(n) for n in vp.CASES}) == len(vp.CASES)


@pytest.mark.parametrize("H", [1, 2, 3])
def test_make_kn_builds_distinct_rows_up_to_the_whole_state_space(H):
    """S = 2^H - 1 and S = 2^H (and, with the permanent all-zero state, S = 2^H - 1 non-zero rows): every datapoint holds
    S distinct rows, and at S = 2^H all of them."""
    for S, S_perm in ((2 ** H - 1, 0), (2 ** H, 0), (2 ** H - 1, 1)):
        if S < 1:
            continue
        ss = vp.make_kn(np.random.RandomState(H), S, H, S_perm, 0)
        assert ss.shape == (vp.N, S, H)
        for n in range(vp.N):
            assert len({r.tobytes() for r in ss[n]}) == S, (H, S, n)
            if S_perm:
                assert ss[n].any(axis=1).all(), (H, S, n)
    for name in vp.TINY:  # ... and the cases' own K^n, every datapoint
        p = vp.make_problem(name)
        for n in range(vp.N):
            assert len({r.tobytes() for r in p["ss"][n]}) == p["S"], (name, n)


def test_tiny_operators_degenerate_as_named():
    """H = 2: the crossover's cut has one value; sparseflip's p0 and p1 lie inside (0, 1) for every parent the formula does
    not pin (a parent of H latents has alpha = 0, so p1 = 0, and no 0 to flip; a parent of none has no 1); H = 1, S = 2:
    no child is new."""
    for name in ("cross_h2", "cross_randflip_h2", "cross_sparseflip_h2"):
        _, _, info = _mirror(name)
        cuts = np.concatenate([np.ravel(g["cuts"]) for d in info["draws"] for g in d if "cuts" in g])
        assert cuts.size and set(cuts.tolist()) == {1}, name
    for name in ("sparseflip_h2", "cross_sparseflip_h2", "sparseflip_h3", "cross_sparseflip_h3"):
        c = vp.CASES[name]
        for s_abs in range(c.H + 1):
            p0, p1 = ec.sparse_probabilities(c.H, s_abs, c.sparseness, c.p_bf)
            if s_abs < c.H:
                assert 0.0 < float(p0) < 1.0, (name, s_abs, p0)
            if 0 < s_abs < c.H:
                assert 0.0 < float(p1) < 1.0, (name, s_abs, p1)
        assert float(ec.sparse_probabilities(c.H, c.H, c.sparseness, c.p_bf)[1]) == 0.0
    cand, counts, _ = _mirror("randflip_h1")
    assert not counts.any()
    cand, counts, _ = _mirror("h1")  # the fast kernel does not de-duplicate: one child, the other state
    p = vp.make_problem("h1")
    assert np.all(counts == 1) and np.all(cand[:, 0, 0] != p["ss"][np.arange(vp.N), _mirror("h1")[2]["parents"][:, 0], 0])
    for name in vp.TINY:
        if name not in vp.FAST and vp.CASES[name].H > 1:
            assert _mirror(name)[1].any(), name  # something new is found: the comparison on the GPU is not vacuous


# ---- every case of the parity tables ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mirror(name):
    return vp.run_mirror(vp.make_problem(name))


def _keys(rows):
    return [bytes(np.packbits(r)) for r in rows]


@pytest.mark.parametrize("name", list(vp.CASES))
def test_case_invariants_and_undecided_share(name):
    """Per case: the undecided share at tau = 2^-18 stays under the 2 % cap; counts stay within children per generation x
    generations; no latent outside the operators' domain changes.  Fast kernel: every slot is its parent with one flip.
    General kernel: the candidates of a generation are new, unique and in np.unique's order."""
    p, c = vp.make_problem(name), vp.CASES[name]
    cand, counts, info = _mirror(name)
    N, H, S_perm = p["N"], p["H"], p["S_perm"]
    assert ec.RACE_TAU == 2.0 ** -18
    und = ec.undecided(info)
    share = und[:, -1].mean()
    print("%s: undecided share %.4f" % (name, share))
    assert share <= UNDECIDED_CAP, (name, share)
    assert cand.shape[0] == N and cand.shape[2] == H and cand.shape[1] <= p["Cmax"]
    assert counts.min() >= 0 and counts.max() <= cand.shape[1]
    if c.bg:
        assert all(cand[n, :counts[n], H - 1].all() for n in range(N))
    if name in vp.FAST:
        par = p["ss"][np.arange(N)[:, None], info["parents"]]
        diff = cand ^ np.repeat(par, c.n_children, axis=1)
        assert np.all(diff.sum(axis=2) == 1) and np.all(np.argmax(diff, axis=2) < H - c.bg)
        return
    gc = info["gen_counts"]
    assert np.array_equal(gc[:, -1], counts) and np.all(np.diff(gc, axis=1) >= 0)
    assert np.all(np.diff(gc, axis=1) <= vp.per_generation(c))
    for n in range(N):
        known = set(_keys(p["ss"][n])) | ({bytes(np.packbits(np.zeros(H, dtype=bool)))} if S_perm else set())
        rows = _keys(cand[n, :counts[n]])
        assert len(set(rows)) == len(rows) and not (set(rows) & known), (name, n)
        for g in range(c.n_gen):
            seg = rows[gc[n, g]:gc[n, g + 1]]
            assert seg == sorted(seg), (name, n, g)


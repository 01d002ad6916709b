"""Problems shared by tests/test_predictive_host.py, tests/test_gpu_predictive.py and tests/test_gpu_precision_merge.py:
Theta, data, hand-built K^n and lpj rows with the NumPy mirror's moments (computed once per problem: lru_cache; do not
modify), the steps of the missing_* fixtures, and the merge cases with their explicit triple-loop reference."""
from functools import lru_cache

import numpy as np

from conftest import load_golden, unpack_bits
from evo_amd.models import predictive_moments_host
from evo_amd.utils.prepost import patch_tops

K_LIST = (1, 2, 3, 4, 5, 8, 9, 12)  # active latents of the eight hand-built states of datapoint 0 (cut to H)


class NoEngine:
    """Host-only paths never touch the engine (the guard of tests/test_host_logic.py)."""

    def __getattr__(self, name):
        raise AssertionError("host-only code path touched the GPU engine: " + name)


class Problem:
    pass


def make_theta(rng, algo, D, H):
    W = rng.normal(size=(D, H)) * 0.4
    if algo == "ebsc":
        return {"W": W, "pi": 0.1, "sigma": np.float64(1.1)}
    A = rng.normal(size=(H, 3)) * 0.2
    return {"W": W, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H) * 0.5, "Psi": np.eye(H) + A @ A.T,
            "sigma2": np.float64(1.3)}


def make_states(rng, N, S, H, background):
    """K^n with S = 8 distinct states per datapoint of 1..3 latents; datapoint 0 holds states of K_LIST active latents
    (cut to the latents there are), datapoint 1 -- where H allows it -- one of 32 = PRED_MAX_K and one of 12."""
    Hv = H - 1 if background else H
    ss = np.zeros((N, S, H), dtype=bool)
    for n in range(N):
        seen = set()
        while len(seen) < S:
            seen.add(tuple(sorted(rng.choice(Hv, rng.randint(1, 4), replace=False))))
        for s, st in enumerate(sorted(seen)):
            ss[n, s, list(st)] = True
        rng.shuffle(ss[n])
    assert S == len(K_LIST)
    ss[0] = False
    ks = []
    for k in K_LIST:  # (H = 10: the last two states have 9 and 10 latents)
        k = min(k, Hv)
        while k in ks:
            k -= 1
        ks.append(k)
    for s, k in enumerate(ks):
        ss[0, s, rng.choice(Hv, k, replace=False)] = True
    if Hv >= 33:
        ss[1, 2] = False
        ss[1, 2, rng.choice(Hv, 32 - (1 if background else 0), replace=False)] = True
        ss[1, 5] = False
        ss[1, 5, rng.choice(Hv, 12, replace=False)] = True
    if background:
        ss[:, :, -1] = True
    return ss


@lru_cache(maxsize=None)
def problem(algo, N, D, H, incomplete=False, S_perm=0, background=False, seed=0):
    """One shape: p.theta, p.Y (NaN at the missing entries), p.x_infr, p.ss (N, 8, H), p.lpj (N, S_perm + 8), p.permanent
    and the mirror's p.mean / p.var (with the noise term) / p.var0 (without) / p.info.  Incomplete data: datapoint 5 has
    no reliable entry."""
    S = 8
    rng = np.random.RandomState(100000 * (algo == "ebsc") + 1000 * H + 10 * D + N + seed + 7 * background + 3 * incomplete)
    p = Problem()
    p.algo, p.N, p.D, p.H, p.S, p.S_perm, p.background, p.incomplete = algo, N, D, H, S, S_perm, background, incomplete
    assert not (background and S_perm)
    p.permanent = {"background": background, "allzero": bool(S_perm), "singletons": False}
    p.theta = make_theta(rng, algo, D, H)
    p.Y = rng.normal(size=(N, D)) * 1.5
    p.x_infr = np.ones((N, D), dtype=bool)
    if incomplete:
        p.x_infr = rng.random_sample((N, D)) >= 0.3
        p.x_infr[:, 0] = True
        p.x_infr[5] = False
        p.Y[~p.x_infr] = np.nan
    p.ss = make_states(rng, N, S, H, background)
    p.lpj = rng.normal(size=(N, S_perm + S)) * 1.5 - 40.0
    xi = p.x_infr if incomplete else None
    p.mean, p.var, p.info = predictive_moments_host(algo_name(algo), p.theta, p.ss, p.lpj, p.Y, xi, S_perm, background, True)
    _, p.var0, _ = predictive_moments_host(algo_name(algo), p.theta, p.ss, p.lpj, p.Y, xi, S_perm, background, False)
    for a in (p.Y, p.x_infr, p.ss, p.lpj, p.mean, p.var, p.var0):
        a.setflags(write=False)
    return p


def algo_name(algo):
    return "bsc" if algo == "ebsc" else "sssc"


def my_data_of(p):
    d = {"y": np.array(p.Y), "x_infr": np.array(p.x_infr)}
    if p.incomplete:
        d["x"] = np.array(p.x_infr)
    return d


# ---- the reference's own numbers: the steps of tests/golden/missing_*.npz -------------------------------------------------
BSC_KEYS = ("W", "pi", "sigma")
SSSC_KEYS = ("W", "pies", "mus", "Psi", "sigma2")


@lru_cache(maxsize=None)
def fixture_steps(algo):
    """[(t, theta, ss, lpj, y_reconstructed)] of missing_<algo>.npz for every step that wrote a reconstruction (EBSC's
    last step ran without do_reconstruction: its array is the one of the step before), with g = the fixture.  Theta =
    the parameters the step's E-step ran with: t0_in_* for t = 0, t{t-1}_out_* after."""
    g = load_golden("missing_%s.npz" % algo)
    keys = BSC_KEYS if algo == "ebsc" else SSSC_KEYS
    H = int(g["H"])
    steps = []
    for t in range(int(g["n_steps"])):
        if not bool(g.get("t%d_do_rec" % t, True)):
            continue
        src = "t0_in_%s" if t == 0 else "t%d_out_%%s" % (t - 1)
        theta = {k: (np.float64(g[src % k]) if g[src % k].ndim == 0 else np.array(g[src % k])) for k in keys}
        steps.append((t, theta, unpack_bits(g["t%d_ss_out" % t], H), g["t%d_lpj_out" % t], g["t%d_y_reconstructed" % t]))
    return g, steps


# ---- precision-weighted merge ---------------------------------------------------------------------------------------------
def merge_reference(Y, V, H, W, C, ph, pw, shift):
    """(sum e / v) / (sum 1 / v) per image element by an explicit loop over pixels, channels and covering patches in
    increasing n; estimates that are NaN or whose variance is NaN or <= 0 are skipped; none valid: NaN."""
    tops, lefts = patch_tops(H, ph, shift), patch_tops(W, pw, shift)
    nc = len(lefts)
    out = np.full((H, W, C), np.nan)
    for y in range(H):
        for x in range(W):
            for c in range(C):
                num = den = 0.0
                cnt = 0
                for ir, t in enumerate(tops):
                    for ic, l in enumerate(lefts):
                        if t <= y < t + ph and l <= x < l + pw:
                            d = ((y - t) * pw + (x - l)) * C + c
                            e, v = Y[ir * nc + ic, d], V[ir * nc + ic, d]
                            if e == e and v > 0.0:
                                w = 1.0 / v
                                num = num + e * w
                                den = den + w
                                cnt += 1
                if cnt:
                    with np.errstate(all="ignore"):
                        out[y, x, c] = np.float64(num) / np.float64(den)
    return out


# (H, W, C, ph, pw, shift)
MERGE_CASES = {"s1_c1": (7, 9, 1, 3, 4, 1), "s2_c1": (7, 9, 1, 3, 4, 2), "s1_c3": (7, 9, 3, 3, 4, 1), "s2_c3": (7, 9, 3, 3, 4, 2)}


@lru_cache(maxsize=None)
def merge_case(name):
    """(geometry, Y, V, reference): estimates with NaN entries, variances with NaN, 0, negative and inf entries, and
    pixel (0, 0) -- covered by patch 0 alone -- without a valid estimate."""
    from evo_amd.utils.prepost import patch_geometry
    H, W, C, ph, pw, shift = geom = MERGE_CASES[name]
    N, D = patch_geometry(H, W, C, ph, pw, shift)
    rng = np.random.RandomState(len(name) + 11 * shift + C)
    Y = rng.normal(size=(N, D)) * 3.0
    V = rng.uniform(0.2, 4.0, size=(N, D))
    Y[rng.random_sample((N, D)) < 0.1] = np.nan
    bad = rng.random_sample((N, D))
    V[bad < 0.05] = np.nan
    V[(bad >= 0.05) & (bad < 0.10)] = 0.0
    V[(bad >= 0.10) & (bad < 0.15)] = -1.5
    V[(bad >= 0.15) & (bad < 0.20)] = np.inf
    V[0, :C] = 0.0  # pixel (0, 0), every channel: its only estimate is invalid
    ref = merge_reference(Y, V, *geom)
    assert np.isnan(ref[0, 0]).all()
    for a in (Y, V, ref):
        a.setflags(write=False)
    return geom, Y, V, ref

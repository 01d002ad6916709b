"""Synthetic statistics-pass problems for test_gpu_stats_paths.py (and their CPU checks in test_stats_problems.py).

A problem is a K^n whose rows are S distinct states drawn from a pool of a few hundred, with the number of active latents
per state drawn from a named profile, plus a well-conditioned Theta (Psi = I + A A^T of low rank).  The pair-bin geometry
of evo_amd.hip (alloc_pair_bins) is restated here so that a test can prove that a bin region overflows instead of hoping
that it does."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evo_amd", "csrc")

# pair_bins.hpp
PB_TILE = 4096
PB_MAX_BINS = 256
# kernels_bsc.hpp: EBSC states with at most this many active latents go through the pair bins
BSC_KR = 4
# evoamd_ctx defaults of the options the cases change
PAIR_BINS_SCALE = 3
PAIR_BINS_NWG = 2048

# latent-count profiles: (weight, lowest, highest) bands; a band beyond H is clipped (or dropped)
PROFILES = {
    "sparse": [(0.05, 0, 0), (0.45, 1, 1), (0.40, 2, 2), (0.10, 3, 4)],
    "mid": [(0.03, 0, 0), (0.17, 1, 1), (0.30, 2, 2), (0.27, 3, 4), (0.18, 5, 8), (0.05, 9, 12)],
    "dense": [(0.02, 0, 0), (0.03, 1, 2), (0.95, 5, 8)],
    # only <= 4 latents in the pool; few4_extra states of 5..8 latents are planted in single datapoints
    "few4": [(0.05, 0, 0), (0.35, 1, 1), (0.35, 2, 2), (0.25, 3, 4)],
    "wide": [(0.02, 0, 0), (0.18, 1, 2), (0.20, 3, 8), (0.25, 9, 16), (0.20, 17, 64), (0.15, 65, 1 << 30)],
    # EBSC: every state a source of 3 or 6 bin entries
    "k34": [(0.02, 0, 0), (0.49, 3, 3), (0.49, 4, 4)],
}
FEW4_EXTRA = 40  # states above four latents in a whole "few4" K^n (the merged 5..8 route wants fewer than ~100)


def _bands(profile, H):
    out = []
    for w, lo, hi in PROFILES[profile]:
        if lo > H:
            continue
        out.append((w, lo, min(hi, H)))
    ws = np.array([b[0] for b in out])
    return out, ws / ws.sum()


def _random_state(rng, H, bands, probs):
    w, lo, hi = bands[rng.choice(len(bands), p=probs)]
    k = int(rng.randint(lo, hi + 1))
    st = np.zeros(H, dtype=bool)
    st[rng.choice(H, k, replace=False)] = True
    return st


def make_pool(rng, H, profile, size):
    """`size` distinct states (every state of H latents when there are fewer); the all-zero state is always there."""
    if H <= 10 and 2 ** H <= size:
        return ((np.arange(2 ** H)[:, None] >> np.arange(H)[None, ::-1]) & 1).astype(bool)
    bands, probs = _bands(profile, H)
    seen = {np.zeros(H, dtype=bool).tobytes()}
    pool = [np.zeros(H, dtype=bool)]
    tries = 0
    while len(pool) < size and tries < 50 * size:
        tries += 1
        st = _random_state(rng, H, bands, probs)
        key = st.tobytes()
        if key not in seen:
            seen.add(key)
            pool.append(st)
    return np.array(pool)


def make_states(rng, N, S, H, profile, pool_size=512):
    pool = make_pool(rng, H, profile, max(pool_size, S))
    assert pool.shape[0] >= S, (pool.shape, S)
    ss = np.empty((N, S, H), dtype=bool)
    for n in range(N):
        ss[n] = pool[rng.choice(pool.shape[0], S, replace=False)]
    if profile == "few4":  # a few datapoints get one state of 5..8 latents (distinct: the pool has none above four)
        assert H >= 8
        for n in rng.choice(N, min(N, FEW4_EXTRA), replace=False):
            st = np.zeros(H, dtype=bool)
            st[rng.choice(H, rng.randint(5, 9), replace=False)] = True
            ss[n, rng.randint(S)] = st
    if ss[0].any(axis=1).all():  # at least one all-zero state (rows stay distinct: datapoint 0 had none)
        ss[0, S - 1] = False
    return ss


# Problems: name -> (algo, profile, N, D, H, S, S_perm, seed).  Spread over H in {2, 3, 63, 64, 65, 129, 512, 1024},
# S in {1, 37, 64, 65, 200, 256, 300}, odd N, even and odd D.
PROBLEMS = {
    "es_mid": ("es3c", "mid", 255, 33, 64, 64, 0, 1),
    "es_dense": ("es3c", "dense", 257, 32, 64, 64, 0, 2),      # even H and D: the flat kernel runs
    "es_chains_big": ("es3c", "mid", 2049, 33, 64, 64, 0, 3),  # N S >= 131072: the K = 4 chains grid exceeds 256
    "es_few4": ("es3c", "few4", 301, 33, 63, 65, 0, 4),
    "es_wide": ("es3c", "wide", 129, 32, 129, 37, 0, 5),
    "es_h2": ("es3c", "sparse", 513, 33, 2, 1, 0, 6),
    "es_h3": ("es3c", "sparse", 129, 32, 3, 7, 0, 7),
    "es_s200": ("es3c", "sparse", 65, 33, 65, 200, 0, 8),
    "es_h512": ("es3c", "sparse", 31, 32, 512, 37, 0, 9),
    "es_h1024": ("es3c", "sparse", 41, 33, 1024, 37, 0, 10),
    "bsc_sparse": ("ebsc", "sparse", 257, 33, 64, 64, 0, 11),
    "bsc_k34": ("ebsc", "k34", 257, 33, 64, 64, 0, 12),         # N S >= 16384 nb: the regions overflow
    "bsc_wide": ("ebsc", "wide", 63, 32, 129, 37, 0, 13),
    "bsc_perm": ("ebsc", "sparse", 127, 33, 65, 256, 1, 14),   # S_perm = 1, S = 256: the wave kernel's largest S
    "bsc_s300": ("ebsc", "mid", 33, 32, 63, 300, 0, 15),       # S > 256: the one-shot kernel
}


def make_problem(name):
    algo, profile, N, D, H, S, S_perm, seed = PROBLEMS[name]
    rng = np.random.RandomState(seed)
    Y = rng.normal(size=(N, D))
    if algo == "es3c":
        W = rng.normal(size=(D, H)) * 0.4
        A = rng.normal(size=(H, 3)) * 0.2
        theta = {"W": W, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H), "Psi": np.eye(H) + A @ A.T,
                 "sigma2": np.float64(1.3)}
    else:
        theta = {"W": rng.normal(size=(D, H)) * 0.5, "pi": np.float64(0.15), "sigma": np.float64(2.0)}
    ss = make_states(rng, N, S, H, profile)
    return {"name": name, "algo": algo, "profile": profile, "N": N, "D": D, "H": H, "S": S, "S_perm": S_perm,
            "Y": Y, "theta": theta, "ss": ss}


def level_census(ss):
    """Active latents per state (N, S)."""
    return ss.sum(axis=-1)


def bin_entries(ss, algo, live=None):
    """Entries the statistics pass appends to the pair bins for this K^n.  ES3C (census route): one per state of two
    latents, k (k - 1) / 2 per state of 3..8 (above eight: the wavefront kernel's atomics).  EBSC: k (k - 1) / 2 per state
    of 2..BSC_KR latents.  `live` (N, S): only those states (q > 0) append."""
    k = level_census(ss).astype(np.int64)
    top = 8 if algo == "es3c" else BSC_KR
    e = np.where((k >= 2) & (k <= top), k * (k - 1) // 2, 0)
    if live is not None:
        e = e * live
    return int(e.sum())


def pair_bins_geometry(N, H, S, scale=PAIR_BINS_SCALE, nwg=PAIR_BINS_NWG):
    """alloc_pair_bins (evo_amd.hip): rf folded rows per bin, nb bins, nwg regions per bin of cap entries each."""
    rf = max(1, PB_TILE // (2 * H))
    nfold = H // 2
    nb = -(-nfold // rf)
    cap = max(64, scale * -(-(N * S) // (nb * nwg)))
    return {"rf": rf, "nb": nb, "nwg": nwg, "cap": cap, "capacity": nb * nwg * cap}


def recut_scale(ss):
    """ensure_bins_capacity: the scale the bins are re-cut to from the census of the last pass (res_cnt = states above
    2 / 4 / 8 latents)."""
    k = level_census(ss)
    NS = k.size
    gt2, gt4, gt8 = int((k > 2).sum()), int((k > 4).sum()), int((k > 8).sum())
    entries = (NS - gt2) + 6.0 * (gt2 - gt4) + 28.0 * (gt4 - gt8)
    return min(64, int(math.ceil(3.0 * 1.25 * entries / NS)))


# Option cases: (id, problem, options, flow, overflow).  Options read by evoamd_configure are set before it; every
# option is restored afterwards.  flow: "once" = lpj_resident + stats; "twice" = a second lpj_resident + stats (the
# census of the first pass is known: re-cut bins).  The K^n of these cases comes from the host, so the statistics pass
# sizes its levels for an unknown K^n (tag 2: no merged levels); DEVICE_CASES cover a K^n the device evolved.
# overflow = True: the case must prove that
# at least one bin region overflows (pigeonhole over the bin capacity).
OVF = {"pair_bins": 2, "pair_bins_scale": 1, "pair_bins_auto": 0, "pair_bins_nwg": 256}
CASES = [
    ("es_defaults", "es_mid", {}, "once", False),
    ("es_bins0", "es_mid", {"pair_bins": 0}, "once", False),
    ("es_bins2", "es_mid", {"pair_bins": 2}, "twice", False),
    ("es_stage0", "es_mid", {"pair_bins": 2, "stats_stage": 0}, "once", False),
    ("es_waves8_chains", "es_mid", {"pair_bins": 2, "census_lists": 0, "stats_waves": 8}, "once", False),
    ("es_waves16_chains", "es_mid", {"pair_bins": 2, "census_lists": 0, "stats_waves": 16}, "once", False),
    # census requires four waves: stats_waves = 8 with the census lists on takes the chains instead (no error)
    ("es_waves8_census", "es_mid", {"pair_bins": 2, "stats_waves": 8}, "once", False),
    ("es_chains_k8auto", "es_mid", {"pair_bins": 2, "census_lists": 0, "sssc_k8": -1}, "twice", False),
    ("es_chains_k8off", "es_mid", {"pair_bins": 2, "census_lists": 0, "sssc_k8": 0}, "once", False),
    ("es_chains_k8on", "es_mid", {"pair_bins": 2, "census_lists": 0, "sssc_k8": 1}, "once", False),
    ("es_nodigest_bins", "es_mid", {"pair_bins": 2, "state_digest": 0}, "once", False),
    ("es_dense_bins2", "es_dense", {"pair_bins": 2}, "once", False),
    ("es_dense_overflow", "es_dense", dict(OVF), "twice", True),
    # the first pass overflows; ensure_bins_capacity re-cuts the bins from its census before the second
    ("es_dense_recut", "es_dense", dict(OVF, pair_bins_auto=1), "twice", True),
    ("es_dense_flat", "es_dense", {"pair_bins": 2, "stats_flat": 1}, "once", False),
    ("es_dense_flat_overflow", "es_dense", dict(OVF, stats_flat=1), "once", True),
    ("es_dense_chains_k8_overflow", "es_dense", dict(OVF, census_lists=0, sssc_k8=1), "once", True),
    ("es_chains_nwg256_k8auto", "es_chains_big", {"pair_bins": 2, "census_lists": 0, "pair_bins_nwg": 256}, "once", False),
    ("es_chains_nwg256_k8on", "es_chains_big",
     {"pair_bins": 2, "census_lists": 0, "pair_bins_nwg": 256, "sssc_k8": 1}, "once", False),
    ("es_chains_nwg256_k8off", "es_chains_big",
     {"pair_bins": 2, "census_lists": 0, "pair_bins_nwg": 256, "sssc_k8": 0}, "once", False),
    ("es_nodigest_nwg256", "es_chains_big", {"pair_bins": 2, "state_digest": 0, "pair_bins_nwg": 256}, "once", False),
    ("es_few4_bins2", "es_few4", {"pair_bins": 2}, "twice", False),
    ("es_wide_bins2", "es_wide", {"pair_bins": 2}, "twice", False),
    ("es_wide_chains", "es_wide", {"pair_bins": 2, "census_lists": 0}, "once", False),
    ("es_h2", "es_h2", {"pair_bins": 2}, "once", False),
    ("es_h3", "es_h3", {"pair_bins": 2}, "once", False),
    ("es_s200", "es_s200", {"pair_bins": 2}, "once", False),
    ("es_h512", "es_h512", {"pair_bins": 2}, "once", False),
    ("es_h1024", "es_h1024", {"pair_bins": 2}, "once", False),
    ("bsc_wave1_bins0", "bsc_sparse", {"bsc_stats_wave": 1, "pair_bins": 0}, "once", False),
    ("bsc_wave1_bins2", "bsc_sparse", {"bsc_stats_wave": 1, "pair_bins": 2}, "once", False),
    ("bsc_wave0_bins0", "bsc_sparse", {"bsc_stats_wave": 0, "pair_bins": 0}, "once", False),
    ("bsc_wave0_bins2", "bsc_sparse", {"bsc_stats_wave": 0, "pair_bins": 2}, "once", False),
    ("bsc_nodigest", "bsc_sparse", {"pair_bins": 2, "state_digest": 0}, "once", False),
    ("bsc_overflow", "bsc_k34", {"pair_bins": 2, "pair_bins_scale": 1, "pair_bins_nwg": 256}, "twice", True),
    ("bsc_wide", "bsc_wide", {"pair_bins": 2}, "once", False),
    ("bsc_perm", "bsc_perm", {"pair_bins": 2}, "once", False),
    ("bsc_s300", "bsc_s300", {"pair_bins": 2}, "once", False),
]
# A K^n evolved on the device (lpj_resident + stats, then evolve_randflip + vary_kn, then the pass under test): the
# statistics pass knows the census of the previous pass and that the candidates came from the device (tag 1), which is
# what the merged 5..8 level (few_above4) and the merged wavefront levels of the chains (few_dense_states) need.
# (id, problem, options, 5..8 quad launches expected in the pass under test: True / False / None = not checked)
CMAX = 4  # candidates per datapoint the engine is configured for
EVOLVE = (2, 2, 20261016)  # parents, children per parent (parents x children <= Cmax), seed
DEVICE_CASES = [
    ("es_few4_device_merge1", "es_few4", {"pair_bins": 2, "merge_small_levels": 1}, False),
    ("es_few4_device_merge0", "es_few4", {"pair_bins": 2, "merge_small_levels": 0}, True),
    ("es_few4_device_chains", "es_few4", {"pair_bins": 2, "census_lists": 0}, None),
]


def few_above4(ss, S, Cmax):
    """few_above4 (evo_amd.hip) from the census of a pass over `ss`: the merged 5..8 route of the next pass."""
    return int((level_census(ss) > 4).sum()) * (1.0 + 4.0 * Cmax / S) <= 256.0


def few_dense_states(ss, S, Cmax):
    """few_dense_states (evo_amd.hip, tag 1): the chains serve both wavefront levels with one launch."""
    k = level_census(ss)
    return int((k > 4).sum()) + int((k > 2).sum()) * Cmax / S <= 1024.0


# read by evoamd_configure (set before it)
CONFIGURE_OPTIONS = ("pair_bins_scale", "pair_bins_nwg", "census_lists", "state_digest")
# what the engine starts with (restored after every case)
DEFAULTS = {"pair_bins": 1, "pair_bins_scale": PAIR_BINS_SCALE, "pair_bins_nwg": PAIR_BINS_NWG, "pair_bins_auto": 1,
            "census_lists": 1, "state_digest": 1, "sssc_k8": -1, "stats_stage": 1, "stats_waves": 0, "stats_flat": 0,
            "merge_small_levels": 1, "bsc_stats_wave": 1}

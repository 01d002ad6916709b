"""Incomplete-data problems for test_gpu_masked_parity.py (and their CPU checks in test_masked_problems.py).

A problem is (algo, profile, N, D, H, S, S_perm, mask pattern, seed): a K^n of _stats_problems.make_states, the
well-conditioned Theta of _stats_problems.make_problem, data, the reliable mask x_infr and the keep-mask x.  Every shape
is the smallest at which the masked code named in its comment can still go wrong.  oracle() is the float64 reference
(oracle/evo_oracle.py); lpj_direct() restates the masked ES3C lpj of one (datapoint, state) from the model's marginal
Gaussian, so that the suite does not rest on one restatement; the functions at the end are oracles that are wrong in
the way a kernel would be (test_masked_problems.py proves that each is rejected by a wide margin)."""
import functools

import numpy as np

import _stats_problems as sp

# tolerances of the GPU checks: the project's own (test_gpu_stats_paths.py, test_device_mstep_matches_host)
LPJ_RTOL = SUM_RTOL = 1e-9   # against the oracle, atol = rtol * max(1, |ref|max)
BASE_RTOL = 1e-12            # between device runs that differ only in summation order
THETA_RTOL, THETA_ATOL = 1e-7, 1e-9  # Theta update: atol = THETA_ATOL * max(1, |ref|max)
COND_CAP = 1e6               # of the H x H systems the Theta update solves

# name -> (algo, profile, N, D, H, S, S_perm, mask pattern, seed)
PROBLEMS = {
    # the golden fixtures' regime (one lane-loop trip over D, no state above 8 latents) plus the degenerate rows: a
    # complete row, a row with one reliable entry, two rows without any, a column that is reliable nowhere else
    "es_d25": ("es3c", "mid", 37, 25, 12, 10, 0, "edge", 101),
    # big_solve's `for (d = lane; d < D; d += 64) if (mrow[d])`: exactly one trip with every lane busy ...
    "es_d64": ("es3c", "mid", 33, 64, 12, 10, 0, "rand30", 102),
    # ... one trip plus a tail trip of one lane ...
    "es_d65": ("es3c", "mid", 33, 65, 12, 10, 0, "rand30", 103),
    # ... three trips with a ragged tail (130 = 2 * 64 + 2); `block`: one row misses the whole aligned slab 64..127, so
    # the second trip adds nothing for it
    "es_d130": ("es3c", "mid", 33, 130, 12, 10, 0, "block", 104),
    # H % GEMM_BM == 0: stats_sssc_masked_products takes the mirrored form (sym_row0 = H) of [Es|Ez]^T Ez;
    # N > 256: colsum_partial_kernel runs over p.nblk = 2 row blocks
    "es_h64": ("es3c", "mid", 300, 33, 64, 20, 0, "rand30", 105),
    # two 64-bit state words; states of 9..65 latents leave the first sssc_big_kernel launch through list 3 and are served
    # by the second at SSSC_KCAP, the one state class above 64 latents from the global-memory slots
    "es_h65_wide": ("es3c", "wide", 41, 32, 65, 24, 0, "rand30", 106),
    # x != x_infr: select_rec_kernel keeps by x, and Yrec^T Ez reads what it wrote
    "es_keep": ("es3c", "mid", 37, 33, 12, 10, 0, "keep", 107),
    # N S = 65920 > 65536, the grid cap of lpj_sssc_masked / stats_sssc_masked_block: sssc_big_kernel's grid-stride loop
    # takes a second trip for 384 states
    "es_grid": ("es3c", "sparse", 1030, 16, 8, 64, 0, "rand30", 108),
    # bsc_lpj_kernel<R>: D <= 64 -> R = 1, one slab of 64 observables, 39 idle lanes; the degenerate rows
    "bsc_d25": ("ebsc", "mid", 37, 25, 12, 10, 0, "edge", 109),
    # 64 < D <= 128 -> R = 2 (the launch site in launch_lpj_bsc): one slab, the second register holds one live lane
    "bsc_d65": ("ebsc", "mid", 37, 65, 12, 10, 0, "rand30", 110),
    # D > 128 -> R = 4, slabs of 256: D = 257 is one above 64 R, a full slab and a second of one lane (D = 129 would still
    # be one slab at the R it selects); `block`: one row misses the aligned columns 64..127, one the last three
    "bsc_dR": ("ebsc", "mid", 37, 257, 12, 10, 0, "block", 111),
    # S_perm = 1: the permanent all-zero state adds q0 * sum(y[obs]^2) to sigma; H = 65: two state words
    "bsc_perm": ("ebsc", "sparse", 65, 33, 65, 64, 1, "rand30", 112),
    # S > 256: the one-shot statistics kernel (no wave kernel) with a mask
    "bsc_s300": ("ebsc", "mid", 33, 32, 20, 300, 0, "rand30", 113),
    # x != x_infr on the EBSC side (select_rec_kernel, Wp = Es^T Yrec)
    "bsc_keep": ("ebsc", "mid", 37, 33, 12, 10, 0, "keep", 114),
    # the lower edge of the latent space (the "sparse" pool holds all 2^H = 4 states, S = 3 of them per datapoint): an
    # H x H grid of four threads, one pair of latents, 2 x 2 systems; D = 8 H: a lazy update writes its backup in
    # sssc_mstep_prepare_kernel, whose four live threads are fewer than the 16 scalars of the block it saves
    "es_h2": ("es3c", "sparse", 37, 16, 2, 3, 0, "rand30", 115),
    "bsc_h2": ("ebsc", "sparse", 37, 9, 2, 3, 0, "rand30", 116),
}
ES_PROBLEMS = tuple(k for k, v in PROBLEMS.items() if v[0] == "es3c")
BSC_PROBLEMS = tuple(k for k, v in PROBLEMS.items() if v[0] == "ebsc")
# the Theta part runs on these: every H x H system of their update is under COND_CAP at the N above, so none had to
# be raised (test_masked_problems.py asserts it).  cond(xpt_szsz), cond(xpt_ss + eps I): es_d65 8.1, 9.1; es_h64 15.9,
# 25.6.  cond(Wq): bsc_d65 8.5; bsc_perm 5.3.  The tiny problems: es_h2 1.6, 3.0; cond(Wq) of bsc_h2 1.1.
THETA_PROBLEMS = ("es_d65", "es_h64", "bsc_d65", "bsc_perm", "es_h2", "bsc_h2")
TINY = ("es_h2", "bsc_h2")
GRID_STRIDE = 7  # es_grid: the oracle's lpj on every 7th datapoint only (the whole oracle would take a minute)

# rows of the `edge` pattern
EDGE_COMPLETE, EDGE_SINGLE, EDGE_EMPTY, EDGE_COLUMN = 0, 1, (2, 5), 3

ES_NAMES = ("xpt_s", "xpt_ss", "xpt_sz", "xpt_szsz", "Wp", "s_sz_outer", "sz_sz_outer", "y_outer_diag", "pad", "Fs")
BSC_NAMES = ("Wp", "Wq", "pies", "sigma", "Fs")


def make_mask(rng, N, D, pattern):
    """(x_infr, x) of a pattern, deterministic from the generator's state."""
    def rand(frac):
        return rng.random_sample((N, D)) >= frac

    if pattern == "block":
        x_infr = np.ones((N, D), dtype=bool)
        for n in range(N):
            length = int(rng.randint(1, max(2, D // 2)))
            start = int(rng.randint(0, D - length + 1))
            x_infr[n, start:start + length] = False
        if D >= 128:  # one row misses a whole aligned 64-column slab
            x_infr[1] = True
            x_infr[1, 64:128] = False
        x_infr[2] = True  # one row's run ends at the last column (the ragged tail of a loop over D must see a hole)
        x_infr[2, D - 3:] = False
        return x_infr, x_infr.copy()
    x_infr = rand(0.3)
    if pattern in ("rand30", "keep"):
        x_infr[~x_infr.any(axis=1), 0] = True  # (no row without a reliable entry outside `edge`)
    if pattern == "keep":
        return x_infr, x_infr & rand(0.2)
    if pattern == "edge":
        x_infr[:, EDGE_COLUMN] = False
        x_infr[EDGE_COMPLETE] = True  # (the one cell where "complete row" and "column never reliable" meet: the row wins)
        x_infr[EDGE_SINGLE] = False
        x_infr[EDGE_SINGLE, D - 1] = True
        for n in EDGE_EMPTY:
            x_infr[n] = False
    return x_infr, x_infr.copy()


def hide(Y, x_infr, how):
    """Y with the entries outside x_infr set to `how` (0.0, nan, 1e300 ...)."""
    return np.where(x_infr, Y, how)


@functools.lru_cache(maxsize=None)
def make_problem(name):
    algo, profile, N, D, H, S, S_perm, pattern, seed = PROBLEMS[name]
    rng = np.random.RandomState(seed)
    Y = rng.normal(size=(N, D))
    if algo == "es3c":  # the Theta of _stats_problems.make_problem
        W = rng.normal(size=(D, H)) * 0.4
        A = rng.normal(size=(H, 3)) * 0.2
        theta = {"W": W, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H), "Psi": np.eye(H) + A @ A.T,
                 "sigma2": np.float64(1.3)}
    else:
        theta = {"W": rng.normal(size=(D, H)) * 0.5, "pi": np.float64(0.15), "sigma": np.float64(2.0)}
    ss = sp.make_states(rng, N, S, H, profile)
    x_infr, x = make_mask(rng, N, D, pattern)
    return {"name": name, "algo": algo, "profile": profile, "N": N, "D": D, "H": H, "S": S, "S_perm": S_perm,
            "pattern": pattern, "Y": Y, "Y0": hide(Y, x_infr, 0.0), "x_infr": x_infr, "x": x, "theta": theta, "ss": ss}


def rows_of(p, rows):
    """The problem restricted to the datapoints `rows` (a slice or an index array)."""
    q = dict(p)
    for k in ("Y", "Y0", "x_infr", "x", "ss"):
        q[k] = np.ascontiguousarray(p[k][rows])
    q["N"] = q["Y"].shape[0]
    return q


# ---- the float64 reference ------------------------------------------------------------------------------------------
def oracle_lpj(p, x_infr=None, Y=None):
    """lpj over K^n (N, S_perm + S) from the oracle, on the reliable entries `x_infr` (default: the problem's) of `Y`
    (default: the problem's data with zeros in the hidden entries, as the device holds them)."""
    from oracle import evo_oracle as orc
    N, D, H, S, S_perm, ss = p["N"], p["D"], p["H"], p["S"], p["S_perm"], p["ss"]
    Y = p["Y0"] if Y is None else Y
    xi = p["x_infr"] if x_infr is None else x_infr
    th = dict(p["theta"])
    lpj = np.empty((N, S_perm + S))
    if p["algo"] == "es3c":
        cnt = orc.sssc_precompute(th, D, xi)
        for n in range(N):
            lpj[n] = orc.sssc_lpj(th, ss[n], Y[n], cnt, {}, xi[n])
    else:
        cnt = orc.bsc_precompute(th, D, H, xi)
        for n in range(N):
            if S_perm:
                lpj[n, 0] = orc.bsc_lpj_allzero(th, Y[n], cnt, xi[n])[0]
            lpj[n, S_perm:] = orc.bsc_lpj(th, ss[n], Y[n], cnt, xi[n])
    return lpj


def oracle(p, x_infr=None, x=None, y_rec_old=None, Y=None, precision=np.float64):
    """{"lpj", "sums", "y_reconstructed", "theta_pre", "ljc"} of the oracle: lpj over K^n, the M-step sums under their
    names in the packed accumulator (ES3C: "pad" = trace_WW) and this step's y_reconstructed.  `x_infr` / `x` replace
    the problem's masks (the complete-data comparison, the wrong-mask variants); `y_rec_old` (EBSC): the M-step reads
    that older reconstruction instead of this step's; `Y` as in oracle_lpj; `precision` (ES3C): the model's
    dtype_precision."""
    from oracle import evo_oracle as orc
    N, D, H, S, S_perm, ss = p["N"], p["D"], p["H"], p["S"], p["S_perm"], p["ss"]
    Y = p["Y0"] if Y is None else Y
    xi = p["x_infr"] if x_infr is None else x_infr
    xk = p["x"] if x is None else x
    th = dict(p["theta"])
    if p["algo"] == "es3c":
        suff = {"ss": ss, "lpj": np.empty((N, S)), "S_perm": 0, "incl": np.zeros((0, H), dtype=bool), "Mprime": S}
        acc = orc.sssc_EM_accumulate(th, suff, Y, use_storage=False, evolve=False, reconstruct_x=xk, x_infr=xi,
                                     precision=precision)
        lpj = suff["lpj"]
        sums = {k: acc[k] for k in ES_NAMES if k in acc}
        if "trace_WW" in acc:
            sums["pad"] = acc["trace_WW"]
        y_rec = acc["y_reconstructed"]
    else:
        lpj = oracle_lpj(p, xi, Y)
        orc.bsc_precompute(th, D, H, xi)
        suff = {"ss": ss, "lpj": lpj, "S_perm": S_perm, "permanent": {"allzero": bool(S_perm), "background": False}}
        y_rec = orc.bsc_reconstruct(th, suff, Y, xk, xi)
        sums = dict(orc.bsc_accumulate(th, suff, Y, xi, y_rec if y_rec_old is None else y_rec_old))
        sums["Fs"] = orc.free_energy_sum(lpj)
    return {"lpj": lpj, "sums": sums, "y_reconstructed": y_rec, "ljc": float(th["ljc"]), "n_reliable": int(xi.sum())}


def oracle_update(p, sums, to_learn=None, n_reliable=None):
    """Theta^new of the oracle's update (sssc_update / bsc_update) from `sums`, which may be the oracle's or the views of
    the device's accumulator.  n_reliable: the count that multiplies the OLD sigma2 / sigma^2 (default: x_infr.sum())."""
    from oracle import evo_oracle as orc
    N, D, H = p["N"], p["D"], p["H"]
    nr = int(p["x_infr"].sum()) if n_reliable is None else n_reliable
    th = {k: np.array(v) for k, v in p["theta"].items()}
    if p["algo"] == "es3c":
        acc = {k: np.array(sums[k], dtype=np.float64) for k in ES_NAMES if k not in ("pad", "Fs")}
        acc["y_inner"] = float(np.sum(sums["y_outer_diag"]))  # sssc.py:748: the reliable entries' squares
        acc["trace_WW"] = float(sums["pad"])
        acc["n_reliable"] = nr
        th["sigma2"] = np.float64(th["sigma2"])
        return orc.sssc_update(th, acc, N, D, H, to_learn or ("W", "pies", "mus", "sigma2", "Psi"))
    th["pi"], th["sigma"] = np.float64(th["pi"]), np.float64(th["sigma"])
    acc = {k: np.array(sums[k], dtype=np.float64) for k in ("Wp", "Wq", "pies", "sigma")}
    th = orc.bsc_update(th, acc, N, D, H, to_learn or ("W", "pi", "sigma"), n_reliable=nr)
    th.pop("pies", None)
    return th


def new_scalars(p, theta_new):
    """ljc and pre1 / sigma2_inv that the next E-step derives from Theta^new (what the device's scalar block holds after
    the update)."""
    from oracle import evo_oracle as orc
    th = dict(theta_new)
    if p["algo"] == "es3c":
        orc.sssc_precompute(th, p["D"], p["x_infr"])
        return {"ljc": float(th["ljc"]), "sigma2": float(th["sigma2"]), "sigma2_inv": float(th["sigma2_inv"])}
    orc.bsc_precompute(th, p["D"], p["H"], p["x_infr"])
    return {"ljc": float(th["ljc"]), "sigma": float(th["sigma"]), "pre1": float(th["pre1"]), "pi": float(th["pi"]),
            "pil_bar": float(th["pil_bar"])}


def update_conditions(p, sums):
    """Condition numbers of the H x H systems the Theta update of `sums` solves."""
    H = p["H"]
    if p["algo"] == "es3c":
        return {"xpt_szsz": np.linalg.cond(sums["xpt_szsz"]), "xpt_ss": np.linalg.cond(sums["xpt_ss"] + 1e-5 * np.eye(H))}
    return {"Wq": np.linalg.cond(sums["Wq"])}


# ---- a second, independent reference of the masked ES3C lpj --------------------------------------------------------
def lpj_direct(theta, y, obs, state):
    """lpj of one (datapoint, state) from the model's formula: given s, y_obs is Gaussian with mean W_A mu_A and covariance
    sigma2 I + W_A Psi_A W_A^T (rows obs, columns A = state).  The sigma2^-|obs| part of the determinant is Theta's
    alone and lives in ljc, as in the reference."""
    W = theta["W"][obs][:, state]
    s2 = float(theta["sigma2"])
    C = s2 * np.eye(int(obs.sum())) + W @ theta["Psi"][state][:, state] @ W.T
    r = y[obs] - W @ theta["mus"][state]
    prior = np.log(theta["pies"] / (1.0 - theta["pies"]))[state].sum()
    logdet = np.linalg.slogdet(C)[1] - obs.sum() * np.log(s2)
    return prior - 0.5 * (logdet + r @ np.linalg.inv(C) @ r)


# ---- oracles that are wrong in the way a kernel would be -------------------------------------------------------------
def mask_ignored_from(x_infr, d0=64):
    """The reliable mask of a kernel whose loop over D forgets the mask from column d0 on (it reads the zeros that
    mask_apply_kernel left there as data)."""
    m = x_infr.copy()
    m[:, d0:] = True
    return m


def lpj_gram(theta, y0, obs, state, complete_gram=False):
    """The masked ES3C lpj in the Gram form of big_solve: b = W_obs^T y_obs, G_A = W_obs^T W_obs restricted to A.
    complete_gram: G_A = (W^T W)_A, what the kernel would use if it kept the complete-data table."""
    Wo = theta["W"][obs][:, state]
    Wg = theta["W"][:, state] if complete_gram else Wo
    s2 = float(theta["sigma2"])
    mu, Psi = theta["mus"][state], theta["Psi"][state][:, state]
    G = Wg.T @ Wg
    b = Wo.T @ y0[obs]
    v = b - G @ mu
    rr = (y0[obs] ** 2).sum() - mu @ (b + v)
    M = G / s2 + np.linalg.inv(Psi)
    prior = np.log(theta["pies"] / (1.0 - theta["pies"]))[state].sum()
    return prior - 0.5 * (np.linalg.slogdet(M)[1] + np.linalg.slogdet(Psi)[1] + rr / s2 - v @ np.linalg.inv(M) @ v / s2 ** 2)


def lpj_complete_gram_above(p, kmin=9):
    """Oracle lpj of an ES3C problem with the complete-data Gram in every state of at least `kmin` latents."""
    lpj = oracle_lpj(p)
    k = p["ss"].sum(axis=-1)
    for n, s in zip(*np.nonzero(k >= kmin)):
        lpj[n, s] = lpj_gram(p["theta"], p["Y0"][n], p["x_infr"][n], p["ss"][n, s], complete_gram=True)
    return lpj


def sigma_without_allzero(p, o):
    """EBSC sigma sum of `o` = oracle(p) without the permanent all-zero state's term q0 * sum(y[obs]^2)."""
    from oracle import evo_oracle as orc
    lpj = o["lpj"]
    q = np.exp(lpj + np.minimum(orc.B_MAX - lpj.max(axis=1), orc.B_MAX_SHFT)[:, None])
    return o["sums"]["sigma"] - float((q[:, 0] / q.sum(axis=1) * (p["Y0"] ** 2).sum(axis=1)).sum())


def prior_only_lpj(p, n):
    """lpj of a datapoint without a reliable entry: the prior's term alone (ES3C: the determinant terms cancel, M_A =
    inv(Psi_A); EBSC: the residual is empty)."""
    th = p["theta"]
    if p["algo"] == "es3c":
        pil = np.log(th["pies"] / (1.0 - th["pies"]))
        return (p["ss"][n] * pil[None, :]).sum(axis=1)
    out = np.log(th["pi"] / (1.0 - th["pi"])) * p["ss"][n].sum(axis=1)
    return np.concatenate((np.zeros(p["S_perm"]), out))

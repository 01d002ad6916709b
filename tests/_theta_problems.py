"""Complete-data problems for test_gpu_theta_parity.py (and their CPU checks in test_theta_problems.py): the device Theta
update (evoamd_mstep_device) over learn sets, H x H solvers, backup and publish routes.

A problem is (algo, profile, N, D, H, S, S_perm, seed, kind): a K^n of _stats_problems.make_states, the Theta recipe of
_masked_problems.make_problem, data without masks.  Every shape is the smallest at which the code named in its comment can
still go wrong.  The reference is oracle/evo_oracle.py (oracle(), oracle_update()); the decisions of evo_amd.hip the
problems rely on are restated at the end (test_theta_problems.py checks them against the source), and wrong_update() is
the oracle's update with one mistake a kernel could make (test_theta_problems.py proves that each is rejected by a wide
margin)."""
import functools

import numpy as np

import _masked_problems as mp
import _stats_problems as sp

LPJ_RTOL, SUM_RTOL, BASE_RTOL = mp.LPJ_RTOL, mp.SUM_RTOL, mp.BASE_RTOL
THETA_RTOL, THETA_ATOL, COND_CAP = mp.THETA_RTOL, mp.THETA_ATOL, mp.COND_CAP

# name -> (algo, profile, N, D, H, S, S_perm, seed, kind).  kind: "" = the plain recipe; "nonsym" = Psi = I + A + 0.3 A^T
# (test_lpj_sssc_wide_states: xpt_szsz and s_sz_outer are non-symmetric too, so a transposed index shows); "clamp" = latent
# 0 in no state and with Psi[0, 0] = 1e-6, latent 1 in every state; "bg" = run with option background_unit = 1 (the last
# latent is NOT in every state: its prior then comes from the override alone, far from xpt_s / N, and not from the clamp
# at 1 - 5e-5 that an always-on latent reaches anyway, 3.9e-5 below the override).
PROBLEMS = {
    # H H = 144: n_part = 1 (one trace block); gjs_resident; H < D <= 8 H with D H = 780 = 5 * 144 + 60: the backup
    # loop `for (e = t; e < DH; e += HH)` of sssc_mstep_prepare_kernel ends in a ragged trip
    "es_h12": ("es3c", "mid", 37, 65, 12, 10, 0, 201, ""),
    # D = 100 > 8 H = 96: BACKUP_SIDE_KERNEL (theta_backup_kernel beside the statistics pass) and W = Wp inv(xpt_szsz)
    # over D = 100 rows, more than one 64-row trip of launch_gemm_nn_raw
    "es_d100": ("es3c", "mid", 37, 100, 12, 10, 0, 202, ""),
    # non-symmetric Psi; D = 24 = 2 H: the backup loop without a ragged trip
    "es_nonsym": ("es3c", "mid", 41, 24, 12, 10, 0, 203, "nonsym"),
    # H H = 1089: n_part = 2, per_block = 545, the second block of sssc_trace_partial_kernel holds 544 elements
    "es_h33": ("es3c", "mid", 61, 40, 33, 16, 0, 204, "nonsym"),
    # the last size of gjs_resident (GJR_MAXN) and of gj_inverse_reg (GJR_N)
    "es_h128": ("es3c", "sparse", 1500, 24, 128, 6, 0, 205, ""),
    # 16-column steps: cdiv(130, 16) = 9, odd (the result is copied from the partner buffer), the last step two columns
    # wide, ragged 64 x 64 tiles; pivoted: gjp_panel<16, 1>; n_part = 17, per_block = 995, last block 980
    "es_h130": ("es3c", "sparse", 1500, 24, 130, 6, 0, 206, ""),
    # n >= 256: gjs32 by default, cdiv(257, 32) = 9 steps (odd), the last one column wide; pivoted: gjp_panel<16, 2>
    "es_h257": ("es3c", "sparse", 3000, 16, 257, 4, 0, 207, ""),
    "es_clamp": ("es3c", "mid", 37, 25, 12, 10, 0, 208, "clamp"),
    "es_bg": ("es3c", "mid", 41, 25, 12, 10, 0, 209, "bg"),
    "bsc_h12": ("ebsc", "mid", 37, 25, 12, 10, 0, 211, ""),
    # S_perm = 1: the permanent all-zero state; two state words
    "bsc_h65": ("ebsc", "sparse", 400, 33, 65, 32, 1, 212, ""),
    # the 16-column SPD steps (9, odd) and gjp_panel<16, 1> on Wq
    "bsc_h130": ("ebsc", "sparse", 1500, 24, 130, 6, 0, 213, ""),
    # S > 256: the one-shot statistics kernel leaves no copy of Wq in tmpA (wq_copy_valid), the update copies it itself
    "bsc_s300": ("ebsc", "mid", 33, 32, 20, 300, 0, 214, ""),
    "bsc_clamp": ("ebsc", "mid", 37, 25, 12, 10, 0, 215, "clamp"),
    "bsc_bg": ("ebsc", "mid", 41, 25, 12, 10, 0, 216, "bg"),
    # ---- the lower edge: H = 1 ... 4 (the "sparse" pool holds all 2^H states) ----
    # H H = 1: one live thread of sssc_mstep_prepare_kernel saves W (8 trips), Psi, mus, pies and all DP_COUNT = 16 scalars
    # of the lazy-Theta backup; 1 x 1 inverses; S = 2^H: K^n is the whole state space
    "es_h1": ("es3c", "sparse", 37, 8, 1, 2, 0, 221, ""),
    # a single state per datapoint: every posterior is a point mass
    "es_h1_s1": ("es3c", "sparse", 37, 8, 1, 1, 0, 222, ""),
    # D = 8 H exactly: the last D of BACKUP_IN_UPDATE; H H = 4 live threads, DP_SIGMA2 (index 6) beyond them
    "es_h2": ("es3c", "sparse", 37, 16, 2, 3, 0, 223, ""),
    # D = 8 H + 1: BACKUP_SIDE_KERNEL at the same H
    "es_h2_d17": ("es3c", "sparse", 37, 17, 2, 3, 0, 224, ""),
    # D = 1: W is one row; S = 2^H
    "es_h2_d1": ("es3c", "sparse", 37, 1, 2, 4, 0, 225, ""),
    # H H = 9 < DP_COUNT: the scalars 9 .. 15 beyond the live threads; non-symmetric Psi and sums
    "es_h3": ("es3c", "sparse", 37, 24, 3, 5, 0, 226, "nonsym"),
    # H H = 16 = DP_COUNT: the first size at which one scalar per live thread is enough
    "es_h4": ("es3c", "sparse", 37, 9, 4, 7, 0, 227, ""),
    # N = 1: every sum is one datapoint's
    "es_n1": ("es3c", "sparse", 1, 8, 2, 4, 0, 228, ""),
    # 1 x 1 Wq
    "bsc_h1": ("ebsc", "sparse", 37, 5, 1, 2, 0, 231, ""),
    "bsc_h2": ("ebsc", "sparse", 37, 5, 2, 3, 0, 232, ""),
}
TINY = tuple(k for k, v in PROBLEMS.items() if v[4] <= 4)
ES_PROBLEMS = tuple(k for k, v in PROBLEMS.items() if v[0] == "es3c")
BSC_PROBLEMS = tuple(k for k, v in PROBLEMS.items() if v[0] == "ebsc")
CLAMP_PROBLEMS = tuple(k for k, v in PROBLEMS.items() if v[8] == "clamp")
THETA_PROBLEMS = tuple(k for k in PROBLEMS if k not in CLAMP_PROBLEMS)
# H >= 128: compared with the oracle's update of the device's own sums only
LARGE = tuple(k for k, v in PROBLEMS.items() if v[4] >= 128)
# Condition numbers of the H x H systems at the N above (test_theta_problems.py prints them and bounds them by COND_CAP;
# the sparse problems needed a pool of 8 H states and N in the thousands before every latent carried posterior mass: with
# the pool of 512, es_h257 had cond(xpt_szsz) = 3.9e16).  cond(xpt_szsz), cond(xpt_ss + eps I): es_h12 4.1, 7.7; es_d100
# 5.1, 8.1; es_nonsym 3.6, 9.5; es_h33 19.2, 23.7; es_h128 24.8, 21.8; es_h130 21.3, 22.5; es_h257 17.2, 16.1; es_bg 3.8,
# 8.9.  cond(Wq): bsc_h12 7.7; bsc_h65 5.2; bsc_h130 6.1; bsc_s300 3.6; bsc_bg 15.8.  The tiny problems: es_h1, es_h1_s1
# 1, 1 (1 x 1 systems); es_h2 3.1, 1.6; es_h2_d17 2.4, 1.8; es_h2_d1 1.6, 1.7; es_h3 2.2, 1.8; es_h4 1.7, 2.9; es_n1 2.7,
# 2.1; cond(Wq): bsc_h1 1; bsc_h2 1.3.

ES_KEYS = ("W", "pies", "mus", "Psi", "sigma2")
BSC_KEYS = ("W", "pi", "sigma")
# learn sets, each a different branch of theta_update_sssc / theta_update_bsc
LEARN_SETS = {
    "es3c": {
        "all": ES_KEYS,               # both inverses in one launch; Psi's finish rides in the trace kernel; NEW W^T W
        "W": ("W",),                  # xpt_szsz alone in the A slot; psi_floor_kernel; no trace
        "Psi": ("Psi",),              # xpt_ss + eps I alone in the A slot; sssc_psi_finish_kernel with the OLD mus
        "Psi+mus": ("Psi", "mus"),    # ... with the NEW mus
        "sigma2": ("sigma2",),        # no inverse; psi_floor_kernel; the trace alone, with the OLD W^T W
        "W+sigma2": ("W", "sigma2"),  # one inverse; the trace alone, with the NEW W^T W
        "pies+mus": ("pies", "mus"),  # the prepare kernel's vectors only
        "none": (),                   # statistics only: no update kernel runs
    },
    "ebsc": {
        "all": BSC_KEYS,
        "W": ("W",),
        "pi": ("pi",),
        "sigma": ("sigma",),
        "pi+sigma": ("pi", "sigma"),
        "none": (),
    },
}
LARGE_SETS = {"es3c": ("all", "W", "Psi"), "ebsc": ("all", "W")}  # "all" plus the single-inverse sets


def learn_sets(name):
    """Names of the learn sets problem `name` runs: every one up to H = 33, "all" plus the single-inverse sets above; the
    clamp problems only those without W and Psi (their H x H systems are singular by construction)."""
    algo, H, kind = PROBLEMS[name][0], PROBLEMS[name][4], PROBLEMS[name][8]
    if kind == "clamp":
        return tuple(k for k, v in LEARN_SETS[algo].items() if "W" not in v and "Psi" not in v)
    if H > 33:
        return LARGE_SETS[algo]
    return tuple(LEARN_SETS[algo])


def _insert_column(ss, at, value):
    """K^n with one more latent at index `at` that is `value` in every state (rows stay distinct)."""
    N, S, H = ss.shape
    out = np.empty((N, S, H + 1), dtype=bool)
    out[..., :at] = ss[..., :at]
    out[..., at] = value
    out[..., at + 1:] = ss[..., at:]
    return out


@functools.lru_cache(maxsize=None)
def make_problem(name):
    algo, profile, N, D, H, S, S_perm, seed, kind = PROBLEMS[name]
    rng = np.random.RandomState(seed)
    Y = rng.normal(size=(N, D))
    if algo == "es3c":  # the Theta of _masked_problems.make_problem
        W = rng.normal(size=(D, H)) * 0.4
        A = rng.normal(size=(H, 3)) * 0.2
        theta = {"W": W, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H), "Psi": np.eye(H) + A @ A.T,
                 "sigma2": np.float64(1.3)}
        if kind == "nonsym":
            B = rng.normal(size=(H, H)) * 0.05
            theta["Psi"] = np.eye(H) + B + 0.3 * B.T
        if kind == "clamp":  # latent 0 is in no state, so this entry enters no lpj; the update must floor it
            theta["Psi"][0, :] = theta["Psi"][:, 0] = 0.0
            theta["Psi"][0, 0] = 1e-6
    else:
        theta = {"W": rng.normal(size=(D, H)) * 0.5, "pi": np.float64(0.15), "sigma": np.float64(2.0)}
    if kind == "clamp":
        ss = _insert_column(_insert_column(sp.make_states(rng, N, S, H - 2, profile), 0, False), 1, True)
    else:
        ss = sp.make_states(rng, N, S, H, profile, pool_size=max(512, 8 * H))  # (every latent in some pool state)
    ones = np.ones((N, D), dtype=bool)
    return {"name": name, "algo": algo, "profile": profile, "N": N, "D": D, "H": H, "S": S, "S_perm": S_perm, "kind": kind,
            "background": kind == "bg", "Y": Y, "Y0": Y, "x_infr": ones, "x": ones, "theta": theta, "ss": ss}


# ---- the float64 reference ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(name):
    """{"lpj", "sums", "ljc"} of the oracle for the complete data of problem `name`: lpj over K^n and the M-step sums under
    their names in the packed accumulator."""
    from oracle import evo_oracle as orc
    p = make_problem(name)
    N, D, H, S, S_perm, ss, Y = p["N"], p["D"], p["H"], p["S"], p["S_perm"], p["ss"], p["Y"]
    th = dict(p["theta"])
    if p["algo"] == "es3c":
        suff = {"ss": ss, "lpj": np.empty((N, S)), "S_perm": 0, "incl": np.zeros((0, H), dtype=bool), "Mprime": S}
        acc = orc.sssc_EM_accumulate(th, suff, Y, use_storage=True, evolve=False)
        lpj = suff["lpj"]
        sums = {k: acc[k] for k in mp.ES_NAMES if k in acc}
    else:
        cnt = orc.bsc_precompute(th, D, H)
        lpj = np.empty((N, S_perm + S))
        for n in range(N):
            if S_perm:
                lpj[n, 0] = orc.bsc_lpj_allzero(th, Y[n], cnt)[0]
            lpj[n, S_perm:] = orc.bsc_lpj(th, ss[n], Y[n], cnt)
        suff = {"ss": ss, "lpj": lpj, "S_perm": S_perm, "permanent": {"allzero": bool(S_perm), "background": False}}
        sums = dict(orc.bsc_accumulate(th, suff, Y))
        sums["Fs"] = orc.free_energy_sum(lpj)
    return {"lpj": lpj, "sums": sums, "ljc": float(th["ljc"])}


def _acc(p, sums):
    keys = ("xpt_s", "xpt_ss", "xpt_sz", "xpt_szsz", "Wp", "s_sz_outer", "sz_sz_outer", "y_outer_diag")
    if p["algo"] == "ebsc":
        keys = ("Wp", "Wq", "pies", "sigma")
    return {k: np.array(sums[k], dtype=np.float64) for k in keys}


def _theta_in(p):
    th = {k: np.array(v) for k, v in p["theta"].items()}
    for k in ("sigma2", "pi", "sigma"):
        if k in th:
            th[k] = np.float64(th[k])
    return th


def oracle_update(p, sums, to_learn, clamp=True):
    """Theta^new of the oracle's complete-data update (sssc_update / bsc_update, background = the problem's) from `sums`,
    the oracle's or the views of the device's accumulator, followed by the clamps of check_params (which the device
    applies and sssc_update / bsc_update do not).  An empty learn set is no update at all."""
    from oracle import evo_oracle as orc
    N, D, H = p["N"], p["D"], p["H"]
    th = _theta_in(p)
    if not to_learn:
        return th
    if p["algo"] == "es3c":
        th = orc.sssc_update(th, _acc(p, sums), N, D, H, tuple(to_learn), background=p["background"])
        th["sigma2"] = np.float64(th["sigma2"])
        return orc.check_params(th, orc.SSSC_POLICY) if clamp else th
    th = orc.bsc_update(th, _acc(p, sums), N, D, H, tuple(to_learn), background=p["background"])
    th.pop("pies", None)
    th["pi"], th["sigma"] = np.float64(th["pi"]), np.float64(th["sigma"])
    return orc.check_params(th, orc.BSC_POLICY) if clamp else th


new_scalars = mp.new_scalars              # ljc, sigma2_inv / pre1 ... of the scalar block behind Theta^new
update_conditions = mp.update_conditions  # cond of xpt_szsz, xpt_ss + eps I / Wq


# ---- the oracle's update with one mistake a kernel could make ---------------------------------------------------------
def wrong_update(p, sums, kind):
    """Theta^new ("all" learned, no clamps) with one mistake:
    old_mus_in_psi: sssc_psi_finish_kernel reads the OLD mus in -2 mus[:, None] * s_sz_outer
    mus_row:        mus[None, :] there (mus[j] for mus[i])
    psi_matmul:     Psi_raw @ inv(.) for the element-wise product (quirk Q2)
    old_wtw:        the trace of sigma2 with the OLD W^T W
    trace_tail:     the trace without its last H H - n_part floor(H H / n_part) elements (per_block rounded down)
    inv_T:          W = Wp inv(xpt_szsz)^T
    no_bg:          pies / pi without the background unit's override
    wt_as_w:        EBSC: W^T = inv(Wq) Wp stored where W belongs, without the transposition"""
    from oracle import evo_oracle as orc
    N, D, H = p["N"], p["D"], p["H"]
    a = _acc(p, sums)
    old = _theta_in(p)
    th = oracle_update(p, sums, LEARN_SETS[p["algo"]]["all"], clamp=False)
    if kind == "no_bg":
        q = dict(p, background=False)
        return oracle_update(q, sums, LEARN_SETS[p["algo"]]["all"], clamp=False)
    if p["algo"] == "ebsc":
        assert kind == "wt_as_w"
        th["W"] = np.ascontiguousarray(th["W"].T).reshape(D, H)
        return th
    if kind in ("old_mus_in_psi", "mus_row", "psi_matmul"):
        m = th["mus"]
        raw = np.outer(m, m) * a["xpt_ss"] + a["xpt_szsz"]
        if kind == "old_mus_in_psi":
            raw -= 2 * old["mus"][:, None] * a["s_sz_outer"]
        elif kind == "mus_row":
            raw -= 2 * m[None, :] * a["s_sz_outer"]
        else:
            raw -= 2 * m[:, None] * a["s_sz_outer"]
        T2inv = np.linalg.inv(a["xpt_ss"] + orc.EPS_PSI * np.eye(H))
        th["Psi"] = raw @ T2inv if kind == "psi_matmul" else raw * T2inv
    elif kind in ("old_wtw", "trace_tail"):
        W = old["W"] if kind == "old_wtw" else th["W"]
        terms = (a["sz_sz_outer"] * np.dot(W.T, W).T).ravel()
        if kind == "trace_tail":
            terms = terms[:n_part(H) * (H * H // n_part(H))]
            assert terms.size < H * H
        th["sigma2"] = np.float64((a["y_outer_diag"].sum() - terms.sum()) / N / D + orc.EPS_SIGMA2)
    elif kind == "inv_T":
        th["W"] = np.dot(a["Wp"], np.linalg.inv(a["xpt_szsz"]).T)
    else:
        raise AssertionError(kind)
    return th


# ---- decisions of evo_amd.hip the problems rely on (test_theta_problems.py holds them against the source) --------------
GJR_N = 128       # kernels_mstep.hpp: gj_inverse_reg_kernel up to this n (launch_inverse_pivoted)
GJR_MAXN = 128    # gjs_resident_kernel up to this n (launch_inverse_spd)
GJS_B = 16        # columns per gjs_step_kernel launch
GJS32 = 32        # columns per gjs32_step_kernel launch
GJS32_FROM = 256  # `c->spd_block == 0 && n >= 256`: the wider step by default
GJP_RPT1_TO = 256  # `rpt = n <= 256 ? 1 : 2`: gjp_panel_kernel<16, 1> up to this n, <16, 2> above
BACKUP_RATIO = 8  # backup_rides_in_update: ES3C with D <= 8 H
SIDE_FLOPS = 8e9  # mstep_plan: PUBLISH_SIDE from this many contraction flops on when Theta stays home


def cdiv(a, b):
    return -(-a // b)


def n_part(H):
    """theta_update_sssc: `n_part = min(1024, cdiv(HH, 1024))` blocks of sssc_trace_partial_kernel."""
    return min(1024, cdiv(H * H, 1024))


def per_block(H):
    return cdiv(H * H, n_part(H))


def solver(H, spd=1, block=0):
    """(kernel family, block steps) launch_inverse takes for an H x H system under options inverse_spd / inverse_block."""
    if not spd:
        if H <= GJR_N:
            return "gj_inverse_reg", 1
        return ("gjp_panel<16,1>" if H <= GJP_RPT1_TO else "gjp_panel<16,2>"), cdiv(H, 16)
    if H <= GJR_MAXN and block == 0:
        return "gjs_resident", 1
    if H >= GJS32 and (block == 32 or (block == 0 and H >= GJS32_FROM)):
        return "gjs32", cdiv(H, GJS32)
    return "gjs", cdiv(H, GJS_B)


def backup_route(p):
    """BackupRoute of mstep_device(theta_to_host=False) with a non-empty learn set."""
    return "in_update" if p["algo"] == "es3c" and p["D"] <= BACKUP_RATIO * p["H"] else "side_kernel"


DP_COUNT = 16     # kernels_mstep.hpp: doubles of the scalar block, the last segment of the lazy-Theta backup
DP_SIGMA2 = 6     # ... and sigma2's place in it (DP_PI = 4 and DP_SIGMA = 5 are EBSC's: set_params_sssc leaves them 0)


def backup_layout(p):
    """Offsets of the segments of theta_bak (theta_segs: W | Psi | mus | pies | scalar block; EBSC: W | scalar block)."""
    D, H = p["D"], p["H"]
    if p["algo"] == "ebsc":
        return {"W": 0, "dpar": D * H, "end": D * H + DP_COUNT}
    at = {"W": 0, "Psi": D * H, "mus": D * H + H * H, "pies": D * H + H * H + H, "dpar": D * H + H * H + 2 * H}
    at["end"] = at["dpar"] + DP_COUNT
    return at


def backup_image(p):
    """What theta_bak holds after a complete backup of the ES3C problem p's Theta, slot by slot; None where the passes
    over K^n write (counters, Fs, ljc_prev) or where only the device's rounding is known (1 / sigma2, ljc)."""
    th, at = p["theta"], backup_layout(p)
    img = [None] * at["end"]
    for k in ("W", "Psi", "mus", "pies"):
        v = np.asarray(th[k], dtype=np.float64).ravel()
        img[at[k]:at[k] + v.size] = [float(x) for x in v]
    for i in (0, 1, 4, 5):  # DP_PRE1, DP_PILBAR, DP_PI, DP_SIGMA: EBSC's
        img[at["dpar"] + i] = 0.0
    img[at["dpar"] + DP_SIGMA2] = float(th["sigma2"])
    return img


def backup_prelude():
    """es_h2_d17 with another sigma2.  evoamd_configure keeps theta_bak across a change of geometry (DevBuf::ensure only
    grows), so a lazy update of this problem (side-kernel route: a complete backup of 58 doubles) on the same context
    decides what the slots hold that an in-update backup of es_h1 (27 doubles) or es_h2 (56) fails to write: the
    restore test does not depend on what fresh device memory happens to contain."""
    p = dict(make_problem("es_h2_d17"))
    p["theta"] = dict(p["theta"], sigma2=np.float64(2.7))
    return p


def second_theta(p):
    """Theta' for a second lazy update on the same context: every scalar and vector differs from the problem's Theta."""
    th = {k: np.array(v) for k, v in p["theta"].items()}
    if p["algo"] == "es3c":
        th["sigma2"] = np.float64(0.85)
        th["mus"] = th["mus"] * 0.5 + 0.25
        th["pies"] = 0.5 - th["pies"]  # (0.1, 0.4) again
        th["W"] = th["W"] * 1.25
    else:
        th["pi"], th["sigma"] = np.float64(0.3), np.float64(1.6)
        th["W"] = th["W"] * 1.25
    return th


def contraction_flops(algo, N, D, H):
    return 2.0 * N * (D + 2.0 * H) * H if algo == "es3c" else 2.0 * N * D * H


def side_stream_shape(D=32, H=512):
    """(N, D, H) of the side-stream problem: the smallest N at which an ES3C context of this D and H reaches SIDE_FLOPS.
    H = 512 (the workload's) keeps N, and with it the pass over K^n, small."""
    N = int(np.ceil(SIDE_FLOPS / (2.0 * (D + 2.0 * H) * H)))
    assert contraction_flops("es3c", N, D, H) >= SIDE_FLOPS > contraction_flops("es3c", N - 1, D, H)
    return N, D, H


@functools.lru_cache(maxsize=None)
def make_side_problem():
    """The ES3C problem of side_stream_shape(): the sparse profile, S = 2, the Theta recipe of make_problem; the pool holds
    4096 states so that every latent occurs (the update must be well posed; nothing bounds its conditioning, and no
    oracle runs at this size)."""
    N, D, H = side_stream_shape()
    rng = np.random.RandomState(301)
    A = rng.normal(size=(H, 3)) * 0.2
    theta = {"W": rng.normal(size=(D, H)) * 0.4, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H),
             "Psi": np.eye(H) + A @ A.T, "sigma2": np.float64(1.3)}
    ss = sp.make_states(rng, N, 2, H, "sparse", pool_size=4096)
    return {"name": "es_side", "algo": "es3c", "profile": "sparse", "N": N, "D": D, "H": H, "S": 2, "S_perm": 0, "kind": "",
            "background": False, "Y": rng.normal(size=(N, D)), "theta": theta, "ss": ss}

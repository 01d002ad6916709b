"""CPU checks of the Theta-update problems (_theta_problems.py): every problem reaches the branch it is named for, the
thresholds those branches hang on are the source's, the H x H systems are well conditioned, the clamp problems give
exactly the clamped values and every other Theta lies strictly inside the clamps, an update that is wrong in the way a
kernel would be differs from the oracle's by at least a thousand times the tolerance the GPU test holds, and the oracle
is quick."""
import os
import re
import time

import numpy as np
import pytest

import _stats_problems as sp
import _theta_problems as tp

MARGIN = 1e3  # a wrong update must miss the GPU tolerance by this factor


def _src(name):
    with open(os.path.join(sp.CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def _excess(got, want):
    """max |got - want| in units of the GPU check's tolerance, (THETA_RTOL + THETA_ATOL) max(1, |want|max) at the most."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / ((tp.THETA_RTOL + tp.THETA_ATOL) * max(1.0, float(np.abs(want).max())))


def _all(p):
    return tp.LEARN_SETS[p["algo"]]["all"]


# ---- regimes -----------------------------------------------------------------------------------------------------------
def test_problems_reach_their_branches():
    P = {n: tp.make_problem(n) for n in tp.PROBLEMS}
    H = {n: P[n]["H"] for n in P}
    # ES3C: the trace blocks
    assert (tp.n_part(12), tp.per_block(12)) == (1, 144)
    assert (H["es_h33"], tp.n_part(33), tp.per_block(33)) == (33, 2, 545) and 33 * 33 - 545 == 544
    assert tp.n_part(130) * tp.per_block(130) > 130 * 130 > (tp.n_part(130) - 1) * tp.per_block(130)  # ragged last block
    assert 257 * 257 % tp.n_part(257) != 0
    # the solvers: (family, block steps)
    assert tp.solver(12) == ("gjs_resident", 1) and tp.solver(12, spd=0) == ("gj_inverse_reg", 1)
    assert H["es_h128"] == tp.GJR_MAXN == tp.GJR_N and tp.solver(128) == ("gjs_resident", 1)
    assert tp.solver(128, spd=0) == ("gj_inverse_reg", 1)
    assert tp.solver(130) == ("gjs", 9) and 130 - 8 * 16 == 2 and tp.solver(130, spd=0) == ("gjp_panel<16,1>", 9)
    assert tp.solver(130, block=16) == ("gjs", 9) and tp.solver(130, block=32) == ("gjs32", 5)
    assert tp.solver(257) == ("gjs32", 9) and 257 - 8 * 32 == 1 and tp.solver(257, spd=0) == ("gjp_panel<16,2>", 17)
    assert tp.solver(257, block=16) == ("gjs", 17) and tp.solver(257, block=32) == ("gjs32", 9)
    for name in ("es_h130", "es_h257", "bsc_h130"):  # an odd number of block steps: the result comes from the partner
        assert tp.solver(H[name])[1] % 2 == 1, name
    # backup routes
    assert tp.backup_route(P["es_d100"]) == "side_kernel" and P["es_d100"]["D"] > 8 * H["es_d100"] and P["es_d100"]["D"] > 64
    p = P["es_h12"]
    assert tp.backup_route(p) == "in_update" and p["H"] < p["D"] <= 8 * p["H"] and (p["D"] * p["H"]) % (p["H"] ** 2) != 0
    assert all(tp.backup_route(P[n]) == "side_kernel" for n in tp.BSC_PROBLEMS)
    # non-symmetric Psi, and with it non-symmetric sums
    for name in ("es_nonsym", "es_h33"):
        Psi, s = P[name]["theta"]["Psi"], tp.oracle(name)["sums"]
        assert np.abs(Psi - Psi.T).max() > 1e-2
        assert np.abs(s["xpt_szsz"] - s["xpt_szsz"].T).max() > MARGIN * tp.THETA_RTOL * np.abs(s["xpt_szsz"]).max()
        assert np.abs(s["s_sz_outer"] - s["s_sz_outer"].T).max() > MARGIN * tp.THETA_RTOL * np.abs(s["s_sz_outer"]).max()
    # EBSC
    assert H["bsc_h12"] == 12 and (H["bsc_h65"], P["bsc_h65"]["S_perm"]) == (65, 1) and H["bsc_h130"] == 130
    assert P["bsc_s300"]["S"] > 256 and all(P[n]["S"] <= 256 for n in tp.BSC_PROBLEMS if n != "bsc_s300")
    assert all(P[n]["S_perm"] == 0 for n in P if n != "bsc_h65")
    # the clamp and background problems
    for name in tp.CLAMP_PROBLEMS:
        ss = P[name]["ss"]
        assert not ss[..., 0].any() and ss[..., 1].all(), name
    assert P["es_clamp"]["theta"]["Psi"][0, 0] < 1e-5
    for name in ("es_bg", "bsc_bg"):
        assert P[name]["background"] and not P[name]["ss"][..., -1].all(), name  # (the override, not the clamp, decides)
    assert sum(P[n]["background"] for n in P) == 2
    for name, p in P.items():  # K^n rows stay distinct
        for n in range(0, p["N"], 7):
            assert len({row.tobytes() for row in p["ss"][n]}) == p["S"], (name, n)


def test_tiny_problems_reach_the_lower_edge():
    """H = 1 ... 4: the live threads of sssc_mstep_prepare_kernel (H H) against the DP_COUNT scalars its backup saves, both
    backup routes at H = 2, S = 2^H, a single state, D = 1, N = 1, and K^n rows that stay distinct in EVERY datapoint."""
    P = {n: tp.make_problem(n) for n in tp.TINY}
    assert set(P) == {"es_h1", "es_h1_s1", "es_h2", "es_h2_d17", "es_h2_d1", "es_h3", "es_h4", "es_n1", "bsc_h1", "bsc_h2"}
    shape = {n: (p["N"], p["D"], p["H"], p["S"]) for n, p in P.items()}
    assert shape == {"es_h1": (37, 8, 1, 2), "es_h1_s1": (37, 8, 1, 1), "es_h2": (37, 16, 2, 3), "es_h2_d17": (37, 17, 2, 3),
                     "es_h2_d1": (37, 1, 2, 4), "es_h3": (37, 24, 3, 5), "es_h4": (37, 9, 4, 7), "es_n1": (1, 8, 2, 4),
                     "bsc_h1": (37, 5, 1, 2), "bsc_h2": (37, 5, 2, 3)}
    assert all(p["profile"] == "sparse" and p["S_perm"] == 0 and not p["background"] for p in P.values())
    dp_count = int(re.search(r"\bDP_COUNT = (\d+)", _src("kernels_mstep.hpp")).group(1))
    sigma2_at = int(re.search(r"\bDP_SIGMA2 = (\d+),", _src("kernels_mstep.hpp")).group(1))
    assert (dp_count, sigma2_at) == (tp.DP_COUNT, tp.DP_SIGMA2) == (16, 6)
    # live threads of the prepare kernel against the scalar block: below H = 4 one scalar per thread is not enough
    for name, live in (("es_h1", 1), ("es_h2", 4), ("es_h3", 9), ("es_h4", 16)):
        assert P[name]["H"] ** 2 == live, name
    assert 1 <= sigma2_at and 4 <= sigma2_at < 9 < dp_count == 16  # sigma2 beyond the live threads at H = 1 and H = 2
    # routes: in the update up to D = 8 H, the side kernel one above; always the side kernel for EBSC
    for name in tp.TINY:
        want = "in_update" if name.startswith("es_") and name != "es_h2_d17" else "side_kernel"
        assert tp.backup_route(P[name]) == want, name
    assert P["es_h2"]["D"] == tp.BACKUP_RATIO * P["es_h2"]["H"] and P["es_h2_d17"]["D"] == tp.BACKUP_RATIO * 2 + 1
    # the prelude of the restore test (test_gpu_theta_parity.py): es_h2_d17's backup covers the slots of es_h1 and es_h2
    # from which a restore reads sigma2, with values that are not the expected one
    filler = tp.backup_prelude()
    lay = tp.backup_layout(filler)
    assert filler["theta"]["sigma2"] != P["es_h2"]["theta"]["sigma2"] == 1.3
    for name in ("es_h1", "es_h2"):
        slot = tp.backup_layout(P[name])["dpar"] + tp.DP_SIGMA2
        assert tp.backup_layout(P[name])["end"] <= lay["end"] == 58, name
        held = tp.backup_image(filler)[slot]
        print("%s: the backup slot of sigma2 (%d) holds %r after the prelude" % (name, slot, held))
        assert held is not None and held != 1.3, (name, slot, held)
    # the state space
    for name in ("es_h1", "es_h2_d1", "es_n1", "bsc_h1"):
        assert P[name]["S"] == 2 ** P[name]["H"], name
    assert P["es_h1_s1"]["S"] == 1 and P["es_h2_d1"]["D"] == 1 and P["es_n1"]["N"] == 1
    for name, p in P.items():
        for n in range(p["N"]):
            assert len({row.tobytes() for row in p["ss"][n]}) == p["S"], (name, n)
        if p["N"] > 1:
            assert p["ss"].any(axis=(0, 1)).all(), name  # every latent in some state
    # es_h3: non-symmetric Psi and sums, as for es_nonsym
    Psi, s = P["es_h3"]["theta"]["Psi"], tp.oracle("es_h3")["sums"]
    assert np.abs(Psi - Psi.T).max() > 1e-2
    assert np.abs(s["xpt_szsz"] - s["xpt_szsz"].T).max() > MARGIN * tp.THETA_RTOL * np.abs(s["xpt_szsz"]).max()
    assert np.abs(s["s_sz_outer"] - s["s_sz_outer"].T).max() > MARGIN * tp.THETA_RTOL * np.abs(s["s_sz_outer"]).max()
    # every oracle result is finite
    for name, p in P.items():
        o = tp.oracle(name)
        assert np.isfinite(o["lpj"]).all(), name
        th = tp.oracle_update(p, o["sums"], tp.LEARN_SETS[p["algo"]]["all"])
        assert all(np.isfinite(np.asarray(v)).all() for v in th.values()), name


def test_learn_sets_of_every_problem():
    es, bsc = tp.LEARN_SETS["es3c"], tp.LEARN_SETS["ebsc"]
    assert [tuple(sorted(v)) for v in es.values()] == [tuple(sorted(v)) for v in (
        tp.ES_KEYS, ("W",), ("Psi",), ("Psi", "mus"), ("sigma2",), ("W", "sigma2"), ("pies", "mus"), ())]
    assert [tuple(sorted(v)) for v in bsc.values()] == [tuple(sorted(v)) for v in (
        tp.BSC_KEYS, ("W",), ("pi",), ("sigma",), ("pi", "sigma"), ())]
    for name, v in tp.PROBLEMS.items():
        sets = tp.learn_sets(name)
        if v[8] == "clamp":
            assert sets == (("sigma2", "pies+mus", "none") if v[0] == "es3c" else ("pi", "sigma", "pi+sigma", "none")), name
        elif v[4] <= 33:
            assert sets == tuple(tp.LEARN_SETS[v[0]]), name
        else:
            assert sets == (("all", "W", "Psi") if v[0] == "es3c" else ("all", "W")), name


def test_side_stream_problem():
    N, D, H = tp.side_stream_shape()
    assert tp.contraction_flops("es3c", N, D, H) >= tp.SIDE_FLOPS > tp.contraction_flops("es3c", N - 1, D, H)
    p = tp.make_side_problem()
    assert (p["N"], p["D"], p["H"], p["S"]) == (N, D, H, 2) and p["ss"].shape == (N, 2, H)
    assert p["ss"].any(axis=(0, 1)).all()  # every latent occurs
    assert p["ss"].sum(axis=-1).max() <= 4  # sparse


# ---- decision constants ------------------------------------------------------------------------------------------------
def test_decision_constants_match_the_source():
    ms, hip = _src("kernels_mstep.hpp"), _src("evo_amd.hip")
    for name in ("GJR_N", "GJR_MAXN", "GJS_B", "GJS32"):
        assert _define(ms, name) == getattr(tp, name), name
    for line in ("if (n <= GJR_N) {",
                 "const int rpt = n <= %d ? 1 : 2;  // rows per thread of the panel kernel" % tp.GJP_RPT1_TO,
                 "for (int p0 = 0; p0 < n; p0 += 16, flip ^= 1) {",
                 "if (n <= GJR_MAXN && c->spd_block == 0) {",
                 "if (n >= GJS32 && (c->spd_block == 32 || (c->spd_block == 0 && n >= %d))) {" % tp.GJS32_FROM,
                 "for (int p0 = 0; p0 < n; p0 += GJS32, flip32 ^= 1)",
                 "for (int p0 = 0; p0 < n; p0 += GJS_B, flip ^= 1)",
                 "if (c->spd_inverse && !force_pivot) return launch_inverse_spd(c, A, B, n);",
                 "const int n_part = (int)std::min<i64>(1024, cdiv(HH, 1024));",
                 "return c->model == EVOAMD_MODEL_SSSC && c->D <= %d * c->H;" % tp.BACKUP_RATIO,
                 "if (c->mbox_side && contraction_flops(c) >= (theta_out ? 8e10 : 8e9))",
                 "if (!c->wq_copy_valid || p.force_pivot)"):
        assert line in hip, line
    assert tp.SIDE_FLOPS == 8e9
    assert "cdiv(HH, n_part), c->colpart" in hip  # per_block
    flops = hip[hip.index("static double contraction_flops("):]
    assert "2.0 * (double)c->N * (c->D + 2.0 * c->H) * c->H : 2.0 * (double)c->N * c->D * c->H;" in flops[:flops.index("\n}\n")]
    names = set(re.findall(r'^    \{"(\w+)", OPT_', hip, re.M))  # the rows of the option table
    assert {"background_unit", "inverse_spd", "inverse_block", "theta_copy_engine", "mailbox_side_stream",
            "sssc_precision"} <= names
    # the clamps the kernels restate: eps_pies, check_params' tol, the background prior
    from oracle import evo_oracle as orc
    assert (orc.EPS_PIES, orc.TOL, orc.EPS_PSI, orc.EPS_SIGMA2) == (5e-5, 1e-5, 1e-5, 1e-5)
    for line in ("if (p <= 5e-5) p = 5e-5;  // eps_pies", "if (p >= 1.0 - 5e-5) p = 1.0 - 5e-5;",
                 "if (bg_unit && i == H - 1) p = 1.0 - 1.1e-5;", "if (i == j && v < 1e-5) v = 1e-5;"):
        assert line in ms, line


# ---- conditioning, time ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tp.THETA_PROBLEMS)
def test_problems_are_well_conditioned(name):
    p = tp.make_problem(name)
    conds = tp.update_conditions(p, tp.oracle(name)["sums"])
    print(name, {k: "%.3g" % v for k, v in conds.items()})
    assert all(v <= tp.COND_CAP for v in conds.values()), conds


def test_oracle_of_the_largest_problem_is_quick():
    tp.oracle.cache_clear()
    t = time.perf_counter()
    o = tp.oracle("es_h257")
    assert time.perf_counter() - t < 60.0
    assert np.isfinite(o["lpj"]).all()


# ---- clamps ------------------------------------------------------------------------------------------------------------
def test_clamp_problems_give_the_clamped_values():
    from oracle import evo_oracle as orc
    p = tp.make_problem("es_clamp")
    s = tp.oracle("es_clamp")["sums"]
    assert s["xpt_s"][0] == 0.0 and s["xpt_sz"][0] == 0.0 and abs(s["xpt_s"][1] - p["N"]) <= 1e-12 * p["N"]
    assert np.linalg.cond(s["xpt_szsz"]) > 1e15  # singular by construction: no learn set with W or Psi here
    th = tp.oracle_update(p, s, ("pies", "mus"))
    assert th["pies"][0] == 5e-5 and th["pies"][1] == 1.0 - 5e-5 and th["mus"][0] == 0.0
    assert ((th["pies"][2:] > 5e-5) & (th["pies"][2:] < 1.0 - 5e-5)).all()
    want = p["theta"]["Psi"].copy()
    want[0, 0] = orc.TOL
    assert p["theta"]["Psi"][0, 0] == 1e-6 and np.array_equal(th["Psi"], want)
    # without the clamps of check_params the floor is missing: the oracle's update alone is not the reference
    assert tp.oracle_update(p, s, ("pies", "mus"), clamp=False)["Psi"][0, 0] == 1e-6
    assert np.array_equal(tp.oracle_update(p, s, ())["Psi"], p["theta"]["Psi"])  # no update, no floor
    p = tp.make_problem("bsc_clamp")
    s = tp.oracle("bsc_clamp")["sums"]
    assert s["pies"][0] == 0.0 and abs(s["pies"][1] - p["N"]) <= 1e-12 * p["N"]
    th = tp.oracle_update(p, s, ("pi",))
    assert th["pi"] == (s["pies"] / p["N"]).sum() / p["H"] and 1.0 / p["H"] < th["pi"] < 1.0 - 1e-5


@pytest.mark.parametrize("name", tp.THETA_PROBLEMS)
def test_theta_lies_strictly_inside_the_clamps(name):
    """Theta and Theta^new of every learn set: check_params changes nothing, no bound is met."""
    p = tp.make_problem(name)
    s = tp.oracle(name)["sums"]
    thetas = [("input", {k: np.array(v) for k, v in p["theta"].items()})]
    thetas += [(ls, tp.oracle_update(p, s, tp.LEARN_SETS[p["algo"]][ls], clamp=False)) for ls in tp.learn_sets(name)]
    for label, th in thetas:
        if p["algo"] == "es3c":
            pies = th["pies"][:-1] if p["background"] and label in ("all", "pies+mus") else th["pies"]
            assert ((pies > 5e-5) & (pies < 1.0 - 5e-5)).all(), (name, label)
            assert (th["pies"] > 1e-5).all() and (th["pies"] < 1.0 - 1e-5).all(), (name, label)
            assert (np.diag(th["Psi"]) > 1e-5).all() and th["sigma2"] > 2e-5, (name, label)
        else:
            assert 1e-5 < th["pi"] < 1.0 - 1e-5 and th["sigma"] > 1e-5, (name, label)
    for ls in tp.learn_sets(name):
        a = tp.oracle_update(p, s, tp.LEARN_SETS[p["algo"]][ls], clamp=False)
        b = tp.oracle_update(p, s, tp.LEARN_SETS[p["algo"]][ls])
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, ls, k)


# ---- sensitivity: an update wrong in one place is rejected -----------------------------------------------------------------
def _proof(name, kind, key):
    p = tp.make_problem(name)
    s = tp.oracle(name)["sums"]
    good = tp.oracle_update(p, s, _all(p), clamp=False)
    bad = tp.wrong_update(p, s, kind)
    x = _excess(bad[key], good[key])
    print("%s %s: %s off by %.3g tolerances" % (name, kind, key, x))
    assert x >= MARGIN, (name, kind, key, x)
    for k in good:  # ... and nothing else moved
        if k != key:
            assert np.array_equal(bad[k], good[k]), (name, kind, k)


@pytest.mark.parametrize("name", ["es_h12", "es_nonsym", "es_h33"])
@pytest.mark.parametrize("kind", ["old_mus_in_psi", "mus_row", "psi_matmul"])
def test_sensitive_to_a_wrong_psi(name, kind):
    _proof(name, kind, "Psi")


@pytest.mark.parametrize("name", ["es_h12", "es_d100", "es_h33"])
def test_sensitive_to_the_old_gram_in_sigma2(name):
    _proof(name, "old_wtw", "sigma2")


def test_sensitive_to_a_trace_without_its_last_elements():
    H = tp.make_problem("es_h33")["H"]
    assert H * H - tp.n_part(H) * (H * H // tp.n_part(H)) == 1
    _proof("es_h33", "trace_tail", "sigma2")


@pytest.mark.parametrize("name", ["es_nonsym", "es_h33"])
def test_sensitive_to_a_transposed_inverse(name):
    _proof(name, "inv_T", "W")


@pytest.mark.parametrize("name", ["bsc_h12", "bsc_s300"])
def test_sensitive_to_a_transposed_ebsc_W(name):
    """Wq = sum_n <s s^T> is symmetric, so inv(Wq^T) is inv(Wq) and a transposed read of Wq cannot show; the transposition
    that can go wrong is the product's: W^T = inv(Wq) Wp written where W belongs."""
    Wq = tp.oracle(name)["sums"]["Wq"]
    assert np.abs(Wq - Wq.T).max() <= 1e-12 * np.abs(Wq).max()
    _proof(name, "wt_as_w", "W")


# the mistakes that make sense at tiny H, at the same margin.  bsc_h2's one mistake is wt_as_w; inv_T needs a
# non-symmetric xpt_szsz, which es_h3 ("nonsym") has and es_h2 has not (test_mistakes_that_cannot_show_...).
TINY_PROOFS = [(name, kind, key) for name in ("es_h2", "es_h3")
               for kind, key in (("old_mus_in_psi", "Psi"), ("mus_row", "Psi"), ("psi_matmul", "Psi"), ("old_wtw", "sigma2"),
                                 ("inv_T", "W")) if (name, kind) != ("es_h2", "inv_T")] + [("bsc_h2", "wt_as_w", "W")]


@pytest.mark.parametrize("name,kind,key", TINY_PROOFS)
def test_tiny_problems_reject_a_wrong_update(name, kind, key):
    _proof(name, kind, key)


def test_mistakes_that_cannot_show_at_one_latent():
    """H = 1: a 1 x 1 matmul is the element-wise product (psi_matmul), mus[None, :] is mus[:, None] (mus_row) and a 1 x 1
    inverse is its own transpose (inv_T): these three give the oracle's update exactly, so es_h1 proves nothing about
    them (es_h2 and es_h3 do).  What does show at H = 1 keeps the margin.  EBSC at H = 1: W^T (1 x D) stored where W
    (D x 1) belongs is the same memory."""
    p = tp.make_problem("es_h1")
    s = tp.oracle("es_h1")["sums"]
    good = tp.oracle_update(p, s, _all(p), clamp=False)
    for kind in ("psi_matmul", "mus_row", "inv_T"):
        bad = tp.wrong_update(p, s, kind)
        for k in good:
            assert _excess(bad[k], good[k]) <= 1e-3, (kind, k)  # rounding of a second evaluation at the most
    _proof("es_h1", "old_mus_in_psi", "Psi")
    _proof("es_h1", "old_wtw", "sigma2")
    p = tp.make_problem("bsc_h1")
    s = tp.oracle("bsc_h1")["sums"]
    good = tp.oracle_update(p, s, _all(p), clamp=False)
    assert np.array_equal(tp.wrong_update(p, s, "wt_as_w")["W"], good["W"])
    # es_h2: Psi is symmetric (the plain recipe), and so is xpt_szsz up to rounding: inv(.)^T is inv(.), at any H
    p = tp.make_problem("es_h2")
    s = tp.oracle("es_h2")["sums"]
    assert np.abs(s["xpt_szsz"] - s["xpt_szsz"].T).max() <= 1e-12 * np.abs(s["xpt_szsz"]).max()
    good = tp.oracle_update(p, s, _all(p), clamp=False)
    assert _excess(tp.wrong_update(p, s, "inv_T")["W"], good["W"]) <= 1e-3


def test_sensitive_to_the_background_override():
    _proof("es_bg", "no_bg", "pies")
    _proof("bsc_bg", "no_bg", "pi")

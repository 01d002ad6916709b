"""CPU checks of the synthetic E-step problems (tests/_estep_problems.py) that test_gpu_estep_paths.py runs: the generator
plants what each case claims, the values of the bit-parity cases are pairwise distinct, the restated selection rule
agrees with oracle.vary_Kn where there are no ties and the tie cases tell the rule from its wrong variants, the
restatements (SPL / CPL ladder, gram2 eligibility, digest layout, fused LDS plan) match the source, and the cases
together reach every vary_kn_kernel instantiation x {digest, word} x S_perm {0, 1}."""
import os
import re

import numpy as np
import pytest

import _estep_problems as ep


def _src(name):
    with open(os.path.join(ep.CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope="module")
def problems():
    return {name: ep.make_problem(name) for name in ep.PROBLEMS}


def test_rows_are_distinct_and_shapes_right(problems):
    for name, p in problems.items():
        N, S, H, C = p["N"], p["S"], p["H"], p["Cmax"]
        assert p["ss"].shape == (N, S, H) and p["cand"].shape == (N, C, H), name
        assert p["lpj"].shape == (N, S + p["S_perm"]) and p["cand_lpj"].shape == (N, C), name
        assert ((p["counts"] >= 0) & (p["counts"] <= C)).all(), name
        for n in range(N):
            assert len({r.tobytes() for r in p["ss"][n]}) == S, (name, n)
        if p["S_perm"]:  # the permanent all-zero state is not part of K^n
            assert p["ss"].any(axis=-1).all(), name
        assert N == 1 or N % 4 == 3, name  # N = 1 or not a multiple of four (the last workgroup is partial)


def test_plants_are_what_they_claim(problems):
    seen = set()
    for name, p in problems.items():
        S, H, ss, cand = p["S"], p["H"], p["ss"], p["cand"]
        for kind, n, (c, info) in p["plants"]:
            seen.add(kind)
            surv = set(ep.survivors(p, n))
            row = cand[n, c] if kind != "all_dup_row" else None
            if kind == "dup_old_last_block":
                assert info >= 64 * ((S - 1) // 64) and np.array_equal(row, ss[n, info]), (name, n, c)
                assert c not in surv
            elif kind == "dup_cand_cross64":
                assert c >= 64 > info and np.array_equal(row, cand[n, info]) and c not in surv, (name, n, c)
            elif kind == "all_dup_row":
                assert c >= 2 and not ep.survivors(p, n), (name, n)
            elif kind == "zero_cand":
                assert not row.any(), (name, n, c)
                if p["S_perm"]:
                    assert c not in surv, (name, n, c)
            elif kind in ("dig_collision_old", "dig_collision_cand", "sat255_old"):
                other = ss[n, info] if kind != "dig_collision_cand" else cand[n, info]
                assert c in surv and not np.array_equal(row, other), (name, kind, n, c)
                assert np.array_equal(np.flatnonzero(row)[:4], np.flatnonzero(other)[:4]), (name, kind, n, c)
                if H <= ep.DIG_MAX_H:
                    assert ep.digest(row) == ep.digest(other), (name, kind, n, c)
                if kind == "sat255_old":
                    k1, k2 = int(row.sum()), int(other.sum())
                    assert k1 > 255 and k2 > 255 and k1 != k2, (name, n, c, k1, k2)
                else:
                    assert row.sum() == other.sum() >= ep.DIG_SLOTS + 1, (name, kind, n, c)
            elif kind == "boundary_latents":
                assert row[H - 1] and (H <= 63 or row[63]) and (H <= 64 or row[64]), (name, n, c)
            elif kind in ("dup_old", "dup_cand"):
                assert c not in surv, (name, kind, n, c)
            else:
                raise AssertionError(kind)
    assert seen >= {"dup_old_last_block", "dup_cand_cross64", "all_dup_row", "zero_cand", "dig_collision_old",
                    "dig_collision_cand", "sat255_old", "boundary_latents"}, seen
    # the zero candidate with S_perm 0 and with S_perm 1; counts 0, 1 and Cmax; the largest latent index with digests
    # (16383) and without (H = 16385)
    zp = {p["S_perm"] for p in problems.values() for k, _, _ in p["plants"] if k == "zero_cand"}
    assert zp == {0, 1}
    assert all({0, 1, p["Cmax"]} <= set(p["counts"].tolist()) for p in problems.values() if p["N"] >= 3)
    for name, H in (("s2c1p1", 16384), ("s2c4p0_h16385", 16385)):
        p = problems[name]
        assert p["H"] == H and any(k == "boundary_latents" for k, _, _ in p["plants"]), name
        assert p["cand"][..., H - 1].any() and p["ss"][..., H - 1].any(), name
    assert ep.digest(np.eye(16384, dtype=bool)[16383]) == 1 | (16383 << 8)


def test_bit_parity_values_are_pairwise_distinct(problems):
    """The synthetic values of the non-tie cases: per row, the old values and the surviving candidates' values are
    pairwise distinct (the oracle breaks ties by NumPy's partition order)."""
    for name, p in problems.items():
        if p["ties"] or p["data"]:  # (data problems: asserted on the oracle's values in the GPU module)
            continue
        for n in range(p["N"]):
            v = np.concatenate([p["lpj"][n, p["S_perm"]:], p["cand_lpj"][n, ep.survivors(p, n)]])
            assert np.unique(v).size == v.size, (name, n)


def test_restated_rule_agrees_with_the_oracle_without_ties(problems):
    for name, p in problems.items():
        if p["ties"] or p["data"]:
            continue
        for Mp in ep.mprimes(p["S"]):
            w_ss, w_lpj, nu, ns = ep.oracle_select(p, Mp)
            tu = ts = 0
            for n in range(p["N"]):
                c = int(p["counts"][n])
                r_ss, r_lpj, u, s = ep.select_rule(p["ss"][n], p["lpj"][n, p["S_perm"]:], p["cand"][n, :c],
                                                   p["cand_lpj"][n, :c], c, Mp, p["S_perm"])
                assert np.array_equal(r_ss, w_ss[n]) and np.array_equal(r_lpj, w_lpj[n, p["S_perm"]:]), (name, Mp, n)
                tu += u
                ts += s
            assert (tu, ts) == (nu, ns), (name, Mp)


def test_planted_non_duplicates_are_accepted_somewhere(problems):
    """The digest-collision, saturated-count and zero (S_perm = 0, fresh) candidates rank above every old state: at
    Mprime = S the oracle accepts each one that survives, so a kernel that dropped one changes K^n, not only a count."""
    n_acc = 0
    for name, p in problems.items():
        if p["ties"] or p["data"]:
            continue
        w_ss, _, _, _ = ep.oracle_select(p, p["S"])
        for kind, n, (c, _) in p["plants"]:
            if kind in ("dig_collision_old", "dig_collision_cand", "sat255_old"):
                assert (w_ss[n] == p["cand"][n, c]).all(axis=1).any(), (name, kind, n, c)
                n_acc += 1
    assert n_acc >= 10


def test_tie_cases_tell_the_rule_from_its_wrong_variants(problems):
    """Each wrong variant of the rule (higher candidate index first among equal values; swap on equality) changes K^n
    or the lpj row of at least one datapoint of the tie cases, with digest-free arithmetic (restated rule only)."""
    for variant in ({"cand_tie": "high"}, {"strict": False}):
        differs = 0
        for name in ep.TIES:
            p = problems[name]
            for Mp in ep.mprimes(p["S"]):
                for n in range(p["N"]):
                    c = int(p["counts"][n])
                    args = (p["ss"][n], p["lpj"][n, p["S_perm"]:], p["cand"][n, :c], p["cand_lpj"][n, :c], c, Mp,
                            p["S_perm"])
                    a, b = ep.select_rule(*args), ep.select_rule(*args, **variant)
                    differs += not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
        assert differs >= 3, (variant, differs)


def test_vary_kn_ladder_matches_the_source():
    """with_spl / with_cpl are the one place that maps S and Cmax to the <SPL, CPL> of vary_kn_kernel; the selection,
    the randflip and the fused launch and the fused plan all go through them."""
    hip = _src("evo_amd.hip")

    def ladder(name, arg):
        body = hip[hip.index("static void %s(int %s, F &&f) {" % (name, arg)):]
        body = body[:body.index("\n}\n")]
        rows = re.findall(r"if \(%s <= (\d+)\) f\(std::integral_constant<int, (\d+)>\{\}\);" % arg, body)
        last = re.search(r"\n  else f\(std::integral_constant<int, (\d+)>\{\}\);", body)
        assert last and body.count("integral_constant") == len(rows) + 1, body
        return [(int(lim), int(v)) for lim, v in rows], int(last.group(1))

    s_rows, s_last = ladder("with_spl", "S")
    c_rows, c_last = ladder("with_cpl", "Cmax")
    assert len(s_rows) == 4 and c_rows == [(64, 1)], (s_rows, c_rows)
    for lim, spl in s_rows:
        assert ep.vk_instantiation(lim, 64) == (spl, 1) and ep.vk_instantiation(lim, 65) == (spl, c_last)
        assert ep.vk_instantiation(lim + 1, 1)[0] > spl
    assert ep.vk_instantiation(1024, 64) == (s_last, 1)
    assert ep.vk_instantiation(513, 256) == (s_last, c_last)
    kc = _src("kernels_common.hpp")
    assert _define(kc, "VK_MAX_S_PER_LANE") == ep.VK_MAX_S_PER_LANE and _define(kc, "VK_MAX_C_PER_LANE") == ep.VK_MAX_C_PER_LANE
    # nobody maps S or Cmax on the side: every launch of the three kernels takes its template arguments from them
    assert "vary_kn_kernel<decltype(spl)::value, decltype(cpl)::value><<<" in hip
    assert "evolve_randflip_kernel<decltype(spl)::value><<<" in hip
    assert hip.count("sssc_estep_fused_kernel<decltype(spl)::value, ") == 2 == len(re.findall(r"sssc_estep_fused_kernel<[^>]*><<<", hip))
    assert hip.count("vary_kn_kernel<") == 1 == hip.count("evolve_randflip_kernel<")
    # the fused E-step sizes its rows with the same ladder
    assert "with_spl(c->S, [&](auto spl) { p.spl = decltype(spl)::value; });" in hip
    assert "st.lds_wave_bytes = fused_lds_wave_bytes(p.spl, st.kc_big);" in hip


def test_gram2_rule_matches_the_source():
    hip = _src("evo_amd.hip")
    body = hip[hip.index("static int launch_bsc_lpj("):]
    body = body[:body.index("\n}\n")]
    for line in ("if (!c->bsc_direct && b.tag != 2 && !b.mask) {",
                 "const int rows_cap = 512 / b.C + 2;",
                 "const size_t lds = (size_t)rows_cap * c->H * sizeof(double);",
                 "const bool hw_ok = c->HW == 1 || c->HW == 2 || c->HW == 4 || c->HW == 8 || c->HW == 16;",
                 "if (!b.shared && (hw_ok || dg) && (c->H % 2) == 0 && lds <= 40 * 1024) {"):
        assert line in body, line
    assert "return states == c->states ? c->dig : states == c->cand ? c->cand_dig : nullptr;" in hip
    assert "if (!c->use_digest) return nullptr;" in hip
    # Cmax = 1: every H >= 10 goes to the other kernel
    assert ep.gram2_eligible(8, 1) and not any(ep.gram2_eligible(H, 1) for H in range(10, 200, 2))


def test_digest_layout_matches_the_source():
    cm = _src("common.hpp")
    assert _define(cm, "DIG_IDX_BITS") == ep.DIG_IDX_BITS and _define(cm, "DIG_SLOTS") == ep.DIG_SLOTS
    assert "#define DIG_MAX_H (1 << DIG_IDX_BITS)" in cm
    assert "if (k < DIG_SLOTS) d |= (u64)h << (8 + DIG_IDX_BITS * k);" in cm
    assert "return d | (u64)(k < 255 ? k : 255);" in cm
    assert "if (H <= DIG_MAX_H) {" in _src("evo_amd.hip")
    st = np.zeros(300, dtype=bool)
    st[[3, 64, 100, 299]] = True
    assert ep.digest(st) == 4 | (3 << 8) | (64 << 22) | (100 << 36) | (299 << 50)
    st[5:270] = True
    assert ep.digest(st) & 0xFF == 255


def test_fused_plan_matches_the_source_and_never_halves():
    """estep_plan restated: at every S <= 1024 and every H the fused E-step admits, neither the halving of W nor
    the kc_big shrink of the second launch fires and the REQUIRE on the LDS cannot refuse.  At S = 1024 the second
    launch (kc_big = 64) sits 64 bytes under the limit -- the case test_gpu_estep_paths runs."""
    hip = _src("evo_amd.hip")
    for line in ("const size_t tab = (size_t)4 * c->H * sizeof(double);",
                 "st.W = stage == 0 ? 4 : 1;",
                 "st.kc_big = stage == 0 ? 16 : SSSC_KCAP;",
                 "auto lds_of = [&](int w) { return (stage == 0 ? tab : 0) + (size_t)w * st.lds_wave_bytes; };",
                 "while (stage == 1 && lds_of(1) > FUSED_LDS_MAX && st.kc_big > 16) {",
                 "while (st.W > 1 && lds_of(st.W) > FUSED_LDS_MAX) st.W >>= 1;",
                 'REQUIRE(st.lds <= FUSED_LDS_MAX, "fused E-step: S too large for the LDS rows");',
                 "f.stage_d1 = stage == 0;"):
        assert line in hip, line
    assert "#define FUSED_LDS_MAX (150 * 1024)" in hip and ep.FUSED_LDS_MAX == 150 * 1024
    kf = _src("kernels_fused.hpp")
    body = kf[kf.index("inline int fused_lds_wave_bytes("):]
    body = body[:body.index("\n}\n")]
    terms = re.findall(r"b \+?= ([^;]+);", body)
    assert terms == ["SPL * 64 * 8 * 2", "64 * 8 * 3", "64 * 2 * 2", "64 * 4 * 3", "32 * 4", "(16 * 8 + 16) * 4",
                     "(4 * kc_big * kc_big + 5 * kc_big) * 8 + ((kc_big * 4 + 7) / 8) * 8"], terms
    assert _define(_src("kernels_sssc.hpp"), "SSSC_KCAP") == ep.SSSC_KCAP
    for S in range(1, 1025):
        for H in (2, 64, 256, 512, 1024):
            for st in ep.fused_launch_plan(S, H):
                assert st["halvings"] == 0 and st["shrinks"] == 0 and st["lds"] <= ep.FUSED_LDS_MAX, (S, H, st)
    assert ep.fused_launch_plan(1024, 64)[1]["lds"] == ep.FUSED_LDS_MAX - 64


def test_every_instantiation_dedup_and_s_perm_is_reached():
    """Every selection case runs with state_digest 1 and 0; H > DIG_MAX_H has no digests.  Together: all 40
    <SPL, CPL> x {digest, word} x S_perm combinations."""
    reached = set()
    for name, (model, N, D, H, S, S_perm, Cmax, data, seed) in ep.SELECTION.items():
        assert 1 <= S <= 64 * ep.VK_MAX_S_PER_LANE and 1 <= Cmax <= 64 * ep.VK_MAX_C_PER_LANE, name
        for d in (1, 0):
            reached.add(ep.vk_instantiation(S, Cmax) + ("digest" if ep.uses_digests(H, d) else "word", S_perm))
    want = {(s, c, dd, sp) for s in (1, 2, 4, 8, 16) for c in (1, 4) for dd in ("digest", "word") for sp in (0, 1)}
    assert reached == want, sorted(want - reached)
    # the row statistics are compared after S_perm = 1 and after SPL 8 and 16
    data = [v for v in ep.SELECTION.values() if v[7]]
    assert {v[5] for v in data} == {0, 1}
    assert {8, 16} <= {ep.vk_instantiation(v[4], v[6])[0] for v in data}
    assert {4} <= {ep.vk_instantiation(v[4], v[6])[1] for v in data}


def test_candidate_lpj_cases_take_the_routes_they_name():
    routes = {}
    for name, (model, N, D, H, Cmax, opts, seed, ks) in ep.CAND_LPJ.items():
        if model == "bsc":
            routes[name] = ep.gram2_eligible(H, Cmax, opts.get("state_digest", 1), opts.get("bsc_direct", 0))
    assert routes == {"bsc_h_odd": False, "bsc_hw3_nodigest": False, "bsc_hw3_digest": True, "bsc_c1_h10": False,
                      "bsc_c1_h8": True, "bsc_direct": False, "bsc_h1": False, "bsc_h2": True}  # (H = 1 is odd)
    for name, H, ks in (("es_h1", 1, {0, 1}), ("es_h2", 2, {0, 1, 2}), ("es_h3_nodigest", 3, {0, 1, 2, 3})):
        p = ep.make_cand_problem(name)
        k = p["cand"].sum(axis=-1)
        valid = np.arange(p["Cmax"])[None, :] < p["counts"][:, None]
        assert p["H"] == H and set(k[valid].tolist()) == ks, name  # every state size the space has, all-on included
        assert p["counts"].min() < p["Cmax"] == p["counts"][0], name
        assert H * (H - 1) // 2 == {1: 0, 2: 1, 3: 3}[H]  # pairs of latents
    assert ep.uses_digests(3, 0) is False
    for name, H in (("bsc_h1", 1), ("bsc_h2", 2)):
        p = ep.make_cand_problem(name)
        k = p["cand"].sum(axis=-1)
        assert p["H"] == H and set(k[np.arange(p["Cmax"])[None, :] < p["counts"][:, None]].tolist()) == set(range(H + 1)), name
    assert (ep.CAND_LPJ["bsc_h_odd"][3] % 2, (ep.CAND_LPJ["bsc_hw3_nodigest"][3] + 63) // 64) == (1, 3)
    for name in ("es_mixed_k", "es_mixed_k_nodigest"):
        p = ep.make_cand_problem(name)
        k = p["cand"].sum(axis=-1)
        # one datapoint mixes every chain level: k <= 2, 3..4, 5..8, above 8, above 64
        assert set(k[0, :p["counts"][0]].tolist()) >= {0, 1, 2, 3, 4, 5, 8, 9, 64, 65}, name
        assert p["counts"].min() < p["Cmax"] == p["counts"][0], name


def test_device_flow_and_fused_cases_fit_the_operators():
    for name, (N, D, H, S, npar, nch, Mp, seed) in ep.DEVICE_FLOW.items():
        assert npar * nch > 64 and npar * nch <= 64 * ep.VK_MAX_C_PER_LANE and npar <= 64 and nch <= 8, name
        assert 1 <= Mp <= S
    assert {v[3] for v in ep.DEVICE_FLOW.values()} == {257, 513, 1024}
    for name, (N, D, H, S, npar, nch, Mp, dense, seed) in ep.FUSED.items():
        # fused_shape_ok: H even, at most 1024, children per datapoint at most 64, B rows in MAIN_LPJ_LDS_MAX
        assert H % 2 == 0 and 2 <= H <= 1024 and npar * nch <= 64 and npar <= min(S, 64) and nch <= 8, name
        assert ((1024 // S + 2) * H + (4 * H if H <= 512 else 0)) * 8 <= 48 * 1024, name
    assert {v[3] for v in ep.FUSED.values()} >= {65, 257, 513, 1024}
    assert any(v[7] for v in ep.FUSED.values())
    for name, (N, D, H, S, npar, nch, Mp, seed) in ep.SPL_FLOW.items():
        assert H % 2 == 0 and npar * nch <= 64 and npar <= min(S, 64) and nch <= 8 and 1 <= Mp <= S, name
        assert ((1024 // S + 2) * H + 4 * H) * 8 <= 48 * 1024, name
    assert sorted(ep.vk_instantiation(v[3], v[4] * v[5]) for v in ep.SPL_FLOW.values()) == [(s, 1) for s in (1, 2, 4, 8, 16)]
    hip = _src("evo_amd.hip")
    assert "#define MAIN_LPJ_LDS_MAX (48 * 1024)" in hip
    assert "((size_t)(1024 / c->S + 2) * c->H + (c->H <= 512 ? (size_t)4 * c->H : 0)) * sizeof(double) <= MAIN_LPJ_LDS_MAX;" in hip

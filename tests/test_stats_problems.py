"""CPU checks of the synthetic statistics-pass problems (tests/_stats_problems.py) that test_gpu_stats_paths.py runs: the
generator yields what each profile claims, the Python restatement of the pair-bin geometry matches the source, every
case labelled "overflow" overflows a bin region by pigeonhole, and every producer launch that appends to the pair bins
has its grid checked against the regions per bin."""
import os
import re

import numpy as np
import pytest

import _stats_problems as sp


def _src(name):
    with open(os.path.join(sp.CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope="module")
def problems():
    return {name: sp.make_problem(name) for name in sp.PROBLEMS}


def test_rows_are_distinct_and_hold_an_all_zero_state(problems):
    for name, p in problems.items():
        ss = p["ss"]
        assert ss.shape == (p["N"], p["S"], p["H"]), name
        for n in range(p["N"]):
            assert len({row.tobytes() for row in ss[n]}) == p["S"], (name, n)
        assert not ss.any(axis=-1).all(), name + ": no all-zero state"


def test_profiles_give_the_levels_they_claim(problems):
    for name, p in problems.items():
        k = sp.level_census(p["ss"]).ravel()
        prof, H = p["profile"], p["H"]
        if prof == "sparse":
            assert (k <= 2).mean() >= 0.8 and k.max() <= 4, name
        elif prof == "mid":
            for lo, hi in ((0, 2), (3, 4), (5, 8), (9, 12)):
                assert ((k >= lo) & (k <= hi)).mean() > 0.02, (name, lo, hi)
        elif prof == "dense":
            assert ((k >= 5) & (k <= 8)).mean() >= 0.9, name
        elif prof == "few4":
            above = int((k > 4).sum())
            assert 0 < above <= sp.FEW4_EXTRA < 100 and k.max() <= 8, (name, above)
        elif prof == "wide":
            for lo, hi in ((9, 16), (17, 64)) + (((65, H),) if H > 64 else ()):
                assert ((k >= lo) & (k <= hi)).any(), (name, lo, hi)
        elif prof == "k34":
            assert np.isin(k, (0, 3, 4)).all() and ((k == 3) | (k == 4)).mean() > 0.95, name
        else:
            raise AssertionError("unknown profile " + prof)


def test_problems_spread_over_the_shapes_of_the_issue():
    Hs = {v[4] for v in sp.PROBLEMS.values()}
    Ss = {v[5] for v in sp.PROBLEMS.values()}
    assert {2, 3, 63, 64, 65, 129, 512, 1024} <= Hs
    assert {1, 37, 64, 65, 200, 256, 300} <= Ss
    assert all(v[2] % 2 == 1 for v in sp.PROBLEMS.values())  # odd N
    assert {v[3] % 2 for v in sp.PROBLEMS.values()} == {0, 1}


def test_pair_bin_constants_match_the_source():
    pbh = _src("pair_bins.hpp")
    assert _define(pbh, "PB_TILE") == sp.PB_TILE
    assert _define(pbh, "PB_MAX_BINS") == sp.PB_MAX_BINS
    assert _define(_src("kernels_bsc.hpp"), "BSC_KR") == sp.BSC_KR
    hip = _src("evo_amd.hip")
    assert re.search(r"\bint bins_scale = %d;" % sp.PAIR_BINS_SCALE, hip)
    assert re.search(r"\bint bins_nwg = %d;" % sp.PAIR_BINS_NWG, hip)


def test_pair_bin_geometry_restates_alloc_pair_bins():
    hip = _src("evo_amd.hip")
    body = hip[hip.index("static int alloc_pair_bins("):]
    body = body[:body.index("\n}\n")]
    # the expressions pair_bins_geometry() restates, as they stand in the source
    for line in ("pb.rf = std::max(1, PB_TILE / (2 * H));",
                 "const int nfold = (H - 1 + 1) / 2;",
                 "pb.nb = (int)cdiv(nfold, pb.rf);",
                 "pb.nwg = c->bins_nwg;",
                 "pb.cap = (int)std::max<i64>(64, (i64)scale * cdiv((i64)N * S, (i64)pb.nb * pb.nwg));",
                 "const size_t ne = (size_t)pb.nb * pb.nwg * pb.cap;"):
        assert line in body, line
    assert "if (H >= 2 && H <= 1024)" in body
    # the arithmetic itself, written out once more
    for H in (2, 3, 63, 64, 65, 129, 512, 1024):
        for N, S, scale, nwg in ((255, 64, 3, 2048), (257, 64, 1, 256), (9, 37, 64, 768)):
            g = sp.pair_bins_geometry(N, H, S, scale, nwg)
            rf = max(1, 4096 // (2 * H))
            nb = (H // 2 + rf - 1) // rf
            assert (g["rf"], g["nb"]) == (rf, nb)
            assert g["cap"] == max(64, scale * ((N * S + nb * nwg - 1) // (nb * nwg)))
            assert 1 <= g["nb"] <= sp.PB_MAX_BINS and 2 * g["rf"] * H <= sp.PB_TILE + 2 * H
    assert sp.pair_bins_geometry(1, 64, 1)["nb"] == 1
    assert sp.pair_bins_geometry(1, 512, 1)["nb"] == 64
    assert sp.pair_bins_geometry(1, 1024, 1)["nb"] == sp.PB_MAX_BINS


def test_options_of_the_cases_exist():
    hip = _src("evo_amd.hip")
    names = set(re.findall(r'^    \{"(\w+)", OPT_', hip, re.M))  # the rows of the option table
    used = {k for c in sp.CASES for k in c[2]} | set(sp.DEFAULTS) | {"debug_fail_stats", "debug_poison_list"}
    assert used <= names, used - names
    assert set(sp.CONFIGURE_OPTIONS) <= names
    for c in sp.CASES:
        assert set(c[2]) <= set(sp.DEFAULTS), c[0]
        assert c[1] in sp.PROBLEMS and c[3] in ("once", "twice"), c[0]
    for c in sp.DEVICE_CASES:
        assert set(c[2]) <= set(sp.DEFAULTS) and c[1] in sp.PROBLEMS, c[0]
    ids = [c[0] for c in sp.CASES + sp.DEVICE_CASES]
    assert len(set(ids)) == len(ids)


def test_device_cases_meet_the_merged_route_conditions(problems):
    """The census of the first pass (over the uploaded K^n) is what the pass under test decides from: few_above4 for the
    census cases, few_dense_states for the chains; and the 5..8 level is not empty, so merge_small_levels = 0 launches it."""
    CMAX = sp.CMAX
    n_parents, n_children, _ = sp.EVOLVE
    assert n_parents * n_children <= CMAX
    for cid, name, opts, k58 in sp.DEVICE_CASES:
        p = problems[name]
        k = sp.level_census(p["ss"])
        assert ((k >= 5) & (k <= 8)).any(), cid
        if opts.get("census_lists", 1):
            assert sp.few_above4(p["ss"], p["S"], CMAX), cid
        else:
            assert sp.few_dense_states(p["ss"], p["S"], CMAX), cid


def test_overflow_cases_overflow_by_pigeonhole(problems):
    """More bin entries than nb x nwg x cap: at least one region of one bin is full and its producer falls back to the
    global atomics."""
    n = 0
    for cid, name, opts, flow, overflow in sp.CASES:
        if not overflow:
            continue
        n += 1
        p = problems[name]
        assert opts.get("pair_bins") == 2, cid
        g = sp.pair_bins_geometry(p["N"], p["H"], p["S"], opts.get("pair_bins_scale", sp.PAIR_BINS_SCALE),
                                  opts.get("pair_bins_nwg", sp.PAIR_BINS_NWG))
        entries = sp.bin_entries(p["ss"], p["algo"])
        assert entries > 2 * g["capacity"], (cid, entries, g)  # margin: states with q = 0 append nothing
        if opts.get("pair_bins_auto", 1) and p["algo"] == "es3c":
            g2 = sp.pair_bins_geometry(p["N"], p["H"], p["S"], sp.recut_scale(p["ss"]), g["nwg"])
            assert g2["capacity"] > entries, (cid, entries, g2)
    assert n >= 4
    # the EBSC overflow problem: N S >= 16384 nb with nwg = 256 (cap = 64 entries per region at least)
    p = problems["bsc_k34"]
    assert p["N"] * p["S"] >= 16384 * sp.pair_bins_geometry(p["N"], p["H"], p["S"])["nb"]
    # the chains cases of the first suspected bug: N S >= 131072, so the K = 4 level's grid (N S / 256) exceeds 256
    p = problems["es_chains_big"]
    assert p["N"] * p["S"] >= 131072


def _launches(text):
    """(kernel, grid expression, argument text, offset) of every <<<...>>> launch."""
    out = []
    for m in re.finditer(r"(\w+)(?:<[^<>;]*>)?<<<", text):
        i = m.end()
        depth, j = 0, i
        while not (depth == 0 and text[j] == ","):
            depth += text[j] in "([{"
            depth -= text[j] in ")]}"
            j += 1
        grid = text[i:j].strip()
        k = text.index(">>>(", j) + 4
        depth, e = 1, k
        while depth:
            depth += text[e] == "("
            depth -= text[e] == ")"
            e += 1
        out.append((m.group(1), grid, text[k:e - 1], m.start()))
    return out


def test_every_binned_producer_launch_has_its_grid_checked():
    """A producer that appends to the pair bins owns region blockIdx.x of every bin: its grid must be clamped to pb.nwg
    and checked on the host (PB_GRID_CHECK) right before the launch."""
    hip = _src("evo_amd.hip")
    consumers = {"pair_bins_reduce_kernel", "sssc_finish_kernel", "bsc_finish_kernel"}
    n = 0
    for kern, grid, args, at in _launches(hip):
        pbs = re.findall(r"\b(pb|bsc_pb)\b", args)
        if not pbs or kern in consumers:
            continue
        n += 1
        assert re.fullmatch(r"\w+", grid), (kern, grid)
        before = hip[:at].splitlines()[-45:]
        assert any(re.search(r"PB_GRID_CHECK\(%s, %s\)" % (pbs[0], grid), l) for l in before), (kern, grid)
    assert n >= 11, n

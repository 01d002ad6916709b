"""CPU checks of the dense-kernel case table (tests/_dense_problems.py) that test_gpu_dense.py runs: the constants of the
restated dispatch are the ones in the sources, every route is reached by at least two cases on a device of 256 compute
units, the cases that claim an edge (empty K chunks, a dropped sym_row0, the scalar fallback of a misaligned base) have
it, and no operand is larger than the suite's limit."""
import os
import re

import numpy as np
import pytest

import _dense_problems as dp


def _src(name):
    with open(os.path.join(dp.CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def _body(text, head):
    body = text[text.index(head):]
    return body[:body.index("\n}\n")]


def test_constants_match_the_sources():
    g = _src("gemm_f64.hpp")
    assert (_define(g, "GEMM_T"), _define(g, "GEMM_BM"), _define(g, "GEMM_BK")) == (dp.GEMM_T, dp.GEMM_BM, dp.GEMM_BK)
    assert "constexpr int MAXW = %d;" % dp.MAXW in g
    hip = _src("evo_amd.hip")
    tn = _body(hip, "static int launch_gemm_tn(evoamd_ctx *c, const double *A")
    assert "const bool big = vec && !deterministic && K >= %d && M >= %d && Nc >= %d &&" % (dp.BIG_K, dp.BIG_MN, dp.BIG_MN) in tn
    assert "(sym_row0 < 0 || (sym_row0 % GEMM_T) == 0);" in tn
    assert "const int T = big ? GEMM_T : GEMM_BM;" in tn
    assert "if (K >= %d && !deterministic) {" % dp.SPLIT_MIN_K in tn
    assert "splits = (%d + tiles - 1) / tiles;" % dp.SPLIT_WG in tn
    assert "const i64 maxs = (K + %d) / %d;" % (dp.SPLIT_ROWS - 1, dp.SPLIT_ROWS) in tn
    assert "if (pc > 1 && K / (8 * pc) < %d) break;" % dp.CHUNK_FLOOR in tn
    assert "if (real > 24 && K / 64 >= 384) per_xcd = 8;" in tn
    assert "if (accumulate && splits < 8) splits = 8;" in tn
    assert "const unsigned wpx = (unsigned)std::max(1, 2 * c->n_cu / 8 - o.spare);" in tn
    fill = "J >= 2 && real * J * 100 >= (i64)8 * wpx * %d && K / J >= %d;" % (dp.FILL_PCT, dp.GROUP_MIN_K)
    assert fill in tn
    f32 = _body(hip, "static int launch_gemm_tn_f32(")
    assert fill in f32
    assert ("if (M >= %d && Nc >= %d && K >= %d && (M %% 4) == 0 && (Nc %% 4) == 0 && gemm_vec_ok_f32(A, lda) && "
            "gemm_vec_ok_f32(B, ldb)) {" % (dp.F32_MN, dp.F32_MN, dp.F32_K)) in f32
    rows32 = _body(hip, "static void launch_rows_f32(")
    assert ("if (Nc >= %d && M >= %d && (Nc %% 4) == 0 && gemm_vec_ok_f32(At, ldat) && gemm_vec_ok_f32(B, ldb)) {"
            % (dp.F32_MN, dp.F32_MN)) in rows32
    assert "static bool gram_is_small(int M, i64 K) { return M <= %d && K <= %d; }" % (dp.GRAM_SMALL_M, dp.GRAM_SMALL_K) in hip
    assert "if (M <= %d && Nc <= %d && K <= %d) {" % ((dp.NN_SMALL,) * 3) in _body(hip, "static bool launch_gemm_nn_raw(")
    assert "*segmax = (int)(n_real / wpx) + 2;" in hip
    assert "static bool gemm_vec_ok(const double *p, int ld) { return (ld % 2) == 0 && ((uintptr_t)p % 16) == 0; }" in hip
    assert "static bool gemm_vec_ok_f32(const float *p, int ld) { return (ld % 4) == 0 && ((uintptr_t)p % 16) == 0; }" in hip
    # production and probe share the launchers: one launch site per kernel outside gemm_f64.hpp
    for kernel in ("gemm_tn128_rows_f64<<<", "gemm_tn128_store_f32<<<", "gemm_nn_naive_f32<<<", "gram_small_kernel<<<",
                   "gemm_nn_small_kernel<<<", "gemm_tn128_sk_f64<<<", "gemm_tn128_sk_f32<<<", "gemm_tn128_f64<<<",
                   "gemm_tn_naive_f32<<<", "colsum_f64<SQUARE><<<"):
        assert hip.count(kernel) == 1, kernel
    # the names of the route record are the header's, in order
    from evo_amd import _lib
    with open(os.path.join(dp.ROOT, "include", "evo_amd.h")) as f:
        hdr = f.read()
    routes = re.findall(r"^#define EVOAMD_ROUTE_([A-Z0-9_]+) (\d+)$", hdr, re.M)
    assert [(n.lower(), int(v)) for n, v in routes] == list(zip(_lib.DENSE_ROUTES, range(len(_lib.DENSE_ROUTES))))
    ops = re.findall(r"^#define EVOAMD_DENSE_([A-Z0-9_]+) (\d+)$", hdr, re.M)
    assert [(n.lower(), int(v)) for n, v in ops] == list(zip(_lib.DENSE_OPS, range(len(_lib.DENSE_OPS))))
    m = re.search(r"typedef struct evoamd_dense_desc \{(.*?)\} evoamd_dense_desc;", hdr, re.S)
    fields = re.findall(r"\b([a-zA-Z_0-9]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in _lib.DenseDesc._fields_], fields
    m = re.search(r"typedef struct evoamd_dense_route \{(.*?)\} evoamd_dense_route;", hdr, re.S)
    assert re.findall(r"\b([a-zA-Z_0-9]+)(?=[,;])", m.group(1)) == [n for n, _ in _lib.DenseRoute._fields_]


def test_every_route_is_reached_twice():
    hit = {r: [] for r in dp.ROUTES}
    for name, c in dp.CASES.items():
        hit[dp.route_key(dp.predict(c, 256))].append(name)
    for pair in dp.MIRROR_PAIRS.values():
        for c in pair:
            assert dp.route_key(dp.predict(c, 256)) in hit
    assert all(len(v) >= 2 for v in hit.values()), {r: v for r, v in hit.items() if len(v) < 2}
    # the names say where a case is meant to go
    prefixes = {"gram_": "gram_small", "s64_": "tn64_scalar", "v64_": "tn64_vec", "t128_split_": "tn128_split",
                "t128_sk_": "tn128_streamk+ws", "t128_atomic_": "tn128_streamk", "t128_grouped_": "tn128_grouped",
                "rows_f32_": None, "rows_": "rows", "nn_small_": "nn_small", "nn_vec_": "nn_vec", "nn_scalar_": "nn_scalar",
                "f32_sk_": "f32_streamk+ws", "f32_atomic_": "f32_streamk", "f32_grouped_": "f32_grouped",
                "f32_naive_": "f32_naive", "colsum": "colsum"}
    for name, c in dp.CASES.items():
        pre = next(p for p in prefixes if name.startswith(p))
        if prefixes[pre]:
            assert dp.route_key(dp.predict(c, 256)) == prefixes[pre], name
    for name in dp.ROUNDING:
        assert name in dp.CASES, name
    assert {dp.route_key(dp.predict(dp.CASES[n], 256)) for n in dp.ROUNDING} == set(dp.ROUTES)


def test_misaligned_variants_fall_back_to_the_scalar_routes():
    """A base one element off, or a leading dimension that is no whole number of 16-byte pieces, must not reach a kernel
    with 16-byte loads; the tight and the wide variant of the same shape do."""
    n_vec = 0
    for name, c in dp.CASES.items():
        if c["ld"] not in ("off", "odd") or c["op"] in ("colsum", "colsum_sq", "rows"):
            continue
        r = dp.predict(c, 256)["route"]
        assert r not in dp.VECTOR_ROUTES, (name, r)
        if r in dp.SCALAR_ROUTES:
            t = dp.predict(dict(c, ld="tight"), 256)["route"]
            w = dp.predict(dict(c, ld="wide"), 256)["route"]
            assert t == w, name
            n_vec += t in dp.VECTOR_ROUTES
    assert n_vec >= 8
    for route in dp.VECTOR_ROUTES | {"rows"}:  # each vector route tight and with padded rows
        lds = {c["ld"] for c in dp.CASES.values() if dp.predict(c, 256)["route"] == route}
        lds |= {c["ld"] for p in dp.MIRROR_PAIRS.values() for c in p if dp.predict(c, 256)["route"] == route}
        assert {"tight", "wide"} <= lds, (route, lds)


def test_cases_have_the_edges_they_claim():
    C = dp.CASES
    # accumulate at K = 40: eight chunks of one slab, five of them empty
    for name in ("s64_40_65_33_acc", "v64_40_66_34_acc"):
        assert dp.predict(C[name])["splits"] == 8 and dp.chunk_rows(C[name]) == (16, 5), name
    assert dp.chunk_rows(C["s64_200_65_3"]) == (32, 1) and dp.predict(C["s64_200_65_3"])["splits"] == 8
    assert dp.chunk_rows(C["s64_130_70_34_off"]) == (32, 3)
    # split and unsplit routes with a C that must be overwritten (NaN prefill) and with c_is_zero
    for want_split in (False, True):
        for c_zero in (False, True):
            assert any((dp.predict(c)["splits"] > 1) == want_split and c["c_zero"] == c_zero and not c["acc"]
                       for c in C.values() if c["op"] == "tn"), (want_split, c_zero)
    # a split product into a wider C (the 2-D clear)
    assert sum(1 for c in C.values() if c["op"] == "tn" and dp.predict(c)["splits"] > 1 and not c["acc"] and
               not c["c_zero"] and dp.layout(c)["ldc"] > c["Nc"]) >= 4
    # sym_row0: kept on a 64- and on a 128-tile route (with a partial symmetric tile), dropped where the tile does not divide it
    assert C["v64_129_130_66_sym64"]["Nc"] % 64 and C["t128_sk_8200_386_258_sym128"]["Nc"] % 128
    assert dp.real_tiles(386, 258, 128, 128) == 9
    for name in ("s64_129_99_66_symdrop", "v64_129_100_66_symdrop"):
        assert C[name]["sym"] % 64 and C[name]["sym"] + C[name]["Nc"] == C[name]["M"]
    assert dp.predict(C["v64_8192_320_256_sym64"])["route"] == "tn64_vec"
    # spare: grouped at wpx 4 with J = 8; nine real tiles stay on stream-K there; grouped without spare at K = 32768
    p = dp.predict(C["t128_grouped_8192_256_256_spare60"])
    assert (p["wpx"], p["J"], p["route"]) == (4, 8, "tn128_grouped")
    p = dp.predict(C["t128_sk_8200_386_258_sym128_spare60"])
    assert (p["wpx"], p["J"], p["route"]) == (4, 3, "tn128_streamk")
    p = dp.predict(C["t128_grouped_32768_256_256"])
    assert (p["wpx"], p["J"], p["route"]) == (64, 128, "tn128_grouped")
    assert dp.predict(C["t128_split_8192_256_256_perxcd4"])["splits"] == 32 != dp.predict(C["t128_split_8192_256_256"])["splits"]
    # the reduce kernel's table of slabs per XCD holds every workgroup that can touch a tile
    for name, c in C.items():
        p = dp.predict(c)
        if p["route"].endswith("streamk") and p["ws"]:
            real = dp.real_tiles(c["M"], c["Nc"], 128, c["sym"] if c["op"] == "tn" else -1)
            assert p["wpx"] // real + 2 <= dp.MAXW, name
    # K tails: 1, below a slab, an odd number of slabs, whole slab pairs
    ks = {c["K"] for c in C.values()}
    assert {1, 2, 5, 15, 16, 17, 32, 40, 72, 8192, 8200, 32768} <= ks
    # mirror pairs: same C layout, the first leaves the mirror to the second
    for a, b in dp.MIRROR_PAIRS.values():
        assert not a["mirror"] and b["mirror"] and a["acc"] and b["acc"]
        assert {k: v for k, v in dp.layout(a).items() if "c" in k} == {k: v for k, v in dp.layout(b).items() if "c" in k}
    a, b = dp.MIRROR_PAIRS["mirror_128_then_64"]
    assert (dp.predict(a)["tile"], dp.predict(b)["tile"]) == (128, 64)


def test_operands_are_small_exact_and_guarded():
    for name, c in list(dp.CASES.items()) + [(k, v) for k, p in dp.MIRROR_PAIRS.items() for v in p]:
        lay = dp.layout(c)
        g = lay["guard"]
        rows_a = c["M"] if c["op"] == "nn" else c["K"]
        assert g >= 1
        assert lay["off_a"] + (rows_a + 2 * g) * lay["lda"] <= dp.MAX_OPERAND, name
        assert lay["off_b"] + (c["K"] + 2 * g) * lay["ldb"] <= dp.MAX_OPERAND, name
        assert lay["off_c"] + (c["M"] + 2 * g) * lay["ldc"] <= dp.MAX_OPERAND, name
        assert 16 * c["K"] < 2 ** 24, name  # every partial sum of the integer pass is exact in float32 too
    for name in ("v64_129_130_66_sym64_wide", "rows_f32_32_130_132_off", "nn_small_70_130_67_ct_wide", "colsum_sq_5_63"):
        c = dp.CASES[name]
        ops = dp.operands(c, 1)
        lay = ops["lay"]
        assert np.abs(ops["A"]).max() <= 4 and (ops["A"] == np.rint(ops["A"])).all()
        rows_a, cols_a = ops["A"].shape
        assert np.array_equal(dp.inner(ops["bufA"], rows_a, cols_a, lay["lda"], lay["off_a"], lay["guard"]), ops["A"])
        assert np.isnan(ops["bufA"]).sum() == ops["bufA"].size - ops["A"].size
        rows_c, cols_c = ops["C0"].shape
        outside = ops["bufC"].copy()
        dp.inner(outside, rows_c, cols_c, lay["ldc"], lay["off_c"], lay["guard"])[:] = 0
        assert np.count_nonzero(outside) == outside.size - rows_c * cols_c and not np.isnan(outside).any()
        if c["sym"] >= 0:
            assert np.array_equal(ops["A"][:, c["sym"]:], ops["B"])
            ref = dp.reference(c, ops)[c["sym"]:]
            assert np.array_equal(ref, ref.T)

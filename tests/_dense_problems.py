"""Dense-kernel cases for test_gpu_dense.py (and their CPU checks in test_dense_problems.py).

A case is one call of the test-only ``Engine.dense_probe``: an op, a shape (K, M, Nc), a stride / alignment variant, the
GemmTnOpts flags and the context options it runs under.  ``predict`` restates the dispatch of launch_gemm_tn,
launch_gemm_tn_f32, launch_gemm_nn_raw and the B = Y W helpers (evo_amd.hip) as a function of the case and the device's
compute units, so that every case names the kernel it is meant to reach and a later retune of a threshold shows as a
route mismatch instead of silently moving the case.  ``operands`` builds the padded buffers: NaN around the logical A and
B, a sentinel around the logical C.

Stride variants (``ld``): "tight" ld = cols; "wide" ld = cols + 2 (+ 4 in float) and a wider C; "off" the base of A one
element into its buffer (8 or 4 bytes off 16-byte alignment), C one element in with ldc = cols + 3; "odd" ld = cols + 1
(cols + 2 in float: no multiple of 4).  The ROWS ops round lda up to a multiple of 4 first, as evoamd_configure does."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evo_amd", "csrc")

# gemm_f64.hpp
GEMM_BM = 64
GEMM_BK = 16
GEMM_T = 128
MAXW = 72
# evo_amd.hip (launch_gemm_tn / launch_gemm_tn_f32 / launch_gemm_nn_raw / gram_is_small)
BIG_K, BIG_MN = 8192, 256         # the 128-tile routes of the f64 contraction
F32_MN, F32_K = 128, 2048         # the matrix-core routes of the f32 contraction
FILL_PCT, GROUP_MIN_K = 93, 256   # grouped split-K: fill of the resident grid, rows of K per chunk
CHUNK_FLOOR = 512                 # split-K on 128-tiles: rows of K per chunk
GRAM_SMALL_M, GRAM_SMALL_K = 512, 4096
NN_SMALL = 1024
SPLIT_MIN_K, SPLIT_WG, SPLIT_ROWS = 128, 512, 64  # 64-tile split: from this K on, this many workgroups, >= rows per chunk

MAX_OPERAND = 32768 * 512  # elements of one operand, padding included
GUARD = 2                  # guard rows in front of and behind every operand
SENTINEL = -7.25e77        # C outside its logical region
OPTIONS = {"gemm_streamk": 1, "gemm_workspace": 1, "gemm_grouped": 1, "gemm_per_xcd": 0}

F32_OPS = ("tn_f32", "rows_f32")
VECTOR_ROUTES = {"tn64_vec", "tn128_split", "tn128_streamk", "tn128_grouped", "f32_streamk", "f32_grouped", "nn_vec",
                 "rows_f32_store"}
SCALAR_ROUTES = {"tn64_scalar", "f32_naive", "nn_scalar", "rows_f32_naive"}


def cdiv(a, b):
    return (a + b - 1) // b


def case(op, K, M, Nc, ld="tight", same=False, det=False, sym=-1, c_zero=False, acc=False, mirror=True, spare=0, diag=False,
         ct=False, opts=None, twice=False, asym=False):
    return dict(op=op, K=K, M=M, Nc=Nc, ld=ld, same=same, det=det, sym=sym, c_zero=c_zero, acc=acc, mirror=mirror,
                spare=spare, diag=diag, ct=ct, opts=dict(opts or {}), twice=twice, asym=asym)


def layout(c):
    """Leading dimensions, base offsets and guard rows of a case (the keyword arguments of Engine.dense_probe)."""
    op, K, M, Nc, v = c["op"], c["K"], c["M"], c["Nc"], c["ld"]
    f32 = op in F32_OPS
    cols_a = K if op == "nn" else M
    cols_c = M if op.startswith("colsum") else Nc
    if op in ("rows", "rows_f32"):
        cols_a = cdiv(M, 4) * 4
    pad = {"tight": 0, "wide": 4 if f32 else 2, "off": 0, "odd": 2 if f32 else 1, "p3": 3}[v]
    lay = dict(lda=cols_a + pad, ldb=0 if op.startswith("colsum") or c["same"] else Nc + pad,
               ldc=cols_c + {"tight": 0, "wide": 2, "off": 3, "odd": 1, "p3": 0}[v], lda2=0, ldct=0,
               off_a=1 if v == "off" else 0, off_b=0, off_c=1 if v == "off" else 0, guard=GUARD)
    if op == "rows_f32":
        lay["lda2"] = K
    if c["ct"]:
        lay["ldct"] = M + pad
    return lay


def aligned(c, lay):
    """(A, B) bases on a 16-byte boundary?  (hipMalloc returns 256-byte aligned buffers.)"""
    n = 4 if c["op"] in F32_OPS else 2
    return (lay["off_a"] + lay["guard"] * lay["lda"]) % n == 0, (lay["off_b"] + lay["guard"] * lay["ldb"]) % n == 0


def real_tiles(M, Nc, T, sym):
    tiles = cdiv(Nc, T) * cdiv(M, T)
    if sym >= 0:
        ts = cdiv(Nc, T)
        tiles -= ts * (ts - 1) // 2
    return tiles


def _record(route, tile=0, splits=1, J=0, wpx=0, segmax=0, ws=0):
    return dict(route=route, tile=tile, splits=splits, J=J, wpx=wpx, segmax=segmax, ws=ws)


def _resident(real, K, n_cu, spare, o):
    """The stream-K / grouped choice both contractions share: (grouped, J, wpx, segmax, ws); segmax comes from the
    workspace helper, which is not called without the workspace."""
    wpx = max(1, 2 * n_cu // 8 - spare)
    segmax = real // wpx + 2
    ws = 1 if o["gemm_workspace"] else 0
    J = 8 * wpx // real
    grouped = bool(ws and o["gemm_grouped"] and J >= 2 and real * J * 100 >= 8 * wpx * FILL_PCT and K // J >= GROUP_MIN_K)
    return grouped, J, wpx, (segmax if ws else 0), ws


def predict(c, n_cu=256):
    """The route record the launcher writes for this case on a device of n_cu compute units."""
    op, K, M, Nc = c["op"], c["K"], c["M"], c["Nc"]
    o = dict(OPTIONS, **c["opts"])
    lay = layout(c)
    a_al, b_al = aligned(c, lay)
    lda, ldb = lay["lda"], (lay["lda"] if c["same"] else lay["ldb"])
    if c["same"]:
        b_al = a_al
    if op.startswith("colsum"):
        return _record("colsum", 64, cdiv(K, 256))
    if op == "rows":
        return _record("rows", GEMM_T)
    if op == "rows_f32":
        vec = Nc >= 128 and M >= 128 and Nc % 4 == 0 and lda % 4 == 0 and a_al and ldb % 4 == 0 and b_al
        return _record("rows_f32_store", GEMM_T) if vec else _record("rows_f32_naive")
    if op == "nn":
        if M <= NN_SMALL and Nc <= NN_SMALL and K <= NN_SMALL:
            return _record("nn_small", 16)
        vec = lda % 2 == 0 and a_al and ldb % 2 == 0 and b_al and K % 2 == 0 and Nc % 2 == 0 and K >= 2 and Nc >= 2
        return _record("nn_vec" if vec else "nn_scalar", GEMM_BM)
    if op == "tn_f32":
        if (M >= F32_MN and Nc >= F32_MN and K >= F32_K and M % 4 == 0 and Nc % 4 == 0 and lda % 4 == 0 and a_al
                and ldb % 4 == 0 and b_al):
            real = cdiv(Nc, GEMM_T) * cdiv(M, GEMM_T)
            grouped, J, wpx, segmax, ws = _resident(real, K, n_cu, c["spare"], o)
            return _record("f32_grouped" if grouped else "f32_streamk", GEMM_T, 8, J, wpx, segmax, ws)
        return _record("f32_naive")
    assert op == "tn", op
    det, sym, acc = c["det"], c["sym"], c["acc"]
    if det and c["same"] and M == Nc and sym < 0 and M <= GRAM_SMALL_M and K <= GRAM_SMALL_K:
        return _record("gram_small", 16)
    vec = lda % 2 == 0 and a_al and ldb % 2 == 0 and b_al and M % 2 == 0 and Nc % 2 == 0 and M >= 2 and Nc >= 2
    big = vec and not det and K >= BIG_K and M >= BIG_MN and Nc >= BIG_MN and (sym < 0 or sym % GEMM_T == 0)
    T = GEMM_T if big else GEMM_BM
    if sym >= 0 and sym % T:
        sym = -1
    tiles = cdiv(Nc, T) * cdiv(M, T)
    real = real_tiles(M, Nc, T, sym)
    splits = 1
    if K >= SPLIT_MIN_K and not det:
        if big:
            per_xcd, best = 1, 0.0
            for pc in range(1, 17):
                if pc > 1 and K // (8 * pc) < CHUNK_FLOOR:
                    break
                eff = (real * pc) / (64.0 * cdiv(real * pc, 64))
                if eff > best + 0.01:
                    best, per_xcd = eff, pc
            if real > 24 and K // 64 >= 384:
                per_xcd = 8
            if o["gemm_per_xcd"] > 0:
                per_xcd = o["gemm_per_xcd"]
            splits = 8 * per_xcd
        else:
            splits = cdiv(SPLIT_WG, tiles)
        splits = min(splits, cdiv(K, SPLIT_ROWS))
        if splits > 1:
            splits = cdiv(splits, 8) * 8
    if acc and splits < 8:
        splits = 8
    if big and splits > 1 and o["gemm_streamk"]:
        grouped, J, wpx, segmax, ws = _resident(real, K, n_cu, c["spare"], o)
        return _record("tn128_grouped" if grouped else "tn128_streamk", T, splits, J, wpx, segmax, ws)
    if big:
        return _record("tn128_split", T, splits)
    return _record("tn64_vec" if vec else "tn64_scalar", T, splits)


def chunk_rows(c, n_cu=256):
    """Rows of K per chunk of a split 64- or 128-tile launch (kps of launch_gemm_tn), and how many chunks are empty."""
    p = predict(c, n_cu)
    kps = cdiv(cdiv(c["K"], p["splits"]), GEMM_BK) * GEMM_BK
    return kps, sum(1 for z in range(p["splits"]) if z * kps >= c["K"])


# ---- the table -----------------------------------------------------------------------------------------------------
SPLITK = {"gemm_streamk": 0}
ATOMICS = {"gemm_workspace": 0}
NOGROUP = {"gemm_grouped": 0}
CASES = {}


def _add(name, *a, **kw):
    assert name not in CASES, name
    CASES[name] = case(*a, **kw)


# gram_small (K, M): one wave per 16 x 16 block, four waves over quarters of K
for _K, _M in ((1, 1), (3, 17), (16, 16), (67, 33), (130, 48)):
    _add("gram_%d_%d" % (_K, _M), "tn", _K, _M, _M, same=True, det=True, twice=True)
_add("gram_67_33_diag", "tn", 67, 33, 33, same=True, det=True, diag=True)
_add("gram_130_48_ld50_diag", "tn", 130, 48, 48, ld="wide", same=True, det=True, diag=True, twice=True)
_add("gram_130_48_off", "tn", 130, 48, 48, ld="off", same=True, det=True, diag=True)
_add("gram_67_33_odd", "tn", 67, 33, 33, ld="odd", same=True, det=True)
# 64-tile scalar loader
_add("s64_1_1_1", "tn", 1, 1, 1)
_add("s64_17_65_63", "tn", 17, 65, 63)
_add("s64_17_65_63_wide", "tn", 17, 65, 63, ld="wide")
_add("s64_130_70_34_off", "tn", 130, 70, 34, ld="off")          # split, K tail in the last non-empty chunk
_add("s64_130_70_34_odd", "tn", 130, 70, 34, ld="odd")
_add("s64_200_65_3", "tn", 200, 65, 3)                           # split, one empty chunk
_add("s64_200_65_3_czero", "tn", 200, 65, 3, c_zero=True, ld="wide")
_add("s64_40_65_33_acc", "tn", 40, 65, 33, acc=True)             # accumulate: 8 chunks of 16 rows, 3..7 empty
_add("s64_300_65_33_det", "tn", 300, 65, 33, det=True, twice=True)
_add("s64_129_99_66_symdrop", "tn", 129, 99, 66, sym=33)         # sym_row0 no multiple of the tile: dropped
# 64-tile 16-byte loader
_add("v64_2_2_2", "tn", 2, 2, 2)
_add("v64_15_66_62", "tn", 15, 66, 62)
_add("v64_15_66_62_wide", "tn", 15, 66, 62, ld="wide")
_add("v64_15_66_62_czero", "tn", 15, 66, 62, c_zero=True)
_add("v64_129_130_66_sym64", "tn", 129, 130, 66, sym=64)         # split; a partial symmetric tile, mirrored
_add("v64_129_130_66_sym64_wide", "tn", 129, 130, 66, sym=64, ld="wide")
_add("v64_300_66_66_det", "tn", 300, 66, 66, det=True, twice=True)   # unsplit: 19 slabs, interior loop and tail
_add("v64_512_128_64_det", "tn", 512, 128, 64, det=True)         # whole tiles, K a whole number of slabs
_add("v64_130_70_34", "tn", 130, 70, 34)
_add("v64_129_194_130_sym64_asym", "tn", 129, 194, 130, sym=64, asym=True)   # which elements the mirror writes
_add("v64_130_70_34_czero", "tn", 130, 70, 34, c_zero=True)
_add("v64_40_66_34_acc", "tn", 40, 66, 34, acc=True, ld="wide")
_add("v64_129_100_66_symdrop", "tn", 129, 100, 66, sym=34)
_add("v64_8192_320_256_sym64", "tn", 8192, 320, 256, sym=64)     # 64 is no multiple of 128: stays on 64-tiles, hint kept
# 128-tile routes: split-K, stream-K through the workspace, stream-K with atomics, grouped
for _tag, _K, _M, _Nc, _sym in (("8192_256_256", 8192, 256, 256, -1), ("8200_258_260", 8200, 258, 260, -1),
                                ("8200_386_258_sym128", 8200, 386, 258, 128)):
    _add("t128_split_" + _tag, "tn", _K, _M, _Nc, sym=_sym, opts=SPLITK)
    _add("t128_sk_" + _tag, "tn", _K, _M, _Nc, sym=_sym, twice=True)
    _add("t128_atomic_" + _tag, "tn", _K, _M, _Nc, sym=_sym, opts=ATOMICS)
_add("t128_grouped_8192_256_256_spare60", "tn", 8192, 256, 256, spare=60, twice=True)   # wpx 4, J 8
_add("t128_grouped_8200_258_260_spare55", "tn", 8200, 258, 260, spare=55, twice=True)             # wpx 9, 9 tiles x 8 chunks
_add("t128_grouped_8200_386_258_sym128_spare55", "tn", 8200, 386, 258, sym=128, spare=55)
_add("t128_sk_8200_386_258_sym128_spare60", "tn", 8200, 386, 258, sym=128, spare=60)    # nine real tiles: J 3 fills 27 of 32
_add("t128_grouped_32768_256_256", "tn", 32768, 256, 256)
_add("t128_sk_8200_386_258_sym128_asym", "tn", 8200, 386, 258, sym=128, asym=True)
_add("t128_sk_32768_256_256_nogroup", "tn", 32768, 256, 256, opts=NOGROUP)
for _r, _o in (("split", SPLITK), ("sk", {}), ("atomic", ATOMICS)):
    _add("t128_%s_8200_258_260_wide" % _r, "tn", 8200, 258, 260, ld="wide", opts=_o)
    _add("t128_%s_8192_256_256_acc" % _r, "tn", 8192, 256, 256, acc=True, opts=_o)
_add("t128_grouped_8200_258_260_spare55_wide", "tn", 8200, 258, 260, ld="wide", spare=55)
_add("t128_grouped_8192_256_256_spare60_acc", "tn", 8192, 256, 256, spare=60, acc=True)
_add("t128_split_8192_256_256_czero", "tn", 8192, 256, 256, c_zero=True, opts=SPLITK)
_add("t128_atomic_8200_258_260_czero_wide", "tn", 8200, 258, 260, c_zero=True, ld="wide", opts=ATOMICS)
_add("t128_split_8192_256_256_perxcd4", "tn", 8192, 256, 256, opts=dict(SPLITK, gemm_per_xcd=4))
_add("s64_8200_258_260_off", "tn", 8200, 258, 260, ld="off")     # the 128-tile shapes with a base off alignment
_add("s64_8192_256_256_odd", "tn", 8192, 256, 256, ld="odd")
# rows: whole K per 128-tile
for _K in (1, 5, 16, 32, 40, 72):
    _add("rows_%d_129_130" % _K, "rows", _K, 129, 130)
for _M in (128, 131, 258):
    for _Nc in (128, 130, 258):
        _add("rows_24_%d_%d" % (_M, _Nc), "rows", 24, _M, _Nc)
_add("rows_32_256_256", "rows", 32, 256, 256)                    # whole tiles, one slab pair: the mask-free drain alone
_add("rows_64_258_130_wide", "rows", 64, 258, 130, ld="wide")
_add("rows_24_1154_130", "rows", 24, 1154, 130)                  # 10 row tiles: the XCD decode wraps
# nn
_add("nn_small_1_1_1", "nn", 1, 1, 1, twice=True)
_add("nn_small_17_33_19", "nn", 17, 33, 19)
_add("nn_small_70_130_67_ct", "nn", 70, 130, 67, ct=True, twice=True)
_add("nn_small_70_130_67_ct_wide", "nn", 70, 130, 67, ct=True, ld="wide")
_add("nn_small_70_130_67_off", "nn", 70, 130, 67, ld="off")
_add("nn_vec_34_1030_66", "nn", 34, 1030, 66)
_add("nn_vec_34_1030_66_wide", "nn", 34, 1030, 66, ld="wide")
_add("nn_vec_64_1088_128", "nn", 64, 1088, 128)                  # whole tiles, four slabs: the mask-free drain
_add("nn_vec_96_1088_128", "nn", 96, 1088, 128)                  # interior loop, then the drain
_add("nn_vec_2_1025_2", "nn", 2, 1025, 2)
_add("nn_scalar_33_1030_66", "nn", 33, 1030, 66)
_add("nn_scalar_34_1030_66_off", "nn", 34, 1030, 66, ld="off")
_add("nn_scalar_34_1030_66_odd", "nn", 34, 1030, 66, ld="odd")
# f32
_add("f32_sk_2048_128_128", "tn_f32", 2048, 128, 128, twice=True)
_add("f32_sk_2056_132_260", "tn_f32", 2056, 132, 260, twice=True)
_add("f32_sk_2056_132_260_wide", "tn_f32", 2056, 132, 260, ld="wide")
_add("f32_atomic_2056_132_260", "tn_f32", 2056, 132, 260, opts=ATOMICS)
_add("f32_grouped_4096_128_128_spare62", "tn_f32", 4096, 128, 128, spare=62, twice=True)   # wpx 2, J 16
_add("f32_atomic_2048_128_128", "tn_f32", 2048, 128, 128, opts=ATOMICS)
_add("f32_sk_2056_260_256_spare63", "tn_f32", 2056, 260, 256, spare=63)                    # wpx 1: 6 tiles, J 1 -> stream-K
_add("f32_grouped_2048_256_256_spare63", "tn_f32", 2048, 256, 256, spare=63)               # wpx 1, 4 tiles x 2 chunks
_add("f32_grouped_2048_256_256_spare63_wide", "tn_f32", 2048, 256, 256, spare=63, ld="wide")
_add("f32_atomic_2056_132_260_wide", "tn_f32", 2056, 132, 260, ld="wide", opts=ATOMICS)
_add("f32_naive_100_30_20", "tn_f32", 100, 30, 20)
_add("f32_naive_2056_132_260_off", "tn_f32", 2056, 132, 260, ld="off")
_add("f32_naive_2056_132_260_odd", "tn_f32", 2056, 132, 260, ld="odd")
_add("f32_naive_2048_130_128", "tn_f32", 2048, 130, 128)
for _H in (128, 130, 132):
    for _N in (128, 130):
        for _D in (5, 32):
            _add("rows_f32_%d_%d_%d" % (_D, _N, _H), "rows_f32", _D, _N, _H)
_add("rows_f32_32_130_132_wide", "rows_f32", 32, 130, 132, ld="wide")
_add("rows_f32_32_130_132_off", "rows_f32", 32, 130, 132, ld="off")
_add("rows_f32_32_130_132_odd", "rows_f32", 32, 130, 132, ld="odd")
_add("rows_f32_5_100_30", "rows_f32", 5, 100, 30)
# colsum (R, Cn) with ldx = Cn + 3 into a prefilled out
for _R in (1, 5, 4097):
    for _Cn in (1, 63, 65, 130):
        for _op in ("colsum", "colsum_sq"):
            _add("%s_%d_%d" % (_op, _R, _Cn), _op, _R, _Cn, 1, ld="p3")
_add("colsum_300_65_tight", "colsum", 300, 65, 1)

# two accumulating calls over the two parts of K, the first without the mirror: (first, second) -- stats_contract_block
MIRROR_PAIRS = {
    "mirror_64": (case("tn", 150, 194, 130, sym=64, acc=True, mirror=False), case("tn", 150, 194, 130, sym=64, acc=True)),
    # a long chunk on 128-tiles, then a short last chunk on 64-tiles that mirrors
    "mirror_128_then_64": (case("tn", 8200, 386, 258, sym=128, acc=True, mirror=False, ld="wide"),
                           case("tn", 4100, 386, 258, sym=128, acc=True, ld="wide")),
}

# one Gaussian case per kernel for the rounding bound
ROUNDING = ["gram_130_48_ld50_diag", "s64_130_70_34_off", "v64_300_66_66_det", "v64_130_70_34", "t128_split_8200_258_260",
            "t128_sk_8200_258_260", "t128_atomic_8200_258_260", "t128_grouped_8200_258_260_spare55", "rows_40_129_130",
            "nn_small_70_130_67_ct", "nn_vec_34_1030_66", "nn_scalar_33_1030_66", "f32_sk_2056_132_260",
            "f32_atomic_2056_132_260", "f32_grouped_4096_128_128_spare62", "f32_naive_100_30_20", "rows_f32_32_130_132",
            "rows_f32_32_130_130", "colsum_4097_65", "colsum_sq_4097_65"]

# every route (and stream-K with and without its workspace) must be reached by at least two cases at 256 compute units
ROUTES = ["gram_small", "tn64_scalar", "tn64_vec", "tn128_split", "tn128_streamk+ws", "tn128_streamk", "tn128_grouped",
          "f32_streamk+ws", "f32_streamk", "f32_grouped", "f32_naive", "nn_small", "nn_vec", "nn_scalar", "rows",
          "rows_f32_store", "rows_f32_naive", "colsum"]


def route_key(p):
    return p["route"] + ("+ws" if p["route"].endswith("streamk") and p["ws"] else "")


# ---- operands ------------------------------------------------------------------------------------------------------
def padded(logical, ld, off, guard, fill):
    rows, cols = logical.shape
    buf = np.full(off + (rows + 2 * guard) * ld, fill, dtype=logical.dtype)
    buf[off:].reshape(rows + 2 * guard, ld)[guard:guard + rows, :cols] = logical
    return buf


def inner(buf, rows, cols, ld, off, guard):
    """The logical rows x cols of a padded buffer (a view)."""
    return buf[off:].reshape(rows + 2 * guard, ld)[guard:guard + rows, :cols]


def operands(c, seed, gaussian=False, zero_c=False):
    """Logical A, B (float64 values; exact small integers unless ``gaussian``) and the C prefill of a case, and the padded
    buffers Engine.dense_probe takes.  A and B carry NaN outside their logical region; C carries SENTINEL outside and NaN
    (a product that must overwrite it), zeros (c_is_zero, the f32 contraction) or small integers (accumulate, colsum)
    inside."""
    op, K, M, Nc = c["op"], c["K"], c["M"], c["Nc"]
    rng = np.random.default_rng(seed)
    ta = np.float32 if op in F32_OPS else np.float64
    tc = np.float32 if op == "rows_f32" else np.float64
    draw = (lambda *s: rng.standard_normal(s)) if gaussian else (lambda *s: rng.integers(-4, 5, size=s).astype(np.float64))
    lay = layout(c)
    g = lay["guard"]
    colsum = op.startswith("colsum")
    A = draw(M, K) if op == "nn" else draw(K, M)
    B = None if colsum or c["same"] else draw(K, Nc)
    if c["sym"] >= 0 and not c["asym"]:
        A[:, c["sym"]:] = B  # rows sym_row0 .. of C are B^T B
    A = A.astype(ta)
    B = None if B is None else B.astype(ta)
    rows_c, cols_c = (1, M) if colsum else (M, Nc)
    if zero_c:  # (the first call of a mirror pair: the accumulator as stats_compute clears it)
        C0 = np.zeros((rows_c, cols_c), dtype=tc)
    elif c["acc"] or colsum:
        C0 = rng.integers(-9, 10, size=(rows_c, cols_c)).astype(tc)
    elif c["c_zero"] or op == "tn_f32":
        C0 = np.zeros((rows_c, cols_c), dtype=tc)
    else:
        C0 = np.full((rows_c, cols_c), np.nan, dtype=tc)
    out = dict(A=A, B=B, C0=C0, lay=lay,
               bufA=padded(A, lay["lda"], lay["off_a"], g, np.nan),
               bufB=None if B is None else padded(B, lay["ldb"], lay["off_b"], g, np.nan),
               bufC=padded(C0, lay["ldc"], lay["off_c"], g, tc(SENTINEL) if tc is np.float64 else tc(-7.25e30)),
               bufA2=None, side=None)
    if op == "rows_f32":
        out["bufA2"] = padded(np.ascontiguousarray(A.T), lay["lda2"], 0, g, np.nan)
    if c["ct"]:
        out["side"] = padded(np.full((Nc, M), np.nan), lay["ldct"], 0, g, SENTINEL)
    elif c["diag"]:
        out["side"] = padded(np.full((M, 1), np.nan), 1, 0, g, SENTINEL)
    return out


def reference(c, ops):
    """The product in float64 from the (already rounded) operands; exact for the integer operands."""
    A, B = ops["A"].astype(np.float64), None if ops["B"] is None else ops["B"].astype(np.float64)
    op = c["op"]
    if op == "colsum":
        return A.sum(axis=0, keepdims=True)
    if op == "colsum_sq":
        return (A * A).sum(axis=0, keepdims=True)
    if op == "nn":
        return A @ B
    C = A.T @ (A if c["same"] else B)
    if c["asym"]:
        # the hint is a promise the launcher does not verify: with a block that is NOT symmetric the result shows what
        # the mirror touches -- the strictly lower tiles become the transposed upper ones, diagonal tiles stay as computed
        T = predict(c)["tile"]
        blk = C[c["sym"]:]
        i, j = np.indices(blk.shape)
        low = (i // T) > (j // T)
        blk[low] = blk.T[low]
    return C


def magnitude(c, ops):
    """|A|^T |B| of the componentwise rounding bound."""
    A, B = np.abs(ops["A"].astype(np.float64)), None if ops["B"] is None else np.abs(ops["B"].astype(np.float64))
    op = c["op"]
    if op == "colsum":
        return A.sum(axis=0, keepdims=True)
    if op == "colsum_sq":
        return (A * A).sum(axis=0, keepdims=True)
    if op == "nn":
        return A @ B
    return A.T @ (A if c["same"] else B)


def gamma(n, u):
    return n * u / (1.0 - n * u)

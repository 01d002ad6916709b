"""Exact parity of the dense kernels (gemm_f64.hpp and the f32 forms) on an MI355X, one launch at a time through the
test-only ``Engine.dense_probe``, which calls the launchers of the hot path with the strides, base alignments and options
the real callers use.  The cases and the restated dispatch are in tests/_dense_problems.py (CPU checks:
test_dense_problems.py).

Exact pass: operands are integers in [-4, 4], so every product and every partial sum is representable in float64 (and in
float32: 16 K < 2^24) in any order of summation -- the result must EQUAL the integer product on every route, atomics
included; a dropped, repeated or misplaced term cannot hide in a tolerance.  (The reference is NumPy's float64 product of
the integer-valued operands: every partial sum is an integer below 2^53, so it is the int64 product digit for digit,
from BLAS instead of NumPy's unblocked integer loop.)  A and B carry NaN everywhere outside their
logical rows x columns (padding columns, guard rows, the element in front of an offset base): a missing mask shows as a
NaN in C.  C carries a sentinel outside its logical region, which must come back bit for bit.

Rounding pass: Gaussian operands on one case per kernel against the componentwise bound |C - C^| <= 2 gamma_K |A|^T |B|,
gamma_K = K u / (1 - K u), u = 2^-53 (both the kernel and the NumPy product C^ satisfy the standard bound in any order);
for the f32 kernels the operands are rounded to float32 first, C^ is their float64 product and the bound is
gamma_(K+2) |A|^T |B| with u = 2^-24.  It catches a narrower accumulator, which integers cannot."""
import numpy as np
import pytest

import _dense_problems as dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from evo_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


def _probe(engine, c, ops, bufC=None):
    """One call of the case under its options (restored afterwards): (C buffer, side buffer, route record)."""
    lay = ops["lay"]
    changed = {k: v for k, v in c["opts"].items() if v != dp.OPTIONS[k]}
    try:
        for k, v in changed.items():
            engine.set_option(k, v)
        return engine.dense_probe(c["op"], ops["bufA"], ops["bufB"], ops["bufC"] if bufC is None else bufC, c["M"], c["Nc"],
                                  c["K"], A2=ops["bufA2"], side=ops["side"], same_operand=c["same"],
                                  deterministic=c["det"], sym_row0=c["sym"], c_is_zero=c["c_zero"], accumulate=c["acc"],
                                  mirror=c["mirror"], spare=c["spare"], diag=c["diag"], **lay)
    finally:
        for k in changed:
            engine.set_option(k, dp.OPTIONS[k])


def _bits(x):
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def _check_route(c, route, name):
    want = dp.predict(c, route["n_cu"])
    got = {k: route[k] for k in want}
    assert got == want, (name, got, want)


def _split_c(c, ops, Cbuf):
    """(logical C, C buffer with the logical region blanked) -- the second must equal the blanked prefill bit for bit."""
    lay = ops["lay"]
    rows, cols = ops["C0"].shape
    out = Cbuf.copy()
    view = dp.inner(out, rows, cols, lay["ldc"], lay["off_c"], lay["guard"])
    logical = view.copy()
    view[:] = 0
    return logical, out


def _check_outside(c, ops, Cbuf, name):
    _, got = _split_c(c, ops, Cbuf)
    _, want = _split_c(c, ops, ops["bufC"])
    assert np.array_equal(_bits(got), _bits(want)), "%s: C outside its M x Nc region was written" % name


def _check_side(c, ops, side, logical, name):
    lay = ops["lay"]
    g = lay["guard"]
    if c["diag"]:
        assert np.array_equal(_bits(side[:g]), _bits(ops["side"][:g])) and np.array_equal(_bits(side[-g:]), _bits(ops["side"][-g:])), name
        # the diagonal is the value stored in C, bit for bit
        assert np.array_equal(_bits(side[g:-g]), _bits(np.ascontiguousarray(np.diagonal(logical)))), name
    if c["ct"]:
        ct = dp.inner(side, c["Nc"], c["M"], lay["ldct"], 0, g)
        assert np.array_equal(_bits(np.ascontiguousarray(ct)), _bits(np.ascontiguousarray(logical.T))), name
        blank, want = side.copy(), ops["side"].copy()
        dp.inner(blank, c["Nc"], c["M"], lay["ldct"], 0, g)[:] = 0
        dp.inner(want, c["Nc"], c["M"], lay["ldct"], 0, g)[:] = 0
        assert np.array_equal(_bits(blank), _bits(want)), "%s: C^T outside its region was written" % name


@pytest.mark.parametrize("name", list(dp.CASES))
def test_exact(engine, name):
    c = dp.CASES[name]
    ops = dp.operands(c, seed=len(name) + c["K"] + 7 * c["M"])
    Cbuf, side, route = _probe(engine, c, ops)
    _check_route(c, route, name)
    logical, _ = _split_c(c, ops, Cbuf)
    want = dp.reference(c, ops)
    if c["acc"] or c["op"].startswith("colsum"):
        want = want + ops["C0"]
    assert not np.isnan(logical).any(), "%s: NaN in C (a read outside the operands, or C not overwritten)" % name
    np.testing.assert_array_equal(logical.astype(np.float64), want, err_msg=name)
    _check_outside(c, ops, Cbuf, name)
    _check_side(c, ops, side, logical, name)
    if (c["sym"] >= 0 and not c["asym"]) or c["same"]:  # the lower blocks are the transposed upper ones
        blk = logical[max(c["sym"], 0):]
        assert np.array_equal(_bits(np.ascontiguousarray(blk)), _bits(np.ascontiguousarray(blk.T))), name
    if c["twice"]:  # fixed order of summation: the same route and the same bits again
        C2, side2, route2 = _probe(engine, c, ops)
        assert route2 == route, name
        assert np.array_equal(_bits(C2), _bits(Cbuf)), name
        if side is not None:
            assert np.array_equal(_bits(side2), _bits(side)), name


@pytest.mark.parametrize("name", [n for n in dp.ROUNDING if dp.CASES[n]["twice"] or dp.CASES[n]["det"]])
def test_deterministic_routes_repeat_their_bits(engine, name):
    """gram_small, nn_small, the deterministic 64-tile form and the two workspace reduces add in a fixed order: Gaussian
    operands give the same bits twice."""
    c = dp.CASES[name]
    ops = dp.operands(c, seed=11, gaussian=True)
    C1, s1, r1 = _probe(engine, c, ops)
    C2, s2, r2 = _probe(engine, c, ops)
    assert r1 == r2 and np.array_equal(_bits(C1), _bits(C2)), name
    assert s1 is None or np.array_equal(_bits(s1), _bits(s2)), name


@pytest.mark.parametrize("name", dp.ROUNDING)
def test_rounding(engine, name):
    c = dp.CASES[name]
    ops = dp.operands(c, seed=5, gaussian=True)
    if c["op"].startswith("colsum"):  # (the integer prefill of `out` is exact in the sum)
        ops["C0"][:] = 0
        ops["bufC"] = dp.padded(ops["C0"], ops["lay"]["ldc"], ops["lay"]["off_c"], ops["lay"]["guard"], dp.SENTINEL)
    Cbuf, side, route = _probe(engine, c, ops)
    _check_route(c, route, name)
    logical, _ = _split_c(c, ops, Cbuf)
    ref, mag = dp.reference(c, ops), dp.magnitude(c, ops)
    K = c["K"]
    if c["op"] in dp.F32_OPS:
        bound = dp.gamma(K + 2, 2.0 ** -24) * mag
    else:
        bound = 2 * dp.gamma(K, 2.0 ** -53) * mag
    err = np.abs(logical.astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print("%s: largest error / bound = %.3g" % (name, worst))
    assert not np.isnan(logical).any() and (err <= bound).all(), (name, worst)
    _check_outside(c, ops, Cbuf, name)
    _check_side(c, ops, side, logical, name)


@pytest.mark.parametrize("name", list(dp.MIRROR_PAIRS))
def test_mirror_after_two_accumulating_calls(engine, name):
    """stats_contract_block's pattern: the blocks of K accumulate into one C, only the last call mirrors the symmetric
    block; the result is the full symmetric sum."""
    a, b = dp.MIRROR_PAIRS[name]
    oa, ob = dp.operands(a, seed=21, zero_c=True), dp.operands(b, seed=22)
    C1, _, r1 = _probe(engine, a, oa)
    _check_route(a, r1, name)
    C2, _, r2 = _probe(engine, b, ob, bufC=C1)
    _check_route(b, r2, name)
    logical, _ = _split_c(b, oa, C2)
    want = dp.reference(a, oa) + dp.reference(b, ob)
    np.testing.assert_array_equal(logical, want, err_msg=name)
    blk = logical[a["sym"]:]
    assert np.array_equal(blk, blk.T)
    _check_outside(b, oa, C2, name)


def test_rows_probe_refuses_what_configure_never_grants(engine):
    """The B = Y W launch from Y^T has no scalar form: evoamd_configure keeps Y^T only for an even H and rounds its leading
    dimension up to 4.  The probe refuses a misaligned call instead of running it."""
    from evo_amd._lib import EvoAmdError
    for ld in ("off", "odd"):
        c = dp.case("rows", 24, 130, 130, ld=ld)
        with pytest.raises(EvoAmdError):
            _probe(engine, c, dp.operands(c, seed=1))

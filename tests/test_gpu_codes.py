"""Posterior code readout on the GPU: Engine.posterior_codes / download_posterior (csrc/kernels_codes.hpp) and
Model.encode.

1. kernel against its NumPy mirror (evo_amd.codes.codes_from_dense) on the device's own dense rows, lpj and K^n:
   np.array_equal on every array -- p and m are copies of row entries, the order is fixed, and map_q is evaluated with
   the same additions and multiplications in the same order on both sides;
2. the dense rows against the reference's formulas (oracle/evo_oracle.py) at rtol 1e-8 / atol 1e-9, the tolerance
   tests/test_gpu_models.py holds y_reconstructed = E W^T to, and map_q against q.max() / (sum q + tiny) at 1e-12;
3. Model.encode for both models, host-synchronised and device-resident;
4. the argument and call-order checks.
"""
import numpy as np
import pytest

from evo_amd.codes import F64_TINY, codes_from_dense
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import init_states
from oracle import evo_oracle as orc

pytestmark = pytest.mark.gpu

FIELDS = ("idx", "p", "m", "nnz", "map_slot", "map_q", "map_state")

# name -> (algo, N, D, H, S, S_perm)
SHAPES = {
    "es3c": ("es3c", 37, 8, 70, 12, 0),
    "es3c_perm": ("es3c", 37, 8, 70, 12, 1),
    "ebsc": ("ebsc", 37, 8, 130, 12, 0),
    "ebsc_large_h": ("ebsc", 5, 4, 1100, 4, 0),  # beyond the register stripe (H > 512): the LDS home
}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _theta(rng, algo, D, H):
    W = rng.normal(size=(D, H)) * 0.4
    if algo == "ebsc":
        return {"W": W, "pi": 0.1, "sigma": 1.1}
    A = rng.normal(size=(H, 3)) * 0.2
    return {"W": W, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H) * 0.5, "Psi": np.eye(H) + A @ A.T,
            "sigma2": np.float64(1.3)}


def _states(rng, N, S, H):
    """K^n with S distinct states per datapoint.  Even n: 'many' -- states of 2..3 latents drawn from all of H except
    3 and 9, more than five distinct latents in all; datapoint 0 also holds the state {3, 9}, whose latents occur in no
    other of its states.  Odd n: 'few' -- S subsets of ceil(log2 S) (< 5) latents."""
    ss = np.zeros((N, S, H), dtype=bool)
    k_few = int(np.ceil(np.log2(S)))
    assert k_few < 5
    others = np.array([h for h in range(H) if h not in (3, 9)])
    for n in range(N):
        seen = set()
        if n % 2 == 0:
            while len(seen) < S:
                seen.add(tuple(sorted(rng.choice(others, rng.randint(2, 4), replace=False))))
        else:
            lat = rng.choice(H, k_few, replace=False)
            for code in rng.choice(2 ** k_few, S, replace=False):
                seen.add(tuple(sorted(lat[[j for j in range(k_few) if (code >> j) & 1]])))
        for s, st in enumerate(sorted(seen, key=lambda t: (len(t), t))):
            ss[n, s, list(st)] = True
        rng.shuffle(ss[n])
    ss[0, S // 2] = False
    ss[0, S // 2, [3, 9]] = True
    assert len({st.tobytes() for st in ss[0]}) == S
    assert not np.delete(ss[0], S // 2, axis=0)[:, [3, 9]].any()
    assert np.unique(np.nonzero(ss[0])[1]).size > 5 and np.unique(np.nonzero(ss[1])[1]).size < 5
    return ss


def _setup(eng, name, seed=0, nan_frac=0.0):
    """Configure the engine for a shape and make data, K^n and Theta resident.  Returns the host copies."""
    algo, N, D, H, S, S_perm = SHAPES[name]
    rng = np.random.RandomState(seed)
    Y = rng.normal(size=(N, D))
    x_infr = np.ones((N, D), dtype=bool)
    if nan_frac:
        x_infr = rng.random_sample((N, D)) >= nan_frac
        x_infr[:, 0] = True  # every datapoint keeps a reliable entry
        Y[~x_infr] = np.nan
    theta = _theta(rng, algo, D, H)
    ss = _states(rng, N, S, H)
    eng.set_option("ebsc_f32", 0)
    eng.f32 = False
    eng.configure("bsc" if algo == "ebsc" else "sssc", N, D, H, S, S_perm, 4)
    eng.upload_data(Y)
    if nan_frac:
        eng.upload_masks(x_infr)
        eng.set_reliable_fraction(x_infr.sum() / float(N))
    else:
        eng.set_reliable_fraction(None)
    eng.upload_states(ss)
    _set_params(eng, algo, theta)
    return algo, Y, x_infr, theta, ss, S_perm, rng


def _set_params(eng, algo, theta):
    if algo == "ebsc":
        eng.set_params_bsc(theta["W"], theta["pi"], theta["sigma"])
    else:
        eng.set_params_sssc(theta["W"], theta["pies"], theta["mus"], theta["Psi"], theta["sigma2"])


def _assert_codes_equal(got, want, what):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        if b is None:
            assert a is None, (what, f)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a, b), "%s: %s differs from the mirror at %s" % (what, f, np.argwhere(a != b)[:4].tolist())


# ---- 1. kernel against mirror ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_equals_mirror_bit_for_bit(eng, name):
    algo, Y, _, theta, ss, S_perm, rng = _setup(eng, name)
    N, S, H = ss.shape
    lpj = rng.normal(size=(N, S + S_perm)) * 2.0
    lpj[1 % N, [S_perm + 2, S_perm + 3]] = lpj[1 % N].max() + 1.0   # MAP tie inside K^n: the first slot wins
    if S_perm:
        lpj[2, 0] = lpj[2].max() + 3.0                              # the permanent state is the MAP state
        lpj[3, [0, 4]] = lpj[3].max() + 0.5                         # tie between the permanent slot and K^n
    eng.upload_lpj(lpj)
    eng.stats()
    Es, Ez = eng.download_posterior()
    assert (Ez is None) == (algo == "ebsc") and Es.shape == (N, H)
    lpj_d, packed = eng.download_lpj(), eng.download_states_packed()
    assert np.array_equal(lpj_d, lpj) and np.array_equal(packed, np.packbits(ss, axis=-1))
    # datapoint 0: latents 3 and 9 occur in one state only, so each marginal is that state's weight: an exact tie
    assert Es[0, 3] == Es[0, 9] > 0.0
    homes = {"ebsc_large_h": (-1, 2)}.get(name, (-1, 0, 1, 2))  # registers need H <= 512
    try:
        for home in homes:
            eng.set_option("codes_path", home)
            for p_min in (0.0, float(Es[0, 3])):  # the second one is an entry value: equality must exclude it
                for A in (1, 5, 64):
                    got = eng.posterior_codes(A, p_min)
                    want = codes_from_dense(Es, Ez, lpj_d, packed, A, p_min, S_perm)
                    _assert_codes_equal(got, want, "%s home %d A %d p_min %g" % (name, home, A, p_min))
                    if p_min == 0.0 and A == 5:
                        assert (got.nnz > 5).any() and (got.nnz < 5).any()
                    if p_min > 0.0:  # both tied entries EQUAL p_min: neither is in the code
                        assert not np.isin(got.idx[0], (3, 9)).any()
    finally:
        eng.set_option("codes_path", -1)
    got = eng.posterior_codes(64, 0.0)
    row0 = got.idx[0].tolist()
    assert row0.index(3) < row0.index(9) and got.p[0, row0.index(3)] == got.p[0, row0.index(9)]  # tie: lower index first
    assert got.map_slot[1 % N] == S_perm + 2
    if S_perm:
        assert got.map_slot[2] == 0 and not got.map_state[2].any() and got.map_slot[3] == 0
    k = got.map_slot[0] - S_perm
    if k >= 0:
        assert np.array_equal(got.map_states()[0], ss[0, k])
    # the sparse code of an untruncated datapoint is the dense row
    dEs, dEz = got.to_dense()
    keep = got.nnz <= 64
    assert keep.any() and np.array_equal(dEs[keep], Es[keep])
    if Ez is not None:
        assert np.array_equal(dEz[keep], Ez[keep])


# ---- 2. dense rows against the reference's formulas ------------------------------------------------------------------
def _check_rows(eng, want_Es, want_Ez, want_lpj):
    Es, Ez = eng.download_posterior()
    err = np.abs(Es - want_Es).max()
    print("max |Es - oracle| = %.3e" % err, "" if want_Ez is None else "max |Ez - oracle| = %.3e" % np.abs(Ez - want_Ez).max())
    np.testing.assert_allclose(Es, want_Es, rtol=1e-8, atol=1e-9)
    if want_Ez is not None:
        np.testing.assert_allclose(Ez, want_Ez, rtol=1e-8, atol=1e-9)
    q = np.exp(want_lpj - want_lpj.max(axis=1)[:, None])
    want_q = q.max(axis=1) / (q.sum(axis=1) + F64_TINY)
    got = eng.posterior_codes(16, 0.0)
    print("max rel |map_q - oracle| = %.3e" % np.abs(got.map_q / want_q - 1.0).max())
    np.testing.assert_allclose(got.map_q, want_q, rtol=1e-12, atol=0)
    gap = np.sort(want_lpj, axis=1)
    clear = gap[:, -1] - gap[:, -2] > 1e-9  # (an oracle tie could resolve either way under rounding)
    assert np.array_equal(got.map_slot[clear], np.argmax(want_lpj, axis=1)[clear])


@pytest.mark.parametrize("nan_frac", [0.0, 0.3])
def test_ebsc_rows_against_reference_formulas(eng, nan_frac):
    algo, Y, x_infr, theta, ss, S_perm, _ = _setup(eng, "ebsc", seed=1, nan_frac=nan_frac)
    N, S, H = ss.shape
    if nan_frac:
        eng.set_option("reconstruct_in_stats", 1)  # the masked pass forms the y_reconstructed its Wp contraction reads
    eng.lpj_resident()
    eng.stats()
    th = dict(theta)
    counters = orc.bsc_precompute(th, Y.shape[1], H, x_infr)
    want_lpj = np.array([orc.bsc_lpj(th, ss[n], Y[n], counters, x_infr[n]) for n in range(N)])
    q = np.exp(want_lpj - want_lpj.max(axis=1)[:, None])
    want_Es = np.einsum("ns,nsh->nh", q, ss) / (q.sum(axis=1) + F64_TINY)[:, None]
    _check_rows(eng, want_Es, None, want_lpj)


@pytest.mark.parametrize("name", ["es3c", "es3c_perm"])
def test_es3c_rows_against_reference_formulas(eng, name):
    algo, Y, _, theta, ss, S_perm, _ = _setup(eng, name, seed=2)
    N, S, H = ss.shape
    eng.lpj_resident()
    eng.stats()
    want_Es, want_Ez, want_lpj = np.empty((N, H)), np.empty((N, H)), np.empty((N, S + S_perm))
    for n in range(N):
        suff_n = {"ss": ss[n:n + 1].copy(), "lpj": np.empty((1, S + S_perm)), "S_perm": S_perm,
                  "incl": np.zeros((S_perm, H), dtype=bool), "Mprime": 0}
        acc = orc.sssc_EM_accumulate(dict(theta), suff_n, Y[n:n + 1], evolve=False)
        want_Es[n], want_Ez[n], want_lpj[n] = acc["xpt_s"], acc["xpt_sz"], suff_n["lpj"][0]
    _check_rows(eng, want_Es, want_Ez, want_lpj)


# ---- 3. Model.encode -------------------------------------------------------------------------------------------------
def _snapshot(d):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _assert_same_dict(d, snap, what):
    assert list(d.keys()) == list(snap.keys()), what
    for k, v in snap.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(d[k], v), (what, k)
        else:
            assert d[k] is v or d[k] == v, (what, k)


@pytest.mark.parametrize("mode", ["sync_host", "device_resident"])
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_model_encode(eng, algo, mode):
    N, D, H, S = 45, 10, 48, 16   # H <= 64: no code is ever cut at max_active = 64
    rng = np.random.RandomState(5)
    np.random.seed(6)
    Y = rng.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    kw = {} if mode == "sync_host" else {"rng": "device", "sync_host": False}
    model = (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, **kw)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 6, 1, 1)
    for _ in range(2):
        _, _, _, theta = model.step(theta, suff, my_data)
    ids = (id(theta), id(suff), id(my_data), id(suff["ss"]), id(suff["lpj"]), id(my_data["y"]))
    snaps = (_snapshot(theta), _snapshot(suff), _snapshot(my_data))
    codes = model.encode(theta, suff, my_data, max_active=64, p_min=0.0, dense=True)
    assert ids == (id(theta), id(suff), id(my_data), id(suff["ss"]), id(suff["lpj"]), id(my_data["y"]))
    for d, snap, what in zip((theta, suff, my_data), snaps, ("model_params", "my_suff_stat", "my_data")):
        _assert_same_dict(d, snap, what)
    assert codes.Es.shape == (N, H) and (codes.Ez is None) == (algo == "ebsc") and (codes.m is None) == (algo == "ebsc")
    S_perm = suff["S_perm"]
    lpj_d, packed = eng.download_lpj(), eng.download_states_packed()
    if mode == "sync_host":  # the caller's arrays are what the pass read
        assert np.array_equal(lpj_d, suff["lpj"]) and np.array_equal(packed, np.packbits(suff["ss"], axis=-1))
    _assert_codes_equal(codes, codes_from_dense(codes.Es, codes.Ez, lpj_d, packed, 64, 0.0, S_perm), algo + " " + mode)
    assert (codes.nnz <= 64).all() and (codes.nnz > 0).all()
    dEs, dEz = codes.to_dense()
    assert np.array_equal(dEs, codes.Es)
    if algo == "es3c":
        assert np.array_equal(dEz, codes.Ez)
    # the defaults: 16 slots, no dense rows; and the rows are a distribution's marginals
    short = model.encode(theta, suff, my_data)
    assert short.idx.shape == (N, 16) and short.Es is None and short.Ez is None
    assert np.array_equal(short.idx, codes.idx[:, :16]) and np.array_equal(short.nnz, codes.nnz)
    assert (codes.Es >= 0).all() and (codes.Es <= 1 + 1e-12).all() and (codes.map_q > 0).all() and (codes.map_q <= 1).all()
    # training goes on from the same state
    F, _, _, _ = model.step(theta, suff, my_data)
    assert np.isfinite(F)


def test_model_encode_incomplete_data(eng):
    N, D, H, S = 33, 12, 40, 12
    rng = np.random.RandomState(8)
    np.random.seed(9)
    Y = rng.normal(size=(N, D))
    x_infr = rng.random_sample((N, D)) >= 0.3
    x_infr[:, 0] = True
    Y[~x_infr] = np.nan
    my_data = {"y": Y, "x_infr": x_infr, "x": x_infr.copy()}
    model = BSC(D, H, S, engine=eng)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 6, 1, 1)
    _, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
    codes = model.encode(theta, suff, my_data, max_active=8, dense=True)
    want = codes_from_dense(codes.Es, None, eng.download_lpj(), eng.download_states_packed(), 8, 0.0, suff["S_perm"])
    _assert_codes_equal(codes, want, "ebsc incomplete")
    F, _, _, _ = model.step(theta, suff, my_data, do_reconstruction=True)
    assert np.isfinite(F)


# ---- 4. errors -------------------------------------------------------------------------------------------------------
def test_call_order_and_argument_checks(eng):
    algo, Y, _, theta, ss, S_perm, rng = _setup(eng, "es3c", seed=3)
    with pytest.raises(RuntimeError, match="evoamd_stats"):
        eng.posterior_codes()
    with pytest.raises(RuntimeError, match="evoamd_stats"):
        eng.download_posterior()
    eng.lpj_resident()
    eng.stats()
    assert eng.posterior_codes(3, 0.0).idx.shape == (ss.shape[0], 3)
    for bad in (dict(max_active=0), dict(max_active=65), dict(p_min=-1e-3), dict(p_min=float("nan"))):
        with pytest.raises(RuntimeError, match="max_active|p_min"):
            eng.posterior_codes(**bad)
    eng.posterior_codes(64, 0.5)  # the refused calls left the rows valid
    _set_params(eng, algo, theta)
    with pytest.raises(RuntimeError, match="evoamd_stats"):
        eng.posterior_codes()
    with pytest.raises(RuntimeError, match="evoamd_stats"):
        eng.download_posterior()
    eng.lpj_resident()
    eng.stats()
    eng.upload_states(ss)  # K^n changed under the rows: they no longer belong together
    with pytest.raises(RuntimeError, match="evoamd_stats"):
        eng.posterior_codes()


def test_float32_mode_is_refused(eng):
    N, D, H, S = 32, 8, 16, 8
    np.random.seed(4)
    Y = np.random.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = BSC(D, H, S, engine=eng, dtype=np.float32)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1)
    _, _, _, theta = model.step(theta, suff, my_data)
    with pytest.raises(RuntimeError, match="float32 mode"):
        model.encode(theta, suff, my_data)

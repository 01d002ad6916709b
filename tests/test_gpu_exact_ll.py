"""Exact log-likelihood on the GPU beyond the H < 12 state table: Engine.loglik_exact (csrc/kernels_exact.hpp) and
Model.exact_log_likelihood.

1. agreement with free_energy(full=True) and the reference's fixtures where both run;
2. H = 13, where no table exists: L, the per-datapoint terms and the exact posterior marginals against the oracle;
3. chunking: several chunks, one chunk, a partial chunk, fewer states than lanes, rows whose running maximum moves late;
4. two calls give the same bits; the EM state on the device is not disturbed;
5. incomplete data;
6. argument errors.

Tolerances.  L and ll: rtol 1e-11 (test_full_free_energy's; at most 2^13 positive terms per sum).  Marginals: rtol 1e-10.
Against free_energy(full=True) of the same model: rtol 1e-12 -- the same lpj kernels, only the order of the sum differs.
Every oracle reference comes from tests/_exact_problems.py, computed once per shape."""
import numpy as np
import pytest

from _exact_problems import fold_in_chunks, my_data_of, problem
from conftest import load_golden
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import init_states

pytestmark = pytest.mark.gpu

ALGOS = ["ebsc", "es3c"]
BSC_KEYS = ("W", "pi", "sigma")
SSSC_KEYS = ("W", "pies", "mus", "Psi", "sigma2")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _suff(N, S, H, background=False):
    np.random.seed(0)
    perm = {"background": background, "allzero": False, "singletons": False}
    return init_states(N, S, H, "fit", "randflip", 2, 1, 1, permanent=perm)


def _copy(d):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _model_and_inputs(eng, p, **kw):
    S = 2 if p.H < 6 else 4
    model = (BSC if p.algo == "ebsc" else SSSC)(p.D, p.H, S, engine=eng, **kw)
    return model, my_data_of(p), _copy(p.theta), _suff(p.N, S, p.H, p.background)


def _check_against_oracle(p, got, what):
    L, ll, marg = got
    print("%s: L %.15g (oracle %.15g), max rel ll %.3g, max rel marg %.3g"
          % (what, L, p.L, np.abs(ll / p.ll - 1).max(), np.abs(marg / p.marg - 1).max()))
    np.testing.assert_allclose(L, p.L, rtol=1e-11, err_msg=what)
    np.testing.assert_allclose(ll, p.ll, rtol=1e-11, err_msg=what)
    np.testing.assert_allclose(marg, p.marg, rtol=1e-10, err_msg=what)
    if p.background:
        assert (marg[:, -1] == 1.0).all(), what


# ---- 1. agreement with the existing path -----------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("fixture", ["full_F", "background"])
def test_agrees_with_full_free_energy_and_fixture(eng, algo, fixture):
    bg = fixture == "background"
    g = load_golden(fixture + ".npz")
    H, D, N, S = (7, 9, 20, 10) if bg else (8, 16, 30, 10)
    pre = "full_%s_" % algo if bg else algo + "_"
    Y = g[pre + "Y"]
    theta = {k: np.array(g[pre + k]) for k in (BSC_KEYS if algo == "ebsc" else SSSC_KEYS)}
    for k in ("pi", "sigma", "sigma2"):
        if k in theta:
            theta[k] = np.float64(theta[k])
    np.random.seed(0)
    suff = init_states(N, S, H, "fit", "randflip", 5, 1, 1,
                       permanent={"background": bg, "allzero": False, "singletons": False})
    model = (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    L = model.exact_log_likelihood(my_data, theta, suff)
    assert isinstance(L, float)
    L_table = model.free_energy(my_data, dict(theta), suff, full=True)
    print("%s %s: exact %.15g table %.15g golden %.15g" % (algo, fixture, L, L_table, float(g[pre + "L"])))
    np.testing.assert_allclose(L, float(g[pre + "L"]), rtol=1e-11)
    np.testing.assert_allclose(L, L_table, rtol=1e-12)
    L2, ll, marg = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True, chunk_states=64)
    assert marg is None and ll.shape == (N,)
    np.testing.assert_allclose(L2, L_table, rtol=1e-12)


# ---- 2. beyond the table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_beyond_the_state_table(eng, algo):
    p = problem(algo, 13, 8, 6)
    model = (BSC if algo == "ebsc" else SSSC)(p.D, p.H, 10, engine=eng)
    my_data, theta = my_data_of(p), _copy(p.theta)
    np.random.seed(0)
    suff = init_states(p.N, 10, 13, "fit", "randflip", 5, 1, 1)
    assert suff["sm"] is None
    snaps = (_copy(theta), _copy(suff), _copy(my_data))
    got = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True, marginals=True)
    for d, snap in zip((theta, suff, my_data), snaps):  # the three dicts stay as they were
        assert list(d.keys()) == list(snap.keys())
        for k, v in snap.items():
            assert np.array_equal(d[k], v) if isinstance(v, np.ndarray) else (d[k] is v or d[k] == v), k
    assert got[1].shape == (p.N,) and got[2].shape == (p.N, p.H)
    _check_against_oracle(p, got, algo + " H=13")
    L_only = model.exact_log_likelihood(my_data, theta, suff, chunk_states=1024)
    np.testing.assert_allclose(L_only, p.L, rtol=1e-11)
    with pytest.raises(ValueError, match="max_H"):
        model.exact_log_likelihood(my_data, theta, suff, max_H=12)
    with pytest.raises(AssertionError):  # the table path still stops at H = 12
        model.free_energy(my_data, theta, suff, full=True)


# ---- 3. chunking -----------------------------------------------------------------------------------------------------
# (H, background, chunk sizes): two chunks and one; the index space equal to one chunk; fewer states than lanes; eight
# chunks against the automatic choice; with the background unit one chunk, and two whose first starts from m = -inf.
CHUNK_CASES = [(7, False, (64, 128)), (6, False, (64,)), (3, False, (64, 0)), (9, False, (64, 0)),
               (7, True, (64,)), (8, True, (64, 0))]


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("H,background,chunks", CHUNK_CASES)
def test_chunking(eng, algo, H, background, chunks):
    p = problem(algo, H, 6, 5, background)  # N = 5: a partial workgroup of waves
    model, my_data, theta, suff = _model_and_inputs(eng, p)
    runs = []
    for C in chunks:
        got = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True, marginals=True, chunk_states=C)
        _check_against_oracle(p, got, "%s H=%d bg=%d chunk=%d" % (algo, H, background, C))
        runs.append(got)
    for other in runs[1:]:
        np.testing.assert_allclose(other[0], runs[0][0], rtol=1e-11)
        np.testing.assert_allclose(other[1], runs[0][1], rtol=1e-11)
        np.testing.assert_allclose(other[2], runs[0][2], rtol=1e-10)
    # the NumPy mirror of the recursion, cut at the same boundaries
    ll_m, marg_m = fold_in_chunks(p, chunks[0])
    np.testing.assert_allclose(runs[0][1], ll_m, rtol=1e-11)
    np.testing.assert_allclose(runs[0][2], marg_m, rtol=1e-10)
    if H >= 7 and not background:  # the running maximum moves in a late chunk for some rows only
        late = p.lpj.argmax(axis=1) + 1 >= 64
        assert late.any() and not late.all()


# ---- 4. reproducibility and isolation --------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_same_bits_twice(eng, algo):
    p = problem(algo, 9, 6, 5)
    model, my_data, theta, suff = _model_and_inputs(eng, p)
    for C in (64, 0):
        a = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True, marginals=True, chunk_states=C)
        b = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True, marginals=True, chunk_states=C)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("algo", ALGOS)
def test_em_state_is_not_disturbed(eng, algo):
    """step, [exact_log_likelihood,] step: the second step gives the same F, Theta and K^n with and without the call.
    Both branches hand the second step a host copy of Theta, so they run the same code but for the call.  K^n must be
    equal; F and Theta are held to 1e-12 / 1e-9, not to the bit: the statistics pass sums with f64 atomics, whose
    order -- and with it the last bits of the Theta the first step returns -- changes from run to run."""
    N, D, H, S = 40, 8, 10, 8
    p = problem(algo, H, D, N)
    out = []
    for with_call in (False, True):
        np.random.seed(2)
        model = (BSC if algo == "ebsc" else SSSC)(D, H, S, rng="device", sync_host=False, engine=eng, seed=4,
                                                   device_mstep=True)
        my_data = my_data_of(p)
        suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1)
        theta = model.check_params(model.standard_init(my_data))
        _, _, _, theta = model.step(theta, suff, my_data)
        theta = dict(theta.copy())
        if with_call:
            kn, lpj = eng.download_states_packed(), eng.download_lpj()
            L, ll, marg = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True, marginals=True,
                                                     chunk_states=256)
            assert np.isfinite(L) and np.isfinite(ll).all() and np.isfinite(marg).all()
            assert np.array_equal(eng.download_states_packed(), kn) and np.array_equal(eng.download_lpj(), lpj)
        F, _, _, theta2 = model.step(theta, suff, my_data)
        theta2 = dict(theta2.copy())
        out.append((F, theta2, eng.download_states_packed()))
    (F0, th0, kn0), (F1, th1, kn1) = out
    print("%s: F %.17g / %.17g" % (algo, F0, F1))
    assert np.array_equal(kn0, kn1)
    np.testing.assert_allclose(F1, F0, rtol=1e-12)
    for k in (BSC_KEYS if algo == "ebsc" else SSSC_KEYS):
        np.testing.assert_allclose(th1[k], th0[k], rtol=1e-9, atol=1e-12, err_msg=k)


# ---- 5. incomplete data ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_incomplete_data(eng, algo):
    p = problem(algo, 7, 9, 8, False, 0.2)
    assert p.x_infr.any(axis=1).all() and 0.1 < 1.0 - p.x_infr.mean() < 0.3
    model, my_data, theta, suff = _model_and_inputs(eng, p)
    L, ll, marg = model.exact_log_likelihood(my_data, theta, suff, per_datapoint=True, marginals=True, chunk_states=64)
    ll_m, marg_m = fold_in_chunks(p, 64)
    print("%s incomplete: max rel ll %.3g" % (algo, np.abs(ll / ll_m - 1).max()))
    np.testing.assert_allclose(ll, ll_m, rtol=1e-11)
    np.testing.assert_allclose(marg, marg_m, rtol=1e-10)
    np.testing.assert_allclose(L, p.L, rtol=1e-11)


# ---- 6. argument errors (last: they configure the engine directly) --------------------------------------------------
def test_argument_errors(eng):
    p = problem("ebsc", 7, 6, 5)
    model, my_data, theta, suff = _model_and_inputs(eng, p)
    model.exact_log_likelihood(my_data, theta, suff)
    for bad in (96, 32, 1, -64):
        with pytest.raises(RuntimeError, match="chunk_states"):
            eng.loglik_exact(False, bad)
    Fs, ll, marg = eng.loglik_exact(False, 64, per_datapoint=False)  # the refused calls left everything usable
    assert ll is None and marg is None
    np.testing.assert_allclose(Fs, p.ll.sum(), rtol=1e-11)
    rng = np.random.RandomState(0)
    for H, background in ((33, False), (34, True)):  # 33 latents vary: past the Python guard, the library refuses
        eng.set_option("ebsc_f32", 0)
        eng.f32 = False
        eng.configure("bsc", 4, 3, H, 2, 0, 1)
        eng.upload_data(rng.normal(size=(4, 3)))
        eng.set_params_bsc(rng.normal(size=(3, H)), 0.1, 1.0)
        with pytest.raises(RuntimeError, match="33 latents vary"):
            eng.loglik_exact(background)

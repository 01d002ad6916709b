"""Model.predictive_log_score / Engine.predictive_score (csrc/kernels_predictive_score.hpp) on the GPU.

1. the kernel against its NumPy mirror (evo_amd.models.predictive_log_score_host; references from
   tests/_predictive_score_problems.py, computed once per problem) at the shapes of tests/test_gpu_predictive.py: N = 30 and
   37 (no multiple of the 4 waves of a workgroup), D = 25 (below one wave), 64, 70 (a ragged second register per lane) and
   512 (8 registers per lane), H = 10 and 70 (two state words), states of 0 .. 32 active latents, both models, complete
   and incomplete data, S_perm 0 / 1, the background unit, sync_host True / False, noise on and -- ES3C -- off.
   Tolerances, those the predictive moments are held to: logp rtol 1e-8 / atol 1e-9 max(1, max |ref|), pit atol 1e-9,
   logp_n and score the same relative tolerance on their sums; the NaN and -inf patterns, count and the counters exactly;
2. bit stability: the same call twice, and with every unscored value of y_true replaced by NaN and by 1e300;
3. consistency of score, logp and count;
4. S = 1: the normal log density at the mean and var of the engine's own predictive_moments;
5. refusals, each leaving K^n, lpj, the candidate batch and the validity record as they were;
6. non-interference: step / step with a call in between, encode after it, the three dicts untouched;
7. the kernel class is named.
"""
import numpy as np
import pytest

from _predictive_problems import my_data_of, problem
from _predictive_score_problems import N_NOT_QUERIED, score_problem
from evo_amd import _lib
from evo_amd._lib import EvoAmdError
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC, predictive_log_score_host
from evo_amd.variational import init_states

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _model(eng, algo, D, H, S, sync_host=True, **kw):
    if not sync_host:
        kw.update(rng="device", sync_host=False)
    return (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, **kw)


def _suff(N, S, H, permanent, ss, lpj):
    suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1, permanent=dict(permanent))
    assert suff["ss"].shape == ss.shape and suff["lpj"].shape == lpj.shape
    suff["ss"], suff["lpj"] = np.array(ss), np.array(lpj)
    return suff


def _assert_matches_mirror(score, info, q, what):
    want = q.info
    logp, pit, wl, wp = info["logp"], info["pit"], want["logp"], want["pit"]
    assert logp.dtype == pit.dtype == np.float64 and logp.shape == pit.shape == wl.shape
    assert info["count"].dtype == np.int32 and np.array_equal(info["count"], want["count"]), what
    for name in ("n_singular", "n_skipped", "n_not_queried", "n_bad_values"):
        assert info[name] == want[name], (what, name)
    assert np.array_equal(np.isnan(logp), np.isnan(wl)) and np.array_equal(np.isnan(pit), np.isnan(wp)), what
    assert np.array_equal(np.isneginf(logp), np.isneginf(wl)), what
    ok = np.isfinite(wl)
    lmax = max(1.0, float(np.abs(wl[ok]).max()))
    nmax = max(1.0, float(np.abs(want["logp_n"]).max()))
    print("%s: max |logp - ref| = %.3g (max |ref| %.3g), max |pit - ref| = %.3g, max |logp_n - ref| = %.3g (max %.3g), "
          "score - ref = %.3g" % (what, np.abs(logp[ok] - wl[ok]).max(), lmax, np.abs(pit[ok] - wp[ok]).max(),
                                  np.abs(info["logp_n"] - want["logp_n"]).max(), nmax, score - q.score))
    np.testing.assert_allclose(logp[ok], wl[ok], rtol=1e-8, atol=1e-9 * lmax, err_msg=what)
    np.testing.assert_allclose(pit[ok], wp[ok], rtol=0, atol=1e-9, err_msg=what)
    np.testing.assert_allclose(info["logp_n"], want["logp_n"], rtol=1e-8, atol=1e-9 * nmax, err_msg=what)
    np.testing.assert_allclose(score, q.score, rtol=1e-8, atol=1e-9, err_msg=what)


# (algo, N, D, H, incomplete, S_perm, background), noise, sync_host: the shapes of tests/test_gpu_predictive.py::CASES, and
# ES3C without noise on complete data with the all-zero state (a point mass) and at the register limit
CASES = [
    (("es3c", 30, 25, 10, False, 1, False), True, True),
    (("es3c", 37, 70, 70, False, 1, False), True, False),
    (("es3c", 37, 64, 70, True, 0, False), False, True),
    (("es3c", 37, 70, 70, True, 1, False), True, True),
    (("es3c", 30, 25, 10, True, 0, True), True, False),
    (("es3c", 30, 512, 10, False, 0, False), False, True),
    (("es3c", 30, 25, 10, False, 1, False), False, False),
    (("es3c", 30, 512, 10, True, 1, False), True, True),
    (("ebsc", 37, 25, 70, False, 1, False), True, True),
    (("ebsc", 30, 70, 10, True, 0, False), True, True),
    (("ebsc", 37, 64, 10, False, 0, True), True, False),
    (("ebsc", 30, 512, 10, True, 1, False), True, True),
]


def _call(eng, q, sync_host, y_true=None, per_entry=True):
    p = q.p
    model = _model(eng, p.algo, p.D, p.H, p.S, sync_host)
    suff, my_data, theta = _suff(p.N, p.S, p.H, p.permanent, p.ss, p.lpj), my_data_of(p), dict(p.theta)
    keys = (list(theta), list(suff), list(my_data))
    score, info = model.predictive_log_score(theta, suff, my_data, q.y_true if y_true is None else y_true, query=q.query_arg,
                                             noise=q.noise, per_entry=per_entry)
    assert keys == (list(theta), list(suff), list(my_data))  # nothing written into the three dicts
    assert np.array_equal(suff["ss"], p.ss) and np.array_equal(suff["lpj"], p.lpj)
    assert np.array_equal(my_data["y"], p.Y, equal_nan=True) and np.array_equal(my_data["x_infr"], p.x_infr)
    return score, info


def _same_bits(a, b):
    sa, ia = a
    sb, ib = b
    assert np.array_equal(np.float64(sa).view(np.uint64), np.float64(sb).view(np.uint64)) and ia.keys() == ib.keys()
    for k in ia:
        if isinstance(ia[k], np.ndarray):
            assert np.array_equal(ia[k].view(np.uint64 if ia[k].dtype == np.float64 else ia[k].dtype),
                                  ib[k].view(np.uint64 if ib[k].dtype == np.float64 else ib[k].dtype)), k
        else:
            assert ia[k] == ib[k], k


@pytest.mark.parametrize("case,noise,sync_host", CASES)
def test_kernel_equals_mirror(eng, case, noise, sync_host):
    q = score_problem(*case, noise=noise)
    score, info = _call(eng, q, sync_host)
    _assert_matches_mirror(score, info, q, "%r noise=%s" % (case, noise))
    assert info["n_not_queried"] >= 1 and info["count"][N_NOT_QUERIED] == 0 and info["logp_n"][N_NOT_QUERIED] == 0.0
    assert info["n_bad_values"] >= 4 and info["n_skipped"] == (1 if q.p.incomplete else 0)
    # 3. consistency
    logp, count = info["logp"], info["count"]
    scored = q.query & np.isfinite(np.where(q.query, q.y_true, 0.0))
    visited = scored.any(axis=1) & q.p.x_infr.any(axis=1)
    assert np.array_equal(count, np.where(visited, scored.sum(axis=1), 0))  # (no singular system in these problems)
    assert np.array_equal(~np.isnan(logp), scored & visited[:, None])
    fin = np.isfinite(logp)
    assert fin.sum() == count.sum()  # (no entry without a density in these problems)
    assert score == pytest.approx(logp[fin].sum() / count.sum(), rel=1e-12)
    np.testing.assert_allclose(info["logp_n"], np.where(fin, logp, 0.0).sum(axis=1), rtol=1e-12, atol=1e-12)
    ok = ~np.isnan(info["pit"])
    assert ((info["pit"][ok] >= 0.0) & (info["pit"][ok] <= 1.0)).all()
    # without per_entry: the same sums, no arrays
    score2, info2 = _call(eng, q, sync_host, per_entry=False)
    assert "logp" not in info2 and "pit" not in info2
    assert score2 == score and np.array_equal(info2["logp_n"], info["logp_n"]) and np.array_equal(info2["count"], count)


@pytest.mark.parametrize("case,noise,sync_host", [CASES[3], CASES[5], CASES[10]])
def test_bits_are_stable(eng, case, noise, sync_host):
    q = score_problem(*case, noise=noise)
    first = _call(eng, q, sync_host)
    _same_bits(first, _call(eng, q, sync_host))
    for garbage in (np.nan, 1e300):
        y = np.array(q.y_true)
        y[~q.query] = garbage
        _same_bits(first, _call(eng, q, sync_host, y_true=y))
    if q.query_arg is not None:  # an explicit query: other values at entries the query does not name are not read either
        y = np.where(q.query, q.y_true, -3.25)
        _same_bits(first, _call(eng, q, sync_host, y_true=y))


@pytest.mark.parametrize("algo,incomplete", [("es3c", False), ("es3c", True), ("ebsc", True)])
def test_one_state_is_the_gaussian_of_the_moments(eng, algo, incomplete):
    p = problem(algo, 30, 25, 10, incomplete, 0, False)
    S = 1
    ss, lpj = np.array(p.ss[:, 2:3]), np.array(p.lpj[:, 2:3])
    model = _model(eng, algo, p.D, p.H, S)
    suff = init_states(p.N, S, p.H, "fit", "randflip", 1, 1, 1, permanent=dict(p.permanent))
    suff["ss"], suff["lpj"] = ss, lpj
    mean, var, _ = model.predictive_moments(dict(p.theta), suff, my_data_of(p))
    rng = np.random.RandomState(3)
    y_true = np.where(np.isnan(mean), 0.0, mean) + rng.normal(size=mean.shape) * 2.0
    query = np.ones(mean.shape, dtype=bool)
    score, info = model.predictive_log_score(dict(p.theta), suff, my_data_of(p), y_true, query=query, per_entry=True)
    ok = ~np.isnan(mean)
    assert info["n_skipped"] == (1 if incomplete else 0) == int((~ok).all(axis=1).sum())
    want = -0.5 * (np.log(2.0 * np.pi * var[ok]) + (y_true[ok] - mean[ok]) ** 2 / var[ok])
    print("%s incomplete=%s: max |logp - N(y; mean, var)| = %.3g" % (algo, incomplete, np.abs(info["logp"][ok] - want).max()))
    np.testing.assert_allclose(info["logp"][ok], want, rtol=1e-10, atol=1e-10)
    assert np.isnan(info["logp"][~ok]).all()
    assert score == pytest.approx(want.mean(), rel=1e-10)


def test_singular_system_is_counted(eng):
    """The problem of tests/test_gpu_predictive.py::test_singular_system_is_counted: a dead latent (zero row and column of
    Psi) in one state of datapoint 2, whose reliable entries see W_A = 0; datapoint 5 has no reliable entry."""
    rng = np.random.RandomState(4)
    H, D, N, S = 10, 25, 30, 8
    p = problem("es3c", N, D, H, True, 0, False)
    theta = dict(p.theta)
    theta["Psi"] = np.array(theta["Psi"])
    theta["Psi"][2, :] = theta["Psi"][:, 2] = 0.0
    theta["W"] = np.array(theta["W"])
    ss = np.array(p.ss)
    ss[:, :, 2] = False
    ss[2, 4] = False
    ss[2, 4, [1, 2]] = True
    x_infr = np.array(p.x_infr)
    x_infr[2] = False
    x_infr[2, :3] = True
    theta["W"][:3, [1, 2]] = 0.0
    Y = np.where(x_infr, rng.normal(size=(N, D)), np.nan)
    y_true = rng.normal(size=(N, D)) * 2.0
    my_data = {"y": Y, "x_infr": x_infr, "x": x_infr.copy()}
    want_score, want = predictive_log_score_host("sssc", theta, ss, p.lpj, Y, y_true, ~x_infr, x_infr)
    assert want["n_singular"] == 1 and want["n_skipped"] == 1
    model = _model(eng, "es3c", D, H, S)
    score, info = model.predictive_log_score(theta, _suff(N, S, H, p.permanent, ss, p.lpj), my_data, y_true, per_entry=True)
    assert info["n_singular"] == 1 and info["n_skipped"] == 1 and info["n_not_queried"] == want["n_not_queried"]
    assert np.isnan(info["logp"][2]).all() and np.isnan(info["pit"][2]).all() and info["count"][2] == 0 and info["logp_n"][2] == 0.0
    assert np.array_equal(info["count"], want["count"]) and np.array_equal(np.isnan(info["logp"]), np.isnan(want["logp"]))
    ok = ~np.isnan(want["logp"])
    lmax = max(1.0, float(np.abs(want["logp"][ok]).max()))
    np.testing.assert_allclose(info["logp"][ok], want["logp"][ok], rtol=1e-8, atol=1e-9 * lmax)
    np.testing.assert_allclose(info["pit"][ok], want["pit"][ok], rtol=0, atol=1e-9)
    np.testing.assert_allclose(score, want_score, rtol=1e-8, atol=1e-9)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _candidates(eng):
    try:
        return eng.download_candidates()
    except EvoAmdError:  # (no batch on the device)
        return ()


def _device_state(eng):
    return (eng.download_states_packed(), eng.download_lpj(), _candidates(eng), eng.debug_validity())


def _assert_state_kept(eng, before):
    after = _device_state(eng)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    assert len(before[2]) == len(after[2])
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert before[3] == after[3], {k: (before[3][k], after[3][k]) for k in before[3] if before[3][k] != after[3][k]}


def test_refusals_leave_the_context_as_it_was(eng):
    q = score_problem("es3c", 37, 64, 70, True, 0, False, noise=True)
    p = q.p
    model = _model(eng, "es3c", p.D, p.H, p.S)
    suff, my_data, theta = _suff(p.N, p.S, p.H, p.permanent, p.ss, p.lpj), my_data_of(p), dict(p.theta)
    good = model.predictive_log_score(theta, suff, my_data, q.y_true, per_entry=True)
    before = _device_state(eng)
    # wrong shapes, a query that is not bool
    for y, qq in ((q.y_true[:, :-1], None), (q.y_true[:-1], None), (q.y_true, q.query[:, :-1]), (q.y_true, q.query.astype(np.uint8))):
        with pytest.raises(ValueError, match="shape"):
            model.predictive_log_score(theta, suff, my_data, y, query=qq)
    with pytest.raises(ValueError, match=r"\(N, D\)"):
        eng.predictive_score(q.y_true[:-1], q.query[:-1])
    _assert_state_kept(eng, before)
    # a state of 33 latents: in a datapoint without a scored entry it is not visited and not refused ...
    ss = np.array(p.ss)
    assert ss[1, 2].sum() == 32 and q.info["count"][1] > 0
    ss[1, 2, np.flatnonzero(~ss[1, 2])[0]] = True
    suff33 = _suff(p.N, p.S, p.H, p.permanent, ss, p.lpj)
    query = np.array(q.query)
    query[1] = False
    score, info = model.predictive_log_score(theta, suff33, my_data, q.y_true, query=query)
    assert np.isfinite(score) and info["count"][1] == 0 and info["n_not_queried"] == q.info["n_not_queried"] + 1
    # ... in a visited one the call is refused, with that K^n on the device as it was
    before = _device_state(eng)
    with pytest.raises(EvoAmdError, match=r"evoamd_predictive_score: datapoint n = 1 .*k = 33"):
        eng.predictive_score(q.y_true, q.query)
    _assert_state_kept(eng, before)
    with pytest.raises(EvoAmdError, match=r"evoamd_predictive_score: datapoint n = 1 .*k = 33"):
        model.predictive_log_score(theta, suff33, my_data, q.y_true)
    # the context serves the next call with the same bits as before
    _same_bits(good, model.predictive_log_score(theta, suff, my_data, q.y_true, per_entry=True))


def test_ebsc_without_noise_and_complete_default_query_are_refused(eng):
    q = score_problem("ebsc", 37, 25, 70, False, 1, False, noise=True)
    p = q.p
    model = _model(eng, "ebsc", p.D, p.H, p.S)
    suff, my_data, theta = _suff(p.N, p.S, p.H, p.permanent, p.ss, p.lpj), my_data_of(p), dict(p.theta)
    good = model.predictive_log_score(theta, suff, my_data, q.y_true, query=q.query, per_entry=True)
    before = _device_state(eng)
    with pytest.raises(ValueError, match="EBSC without noise"):
        model.predictive_log_score(theta, suff, my_data, q.y_true, query=q.query, noise=False)
    with pytest.raises(EvoAmdError, match="EBSC without the noise term"):
        eng.predictive_score(q.y_true, q.query, noise=False)
    with pytest.raises(ValueError, match="nothing to score"):
        model.predictive_log_score(theta, suff, my_data, q.y_true)
    _assert_state_kept(eng, before)
    _same_bits(good, model.predictive_log_score(theta, suff, my_data, q.y_true, query=q.query, per_entry=True))
    # a query that names nothing: NaN score, every datapoint not visited
    score, info = model.predictive_log_score(theta, suff, my_data, q.y_true, query=np.zeros_like(q.query), per_entry=True)
    assert np.isnan(score) and info["n_not_queried"] == p.N and not info["count"].any() and np.isnan(info["logp"]).all()


def test_d_above_the_register_limit_is_refused(eng):
    p = problem("ebsc", 30, 512, 10, True, 1, False)
    D = 513
    rng = np.random.RandomState(1)
    model = _model(eng, "ebsc", D, p.H, p.S)
    theta = {"W": rng.normal(size=(D, p.H)), "pi": 0.1, "sigma": np.float64(1.0)}
    my_data = {"y": rng.normal(size=(p.N, D)), "x_infr": np.ones((p.N, D), dtype=bool)}
    suff = _suff(p.N, p.S, p.H, p.permanent, p.ss, p.lpj)
    with pytest.raises(EvoAmdError, match=r"D = 513, at most 512 observables are supported \(64 lanes x 8 registers\)"):
        model.predictive_log_score(theta, suff, my_data, my_data["y"], query=np.ones((p.N, D), dtype=bool))
    before = _device_state(eng)
    with pytest.raises(EvoAmdError, match="D = 513"):
        eng.predictive_score(my_data["y"], np.ones((p.N, D), dtype=bool))
    _assert_state_kept(eng, before)


def test_float32_mode_is_refused(eng):
    N, D, H, S = 32, 8, 16, 8
    np.random.seed(4)
    Y = np.random.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = BSC(D, H, S, engine=eng, dtype=np.float32)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1)
    with pytest.raises(NotImplementedError, match="float32 mode"):
        model.predictive_log_score(theta, suff, my_data, Y, query=np.ones_like(Y, dtype=bool))


# ---- 6. non-interference ----------------------------------------------------------------------------------------------------
def _run_steps(eng, algo, sync_host, with_call):
    N, D, H, S = 45, 10, 48, 16
    rng = np.random.RandomState(5)
    np.random.seed(6)
    Y = rng.normal(size=(N, D))
    query = rng.random_sample((N, D)) < 0.4
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, rng="device", sync_host=sync_host, seed=11)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 6, 1, 1)
    out = []
    F, nu, _, theta = model.step(theta, suff, my_data)
    out.append((F, nu))
    if with_call:
        keys = (list(theta), list(suff), list(my_data))
        score, info = model.predictive_log_score(theta, suff, my_data, Y, query=query)
        assert keys == (list(theta), list(suff), list(my_data))
        assert np.isfinite(score) and info["count"].sum() == query.sum() and info["n_singular"] == info["n_skipped"] == 0
    F, nu, _, theta = model.step(theta, suff, my_data)
    out.append((F, nu))
    if with_call:
        model.predictive_log_score(theta, suff, my_data, Y, query=query)
    codes = model.encode(theta, suff, my_data, max_active=8)
    return out, eng.download_states_packed(), {k: np.array(v) for k, v in theta.items()}, codes


@pytest.mark.parametrize("sync_host", [True, False])
@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_steps_and_encode_are_not_disturbed(eng, algo, sync_host):
    """Two steps with a call between them against two steps without, compared as
    tests/test_gpu_predictive.py::test_steps_and_encode_are_not_disturbed compares them (the statistics pass sums through
    f64 atomics: Theta and what is formed under it are held to 1e-12, the rest bit for bit)."""
    a = _run_steps(eng, algo, sync_host, with_call=False)
    b = _run_steps(eng, algo, sync_host, with_call=True)
    assert a[0][0] == b[0][0], (a[0], b[0])  # F and S_nunique of the first step
    assert a[0][1][1] == b[0][1][1]  # S_nunique of the second
    np.testing.assert_allclose(a[0][1][0], b[0][1][0], rtol=1e-12)
    assert np.array_equal(a[1], b[1])  # K^n
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        np.testing.assert_allclose(a[2][k], b[2][k], rtol=1e-12, atol=1e-12 * float(np.max(np.abs(a[2][k]))), err_msg=k)
    for f in ("idx", "nnz", "map_slot", "map_state"):
        assert np.array_equal(getattr(a[3], f), getattr(b[3], f)), f
    for f in ("p", "m", "map_q"):
        x, y = getattr(a[3], f), getattr(b[3], f)
        assert (x is None and y is None) or np.allclose(x, y, rtol=1e-10, atol=1e-12), f


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_device_state_is_left_bit_for_bit(eng, algo):
    """Fixed Theta: K^n, lpj, the candidate batch, the validity record, Theta, the moments predictive_moments left and the
    codes of a statistics pass read the same bits before and after Engine.predictive_score."""
    N, D, H, S = 45, 10, 48, 16
    rng = np.random.RandomState(5)
    np.random.seed(6)
    Y = rng.normal(size=(N, D))
    query = rng.random_sample((N, D)) < 0.4
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    model = (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng, rng="device", sync_host=False, seed=11)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 6, 1, 1)
    _, _, _, theta = model.step(theta, suff, my_data)
    codes0 = model.encode(theta, suff, my_data, max_active=8, dense=True)
    mean0, var0, _ = eng.predictive_moments()
    before = _device_state(eng)
    th0 = eng.get_params_bsc() if algo == "ebsc" else eng.get_params_sssc()
    res = eng.predictive_score(Y, query, per_entry=True)
    assert res["total_count"] == query.sum() and np.isfinite(res["sum"])
    _assert_state_kept(eng, before)
    th1 = eng.get_params_bsc() if algo == "ebsc" else eng.get_params_sssc()
    for k in th0:
        assert np.array_equal(th0[k], th1[k]), k
    assert np.array_equal(eng.download_predictive("mean"), mean0) and np.array_equal(eng.download_predictive("var"), var0)
    codes1 = eng.posterior_codes(8, 0.0)  # the rows of the statistics pass are still the current ones
    score2, info2 = model.predictive_log_score(theta, suff, my_data, Y, query=query, per_entry=True)
    assert np.array_equal(res["logp"], info2["logp"], equal_nan=True) and np.array_equal(res["pit"], info2["pit"], equal_nan=True)
    assert score2 == res["sum"] / res["total_count"]
    codes2 = model.encode(theta, suff, my_data, max_active=8, dense=True)
    for f in ("idx", "p", "m", "nnz", "map_slot", "map_q", "map_state"):
        for c in (codes1, codes2):
            x, y = getattr(codes0, f), getattr(c, f)
            assert (x is None and y is None) or np.array_equal(x, y), f
    assert np.array_equal(codes0.Es, codes2.Es)


def test_kernel_class_is_named(eng):
    assert _lib.KERNEL_IDS_EXTRA["predictive_score"] == 34
    assert eng.lib.evoamd_kernel_name(34) == b"predictive_score"
    q = score_problem("ebsc", 37, 25, 70, False, 1, False, noise=True)
    eng.timing(("predictive_score",))
    eng.timing_reset()
    _call(eng, q, True)
    ms, launches = eng.kernel_time_ms("predictive_score")
    eng.timing(False)
    assert launches == 1 and ms > 0.0

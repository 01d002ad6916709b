"""Local search on K^n on the GPU (Engine.sweep_propose / Engine.sweep_states / Model.sweep_resident_states,
csrc/kernels_sweep.hpp) against its NumPy mirror (evo_amd.variational.sweep_states_host) and by brute force.

1. proposals against the mirror; 2. the loop against the separate calls, bit for bit; 3. the rows it leaves equal a fresh
pass; 4. monotone and closed, by brute force at H = 10; 5. an under-seeded K^n improves; 6. refusals leave everything as
it was; 7. the Model level; 8. the plain, _ex and _nb entry points of the library give the same bits.
"""
import ctypes
import functools

import numpy as np
import pytest

import _sweep_problems as sp
from _seed_problems import make_data, make_theta
from evo_amd import _lib
from evo_amd._lib import check, dptr, i32ptr
from evo_amd.engine import Engine, EvoAmdError
from evo_amd.models import BSC, SSSC
from evo_amd.variational import seed_states_host, sweep_states_host

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ALLZERO = {"background": False, "allzero": True, "singletons": False}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def model_eng():
    e = Engine(0)
    yield e
    e.close()


def _set_theta(eng, model, th):
    if model == "sssc":
        eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    else:
        eng.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))


def _install(eng, p, Cmax=None):
    eng.configure(p.model, p.N, p.D, p.H, p.S, p.S_perm, p.Cmax if Cmax is None else Cmax)
    eng.upload_data(p.Y)
    _set_theta(eng, p.model, p.theta)
    eng.upload_states(p.ss)


def _logsumexp(rows):
    m = rows.max(axis=1)
    return m + np.log(np.exp(rows - m[:, None]).sum(axis=1))


# ---- 1. proposals against the mirror -------------------------------------------------------------------------------------
def _check_against_mirror(eng, p):
    _install(eng, p)
    res = eng.sweep_propose(p.P, p.q)
    cand, counts, lpjc = eng.download_candidates()
    rows = eng.download_lpj()
    assert np.array_equal(eng.download_states(), p.ss)
    err = np.abs(rows - p.lpj) / np.maximum(1.0, np.abs(p.lpj))
    print("%s: rows against the oracle %.3g" % (p.algo, err.max()))
    assert err.max() <= RTOL
    # the mirror on the GPU's own rows: the choice of the parents is exact
    m = sp.SweepProblem()
    m.N, m.Cmax = p.N, p.Cmax
    m.cand, m.counts, m.scores, m.best_flip, m.gain, m.n_capped, m.margin = sweep_states_host(
        p.model, p.theta, p.Y, p.ss, rows, p.S_perm, p.P, p.q)
    undecided = sp.compare_proposals(m, cand, counts)
    print("%s: %d of %d datapoints undecided, smallest margin %.3g" % (p.algo, len(undecided), p.N, m.margin.min()))
    assert len(undecided) <= 0.02 * p.N
    decided = np.setdiff1d(np.arange(p.N), undecided)
    assert np.array_equal(res["best_flip"][decided], m.best_flip[decided])
    assert np.array_equal(res["n_capped"], m.n_capped)
    worst = 0.0
    for n in range(p.N):
        c = counts[n]
        assert np.isnan(res["score"][n, c:]).all()
        if c:
            e = np.abs(res["score"][n, :c] - lpjc[n, :c]) / np.maximum(1.0, np.abs(lpjc[n, :c]))
            worst = max(worst, e.max())
        par = np.lexsort((np.arange(p.S), -rows[n, p.S_perm:]))[0]
        base = rows[n, p.S_perm + par]
        if np.isfinite(m.gain[n]):
            assert abs(res["gain"][n] - m.gain[n]) <= RTOL * max(1.0, abs(base)), (n, res["gain"][n], m.gain[n])
        else:
            assert np.array_equal(res["gain"][n], m.gain[n], equal_nan=True), (n, res["gain"][n], m.gain[n])
    print("%s: scores against the evaluated lpj %.3g" % (p.algo, worst))
    assert worst <= RTOL
    return res, cand, counts


@pytest.mark.parametrize("name", list(sp.CASES))
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_proposals_equal_the_mirror(eng, algo, name):
    _check_against_mirror(eng, sp.problem(algo, name))


def test_caps(eng):
    p = sp.caps_problem()
    res, cand, counts = _check_against_mirror(eng, p)
    assert np.array_equal(res["n_capped"], (p.sizes >= 8).astype(np.int32))
    assert (counts[p.sizes == 10] == 0).all() and (counts[p.sizes < 10] == p.q).all()
    assert np.isnan(res["gain"][p.sizes == 9]).all() and (res["gain"][p.sizes == 10] == -np.inf).all()


# ---- 2. / 3. the loop against the separate calls, the rows it leaves ----------------------------------------------------------
def _state(eng):
    return eng.download_states_packed(), eng.download_lpj()


@pytest.mark.parametrize("name", ["ragged_perm", "s200"])
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_loop_equals_separate_calls(eng, algo, name):
    p = sp.problem(algo, name)
    _install(eng, p)
    trace, n_done, cert = eng.sweep_states(1, p.P, p.q, stop_when_quiet=False)
    one = _state(eng)
    assert n_done == 1 and trace.shape == (1, 3)
    eng.upload_states(p.ss)
    res = eng.sweep_propose(p.P, p.q, want_scores=False)
    eng.set_estep_counts(0.0, 0.0)
    sums = eng.vary_kn(p.S)
    sep = _state(eng)
    assert np.array_equal(one[0], sep[0]) and np.array_equal(one[1], sep[1])
    assert np.array_equal(trace[0, 1:], sums), (trace, sums)
    for k in ("best_flip", "gain", "n_capped"):
        assert np.array_equal(cert[k], res[k], equal_nan=True), k
    assert not np.array_equal(one[0], np.packbits(p.ss, axis=-1)), "the sweep changed nothing"
    want = _logsumexp(one[1]).sum()
    assert abs(trace[0, 0] - want) <= RTOL * max(1.0, abs(want))
    # three sweeps are three single sweeps, and two runs give the same bits
    eng.upload_states(p.ss)
    t3, n3, c3 = eng.sweep_states(3, p.P, p.q, stop_when_quiet=False)
    three = _state(eng)
    eng.upload_states(p.ss)
    singles = [eng.sweep_states(1, p.P, p.q, stop_when_quiet=False) for _ in range(3)]
    again = _state(eng)
    assert n3 == 3
    assert np.array_equal(three[0], again[0]) and np.array_equal(three[1], again[1])
    assert np.array_equal(t3, np.concatenate([s[0] for s in singles]))
    for k in c3:
        assert np.array_equal(c3[k], singles[-1][2][k], equal_nan=True), k
    eng.upload_states(p.ss)
    t3b, _, _ = eng.sweep_states(3, p.P, p.q, stop_when_quiet=False)
    rerun = _state(eng)
    assert np.array_equal(t3, t3b) and np.array_equal(three[0], rerun[0]) and np.array_equal(three[1], rerun[1])
    # 3. the rows the loop leaves are those of a pass over the K^n it leaves
    eng.upload_states(eng.download_states())
    eng.lpj_resident()
    assert np.array_equal(eng.download_lpj(), three[1])


# ---- 4. monotone and closed ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(algo):
    return sp.build(algo, 33, 6, 10, 20, 0, 1, 10, 3, 3, 500)


@pytest.mark.parametrize("algo", sp.ALGOS)
def test_monotone_and_closed(eng, algo):
    p = _small(algo)
    _install(eng, p)
    trace, n_done, cert = eng.sweep_states(40, 1, p.Cmax, stop_when_quiet=True)
    print("%s: quiet after %d sweeps, Fs %s, swapped %s" % (algo, n_done, trace[:, 0], trace[:, 2]))
    assert 1 <= n_done < 40 and trace[-1, 2] == 0 and (trace[:-1, 2] > 0).all()
    # a swap replaces a state by one of larger lpj: the log-sum-exp of a row can only grow; 1e-12 covers its rounding
    assert (np.diff(trace[:, 0]) >= -1e-12 * np.abs(trace[:-1, 0])).all(), trace[:, 0]
    ss, rows = eng.download_states(), eng.download_lpj()
    assert (cert["n_capped"] == 0).all()
    for n in range(p.N):
        b = int(np.argmax(rows[n]))
        best, state = rows[n, b], ss[n, b]
        tol = RTOL * max(1.0, abs(best))
        nbs = np.repeat(state[None], p.H, axis=0)
        nbs[np.arange(p.H), np.arange(p.H)] ^= True
        lp, _ = eng.lpj_single(p.Y[n], nbs)
        for j in range(p.H):
            held = (ss[n] == nbs[j]).all(axis=1).any()
            if nbs[j].any() and not held:
                assert lp[j] <= best + tol, (n, j, lp[j], best)
        assert cert["gain"][n] <= tol, (n, cert["gain"][n])


# ---- 5. an under-seeded K^n improves ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_seeded_data_improves(eng, algo):
    N, D, H, S, Cmax = 33, 8, 30, 12, 8
    rng = np.random.RandomState(41 if algo == "ebsc" else 42)
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, N, k=3)
    model = sp.model_name(algo)
    eng.configure(model, N, D, H, S, 0, Cmax)
    eng.upload_data(Y)
    _set_theta(eng, model, theta)
    eng.seed_states(2)
    eng.lpj_resident()
    before = eng.posterior_scores(("F", "k_best"))
    trace, n_done, cert = eng.sweep_states(1, 1, Cmax, stop_when_quiet=False)
    after = eng.posterior_scores(("F", "k_best"))
    print("%s: Fs %.9g -> %.9g, best states that gained a latent: %d" % (
        algo, before["F"].sum(), trace[0, 0], (after["k_best"] > before["k_best"]).sum()))
    assert trace[0, 0] > before["F"].sum()
    assert abs(after["F"].sum() - trace[0, 0]) <= RTOL * abs(trace[0, 0])
    assert (after["k_best"] > before["k_best"]).any()
    assert (after["k_best"] <= 3).all()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def _refused(eng, call, match, states=True):
    def snapshot():
        return (eng.download_states_packed() if states else None, eng.download_lpj(), eng.debug_validity())

    before = snapshot()
    with pytest.raises(EvoAmdError, match=match):
        call()
    after = snapshot()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    assert before[2] == after[2], {k: (before[2][k], after[2][k]) for k in before[2] if before[2][k] != after[2][k]}


@pytest.mark.parametrize("algo", sp.ALGOS)
def test_refusals_leave_everything_as_it_was(eng, eng2, algo):
    p = sp.problem(algo, "ragged")
    for e in (eng, eng2):  # eng2: the same calls without the refusals in between
        _install(e, p)
        e.lpj_resident()
        e.evolve_randflip(2, 2, 5, True)
    S, C = p.S, p.Cmax
    for call, match in (
            (lambda: eng.sweep_propose(0, 1), "n_parents"),
            (lambda: eng.sweep_propose(S + 1, 1), "n_parents"),
            (lambda: eng.sweep_propose(1, 0), "n_keep"),
            (lambda: eng.sweep_propose(2, C // 2 + 1), "Cmax"),
            (lambda: eng.sweep_states(1, 1, C + 1), "Cmax"),
            (lambda: eng.sweep_states(1, 1, 1, Mprime=0), "Mprime"),
            (lambda: eng.sweep_states(1, 1, 1, Mprime=S + 1), "Mprime"),
            (lambda: eng.sweep_states(0, 1, 1), "n_sweeps")):
        _refused(eng, call, match)
    eng.set_option("background_unit", 1)
    _refused(eng, lambda: eng.sweep_propose(1, 1), "background_unit")
    _refused(eng, lambda: eng.sweep_states(1, 1, 1), "background_unit")
    eng.set_option("background_unit", 0)
    # the batch of before is still the resident one: selection and a statistics pass behave as after any selection
    for e in (eng, eng2):
        e.set_estep_counts(0.0, 0.0)
    assert np.array_equal(eng.vary_kn(S), eng2.vary_kn(S))
    va, vb = eng.acc_views(eng.stats()), eng2.acc_views(eng2.stats())
    for k in va:  # (the statistics pass sums with atomics: 1e-12 of the largest entry, as tests/test_gpu_refine.py allows)
        assert np.abs(va[k] - vb[k]).max() <= 1e-12 * max(1.0, float(np.abs(vb[k]).max())), k
    codes, codes2 = eng.posterior_codes(max_active=4), eng2.posterior_codes(max_active=4)
    assert np.array_equal(codes.map_slot, codes2.map_slot)
    # masks, bsc_direct, float32, no Theta, no data, no K^n
    eng.upload_masks(np.ones((p.N, p.D), dtype=bool))
    _refused(eng, lambda: eng.sweep_propose(1, 1), "incomplete data")
    eng.upload_masks(None)
    if algo == "ebsc":
        eng.set_option("bsc_direct", 1)
        _set_theta(eng, p.model, p.theta)  # (the option drops what was derived from Theta)
        _refused(eng, lambda: eng.sweep_propose(1, 1), "bsc_direct")
        eng.set_option("bsc_direct", 0)
        eng.set_option("ebsc_f32", 1)
        try:
            p4 = sp.build("ebsc", 9, 8, 16, 6, 0, 1, 4, 2, 2, 1)  # (the float32 mode asks for H % 4 == 0)
            _install(eng, p4)
            _refused(eng, lambda: eng.sweep_propose(1, 1), "float32")
        finally:
            eng.set_option("ebsc_f32", 0)
    eng.configure(p.model, p.N, p.D, p.H, p.S, p.S_perm, p.Cmax)
    _refused(eng, lambda: eng.sweep_propose(1, 1), "Theta")
    _set_theta(eng, p.model, p.theta)
    _refused(eng, lambda: eng.sweep_propose(1, 1), "no data")
    eng.upload_data(p.Y)
    with pytest.raises(EvoAmdError, match="max_rounds = 1 "):
        eng.init_states(1.0 / p.H, 17, max_rounds=1)
    _refused(eng, lambda: eng.sweep_propose(1, 1), "K\\^n is not on the device", states=False)  # (a lost K^n is not downloaded)


def test_refuses_keys_beyond_lds(eng):
    # EBSC keeps 16 bytes per latent: H = 9664 asks for more than a wavefront's share of 150 KiB
    N, D, H = 2, 2, 9664
    eng.configure("bsc", N, D, H, 2, 0, 2)
    eng.upload_data(np.ones((N, D)))
    eng.set_params_bsc(np.ones((D, H)), 0.01, 1.0)
    _refused(eng, lambda: eng.sweep_propose(1, 1), "LDS")


# ---- 7. the Model level ------------------------------------------------------------------------------------------------------
def _suff(ss, permanent=None):
    from evo_amd.variational import init_states
    N, S, H = ss.shape
    suff = init_states(0, S, H, "fit", "randflip", 4, 2, 1, permanent=permanent)
    suff["ss"] = ss.copy()
    suff["lpj"] = np.zeros((N, S + suff["S_perm"]))
    return suff


@pytest.mark.parametrize("S_perm", [0, 1])
@pytest.mark.parametrize("sync_host", [True, False])
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_model_level(model_eng, algo, sync_host, S_perm):
    cls = BSC if algo == "ebsc" else SSSC
    N, D, H, S = 29, 8, 30, 12
    rng = np.random.RandomState(61 if algo == "ebsc" else 62)
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, N, k=3)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    ss = seed_states_host(sp.model_name(algo), theta, Y, S, 2, S_perm)[0]
    # (nothing is drawn: either rng will do; rng="reference" itself asks for sync_host=True)
    model = cls(D, H, S, engine=model_eng, rng="reference" if sync_host else "device", sync_host=sync_host, seed=3)
    suff = _suff(ss, permanent=ALLZERO if S_perm else None)
    assert suff["S_perm"] == S_perm
    if not sync_host:
        suff["ss"] = suff["lpj"] = None
        model.attach_resident_states(suff, my_data, [(0, np.packbits(ss, axis=-1))])
    steps = model._n_steps
    res = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=3, n_parents=2, stop_when_quiet=False)
    assert model._n_steps == steps
    assert res.n_done == 3 and res.n_done_local == 3 and not res.stopped_early
    for a in (res.F, res.S_nunique, res.S_sub):
        assert a.shape == (3,) and a.dtype == np.float64
    assert res.gain.shape == (N,) and res.gain.dtype == np.float64
    assert res.best_flip.shape == (N,) and res.best_flip.dtype == np.int32
    assert res.n_capped.shape == (N,) and res.n_capped.dtype == np.int32 and (res.n_capped == 0).all()
    assert (res.S_sub[0] > 0) and (np.diff(res.F) >= -1e-12 * np.abs(res.F[:-1])).all()
    rows = model_eng.download_lpj()
    if sync_host:
        assert np.array_equal(suff["lpj"], rows) and np.array_equal(suff["ss"], model_eng.download_states())
        assert not np.array_equal(suff["ss"], ss)
    else:
        assert suff["ss"] is None and suff["lpj"] is None
    want = model_eng.ljc + _logsumexp(rows).sum() / N
    assert abs(res.F[-1] - want) <= RTOL * abs(want), (res.F[-1], want)
    codes = model.encode(dict(theta), suff, my_data, max_active=8)
    assert np.array_equal(codes.map_slot, rows.argmax(axis=1))
    with pytest.raises(ValueError, match="incomplete"):
        bad = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
        bad["x_infr"][0, 0] = False
        model.sweep_resident_states(dict(theta), suff, bad)
    with pytest.raises(ValueError, match="background"):
        model.sweep_resident_states(dict(theta), dict(suff, permanent={"background": True, "allzero": False, "singletons": False}),
                                    my_data)


def test_float32_model_refuses(model_eng):
    model = BSC(8, 16, 6, engine=model_eng, dtype=np.float32)
    with pytest.raises(NotImplementedError):
        model.sweep_resident_states({}, {"permanent": {"background": False}}, {})


def test_kernel_class_is_named(eng):
    from evo_amd import _lib
    assert eng.lib.evoamd_kernel_name(_lib.KERNEL_IDS_EXTRA["sweep"]) == b"sweep"


# ---- 8. the three generations of the ABI: Engine goes through the _nb calls alone, so the plain and the _ex calls are made here
def _sweep_buffers(eng, with_score):
    N = eng.N
    out = {"score": np.full((N, eng.Cmax), -7.0) if with_score else None, "best_flip": np.full(N, -7, dtype=np.int32),
           "gain": np.full(N, -7.0), "n_capped": np.full(N, -7, dtype=np.int32)}
    ptr = [None if a is None else (dptr(a) if a.dtype == np.float64 else i32ptr(a)) for a in out.values()]
    return out, ptr


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a if a[k] is not None)


@pytest.mark.parametrize("algo", sp.ALGOS)
def test_plain_ex_and_nb_propose_calls_agree(eng, algo):
    p = sp.problem(algo, "tight")
    _install(eng, p)
    got = []
    for call in ("plain", "ex", "nb"):
        eng.upload_states(p.ss)
        out, ptr = _sweep_buffers(eng, True)
        if call == "plain":
            check(eng.lib.evoamd_sweep_propose(eng._h, p.P, p.q, *ptr))
        elif call == "ex":
            check(eng.lib.evoamd_sweep_propose_ex(eng._h, p.P, p.q, 0, *ptr))
        else:
            so = _lib.SweepOut()
            so.score, so.best_flip, so.gain, so.n_capped = ptr
            check(eng.lib.evoamd_sweep_propose_nb(eng._h, p.P, p.q, 0, ctypes.byref(so)))
        assert not (out["best_flip"] == -7).any() and not (out["n_capped"] == -7).any()
        got.append((out, eng.download_candidates()))
    for out, cands in got[1:]:
        assert _same(out, got[0][0])
        (cand, counts, lpjc), (cand0, counts0, lpjc0) = cands, got[0][1]
        assert np.array_equal(counts, counts0) and counts.sum() > 0
        for n in range(p.N):  # the emitted rows (the batch behind them is not the call's)
            assert np.array_equal(cand[n, :counts[n]], cand0[n, :counts[n]])
            assert np.array_equal(lpjc[n, :counts[n]], lpjc0[n, :counts[n]])


@pytest.mark.parametrize("algo", sp.ALGOS)
def test_plain_ex_and_nb_states_calls_agree(eng, algo):
    p = sp.problem(algo, "tight")
    _install(eng, p)
    got = []
    for call in ("plain", "ex", "nb"):
        eng.upload_states(p.ss)
        out, ptr = _sweep_buffers(eng, False)
        trace, n_done = np.zeros((1, 3)), ctypes.c_int(0)
        head = (eng._h, 1, p.P, p.q, p.S, 0)
        if call == "plain":
            check(eng.lib.evoamd_sweep_states(*head, dptr(trace), ctypes.byref(n_done), *ptr[1:]))
        elif call == "ex":
            check(eng.lib.evoamd_sweep_states_ex(*head, 0, dptr(trace), ctypes.byref(n_done), *ptr[1:]))
        else:
            so = _lib.SweepOut()
            so.best_flip, so.gain, so.n_capped = ptr[1:]
            check(eng.lib.evoamd_sweep_states_nb(*head, 0, dptr(trace), ctypes.byref(n_done), ctypes.byref(so)))
        assert n_done.value == 1 and not (out["best_flip"] == -7).any()
        got.append((out, trace, _state(eng)))
    for out, trace, state in got[1:]:
        assert _same(out, got[0][0]) and np.array_equal(trace, got[0][1])
        assert all(np.array_equal(x, y) for x, y in zip(state, got[0][2]))

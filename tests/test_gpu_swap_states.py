"""The swap neighbourhood of the local search on K^n on the GPU (Engine.sweep_propose / Engine.sweep_states /
Model.sweep_resident_states with neighbourhood="swap" | "both", csrc/kernels_sweep_swap.hpp) against its NumPy mirror
(evo_amd.variational.swap_states_host) and by brute force.

1. proposals against the mirror, "both" against the flip call; 2. neighbourhood="flip" is the call without the keyword;
3. the loop against the separate calls, bit for bit, and the rows it leaves; 4. monotone and closed, by brute force at
H = 10; 5. swaps find what flips miss; 6. refusals leave everything as it was; 7. the Model level.
"""
import ctypes

import numpy as np
import pytest

import _sweep_problems as sp
import _swap_problems as wp
from _seed_problems import make_data, make_theta
from evo_amd import _lib
from evo_amd.engine import Engine, EvoAmdError
from evo_amd.models import BSC, SSSC
from evo_amd.models._models import SweepResult
from evo_amd.variational import seed_states_host, swap_states_host

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ALLZERO = {"background": False, "allzero": True, "singletons": False}
FLIP_KEYS = ("best_flip", "gain", "n_capped")
SWAP_KEYS = ("best_swap", "swap_gain", "n_capped_swap")


@pytest.fixture(scope="module")
def eng():
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


def _install(eng, p, Cmax):
    eng.configure(p.model, p.N, p.D, p.H, p.S, p.S_perm, Cmax)
    eng.upload_data(p.Y)
    _set_theta(eng, p.model, p.theta)
    eng.upload_states(p.ss)


def _logsumexp(rows):
    m = rows.max(axis=1)
    return m + np.log(np.exp(rows - m[:, None]).sum(axis=1))


# ---- 1. proposals against the mirror -------------------------------------------------------------------------------------
def _check_against_mirror(eng, p, nb):
    Cmax = p.P * p.q * (2 if nb == "both" else 1)
    first = np.zeros(p.N, dtype=np.int64)  # the first swap row of every datapoint
    if nb == "both":  # the flip call with the same q: its rows lead, bit for bit
        _install(eng, p, Cmax)
        flip = eng.sweep_propose(p.P, p.q)
        cand_f, counts_f, lpjc_f = eng.download_candidates()
        first = counts_f.astype(np.int64)
    _install(eng, p, Cmax)
    res = eng.sweep_propose(p.P, p.q, neighbourhood=nb)
    cand, counts, lpjc = eng.download_candidates()
    rows = eng.download_lpj()
    assert np.array_equal(eng.download_states(), p.ss)
    err = np.abs(rows - p.lpj) / np.maximum(1.0, np.abs(p.lpj))
    assert err.max() <= RTOL
    if nb == "both":
        for n in range(p.N):
            f = first[n]
            assert counts[n] >= f and np.array_equal(cand[n, :f], cand_f[n, :f]), n
            assert np.array_equal(res["score"][n, :f], flip["score"][n, :f]) and np.array_equal(lpjc[n, :f], lpjc_f[n, :f]), n
        for k in FLIP_KEYS:
            assert np.array_equal(res[k], flip[k], equal_nan=True), k
    else:
        assert all(res[k] is None for k in FLIP_KEYS)
    # the mirror on the GPU's own rows: the choice of the parents is exact
    m_cand, m_counts, m_scores, m_best, m_gain, m_capped, m_margin = swap_states_host(
        p.model, p.theta, p.Y, p.ss, rows, p.S_perm, p.P, p.q)
    got = np.zeros_like(m_cand)
    got_counts = counts - first
    for n in range(p.N):
        assert 0 <= got_counts[n] <= p.P * p.q, (n, counts[n], first[n])
        got[n, :got_counts[n]] = cand[n, first[n]:counts[n]]
    undecided = wp.compare_proposals(p.N, m_margin, m_cand, m_counts, got, got_counts)
    print("%s %s: %d of %d datapoints undecided, smallest margin %.3g" % (p.algo, nb, len(undecided), p.N, m_margin.min()))
    assert len(undecided) <= 0.02 * p.N
    decided = np.setdiff1d(np.arange(p.N), undecided)
    assert np.array_equal(res["best_swap"][decided], m_best[decided])
    assert np.array_equal(res["n_capped_swap"], m_capped)
    worst = 0.0
    for n in range(p.N):
        f, c = first[n], counts[n]
        assert np.isnan(res["score"][n, c:]).all()
        if c > f:
            e = np.abs(res["score"][n, f:c] - lpjc[n, f:c]) / np.maximum(1.0, np.abs(lpjc[n, f:c]))
            worst = max(worst, e.max())
        par = np.lexsort((np.arange(p.S), -rows[n, p.S_perm:]))[0]
        base = rows[n, p.S_perm + par]
        if np.isfinite(m_gain[n]):
            assert abs(res["swap_gain"][n] - m_gain[n]) <= RTOL * max(1.0, abs(base)), (n, res["swap_gain"][n], m_gain[n])
        else:
            assert res["swap_gain"][n] == m_gain[n] and tuple(res["best_swap"][n]) == (-1, -1), (n, res["swap_gain"][n])
    print("%s %s: swap scores against the evaluated lpj %.3g" % (p.algo, nb, worst))
    assert worst <= RTOL
    return res, counts - first


@pytest.mark.parametrize("nb", ["swap", "both"])
@pytest.mark.parametrize("name", list(wp.CASES))
@pytest.mark.parametrize("algo", wp.ALGOS)
def test_proposals_equal_the_mirror(eng, algo, name, nb):
    _check_against_mirror(eng, wp.problem(algo, name), nb)


@pytest.mark.parametrize("nb", ["swap", "both"])
@pytest.mark.parametrize("algo", wp.ALGOS)
def test_correlated_proposals_equal_the_mirror(eng, algo, nb):
    _check_against_mirror(eng, wp.correlated_problem(algo), nb)


@pytest.mark.parametrize("nb", ["swap", "both"])
def test_caps(eng, nb):
    p = wp.caps_problem()
    res, n_swaps = _check_against_mirror(eng, p, nb)
    assert np.array_equal(res["n_capped_swap"], (p.sizes > 8).astype(np.int32))
    assert (n_swaps[p.sizes > 8] == 0).all() and (n_swaps[p.sizes <= 8] == p.q).all()
    assert (res["swap_gain"][p.sizes > 8] == -np.inf).all() and np.isfinite(res["swap_gain"][p.sizes <= 8]).all()


# ---- 2. the keyword's default is the call without it ------------------------------------------------------------------------
def _state(eng):
    return eng.download_states_packed(), eng.download_lpj()


@pytest.mark.parametrize("algo", wp.ALGOS)
def test_flip_through_the_keyword_is_the_call_without_it(eng, algo):
    p = wp.problem(algo, "ragged_perm")
    out = []
    for kw in ({}, {"neighbourhood": "flip"}):
        _install(eng, p, p.Cmax)
        res = eng.sweep_propose(p.P, p.q, **kw)
        batch = eng.download_candidates()
        eng.upload_states(p.ss)
        trace, n_done, cert = eng.sweep_states(3, p.P, p.q, stop_when_quiet=False, **kw)
        out.append((res, batch, trace, n_done, cert, _state(eng)))
    a, b = out
    assert set(a[0]) == set(b[0]) == {"score", "best_flip", "gain", "n_capped"}
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k], equal_nan=True), k
    assert np.array_equal(a[1][1], b[1][1])
    for n in range(p.N):
        c = a[1][1][n]
        assert np.array_equal(a[1][0][n, :c], b[1][0][n, :c]) and np.array_equal(a[1][2][n, :c], b[1][2][n, :c])
    assert np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert set(a[4]) == set(b[4]) == set(FLIP_KEYS)
    for k in a[4]:
        assert np.array_equal(a[4][k], b[4][k], equal_nan=True), k
    assert np.array_equal(a[5][0], b[5][0]) and np.array_equal(a[5][1], b[5][1])


# ---- 3. the loop against the separate calls, the rows it leaves ----------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_perm", "s200"])
@pytest.mark.parametrize("algo", wp.ALGOS)
def test_loop_equals_separate_calls(eng, algo, name):
    p = wp.problem(algo, name)
    nb = dict(neighbourhood="both")
    _install(eng, p, p.Cmax_both)
    trace, n_done, cert = eng.sweep_states(1, p.P, p.q, stop_when_quiet=False, **nb)
    one = _state(eng)
    assert n_done == 1 and trace.shape == (1, 3)
    assert set(cert) == set(FLIP_KEYS + SWAP_KEYS)
    eng.upload_states(p.ss)
    res = eng.sweep_propose(p.P, p.q, want_scores=False, **nb)
    assert res["score"] is None
    eng.set_estep_counts(0.0, 0.0)
    sums = eng.vary_kn(p.S)
    sep = _state(eng)
    assert np.array_equal(one[0], sep[0]) and np.array_equal(one[1], sep[1])
    assert np.array_equal(trace[0, 1:], sums), (trace, sums)
    for k in cert:
        assert np.array_equal(cert[k], res[k], equal_nan=True), k
    assert not np.array_equal(one[0], np.packbits(p.ss, axis=-1)), "the sweep changed nothing"
    want = _logsumexp(one[1]).sum()
    assert abs(trace[0, 0] - want) <= RTOL * max(1.0, abs(want))
    # three sweeps are three single sweeps, and two runs give the same bits
    eng.upload_states(p.ss)
    t3, n3, c3 = eng.sweep_states(3, p.P, p.q, stop_when_quiet=False, **nb)
    three = _state(eng)
    eng.upload_states(p.ss)
    singles = [eng.sweep_states(1, p.P, p.q, stop_when_quiet=False, **nb) for _ in range(3)]
    again = _state(eng)
    assert n3 == 3
    assert np.array_equal(three[0], again[0]) and np.array_equal(three[1], again[1])
    assert np.array_equal(t3, np.concatenate([s[0] for s in singles]))
    for k in c3:
        assert np.array_equal(c3[k], singles[-1][2][k], equal_nan=True), k
    eng.upload_states(p.ss)
    t3b, _, c3b = eng.sweep_states(3, p.P, p.q, stop_when_quiet=False, **nb)
    rerun = _state(eng)
    assert np.array_equal(t3, t3b) and np.array_equal(three[0], rerun[0]) and np.array_equal(three[1], rerun[1])
    for k in c3:
        assert np.array_equal(c3[k], c3b[k], equal_nan=True), k
    # the rows the loop leaves are those of a pass over the K^n it leaves
    eng.upload_states(eng.download_states())
    eng.lpj_resident()
    assert np.array_equal(eng.download_lpj(), three[1])


# ---- 4. monotone and closed ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", wp.ALGOS)
def test_monotone_and_closed(eng, algo):
    p = wp.small(algo)
    _install(eng, p, p.Cmax_both)
    trace, n_done, cert = eng.sweep_states(40, 1, p.q, stop_when_quiet=True, neighbourhood="both")
    print("%s: quiet after %d sweeps, Fs %s, swapped %s" % (algo, n_done, trace[:, 0], trace[:, 2]))
    assert 1 <= n_done < 40 and trace[-1, 2] == 0 and (trace[:-1, 2] > 0).all()
    # a swap into K^n replaces a state by one of larger lpj: the log-sum-exp of a row can only grow; 1e-12 covers its rounding
    assert (np.diff(trace[:, 0]) >= -1e-12 * np.abs(trace[:-1, 0])).all(), trace[:, 0]
    ss, rows = eng.download_states(), eng.download_lpj()
    assert (cert["n_capped"] == 0).all() and (cert["n_capped_swap"] == 0).all()
    for n in range(p.N):
        b = int(np.argmax(rows[n]))
        best, state = rows[n, b], ss[n, b]
        tol = RTOL * max(1.0, abs(best))
        nbs = [state ^ (np.arange(p.H) == j) for j in range(p.H)]
        nbs += [state ^ ((np.arange(p.H) == a) | (np.arange(p.H) == j)) for a in np.flatnonzero(state) for j in np.flatnonzero(~state)]
        nbs = np.array(nbs)
        lp, _ = eng.lpj_single(p.Y[n], nbs)
        for i in range(len(nbs)):
            held = (ss[n] == nbs[i]).all(axis=1).any()
            if nbs[i].any() and not held:
                assert lp[i] <= best + tol, (n, i, lp[i], best)
        assert cert["gain"][n] <= tol, (n, cert["gain"][n])
        assert cert["swap_gain"][n] <= tol, (n, cert["swap_gain"][n])


# ---- 5. swaps find what flips miss ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", wp.ALGOS)
def test_swaps_find_what_flips_miss(eng, algo):
    p = wp.correlated_problem(algo)
    assert len(p.marked) >= 1
    _install(eng, p, 2 * p.P * p.q)
    t1, n1, c1 = eng.sweep_states(40, p.P, p.q, stop_when_quiet=True)
    assert n1 < 40 and t1[-1, 2] == 0
    rows1 = eng.download_lpj()
    t2, n2, c2 = eng.sweep_states(40, p.P, p.q, stop_when_quiet=True, neighbourhood="both")
    assert n2 < 40 and t2[-1, 2] == 0
    rows2 = eng.download_lpj()
    f1, f2 = _logsumexp(rows1), _logsumexp(rows2)
    print("%s: flips quiet after %d sweeps at Fs %.9g, both after %d more at %.9g; the %d marked datapoints gain %s" % (
        algo, n1, t1[-1, 0], n2, t2[-1, 0], len(p.marked), np.round((f2 - f1)[p.marked], 3)))
    assert (f2[p.marked] > f1[p.marked]).all()
    assert t2[-1, 0] > t1[-1, 0]
    assert (f2 >= f1 - 1e-12 * np.abs(f1)).all()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def _refused(eng, call, match):
    def snapshot():
        return eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.debug_validity()

    before = snapshot()
    with pytest.raises(EvoAmdError, match=match):
        call()
    after = snapshot()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert before[3] == after[3], {k: (before[3][k], after[3][k]) for k in before[3] if before[3][k] != after[3][k]}


@pytest.mark.parametrize("algo", wp.ALGOS)
def test_refusals_leave_everything_as_it_was(eng, algo):
    p = wp.problem(algo, "ragged")
    _install(eng, p, p.Cmax)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    S, C, h, lib = p.S, p.Cmax, eng._h, eng.lib
    trace, n_done = np.zeros((1, 3)), ctypes.c_int(0)

    def raw(rc):
        _lib.check(rc)

    for call, match in (
            (lambda: eng.sweep_propose(1, 1, neighbourhood="swap", incomplete=True), "EVOAMD_SWEEP_INCOMPLETE"),
            (lambda: eng.sweep_states(1, 1, 1, neighbourhood="both", incomplete=True), "EVOAMD_SWEEP_INCOMPLETE"),
            (lambda: raw(lib.evoamd_sweep_propose_nb(h, 1, 1, _lib.SWEEP_NO_FLIP, None)), "EVOAMD_SWEEP_NO_FLIP"),
            (lambda: raw(lib.evoamd_sweep_states_nb(h, 1, 1, 1, S, 1, _lib.SWEEP_NO_FLIP, _lib.dptr(trace), ctypes.byref(n_done),
                                                    None)), "EVOAMD_SWEEP_NO_FLIP"),
            (lambda: eng.sweep_propose(2, C // 4 + 1, neighbourhood="both"), "2 \\* n_parents \\* n_keep"),
            (lambda: eng.sweep_states(1, 2, C // 4 + 1, neighbourhood="both"), "2 \\* n_parents \\* n_keep"),
            (lambda: eng.sweep_propose(2, C // 2 + 1, neighbourhood="swap"), "Cmax"),
            (lambda: eng.sweep_propose(0, 1, neighbourhood="swap"), "n_parents"),
            (lambda: eng.sweep_propose(1, 0, neighbourhood="both"), "n_keep"),
            (lambda: eng.sweep_states(1, 1, 1, Mprime=0, neighbourhood="swap"), "Mprime"),
            (lambda: eng.sweep_states(0, 1, 1, neighbourhood="swap"), "n_sweeps"),
            (lambda: raw(lib.evoamd_sweep_propose_nb(h, 1, 1, 8, None)), "unknown flag"),
            # the _ex calls go on refusing every bit but EVOAMD_SWEEP_INCOMPLETE
            (lambda: raw(lib.evoamd_sweep_propose_ex(h, 1, 1, _lib.SWEEP_SWAP, None, None, None, None)), "unknown flag"),
            (lambda: raw(lib.evoamd_sweep_propose_ex(h, 1, 1, _lib.SWEEP_NO_FLIP, None, None, None, None)), "unknown flag"),
            (lambda: raw(lib.evoamd_sweep_states_ex(h, 1, 1, 1, S, 1, _lib.SWEEP_SWAP, _lib.dptr(trace), ctypes.byref(n_done),
                                                    None, None, None)), "unknown flag"),
            (lambda: raw(lib.evoamd_sweep_states_ex(h, 1, 1, 1, S, 1, _lib.SWEEP_SWAP | _lib.SWEEP_NO_FLIP, _lib.dptr(trace),
                                                    ctypes.byref(n_done), None, None, None)), "unknown flag")):
        _refused(eng, call, match)
    with pytest.raises(ValueError, match="neighbourhood"):
        eng.sweep_propose(1, 1, neighbourhood="two-flip")
    eng.set_option("background_unit", 1)
    _refused(eng, lambda: eng.sweep_propose(1, 1, neighbourhood="swap"), "background_unit")
    eng.set_option("background_unit", 0)
    # masks resident: swaps on incomplete data are out of scope, with or without the permission
    eng.upload_masks(np.ones((p.N, p.D), dtype=bool))
    _refused(eng, lambda: eng.sweep_propose(1, 1, neighbourhood="swap"), "incomplete data")
    _refused(eng, lambda: eng.sweep_states(1, 1, 1, neighbourhood="both"), "incomplete data")
    _refused(eng, lambda: eng.sweep_propose(1, 1, neighbourhood="both", incomplete=True), "EVOAMD_SWEEP_INCOMPLETE")
    eng.upload_masks(None)
    # and the context still sweeps
    trace, n_done, cert = eng.sweep_states(1, 1, 2, neighbourhood="both", stop_when_quiet=False)
    assert n_done == 1


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
@pytest.mark.parametrize("algo", wp.ALGOS)
def test_model_level(model_eng, algo, sync_host, S_perm):
    cls = BSC if algo == "ebsc" else SSSC
    N, D, H, S = 29, 8, 30, 12
    rng = np.random.RandomState(61 if algo == "ebsc" else 62)
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, N, k=3)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    ss = seed_states_host(sp.model_name(algo), theta, Y, S, 2, S_perm)[0]
    model = cls(D, H, S, engine=model_eng, rng="reference" if sync_host else "device", sync_host=sync_host, seed=3)
    suff = _suff(ss, permanent=ALLZERO if S_perm else None)
    assert suff["S_perm"] == S_perm
    if not sync_host:
        suff["ss"] = suff["lpj"] = None
        model.attach_resident_states(suff, my_data, [(0, np.packbits(ss, axis=-1))])
    steps = model._n_steps
    res = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=3, n_parents=2, stop_when_quiet=False,
                                      neighbourhood="both")
    assert model._n_steps == steps
    assert res.n_done == 3 and res.n_done_local == 3 and not res.stopped_early
    for a in (res.F, res.S_nunique, res.S_sub):
        assert a.shape == (3,) and a.dtype == np.float64
    assert res.gain.shape == (N,) and res.gain.dtype == np.float64
    assert res.best_flip.shape == (N,) and res.best_flip.dtype == np.int32
    assert res.n_capped.shape == (N,) and res.n_capped.dtype == np.int32 and (res.n_capped == 0).all()
    assert res.swap_gain.shape == (N,) and res.swap_gain.dtype == np.float64
    assert res.best_swap.shape == (N, 2) and res.best_swap.dtype == np.int32
    assert res.n_capped_swap.shape == (N,) and res.n_capped_swap.dtype == np.int32 and (res.n_capped_swap == 0).all()
    assert (res.S_sub[0] > 0) and (np.diff(res.F) >= -1e-12 * np.abs(res.F[:-1])).all()
    rows = model_eng.download_lpj()
    if sync_host:
        assert np.array_equal(suff["lpj"], rows) and np.array_equal(suff["ss"], model_eng.download_states())
        assert not np.array_equal(suff["ss"], ss)
    else:
        assert suff["ss"] is None and suff["lpj"] is None
    want = model_eng.ljc + _logsumexp(rows).sum() / N
    assert abs(res.F[-1] - want) <= RTOL * abs(want), (res.F[-1], want)
    only = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=1, neighbourhood="swap")
    assert only.gain is None and only.best_flip is None and only.n_capped is None
    assert only.swap_gain.shape == (N,) and only.best_swap.shape == (N, 2) and only.n_capped_swap.shape == (N,)
    plain = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=1)
    assert plain.swap_gain is None and plain.best_swap is None and plain.n_capped_swap is None and plain.gain.shape == (N,)
    for nb in ("swap", "both"):
        with pytest.raises(ValueError, match="incomplete=True with neighbourhood"):
            model.sweep_resident_states(dict(theta), suff, my_data, incomplete=True, neighbourhood=nb)
    with pytest.raises(ValueError, match="neighbourhood"):
        model.sweep_resident_states(dict(theta), suff, my_data, neighbourhood="two-flip")
    with pytest.raises(ValueError, match="background"):
        model.sweep_resident_states(dict(theta), dict(suff, permanent={"background": True, "allzero": False, "singletons": False}),
                                    my_data, neighbourhood="both")


def test_float32_model_refuses(model_eng):
    model = BSC(8, 16, 6, engine=model_eng, dtype=np.float32)
    with pytest.raises(NotImplementedError):
        model.sweep_resident_states({}, {"permanent": {"background": False}}, {}, neighbourhood="both")


def test_sweep_result_takes_the_swap_fields_with_none_defaults():
    r = SweepResult(np.zeros(1), np.zeros(1), np.zeros(1), 1, 1, False, None, None, None)
    assert r.swap_gain is None and r.best_swap is None and r.n_capped_swap is None


def test_kernel_class_is_named(eng):
    assert _lib.KERNEL_IDS_EXTRA["sweep_swap"] == 31
    assert eng.lib.evoamd_kernel_name(31) == b"sweep_swap"
    assert eng.lib.evoamd_kernel_name(_lib.KERNEL_IDS_EXTRA["sweep"]) == b"sweep"

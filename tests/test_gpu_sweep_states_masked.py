"""Local search on K^n from incomplete data on the GPU (Engine.sweep_propose / Engine.sweep_states /
Model.sweep_resident_states with ``incomplete=True``; csrc/kernels_sweep.hpp: sweep_neighbours_kernel<., MASKED>) against its
NumPy mirror (evo_amd.variational.sweep_states_host with ``x_infr``), the oracle's masked lpj and by brute force.

1. proposals against the mirror; 2. the masked kernel on all-True masks against the complete kernel; 3. the flag is a
permission; 4. the loop against the separate calls, bit for bit; 5. closed under one flip, by brute force at H = 10; 6. a
seeded K^n improves; 7. refusals leave everything as it was; 8. the Model level; 9. a complete problem after a masked one on
the same context.
"""
import functools

import numpy as np
import pytest

import _sweep_masked_problems as mp
import _sweep_problems as sp
from _seed_masked_problems import make_mask
from _seed_problems import make_data, make_theta
from evo_amd._lib import SWEEP_INCOMPLETE, check
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


def _install(eng, p, Cmax=None, x_infr="own"):
    """Data (NaN under the mask's False entries), the masks (None: none), Theta, K^n."""
    if isinstance(x_infr, str):
        x_infr = getattr(p, "x_infr", None)
    eng.configure(p.model, p.N, p.D, p.H, p.S, p.S_perm, p.Cmax if Cmax is None else Cmax)
    eng.upload_data(p.Y)
    if x_infr is not None:
        eng.upload_masks(x_infr)
        eng.set_reliable_fraction(x_infr.sum() / float(p.N))  # (enters ljc alone, which no score holds)
    _set_theta(eng, p.model, p.theta)
    eng.upload_states(p.ss)


def _logsumexp(rows):
    m = rows.max(axis=1)
    return m + np.log(np.exp(rows - m[:, None]).sum(axis=1))


# ---- 1. proposals against the mirror -------------------------------------------------------------------------------------
def _check_against_mirror(eng, p, incomplete=True):
    x_infr = getattr(p, "x_infr", None)
    res = eng.sweep_propose(p.P, p.q, incomplete=incomplete)
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
        p.model, p.theta, p.Y, p.ss, rows, p.S_perm, p.P, p.q, x_infr=x_infr)
    undecided = mp.compare_proposals(m, cand, counts, decided_tol=1e-7)
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


@pytest.mark.parametrize("algo,name,missing", mp.all_problems())
def test_proposals_equal_the_mirror(eng, algo, name, missing):
    p = mp.problem(algo, name, missing)
    _install(eng, p)
    _check_against_mirror(eng, p)


def test_caps(eng):
    p = mp.caps_problem()
    _install(eng, p)
    res, cand, counts = _check_against_mirror(eng, p)
    assert np.array_equal(res["n_capped"], (p.sizes >= 8).astype(np.int32))
    assert (counts[p.sizes == 10] == 0).all() and (counts[p.sizes < 10] == p.q).all()
    assert np.isnan(res["gain"][p.sizes == 9]).all() and (res["gain"][p.sizes == 10] == -np.inf).all()


# ---- 2. the masked kernel against the complete kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_perm", "s200", "tight"])
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_all_true_masks_equal_the_complete_kernel(eng, eng2, algo, name):
    p = sp.problem(algo, name)  # complete data
    _install(eng, p, x_infr=np.ones((p.N, p.D), dtype=bool))
    _install(eng2, p, x_infr=None)
    rm = eng.sweep_propose(p.P, p.q, incomplete=True)
    rc = eng2.sweep_propose(p.P, p.q)
    cm, nm, _ = eng.download_candidates()
    cc, nc, _ = eng2.download_candidates()
    rows = eng2.download_lpj()
    decided = np.flatnonzero(p.margin > 1e-7)
    assert len(decided) >= 0.98 * p.N
    worst = 0.0
    for n in decided:
        assert nm[n] == nc[n] and np.array_equal(cm[n, :nm[n]], cc[n, :nc[n]]), n
        c = nc[n]
        if c:
            a, b = rm["score"][n, :c], rc["score"][n, :c]
            worst = max(worst, (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
        base = rows[n, p.S_perm:].max()
        if np.isfinite(rc["gain"][n]):
            worst = max(worst, abs(rm["gain"][n] - rc["gain"][n]) / max(1.0, abs(base)))
        else:
            assert np.array_equal(rm["gain"][n], rc["gain"][n], equal_nan=True)
    print("%s %s: masked against complete scores and gains %.3g" % (algo, name, worst))
    assert worst <= 1e-10
    assert np.array_equal(rm["best_flip"][decided], rc["best_flip"][decided])
    assert np.array_equal(rm["n_capped"], rc["n_capped"])


# ---- 3. the flag is a permission ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_without_masks_the_flag_changes_nothing(eng, algo):
    p = sp.problem(algo, "ragged_perm")
    out = []
    for incomplete in (False, True):
        _install(eng, p, x_infr=None)
        res = eng.sweep_propose(p.P, p.q, incomplete=incomplete)
        out.append((res, eng.download_candidates()))
        _install(eng, p, x_infr=None)
        trace, n_done, cert = eng.sweep_states(2, p.P, p.q, stop_when_quiet=False, incomplete=incomplete)
        out[-1] += (trace, cert, eng.download_states_packed(), eng.download_lpj())
    (ra, ca, ta, certa, ka, la), (rb, cb, tb, certb, kb, lb) = out
    for k in ra:
        assert np.array_equal(ra[k], rb[k], equal_nan=True), k
    assert np.array_equal(ca[1], cb[1])
    for n in range(p.N):
        c = ca[1][n]
        assert np.array_equal(ca[0][n, :c], cb[0][n, :c]) and np.array_equal(ca[2][n, :c], cb[2][n, :c])
    assert np.array_equal(ta, tb) and np.array_equal(ka, kb) and np.array_equal(la, lb)
    for k in certa:
        assert np.array_equal(certa[k], certb[k], equal_nan=True), k


# ---- 4. the loop against the separate calls ----------------------------------------------------------------------------------
def _state(eng):
    return eng.download_states_packed(), eng.download_lpj()


@pytest.mark.parametrize("name,missing", [("ragged_perm", 0.3), ("s200", 0.6)])
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_loop_equals_separate_calls(eng, algo, name, missing):
    p = mp.problem(algo, name, missing)
    _install(eng, p)
    trace, n_done, cert = eng.sweep_states(1, p.P, p.q, stop_when_quiet=False, incomplete=True)
    one = _state(eng)
    assert n_done == 1 and trace.shape == (1, 3)
    eng.upload_states(p.ss)
    res = eng.sweep_propose(p.P, p.q, want_scores=False, incomplete=True)
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
    t3, n3, c3 = eng.sweep_states(3, p.P, p.q, stop_when_quiet=False, incomplete=True)
    three = _state(eng)
    eng.upload_states(p.ss)
    singles = [eng.sweep_states(1, p.P, p.q, stop_when_quiet=False, incomplete=True) for _ in range(3)]
    again = _state(eng)
    assert n3 == 3
    assert np.array_equal(three[0], again[0]) and np.array_equal(three[1], again[1])
    assert np.array_equal(t3, np.concatenate([s[0] for s in singles]))
    for k in c3:
        assert np.array_equal(c3[k], singles[-1][2][k], equal_nan=True), k
    # Fs per sweep never decreases (a swap replaces a state by one of larger lpj; 1e-12 covers the rounding of the sum)
    assert (np.diff(t3[:, 0]) >= -1e-12 * np.abs(t3[:-1, 0])).all(), t3[:, 0]
    # the rows the loop leaves are those of a pass over the K^n it leaves
    eng.upload_states(eng.download_states())
    eng.lpj_resident()
    assert np.array_equal(eng.download_lpj(), three[1])


# ---- 5. closed under one flip, by brute force -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(algo):
    return mp.build(algo, 33, 6, 10, 20, 0, 1, 10, 3, 3, 500, 0.3)


@pytest.mark.parametrize("algo", sp.ALGOS)
def test_monotone_and_closed(eng, algo):
    p = _small(algo)
    _install(eng, p)
    trace, n_done, cert = eng.sweep_states(40, 1, p.Cmax, stop_when_quiet=True, incomplete=True)
    print("%s: quiet after %d sweeps, Fs %s, swapped %s" % (algo, n_done, trace[:, 0], trace[:, 2]))
    assert 1 <= n_done < 40 and trace[-1, 2] == 0 and (trace[:-1, 2] > 0).all()
    assert (np.diff(trace[:, 0]) >= -1e-12 * np.abs(trace[:-1, 0])).all(), trace[:, 0]
    ss, rows = eng.download_states(), eng.download_lpj()
    assert (cert["n_capped"] == 0).all()
    oth = mp.oracle_theta(algo, p.theta, p.D, p.H, p.x_infr)
    for n in range(p.N):
        b = int(np.argmax(rows[n]))
        best, state = rows[n, b], ss[n, b]
        tol = RTOL * max(1.0, abs(best))
        nbs = np.repeat(state[None], p.H, axis=0)
        nbs[np.arange(p.H), np.arange(p.H)] ^= True
        lp = mp.oracle_lpj(algo, oth, p.Y[n], nbs, p.x_infr[n])
        for j in range(p.H):
            held = (ss[n] == nbs[j]).all(axis=1).any()
            if nbs[j].any() and not held:
                assert lp[j] <= best + RTOL * max(1.0, abs(lp[j])), (n, j, lp[j], best)
        assert cert["gain"][n] <= tol, (n, cert["gain"][n])


# ---- 6. a seeded K^n improves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("missing", mp.FRACTIONS)
@pytest.mark.parametrize("algo", sp.ALGOS)
def test_seeded_masked_data_improves(eng, algo, missing):
    rose = []
    for name in ("ragged", "s200"):
        p = mp.problem(algo, name, missing)
        _install(eng, p)
        eng.lpj_resident()
        before = eng.posterior_scores(("F",))["F"].sum()
        trace, n_done, cert = eng.sweep_states(4, p.P, p.q, stop_when_quiet=False, incomplete=True)
        print("%s %s %.1f: Fs %.9g -> %s, gain <= 0 at %d of %d" % (algo, name, missing, before, trace[:, 0],
                                                                   (cert["gain"] <= 0).sum(), p.N))
        assert trace[-1, 0] >= before - 1e-12 * abs(before)
        rose.append(trace[-1, 0] > before + 1e-9 * abs(before))
    assert any(rose)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def _refused(eng, call, match, cands=True):
    def snapshot():
        return (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates() if cands else (),
                eng.debug_validity())

    before = snapshot()
    with pytest.raises(EvoAmdError, match=match):
        call()
    after = snapshot()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    for a, b in zip(before[2], after[2]):
        assert np.array_equal(a, b, equal_nan=True)
    assert before[3] == after[3], {k: (before[3][k], after[3][k]) for k in before[3] if before[3][k] != after[3][k]}


@pytest.mark.parametrize("algo", sp.ALGOS)
def test_refusals_leave_everything_as_it_was(eng, algo):
    p = mp.problem(algo, "ragged", 0.3)
    _install(eng, p)
    eng.sweep_propose(p.P, p.q, incomplete=True)  # a batch is resident
    C = p.Cmax
    none = (None,) * 4
    for call, match in (
            (lambda: eng.sweep_propose(1, 1), "incomplete data"),  # masks present and no permission: the old message
            (lambda: eng.sweep_states(1, 1, 1), "incomplete data"),
            (lambda: check(eng.lib.evoamd_sweep_propose_ex(eng._h, 1, 1, SWEEP_INCOMPLETE | 2, *none)), "unknown flag"),
            (lambda: check(eng.lib.evoamd_sweep_propose_ex(eng._h, 1, 1, 1 << 31, *none)), "unknown flag"),
            (lambda: eng.sweep_propose(2, C // 2 + 1, incomplete=True), "Cmax"),
            (lambda: eng.sweep_states(1, 1, C + 1, incomplete=True), "Cmax"),
            (lambda: eng.sweep_propose(0, 1, incomplete=True), "n_parents"),
            (lambda: eng.sweep_states(1, 1, 1, Mprime=0, incomplete=True), "Mprime")):
        _refused(eng, call, match)
    eng.set_option("background_unit", 1)
    try:
        _refused(eng, lambda: eng.sweep_propose(1, 1, incomplete=True), "background_unit")
        _refused(eng, lambda: eng.sweep_states(1, 1, 1, incomplete=True), "background_unit")
    finally:
        eng.set_option("background_unit", 0)
    eng.sweep_propose(p.P, p.q, incomplete=True)  # admitted


def test_float32_refuses_with_the_flag(eng):
    # (the float32 mode admits no masks at all: the flag alone must not open it)
    eng.set_option("ebsc_f32", 1)
    try:
        p4 = sp.build("ebsc", 9, 8, 16, 6, 0, 1, 4, 2, 2, 1)  # (the float32 mode asks for H % 4 == 0)
        _install(eng, p4, x_infr=None)
        eng.lpj_resident()
        _refused(eng, lambda: eng.sweep_propose(1, 1, incomplete=True), "float32", cands=False)
        _refused(eng, lambda: eng.sweep_states(1, 1, 1, incomplete=True), "float32", cands=False)
    finally:
        eng.set_option("ebsc_f32", 0)
        eng.configure("bsc", 4, 4, 8, 4, 0, 4)


def test_refuses_column_and_list_beyond_lds(eng):
    # the staged column and the list of the reliable entries take 12 D bytes: D = 12900 asks for more than a wavefront's
    # share of 150 KiB at one wavefront per workgroup
    N, D, H = 2, 12900, 4
    rng = np.random.RandomState(3)
    eng.configure("bsc", N, D, H, 2, 0, 2)
    eng.upload_data(rng.normal(size=(N, D)))
    eng.upload_masks(make_mask(rng, N, D, 0.5))
    eng.set_params_bsc(rng.normal(size=(D, H)), 0.3, 1.0)
    ss = np.zeros((N, 2, H), dtype=bool)
    ss[:, 0, 0] = ss[:, 1, 1] = True
    eng.upload_states(ss)
    before = eng.download_states_packed(), eng.debug_validity()
    with pytest.raises(EvoAmdError, match="staged column.*reliable entries.*LDS"):
        eng.sweep_propose(1, 1, incomplete=True)
    assert np.array_equal(eng.download_states_packed(), before[0]) and eng.debug_validity() == before[1]


# ---- 8. the Model level --------------------------------------------------------------------------------------------------------
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
    xi = make_mask(rng, N, D, 0.4)
    Yn = np.where(xi, Y, np.nan)
    my_data = {"y": Yn, "x_infr": xi, "x": xi.copy()}
    ss = seed_states_host(sp.model_name(algo), theta, Yn, S, 2, S_perm, x_infr=xi)[0]
    model = cls(D, H, S, engine=model_eng, rng="reference" if sync_host else "device", sync_host=sync_host, seed=3)
    suff = _suff(ss, permanent=ALLZERO if S_perm else None)
    assert suff["S_perm"] == S_perm
    with pytest.raises(ValueError, match="incomplete"):
        model.sweep_resident_states(dict(theta), suff, my_data)
    if not sync_host:
        suff["ss"] = suff["lpj"] = None
        model.attach_resident_states(suff, my_data, [(0, np.packbits(ss, axis=-1))])
    steps = model._n_steps
    res = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=3, n_parents=2, stop_when_quiet=False,
                                      incomplete=True)
    assert model._n_steps == steps
    assert res.n_done == 3 and res.n_done_local == 3 and not res.stopped_early
    assert res.gain.shape == (N,) and res.best_flip.dtype == np.int32 and (res.n_capped == 0).all()
    assert (res.S_sub[0] > 0) and (np.diff(res.F) >= -1e-12 * np.abs(res.F[:-1])).all()
    kn = model_eng.download_states()
    if sync_host:
        assert np.array_equal(suff["ss"], kn) and np.array_equal(suff["lpj"], model_eng.download_lpj())
        assert not np.array_equal(suff["ss"], ss)
    else:
        assert suff["ss"] is None and suff["lpj"] is None
    # F against the oracle's masked ljc and lpj of the K^n the sweeps left
    oth = mp.oracle_theta(algo, theta, D, H, xi)
    rows = mp.rows_of(algo, theta, Yn, xi, kn, S_perm)
    want = float(oth["ljc"]) + _logsumexp(rows).mean()
    print("%s sync_host=%s S_perm=%d: F %s, oracle %.12g" % (algo, sync_host, S_perm, res.F, want))
    assert abs(res.F[-1] - want) <= 1e-9 * max(1.0, abs(want)), (res.F[-1], want)
    scores = model.posterior_scores(dict(theta), suff, my_data)
    lse = _logsumexp(rows)
    assert (np.abs(scores["F"] - lse) <= 1e-9 * np.maximum(1.0, np.abs(lse))).all()
    with pytest.raises(ValueError, match="incomplete"):
        model.sweep_resident_states(dict(theta), suff, my_data)


# ---- 9. a complete problem after a masked one, on the same context ------------------------------------------------------------------
@pytest.mark.parametrize("algo,first", [("ebsc", "wide_d"), ("es3c", "ragged"), ("es3c", "rows_gmem")])
def test_complete_problem_after_a_masked_one(eng, algo, first):
    p = mp.problem(algo, first, 0.6)
    _install(eng, p)
    eng.sweep_states(2, p.P, p.q, stop_when_quiet=False, incomplete=True)
    big = sp.problem(algo, "s200")  # more states, another H and D; no masks
    _install(eng, big, x_infr=None)
    _check_against_mirror(eng, big, incomplete=False)

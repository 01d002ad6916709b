"""The AIS rescue on the GPU (Engine.ais_posterior / Model.ais_posterior with ``index`` and ``admit``, evoamd_ais_posterior_sel;
csrc/kernels_ais_post.hpp) against the device's own full call, the NumPy mirrors and the oracle's selection.

1. a listed call equals the rows of the full call bit for bit, and the mirror where its chains are decided; 2. the emission
kernel alone (the probe) on the hand-made inputs; 3. admission against host selection; 4. through the model; 5. refusals.
"""
import ctypes

import numpy as np
import pytest

import _ais_masked_problems as mp
import _ais_post_problems as pp
import _ais_rescue_problems as rp
import _sweep_problems as sp
from evo_amd import _lib
from evo_amd.engine import Engine, EvoAmdError
from evo_amd.models import BSC, ais_admit_candidates_host, state_digest
from evo_amd.variational import init_states
from oracle import evo_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-9


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


def _install(eng, p, S=4, Cmax=4, ss=None, x_infr=None):
    eng.configure("bsc", p.N, p.D, p.H, S, 0, Cmax)
    eng.upload_data(p.Y)
    if x_infr is not None:
        eng.upload_masks(np.ascontiguousarray(x_infr))
        eng.set_reliable_fraction(x_infr.sum() / float(p.N))
    eng.set_params_bsc(p.theta["W"], float(p.theta["pi"]), float(p.theta["sigma"]))
    if ss is not None:
        eng.upload_states(ss)


def _close(a, b):
    return np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b))


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f") if isinstance(a[k], np.ndarray)
                                        else a[k] == b[k] for k in a)


def _against_the_mirror(got, want, I):
    """The rule of tests/test_gpu_ais_post.py on the listed rows: decided chains bit for bit, the rest at most MAX_UNDECIDED."""
    decided = want["margin"][I] > rp.MARGIN_DECIDED
    same = (got["chain_flips"] == want["chain_flips"][I]) & (got["chain_map_state"] == want["chain_map_state"][I]).all(axis=2)
    assert same[decided].all(), np.argwhere(decided & ~same)
    for k in ("log_w", "rb", "chain_map_lpj"):
        e = np.abs(got[k] - want[k][I]) / np.maximum(1.0, np.abs(want[k][I]))
        assert (e[decided] <= RTOL).all(), k
    assert (~decided).sum() <= rp.MAX_UNDECIDED * decided.size
    rows = decided.all(axis=1)
    for k in ("p", "p_se", "count", "map_lpj", "ll", "ess", "mean"):
        assert _close(got[k][rows], want[k][I][rows]).all(), k
    assert np.array_equal(got["map_state"][rows], want["map_state"][I][rows])


# ---- 1. listed equals full -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rp.LISTS))
def test_listed_equals_the_rows_of_the_full_call(eng, name):
    p = pp.problem(name)
    I = np.array(rp.LISTS[name])
    _install(eng, p)
    kw = dict(n_chains=p.C, n_keep=p.K, seed=pp.STREAM_SEED, mean=True, keep_chains=True)
    full = eng.ais_posterior(p.betas, **kw)
    got = eng.ais_posterior(p.betas, index=I, **kw)
    assert got.keys() == full.keys()
    for k in full:
        assert got[k].shape == full[k][I].shape and got[k].dtype == full[k].dtype and np.array_equal(got[k], full[k][I]), k
    _against_the_mirror(got, p.want, I)
    # a block boundary inside the list changes nothing, nor does a list of everything
    assert _same(eng.ais_posterior(p.betas, index=I, block=2, **kw), got)
    assert _same(eng.ais_posterior(p.betas, index=np.arange(p.N), **kw), full)
    # first_index is added to the list's entries
    shifted = eng.ais_posterior(p.betas, index=I, first_index=5, **kw)
    assert _same(shifted, {k: v[I] for k, v in eng.ais_posterior(p.betas, first_index=5, **kw).items()})
    assert not np.array_equal(shifted["log_w"], got["log_w"])


def test_listed_equals_the_rows_of_the_full_call_on_incomplete_data(eng):
    name, missing = rp.MASKED_CASE
    p = mp.problem(name, missing)
    I = np.array(rp.MASKED_LIST)
    _install(eng, p, x_infr=p.x_infr)
    kw = dict(n_chains=mp.C, n_keep=3, seed=mp.STREAM_SEED, mean=True, keep_chains=True, incomplete=True)
    full = eng.ais_posterior(p.betas, **kw)
    got = eng.ais_posterior(p.betas, index=I, **kw)
    for k in full:
        assert got[k].shape == full[k][I].shape and np.array_equal(got[k], full[k][I]), k
    _against_the_mirror(got, p.post[3], I)
    assert _same(eng.ais_posterior(p.betas, index=I, block=2, **kw), got)
    eng.upload_masks(None)


# ---- 2. the emission kernel alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("digests", [True, False])
def test_emission_on_the_hand_made_inputs(eng, digests):
    h = rp.HAND
    N, C, H, S, Cmax = h["N"], h["C"], h["H"], h["S"], h["Cmax"]
    rng = np.random.RandomState(1)
    eng.set_option("state_digest", 1 if digests else 0)
    try:
        eng.configure("bsc", N, h["D"], H, S, 0, Cmax)
        eng.upload_data(rng.normal(size=(N, h["D"])))
        eng.set_params_bsc(rng.normal(size=(h["D"], H)), 0.1, 1.0)
        kn = rp.hand_kn()
        eng.upload_states(kn)
        lpj, st = rp.hand_inputs()
        got = eng.ais_post_admit_probe(lpj, st, index=rp.HAND_INDEX)
        cand, counts, _ = eng.download_candidates()
        assert (got["digests"] is not None) == digests
        assert counts[3] == 0, "cand_counts outside the list"
        for i, n in enumerate(rp.HAND_INDEX):
            want, cnt = ais_admit_candidates_host(lpj[i], st[i], kn[n], Cmax)
            assert counts[n] == cnt["n_proposed"] == got["n_proposed"][i], n
            assert np.array_equal(cand[n, :counts[n]], want), n
            assert (got["n_distinct"][i], got["n_new"][i], bool(got["map_held"][i])) == (cnt["n_distinct"], cnt["n_new"],
                                                                                         cnt["map_held"]), n
            if digests:
                assert [int(d) for d in got["digests"][n, :counts[n]]] == [state_digest(row) for row in want], n
        assert np.array_equal(eng.download_states(), kn), "the probe wrote K^n"
        # without a list: every datapoint, row = datapoint
        lpj6, st6 = np.insert(lpj, 3, lpj[0], axis=0), np.insert(st, 3, st[0], axis=0)
        all_rows = eng.ais_post_admit_probe(lpj6, st6)
        cand6, counts6, _ = eng.download_candidates()
        assert counts6[3] == 3 and np.array_equal(cand6[3, :3], cand[0, :3])
        for k in ("n_distinct", "n_new", "n_proposed", "map_held"):
            assert np.array_equal(np.delete(all_rows[k], 3), got[k]), k
    finally:
        eng.set_option("state_digest", 1)


# ---- 3. admission against host selection ---------------------------------------------------------------------------------------
def test_admission_equals_host_selection(eng):
    q = rp.admit_problem()
    p, S, Cmax, I, ss = q.p, q.S, q.Cmax, q.index, q.ss
    _install(eng, p, S, Cmax, ss)
    eng.lpj_resident()
    lpj0 = eng.download_lpj()
    kw = dict(n_chains=p.C, n_keep=p.K, seed=pp.STREAM_SEED, keep_chains=True, mean=True)
    got = eng.ais_posterior(p.betas, index=I, admit=True, Mprime=S, **kw)
    new_ss, new_lpj = eng.download_states(), eng.download_lpj()
    cand, counts, _ = eng.download_candidates()
    # unlisted datapoints: nothing proposed, K^n and lpj as they were
    out = np.setdiff1d(np.arange(p.N), I)
    assert (counts[out] == 0).all()
    assert np.array_equal(new_ss[out], ss[out]) and np.array_equal(new_lpj[out], lpj0[out])
    assert (got["F_after"] >= got["F_before"]).all() and got["S_sub"] > 0.0
    assert (got["n_admitted"] <= got["n_proposed"]).all() and (got["n_proposed"] <= got["n_new"]).all()
    assert (got["n_new"] <= got["n_distinct"]).all() and (got["n_distinct"] <= p.C).all()
    assert got["n_admitted"].sum() > 0
    oth = sp.oracle_theta("ebsc", p.theta, p.D, p.H)
    incl = np.zeros((0, p.H), dtype=bool)
    chain_bool = pp.unpack(got["chain_map_state"], p.H)
    map_bool = pp.unpack(got["map_state"], p.H)
    checked = 0
    for i, n in enumerate(I):
        assert len({row.tobytes() for row in np.packbits(new_ss[n], axis=-1)}) == S, "datapoint %d lost a state" % n
        # the candidates are the mirror's, from the device's own chain_map_*
        fin, cnt = ais_admit_candidates_host(got["chain_map_lpj"][i], chain_bool[i], ss[n], Cmax)
        assert counts[n] == len(fin) and np.array_equal(cand[n, :counts[n]], fin), n
        for k in ("n_distinct", "n_new", "n_proposed"):
            assert got[k][i] == cnt[k], (k, n)
        assert bool(got["map_held_before"][i]) == cnt["map_held"] == bool((ss[n] == map_bool[i]).all(axis=1).any()), n
        held = lambda row: bool((new_ss[n] == row).all(axis=1).any())  # noqa: E731
        assert got["n_admitted"][i] == sum(held(row) for row in fin), n
        assert bool(got["map_held_after"][i]) == held(map_bool[i]), n
        old_lpj = sp.oracle_lpj("ebsc", oth, p.Y[n], ss[n])
        proposed = any((row == map_bool[i]).all() for row in fin)
        if proposed and got["map_lpj"][i] > lpj0[n].min():  # (the device's own rows before)
            assert got["map_held_after"][i], "map_state was proposed above the worst of K^n and is not held (%d)" % n
        if got["map_held_before"][i]:
            assert got["map_held_after"][i] or got["n_admitted"][i] > 0, n
        want_ss, want_lpj = ss[n].copy(), old_lpj.copy()
        if len(fin):
            cand_lpj = sp.oracle_lpj("ebsc", oth, p.Y[n], fin)
            pool = np.sort(np.concatenate([old_lpj, cand_lpj]))
            if len(pool) > 1 and np.diff(pool).min() <= 1e-7 * max(1.0, np.abs(pool).max()):
                continue  # the ranking is not decided at the precision of the rows
            orc.vary_Kn(old_lpj.copy(), cand_lpj.copy(), want_lpj, want_ss, fin, p.H, S, 0, incl, S)
        assert ({r.tobytes() for r in np.packbits(new_ss[n], axis=-1)} == {r.tobytes() for r in np.packbits(want_ss, axis=-1)}), n
        assert _close(np.sort(new_lpj[n]), np.sort(want_lpj)).all(), n
        checked += 1
    print("rescue: %d of %d listed datapoints checked against host selection; n_new %d, n_proposed %d, n_admitted %d, S_sub %.0f"
          % (checked, len(I), got["n_new"].sum(), got["n_proposed"].sum(), got["n_admitted"].sum(), got["S_sub"]))
    assert checked * 2 >= len(I)
    # the chain outputs are those of the call without admit
    _install(eng, p, S, Cmax, ss)
    plain = eng.ais_posterior(p.betas, index=I, **kw)
    for k in plain:
        assert np.array_equal(plain[k], got[k]), k


# ---- 4. through the model ------------------------------------------------------------------------------------------------------
def _suff(ss):
    N, S, H = ss.shape
    suff = init_states(0, S, H, "fit", "randflip", 6, 5, 1)
    suff["ss"] = ss.copy()
    suff["lpj"] = np.zeros((N, S))
    return suff


def test_rescue_through_the_model(model_eng):
    q = rp.admit_problem()
    p, S, I = q.p, q.S, q.index
    model = BSC(p.D, p.H, S, engine=model_eng)
    suff = _suff(q.ss)
    data = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    suff["lpj"] = sp.rows_of("ebsc", p.theta, p.Y, q.ss, 0)
    F0 = model.posterior_scores(p.theta, suff, data)["F"]
    kw = dict(n_chains=p.C, n_temps=p.T, n_keep=p.K, seed=4)
    # without admit nothing of the EM state is written
    before = (model_eng.download_states_packed(), model_eng.download_lpj())
    plain = model.ais_posterior(p.theta, suff, data, index=I, **kw)
    again = model.ais_posterior(p.theta, suff, data, index=I, **kw)
    assert _same(plain, again), "two calls differ"
    after = (model_eng.download_states_packed(), model_eng.download_lpj())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(suff["ss"], q.ss)
    assert set(plain) == {"p", "p_se", "count", "map_lpj", "map_state", "ll", "ess", "log_w_mean", "log_w_min", "log_w_max", "n_flips"}
    assert all(len(v) == len(I) for v in plain.values())
    # an empty list: empty arrays, S_sub = 0
    empty = model.ais_posterior(p.theta, suff, data, index=[], admit=True, **kw)
    assert empty["p"].shape == (0, p.H) and empty["F_after"].shape == (0,) and empty["n_new"].shape == (0,) and empty["S_sub"] == 0.0
    assert np.array_equal(model_eng.download_states_packed(), before[0])
    # admit: K^n comes back, F at the listed rows is F_after
    info = model.ais_posterior(p.theta, suff, data, index=I, admit=True, **kw)
    assert _close(info["F_before"], F0[I]).all() and (info["F_after"] >= info["F_before"]).all() and info["S_sub"] > 0.0
    assert "S_nunique" not in info and info["map_held_before"].dtype == np.bool_ and info["n_new"].dtype == np.int32
    assert np.array_equal(suff["ss"], model_eng.download_states()) and not np.array_equal(suff["ss"], q.ss)
    F1 = model.posterior_scores(p.theta, suff, data)["F"]
    assert _close(F1[I], info["F_after"]).all()
    out = np.setdiff1d(np.arange(p.N), I)
    assert np.array_equal(suff["ss"][out], q.ss[out]) and _close(F1[out], F0[out]).all()
    for k in plain:
        assert np.array_equal(plain[k], info[k]), k
    with pytest.raises(ValueError, match=r"index\[1\] = 0 is repeated"):
        model.ais_posterior(p.theta, suff, data, index=[0, 0], **kw)


def test_candidate_batch_is_untouched_without_admit(eng):
    q = rp.admit_problem()
    p = q.p
    _install(eng, p, q.S, q.Cmax, q.ss)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    before = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.debug_validity())
    a = eng.ais_posterior(p.betas, p.C, p.K, 9, 0, index=q.index, keep_chains=True)
    b = eng.ais_posterior(p.betas, p.C, p.K, 9, 0, index=q.index, keep_chains=True)
    assert _same(a, b)
    after = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.debug_validity())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[3] == after[3]
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    # admit twice from the same start gives the same bits
    res = []
    for _ in range(2):
        _install(eng, p, q.S, q.Cmax, q.ss)
        res.append((eng.ais_posterior(p.betas, p.C, p.K, 9, 0, index=q.index, admit=True, Mprime=q.S), eng.download_states_packed(),
                    eng.download_lpj()))
    assert _same(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(eng, call, match, exc=EvoAmdError):
    before = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.debug_validity())
    with pytest.raises(exc, match=match):
        call()
    after = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.debug_validity())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert before[3] == after[3]


def _sel(eng, p, index, n_index=None, flags=0, Mprime=1, n_chains=3):
    """evoamd_ais_posterior_sel as the ABI takes it: the list unchecked by Python."""
    idx = np.ascontiguousarray(index, dtype=np.int64)
    betas = np.ascontiguousarray(p.betas)
    _lib.check(eng.lib.evoamd_ais_posterior_sel(
        eng._h, n_chains, betas.size - 1, 2, _lib.dptr(betas), 1, 0, 0, flags, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
        len(idx) if n_index is None else n_index, Mprime, None))


def test_refusals_leave_the_context_usable(eng):
    p = pp.problem("partial_chunk")
    S, Cmax = 6, 4
    ss = rp.kn_states(p, S)
    _install(eng, p, S, Cmax, ss)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    b = p.betas
    I = np.array([0, 5, 36])
    first = eng.ais_posterior(b, 3, 2, 1, 0, index=I, keep_chains=True)
    A = _lib.AIS_ADMIT
    for call, match in (
            (lambda: _sel(eng, p, [0, 5, 5]), r"evoamd_ais_posterior_sel: index\[2\] = 5 is repeated"),
            (lambda: _sel(eng, p, [0, 5, 4, 3]), r"evoamd_ais_posterior_sel: index\[2\] = 4 descends"),
            (lambda: _sel(eng, p, [0, 37]), r"evoamd_ais_posterior_sel: index\[1\] = 37 is outside \[0, N = 37\)"),
            (lambda: _sel(eng, p, [-1, 3]), r"evoamd_ais_posterior_sel: index\[0\] = -1 is outside"),
            (lambda: _sel(eng, p, [0, 5], n_index=-1), "evoamd_ais_posterior_sel: n_index = -1 must not be negative"),
            (lambda: _sel(eng, p, [0, 5], flags=A, Mprime=0), r"evoamd_ais_posterior_sel: Mprime = 0 must be in \[1, S = 6\]"),
            (lambda: _sel(eng, p, [0, 5], flags=A, Mprime=7), r"evoamd_ais_posterior_sel: Mprime = 7 must be in \[1, S = 6\]"),
            (lambda: _sel(eng, p, [0, 5], flags=4), "evoamd_ais_posterior_sel: unknown flag"),
            (lambda: _sel(eng, p, [0, 5], flags=_lib.AIS_REVERSE), "evoamd_ais_posterior_sel: unknown flag"),
            # what evoamd_ais_posterior refuses is still refused, the texts unchanged
            (lambda: _sel(eng, p, [0, 5], n_chains=0), "evoamd_ais_posterior: n_chains"),
            (lambda: eng.ais_posterior(b, 3, 0, 1, 0, index=I, admit=True), "evoamd_ais_posterior: n_keep"),
            (lambda: eng.ais_posterior(np.array([0.1, 1.0]), 3, 2, 1, 0, index=I), "evoamd_ais_posterior: betas must start at 0"),
            # the calls without a list do not know the flag
            (lambda: _lib.check(eng.lib.evoamd_ais_posterior_ex(eng._h, 3, b.size - 1, 2, _lib.dptr(b), 1, 0, 0, A, None)),
             "evoamd_ais_posterior_ex: unknown flag")):
        _refused(eng, call, match)
    for bad, match in (([0, 5, 5], r"index\[2\] = 5 is repeated"), ([5, 0], r"index\[1\] = 0 descends"),
                       ([0, 37], r"index\[1\] = 37 is outside")):
        _refused(eng, lambda bad=bad: eng.ais_posterior(b, 3, 2, 1, 0, index=bad), match, exc=ValueError)
    assert _same(eng.ais_posterior(b, 3, 2, 1, 0, index=I, keep_chains=True), first)
    # admit without K^n on the device
    eng.configure("bsc", p.N, p.D, p.H, 50, 0, Cmax)
    eng.upload_data(p.Y)
    eng.set_params_bsc(p.theta["W"], float(p.theta["pi"]), float(p.theta["sigma"]))
    with pytest.raises(EvoAmdError, match="max_rounds = 1 "):
        eng.init_states(1.0 / p.H, 5, max_rounds=1)
    with pytest.raises(EvoAmdError, match="evoamd_ais_posterior_sel: EVOAMD_AIS_ADMIT needs K\\^n on the device"):
        eng.ais_posterior(b, 3, 2, 1, 0, index=I, admit=True)
    assert _same(eng.ais_posterior(b, 3, 2, 1, 0, index=I, keep_chains=True), first)  # (the chains read no K^n)
    _install(eng, p, S, Cmax, ss)
    assert _same(eng.ais_posterior(b, 3, 2, 1, 0, index=I, keep_chains=True), first)

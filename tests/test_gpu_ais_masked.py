"""AIS on incomplete data on the GPU (Engine.ais_loglik / Engine.ais_posterior with ``incomplete=True``, the MASKED kernels of
csrc/kernels_ais.hpp and csrc/kernels_ais_post.hpp) against the NumPy mirrors with ``x_infr`` and the exact answer.

1. device against mirror, every case, fraction and direction, and the posterior call at n_keep = 1 and 3; the wide
   instantiation and a column above 64 KiB of LDS; 2. the values under False; 3. an all-True mask against the complete call;
4. Model.ais_log_likelihood / ais_posterior against Model.exact_log_likelihood on the same incomplete data; 5. determinism,
the stream, write-freedom and the block size; 6. admit=True against host selection with the oracle's masked lpj; 7. the
refusals, the context usable afterwards; 8. the flag without masks.
"""
import numpy as np
import pytest

import _ais_masked_problems as mp
import _ais_post_problems as pp
import _ais_problems as ap
import _sweep_masked_problems as smp
import _sweep_problems as sp
from evo_amd import _lib
from evo_amd.engine import Engine, EvoAmdError
from evo_amd.models import BSC
from evo_amd.variational import init_states, seed_states_host
from oracle import evo_oracle as orc

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the tolerance of tests/test_gpu_ais.py and tests/test_gpu_ais_post.py


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


def _install(eng, p, S=4, Cmax=4, ss=None, Y=None, x_infr="own", rows=slice(None)):
    Y = p.Y if Y is None else Y
    x_infr = p.x_infr if isinstance(x_infr, str) else x_infr
    eng.configure("bsc", len(Y[rows]), p.D, p.H, S, 0, Cmax)
    eng.upload_data(np.ascontiguousarray(Y[rows]))
    if x_infr is not None:
        eng.upload_masks(np.ascontiguousarray(x_infr[rows]))
        eng.set_reliable_fraction(x_infr.sum() / float(p.N))  # (enters ljc alone, which no output here holds)
    eng.set_params_bsc(p.theta["W"], float(p.theta["pi"]), float(p.theta["sigma"]))
    if ss is not None:
        eng.upload_states(ss[rows])


def _close(a, b):
    return np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b))


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def _loglik(eng, p, direction, C=mp.C, **kw):
    return eng.ais_loglik(p.betas, C, mp.STREAM_SEED, 0, reverse=direction == "reverse",
                          s_start=p.s_true if direction == "reverse" else None, keep_states=True, incomplete=True, **kw)


def _check_loglik(p, got, want, label):
    decided = want["margin"] > mp.MARGIN_DECIDED  # (N, C)
    N, C = decided.shape
    fin = ap.unpack_final(got["final"], N, C, p.H)
    same = (fin == want["final_bool"]).all(axis=2) & (got["chain_flips"] == want["chain_flips"])
    err = np.abs(got["log_w"] - want["log_w"]) / np.maximum(1.0, np.abs(want["log_w"]))
    print("%s: %d of %d chains undecided, smallest margin %.3g, log_w against the mirror %.3g, flips %d" % (
        label, (~decided).sum(), decided.size, want["margin"].min(), err[decided].max(), got["n_flips"].sum()))
    assert same[decided].all(), np.argwhere(decided & ~same)
    assert (err[decided] <= RTOL).all()
    assert (~decided).sum() <= mp.MAX_UNDECIDED * decided.size
    rows = decided.all(axis=1)
    for k in ("ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
        assert _close(got[k][rows], want[k][rows]).all(), k
    assert np.array_equal(got["n_flips"][rows], want["n_flips"][rows]) and got["n_flips"].dtype == np.int64
    assert abs(got["sum"] - got["ll"].sum()) <= RTOL * max(1.0, abs(got["sum"]))


def _check_post(p, got, want, label):
    decided = want["margin"] > mp.MARGIN_DECIDED  # (N, C)
    same = (got["chain_flips"] == want["chain_flips"]) & (got["chain_map_state"] == want["chain_map_state"]).all(axis=2)
    err = {k: np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k])) for k in ("log_w", "rb", "chain_map_lpj")}
    print("%s: %d of %d chains undecided, smallest margin %.3g; against the mirror log_w %.3g, rb %.3g, chain_map_lpj %.3g; "
          "p %.3g, p_se %.3g; flips %d" % (label, (~decided).sum(), decided.size, want["margin"].min(), err["log_w"][decided].max(),
                                          err["rb"][decided].max(), err["chain_map_lpj"][decided].max(),
                                          np.abs(got["p"] - want["p"]).max(), np.abs(got["p_se"] - want["p_se"]).max(),
                                          got["n_flips"].sum()))
    assert same[decided].all(), np.argwhere(decided & ~same)
    for k, e in err.items():
        assert (e[decided] <= RTOL).all(), k
    assert (~decided).sum() <= mp.MAX_UNDECIDED * decided.size
    rows = decided.all(axis=1)
    for k in ("p", "p_se", "count", "map_lpj", "ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
        assert got[k].shape == want[k].shape and _close(got[k][rows], want[k][rows]).all(), k
    assert np.array_equal(got["map_state"][rows], want["map_state"][rows]) and got["map_state"].dtype == np.uint8
    assert np.array_equal(got["n_flips"][rows], want["n_flips"][rows]) and got["n_flips"].dtype == np.int64
    # mean = p W^T through the GEMM: every entry, the missing ones included
    assert np.isfinite(got["mean"]).all()
    assert _close(got["mean"], np.dot(got["p"], p.theta["W"].T)).all()
    assert _close(got["mean"][rows], want["mean"][rows]).all()


# ---- 1. device against mirror --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["forward", "reverse"])
@pytest.mark.parametrize("name,missing", mp.all_problems())
def test_device_equals_the_mirror(eng, name, missing, direction):
    p = mp.problem(name, missing)
    assert p.margin > mp.MARGIN_CPU, "the seed of the problems file no longer holds"
    _install(eng, p)
    got = _loglik(eng, p, direction)
    want = p.forward if direction == "forward" else p.reverse
    _check_loglik(p, got, want, "%s %.1f %s" % (name, missing, direction))
    # the datapoint without a reliable entry: prior draws, log w = 0; it is in the sum
    assert not got["log_w"][0].any()
    assert abs(got["ll"][0] - p.H * np.log1p(np.exp(np.log(p.theta["pi"] / (1.0 - p.theta["pi"]))))) <= 1e-12


@pytest.mark.parametrize("K", mp.KEEPS)
@pytest.mark.parametrize("name,missing", mp.all_problems())
def test_posterior_equals_the_mirror(eng, name, missing, K):
    p = mp.problem(name, missing)
    _install(eng, p)
    got = eng.ais_posterior(p.betas, mp.C, K, mp.STREAM_SEED, 0, mean=True, keep_chains=True, incomplete=True)
    _check_post(p, got, p.post[K], "%s %.1f n_keep %d" % (name, missing, K))
    if K == 1:  # the chains are those of ais_loglik, bit for bit
        fwd = _loglik(eng, p, "forward")
        for k in ("log_w", "ll", "ess", "n_flips", "chain_flips"):
            assert np.array_equal(got[k], fwd[k]), k
        assert np.array_equal(got["chain_map_state"].reshape(-1), fwd["final"])


@pytest.mark.parametrize("name", list(mp.EXTRA))
def test_wide_instantiation_and_wide_column(eng, name):
    p = mp.extra_problem(name)
    assert p.margin > mp.MARGIN_CPU, "the seed of the problems file no longer holds"
    _install(eng, p)
    for direction in ("forward", "reverse"):
        _check_loglik(p, _loglik(eng, p, direction, C=p.C), getattr(p, direction), "%s %s" % (name, direction))
    got = eng.ais_posterior(p.betas, p.C, p.K, mp.STREAM_SEED, 0, mean=True, keep_chains=True, incomplete=True)
    _check_post(p, got, p.post, name)


# ---- 2. the values under False never enter -------------------------------------------------------------------------------------
def test_values_under_false_do_not_show(eng):
    p = mp.problem("two_words", 0.6)
    _install(eng, p)
    a = (_loglik(eng, p, "forward"), _loglik(eng, p, "reverse"),
         eng.ais_posterior(p.betas, mp.C, 3, mp.STREAM_SEED, 0, mean=True, keep_chains=True, incomplete=True))
    for Y in (np.where(p.x_infr, p.Y, 1e6), p.Y_full):
        _install(eng, p, Y=Y)
        b = (_loglik(eng, p, "forward"), _loglik(eng, p, "reverse"),
             eng.ais_posterior(p.betas, mp.C, 3, mp.STREAM_SEED, 0, mean=True, keep_chains=True, incomplete=True))
        for x, y in zip(a, b):
            assert _same(x, y)


# ---- 3. an all-True mask against the complete call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ap.CASES))
def test_all_true_mask_agrees_with_the_complete_call(eng, name):
    q = ap.problem(name)
    ones = np.ones_like(q.Y, dtype=bool)
    _install(eng, q, x_infr=None)
    for direction, want in (("forward", q.forward), ("reverse", q.reverse)):
        kw = dict(reverse=direction == "reverse", s_start=q.s_true if direction == "reverse" else None, keep_states=True)
        eng.upload_masks(None)
        plain = eng.ais_loglik(q.betas, ap.C, ap.STREAM_SEED, 0, **kw)
        eng.upload_masks(ones)
        masked = eng.ais_loglik(q.betas, ap.C, ap.STREAM_SEED, 0, incomplete=True, **kw)
        decided = want["margin"] > mp.MARGIN_DECIDED
        fa, fb = (ap.unpack_final(x["final"], q.N, ap.C, q.H) for x in (plain, masked))
        same = (fa == fb).all(axis=2) & (plain["chain_flips"] == masked["chain_flips"])
        err = np.abs(masked["log_w"] - plain["log_w"]) / np.maximum(1.0, np.abs(plain["log_w"]))
        print("%s %s: log w, all-True mask against the complete call %.3g (allowed %.3g)" % (name, direction, err[decided].max(),
                                                                                         mp.ALLTRUE_TOL))
        assert same[decided].all() and (err[decided] <= mp.ALLTRUE_TOL).all()
    eng.upload_masks(None)
    plain = eng.ais_posterior(q.betas, ap.C, 3, ap.STREAM_SEED, 0, keep_chains=True)
    eng.upload_masks(ones)
    masked = eng.ais_posterior(q.betas, ap.C, 3, ap.STREAM_SEED, 0, keep_chains=True, incomplete=True)
    decided = pp.mirror(q, ap.T, ap.C, 3)["margin"] > mp.MARGIN_DECIDED
    same = (plain["chain_flips"] == masked["chain_flips"]) & (plain["chain_map_state"] == masked["chain_map_state"]).all(axis=2)
    err = np.abs(masked["log_w"] - plain["log_w"]) / np.maximum(1.0, np.abs(plain["log_w"]))
    assert same[decided].all() and (err[decided] <= mp.ALLTRUE_TOL).all()
    eng.upload_masks(None)


# ---- 4. exactness through the Model ------------------------------------------------------------------------------------------------
def _suff(ss, Mprime=None):
    N, S, H = ss.shape
    suff = init_states(0, S, H, "fit", "randflip", 6, 5, 1, Mprime=Mprime)
    suff["ss"] = ss.copy()
    suff["lpj"] = np.zeros((N, S))
    return suff


def test_model_brackets_the_exact_answer_on_incomplete_data(model_eng):
    c = mp.EXACT
    p = mp.exact_problem()
    S = 8
    model = BSC(p.D, p.H, S, engine=model_eng)
    suff = _suff(seed_states_host("bsc", p.theta, p.Y, S, 2, 0, x_infr=p.x_infr)[0])
    data = {"y": np.array(p.Y), "x_infr": p.x_infr.copy(), "x": p.x_infr.copy()}
    L_exact, exact, marg = model.exact_log_likelihood(data, dict(p.theta), suff, per_datapoint=True, marginals=True)
    assert np.abs(exact - p.exact).max() <= 1e-9 * np.abs(p.exact).max() and np.abs(marg - p.exact_marg).max() <= 1e-9
    with pytest.raises(ValueError, match="incomplete data"):
        model.ais_log_likelihood(p.theta, suff, data)
    with pytest.raises(ValueError, match="incomplete data"):
        model.ais_posterior(p.theta, suff, data)
    keys = (set(p.theta), set(suff), set(data))
    kw = dict(n_chains=c["C"], n_temps=c["T"], seed=mp.EXACT_STREAM, incomplete=True)
    L_lo, lower = model.ais_log_likelihood(p.theta, suff, data, keep_states=True, **kw)
    assert model.last_ais_seed == mp.EXACT_STREAM  # (one rank: the stream seed the problems file chose the data seed for)
    L_up, upper = model.ais_log_likelihood(p.theta, suff, data, direction="reverse", s_start=p.s_true, keep_states=True, **kw)
    print("L_lower %.6f, exact %.6f, L_upper %.6f" % (L_lo, L_exact, L_up))
    ap.check_bars(lower, upper, exact)
    # L = ljc + sum ll_n / N with the ljc of incomplete data
    assert abs(L_lo - (model_eng.ljc + lower["ll"].mean())) <= RTOL * max(1.0, abs(L_lo))
    assert abs((L_exact - L_lo) - (exact.mean() - lower["ll"].mean())) <= RTOL * max(1.0, abs(L_lo))
    got = model.ais_posterior(p.theta, suff, data, n_keep=c["K"], mean=True, **kw)
    assert (set(p.theta), set(suff), set(data)) == keys, "a call wrote into a dict"
    pp.check_bars(got, marg)
    assert np.array_equal(got["ll"], lower["ll"])
    W = p.theta["W"]
    assert got["mean"].shape == (p.N, p.D) and _close(got["mean"], np.dot(got["p"], W.T)).all()
    # against marg W^T: what the bars of p allow, entry by entry, the hidden entries included
    bar = 5.0 * got["p_se"] + 3.0 / got["ess"][:, None]
    err = np.abs(got["mean"] - np.dot(marg, W.T))
    print("mean against marg W^T: largest error %.3g on the hidden entries, %.3g on the others" % (err[~p.x_infr].max(),
                                                                                                  err[p.x_infr].max()))
    assert (err <= np.dot(bar, np.abs(W).T)).all()
    # the mirrors, where their chains are decided
    rows = (p.post["margin"] > mp.MARGIN_DECIDED).all(axis=1)
    assert rows.any()
    for k in ("p", "p_se", "map_lpj", "ll"):
        assert _close(got[k][rows], p.post[k][rows]).all(), k


# ---- 5. determinism, the stream, write-freedom, the block size ---------------------------------------------------------------------
def test_deterministic_streamed_and_write_free(eng):
    p = mp.problem("two_words", 0.3)
    S, Cmax = 12, 4
    ss = seed_states_host("bsc", p.theta, p.Y, S, 3, 0, x_infr=p.x_infr)[0]
    _install(eng, p, S, Cmax, ss)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    eng.set_option("reconstruct_in_stats", 1)  # (incomplete data: the statistics pass forms y_reconstructed itself)
    eng.stats()
    eng.set_option("reconstruct_in_stats", 0)

    def state():
        return (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.download_posterior()[0],
                eng.debug_validity())

    before = state()
    pkw = dict(n_chains=mp.C, n_keep=3, seed=9, mean=True, keep_chains=True, incomplete=True)
    calls = {
        "forward": lambda C=mp.C: eng.ais_loglik(p.betas, C, 9, 0, keep_states=True, incomplete=True),
        "reverse": lambda C=mp.C: eng.ais_loglik(p.betas, C, 9, 0, reverse=True, s_start=p.s_true, keep_states=True, incomplete=True),
        "posterior": lambda C=mp.C: eng.ais_posterior(p.betas, **dict(pkw, n_chains=C))}
    full = {}
    for name, call in calls.items():
        a, b = call(), call()
        assert _same(a, b), name + ": two calls differ"
        pre = call(3)  # fewer chains are a prefix
        for k in ("log_w", "chain_flips", "rb", "chain_map_lpj", "chain_map_state"):
            if k in a:
                assert np.array_equal(pre[k], a[k][:, :3]), (name, k)
        if "final" in a:
            nb = (p.H + 7) // 8
            assert np.array_equal(pre["final"].reshape(p.N, 3, nb), a["final"].reshape(p.N, mp.C, nb)[:, :3])
        full[name] = a
    after = state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[3], after[3])
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert before[4] == after[4], {k: (before[4][k], after[4][k]) for k in before[4] if before[4][k] != after[4][k]}
    # the resident Y and masks: the masked lpj of K^n, which reads both, is what it was
    eng.lpj_resident()
    assert np.array_equal(eng.download_lpj(), before[1]) and eng.has_masks
    # the block size does not show: one datapoint per block, and a block that does not divide N
    for block in (1, 8):
        assert _same(eng.ais_posterior(p.betas, block=block, **pkw), full["posterior"]), block
    # shards by first_index concatenate to the single call
    cut = 8
    parts = {name: [] for name in calls}
    for rows, first in ((slice(0, cut), 0), (slice(cut, None), cut)):
        _install(eng, p, S, Cmax, rows=rows)
        parts["forward"].append(eng.ais_loglik(p.betas, mp.C, 9, first, keep_states=True, incomplete=True))
        parts["reverse"].append(eng.ais_loglik(p.betas, mp.C, 9, first, reverse=True, s_start=p.s_true[rows], keep_states=True,
                                               incomplete=True))
        parts["posterior"].append(eng.ais_posterior(p.betas, first_index=first, **pkw))
    for name, (a, b) in parts.items():
        for k in full[name]:
            if k != "sum":
                assert np.array_equal(np.concatenate([a[k], b[k]]), full[name][k]), (name, k)


# ---- 6. admit on masked data ---------------------------------------------------------------------------------------------------
def test_admit_equals_host_selection_with_the_masked_lpj(eng):
    p = mp.problem("two_words", 0.3)
    S, Cmax = 12, 4  # Cmax < C: the first four chains are taken
    ss = seed_states_host("bsc", p.theta, p.Y, S, 3, 0, x_infr=p.x_infr)[0]
    _install(eng, p, S, Cmax, ss)
    got = eng.ais_loglik(p.betas, mp.C, mp.STREAM_SEED, 0, keep_states=True, admit=True, Mprime=S, incomplete=True)
    new_ss, new_lpj = eng.download_states(), eng.download_lpj()
    assert (got["F_after"] >= got["F_before"]).all()
    assert got["S_sub"] > 0.0, "no state of any chain entered K^n: the test shows nothing"
    oth = smp.oracle_theta("ebsc", p.theta, p.D, p.H, p.x_infr)
    incl = np.zeros((0, p.H), dtype=bool)
    checked = 0
    for n in range(p.N):
        assert len({row.tobytes() for row in np.packbits(new_ss[n], axis=-1)}) == S, "datapoint %d lost a state" % n
        if not p.x_infr[n].any() or not (p.forward["margin"][n, :Cmax] > mp.MARGIN_DECIDED).all():
            continue  # (without a reliable entry every state of a size has the same lpj: no ranking to check)
        fin = p.forward["final_bool"][n, :Cmax]
        fin = fin[fin.any(axis=1)]  # the all-zero state is skipped
        old_lpj = smp.oracle_lpj("ebsc", oth, p.Y[n], ss[n], p.x_infr[n])
        want_ss, want_lpj = ss[n].copy(), old_lpj.copy()
        if len(fin):
            cand_lpj = smp.oracle_lpj("ebsc", oth, p.Y[n], fin, p.x_infr[n])
            pool = np.sort(np.concatenate([old_lpj, cand_lpj]))
            fresh = [i for i, row in enumerate(fin) if not (ss[n] == row).all(axis=1).any()
                     and not (fin[:i] == row).all(axis=1).any()]
            vals = np.sort(np.concatenate([old_lpj, cand_lpj[fresh]]))
            if len(vals) > 1 and np.diff(vals).min() <= 1e-7 * max(1.0, np.abs(pool).max()):
                continue  # the ranking is not decided at the precision of the rows
            orc.vary_Kn(old_lpj.copy(), cand_lpj.copy(), want_lpj, want_ss, fin, p.H, S, 0, incl, S)
        assert ({r.tobytes() for r in np.packbits(new_ss[n], axis=-1)} == {r.tobytes() for r in np.packbits(want_ss, axis=-1)}), n
        assert _close(np.sort(new_lpj[n]), np.sort(want_lpj)).all(), n
        checked += 1
    print("admit: %d of %d datapoints checked against host selection, S_sub %.0f" % (checked, p.N, got["S_sub"]))
    assert checked >= p.N // 2
    # the chains themselves are those of the call without admit
    _install(eng, p, S, Cmax, ss)
    plain = eng.ais_loglik(p.betas, mp.C, mp.STREAM_SEED, 0, keep_states=True, incomplete=True)
    for k in plain:
        assert np.array_equal(plain[k], got[k]), k


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(eng, call, match):
    before = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.debug_validity())
    with pytest.raises(EvoAmdError, match=match):
        call()
    after = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.debug_validity())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1], equal_nan=True)
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert before[3] == after[3], {k: (before[3][k], after[3][k]) for k in before[3] if before[3][k] != after[3][k]}


def test_refusals_leave_the_context_usable(eng):
    p = mp.problem("partial_chunk", 0.3)
    S, Cmax = 6, 4
    ss = seed_states_host("bsc", p.theta, p.Y, S, 2, 0, x_infr=p.x_infr)[0]
    _install(eng, p, S, Cmax, ss)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    b = p.betas
    INC = _lib.AIS_INCOMPLETE
    first = eng.ais_loglik(b, 3, 1, 0, keep_states=True, incomplete=True)
    first_post = eng.ais_posterior(b, 3, 2, 1, 0, keep_chains=True, incomplete=True)
    for call, match in (
            # masks without the flag: today's texts
            (lambda: eng.ais_loglik(b, 3, 1, 0), "evoamd_ais_loglik: incomplete data \\(masks resident\\) is not supported"),
            (lambda: eng.ais_posterior(b, 3, 2, 1, 0), "evoamd_ais_posterior: incomplete data \\(masks resident\\) is not supported"),
            (lambda: _lib.check(eng.lib.evoamd_ais_loglik(eng._h, 3, mp.T, _lib.dptr(b), 1, 0, INC | 4, None, 1, None)),
             "evoamd_ais_loglik: unknown flag"),
            (lambda: _lib.check(eng.lib.evoamd_ais_loglik(eng._h, 3, mp.T, _lib.dptr(b), 1, 0, INC | 16, None, 1, None)),
             "evoamd_ais_loglik: unknown flag"),
            (lambda: _lib.check(eng.lib.evoamd_ais_posterior_ex(eng._h, 3, mp.T, 2, _lib.dptr(b), 1, 0, 0, INC | 1, None)),
             "evoamd_ais_posterior_ex: unknown flag"),
            (lambda: eng.ais_loglik(b, 0, 1, 0, incomplete=True), "n_chains"),
            (lambda: eng.ais_posterior(b, 3, 0, 1, 0, incomplete=True), "n_keep"),
            (lambda: eng.ais_loglik(b, 3, 1, 0, reverse=True, incomplete=True), "s_start")):
        _refused(eng, call, match)
    eng.set_option("background_unit", 1)
    _refused(eng, lambda: eng.ais_loglik(b, 3, 1, 0, incomplete=True), "evoamd_ais_loglik: option background_unit")
    _refused(eng, lambda: eng.ais_posterior(b, 3, 2, 1, 0, incomplete=True), "evoamd_ais_posterior: option background_unit")
    eng.set_option("background_unit", 0)
    assert _same(eng.ais_loglik(b, 3, 1, 0, keep_states=True, incomplete=True), first)
    assert _same(eng.ais_posterior(b, 3, 2, 1, 0, keep_chains=True, incomplete=True), first_post)
    # options that are read when Theta is installed or the context configured: each on a context of its own shape
    eng.set_option("ebsc_f32", 1)
    try:
        p4 = ap.build(9, 8, 16, 1)  # (the float32 mode asks for H % 4 == 0 and D % 4 == 0)
        _install(eng, p4, x_infr=None)
        for call in (lambda: eng.ais_loglik(b, 3, 1, 0, incomplete=True), lambda: eng.ais_posterior(b, 3, 2, 1, 0, incomplete=True)):
            with pytest.raises(EvoAmdError, match="float32"):
                call()
    finally:
        eng.set_option("ebsc_f32", 0)
    es3c = sp.problem("es3c", "ragged")
    eng.configure("sssc", es3c.N, es3c.D, es3c.H, es3c.S, 0, es3c.Cmax)
    eng.upload_data(es3c.Y)
    th = es3c.theta
    eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    for call in (lambda: eng.ais_loglik(b, 3, 1, 0, incomplete=True), lambda: eng.ais_posterior(b, 3, 2, 1, 0, incomplete=True)):
        with pytest.raises(EvoAmdError, match="ES3C is not supported"):
            call()
    # a D whose column and list do not fit into LDS beside the rows: refused before anything is launched
    N, D, H = 2, 3500, 4
    rng = np.random.RandomState(3)
    eng.configure("bsc", N, D, H, 2, 0, 2)
    eng.upload_data(rng.normal(size=(N, D)))
    eng.upload_masks(rng.random_sample((N, D)) >= 0.5)
    eng.set_params_bsc(rng.normal(size=(D, H)), 0.3, 1.0)
    b2 = np.array([0.0, 0.5, 1.0])
    for call, who in ((lambda: eng.ais_loglik(b2, 2, 1, 0, incomplete=True), "evoamd_ais_loglik"),
                      (lambda: eng.ais_posterior(b2, 2, 1, 1, 0, incomplete=True), "evoamd_ais_posterior")):
        with pytest.raises(EvoAmdError, match=who + ": incomplete data with D = 3500 and H = 4 needs"):
            call()
    _install(eng, p, S, Cmax, ss)
    assert _same(eng.ais_loglik(b, 3, 1, 0, keep_states=True, incomplete=True), first)
    assert _same(eng.ais_posterior(b, 3, 2, 1, 0, keep_chains=True, incomplete=True), first_post)


# ---- 8. the flag without masks -------------------------------------------------------------------------------------------------
def test_flag_without_masks_is_the_plain_call(eng):
    q = ap.problem("two_words")
    _install(eng, q, x_infr=None)
    for kw in (dict(), dict(reverse=True, s_start=q.s_true)):
        plain = eng.ais_loglik(q.betas, ap.C, ap.STREAM_SEED, 0, keep_states=True, **kw)
        assert _same(eng.ais_loglik(q.betas, ap.C, ap.STREAM_SEED, 0, keep_states=True, incomplete=True, **kw), plain)
    plain = eng.ais_posterior(q.betas, ap.C, 3, ap.STREAM_SEED, 0, mean=True, keep_chains=True)
    assert _same(eng.ais_posterior(q.betas, ap.C, 3, ap.STREAM_SEED, 0, mean=True, keep_chains=True, incomplete=True), plain)


def test_masked_kernels_count_in_the_existing_classes(eng):
    p = mp.problem("partial_chunk", 0.3)
    _install(eng, p)
    eng.timing(("ais", "ais_post"))
    eng.timing_reset()
    eng.ais_loglik(p.betas, 2, 1, 0, incomplete=True)
    eng.ais_posterior(p.betas, 2, 2, 1, 0, incomplete=True)
    (ms_a, n_a), (ms_p, n_p) = eng.kernel_time_ms("ais"), eng.kernel_time_ms("ais_post")
    eng.timing(False)
    assert n_a == 1 and ms_a > 0.0 and n_p == 1 and ms_p > 0.0

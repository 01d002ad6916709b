"""Annealed importance sampling on the GPU (Engine.ais_loglik / Model.ais_log_likelihood, csrc/kernels_ais.hpp) against its
NumPy mirror (evo_amd.models.ais_log_likelihood_counter) and the exact answer.

5. device against mirror at the shapes where the chunked scan can go wrong; 6. against Model.exact_log_likelihood on the GPU;
7. determinism, the stream and write-freedom through the Model API with sync_host=False; 8. admit=True against host selection;
9. the refusals of the ABI, each with its text, the context usable afterwards.
"""
import numpy as np
import pytest

import _ais_problems as ap
import _sweep_problems as sp
from evo_amd import _lib
from evo_amd.engine import Engine, EvoAmdError
from evo_amd.models import BSC
from evo_amd.variational import init_states, seed_states_host
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


def _install(eng, p, S=4, Cmax=4, ss=None):
    eng.configure("bsc", p.N, p.D, p.H, S, 0, Cmax)
    eng.upload_data(p.Y)
    eng.set_params_bsc(p.theta["W"], float(p.theta["pi"]), float(p.theta["sigma"]))
    if ss is not None:
        eng.upload_states(ss)


def _close(a, b):
    return np.abs(a - b) <= RTOL * np.maximum(1.0, np.abs(b))


# ---- 5. device against mirror --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["forward", "reverse"])
@pytest.mark.parametrize("name", list(ap.CASES))
def test_device_equals_the_mirror(eng, name, direction):
    p = ap.problem(name)
    want = p.forward if direction == "forward" else p.reverse
    assert min(p.forward["margin"].min(), p.reverse["margin"].min()) > ap.MARGIN_CPU, "the seed of the problems file no longer holds"
    _install(eng, p)
    got = eng.ais_loglik(p.betas, ap.C, ap.STREAM_SEED, 0, reverse=direction == "reverse",
                         s_start=p.s_true if direction == "reverse" else None, keep_states=True)
    decided = want["margin"] > ap.MARGIN_DECIDED  # (N, C)
    fin = ap.unpack_final(got["final"], p.N, ap.C, p.H)
    same = (fin == want["final_bool"]).all(axis=2) & (got["chain_flips"] == want["chain_flips"])
    err = np.abs(got["log_w"] - want["log_w"]) / np.maximum(1.0, np.abs(want["log_w"]))
    print("%s %s: %d of %d chains undecided, smallest margin %.3g, log_w against the mirror %.3g, flips %d" % (
        name, direction, (~decided).sum(), decided.size, want["margin"].min(), err[decided].max(), got["n_flips"].sum()))
    assert same[decided].all(), np.argwhere(decided & ~same)
    assert (err[decided] <= RTOL).all()
    assert (~decided).sum() <= ap.MAX_UNDECIDED * decided.size
    rows = decided.all(axis=1)
    for k in ("ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
        assert _close(got[k][rows], want[k][rows]).all(), k
    assert np.array_equal(got["n_flips"][rows], want["n_flips"][rows]) and got["n_flips"].dtype == np.int64
    assert abs(got["sum"] - got["ll"].sum()) <= RTOL * max(1.0, abs(got["sum"]))


# ---- 6. against the exact answer on the GPU ------------------------------------------------------------------------------------
def _suff(ss, Mprime=None):
    N, S, H = ss.shape
    suff = init_states(0, S, H, "fit", "randflip", 6, 5, 1, Mprime=Mprime)
    suff["ss"] = ss.copy()
    suff["lpj"] = np.zeros((N, S))
    return suff


def test_brackets_the_exact_log_likelihood(model_eng):
    c = ap.MODEL_EXACT
    p = ap.build(c["N"], c["D"], c["H"], ap.MODEL_EXACT_SEED)
    S = 8
    model = BSC(p.D, p.H, S, engine=model_eng)
    suff = _suff(seed_states_host("bsc", p.theta, p.Y, S, 2, 0)[0])
    data = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    L_exact, exact, _ = model.exact_log_likelihood(data, dict(p.theta), suff, per_datapoint=True)
    keys = (set(p.theta), set(suff), set(data))
    seed = ap.MODEL_EXACT_STREAM
    L_lo, lower = model.ais_log_likelihood(p.theta, suff, data, n_chains=c["C"], n_temps=c["T"], seed=seed, keep_states=True)
    assert model.last_ais_seed == seed  # (one rank: the stream seed the problems file chose the data seed for)
    L_up, upper = model.ais_log_likelihood(p.theta, suff, data, n_chains=c["C"], n_temps=c["T"], seed=seed, direction="reverse",
                                           s_start=p.s_true, keep_states=True)
    assert (set(p.theta), set(suff), set(data)) == keys, "the call wrote into a dict"
    print("L_lower %.6f, exact %.6f, L_upper %.6f" % (L_lo, L_exact, L_up))
    ap.check_bars(lower, upper, exact)
    ljc = model_eng.ljc
    assert abs(L_lo - (ljc + lower["ll"].mean())) <= RTOL * max(1.0, abs(L_lo))
    assert set(lower) == {"ll", "ess", "log_w_mean", "log_w_min", "log_w_max", "n_flips", "log_w", "final", "chain_flips"}
    assert lower["final"].shape == (p.N * c["C"] * ((p.H + 7) // 8),) and lower["final"].dtype == np.uint8
    assert model.ais_log_likelihood(p.theta, suff, data, n_chains=c["C"], n_temps=c["T"], seed=seed) == L_lo
    # the mirror, for the seed the model used
    want = ap.mirror(p, c["T"], 4, "forward", seed=model.last_ais_seed)
    ok = want["margin"] > ap.MARGIN_DECIDED
    assert np.array_equal(ap.unpack_final(lower["final"], p.N, c["C"], p.H)[:, :4][ok], want["final_bool"][ok])


# ---- 7. determinism, the stream, write-freedom ---------------------------------------------------------------------------------
def _resident_model(model_eng, p, S, ss, rows=slice(None)):
    model = BSC(p.D, p.H, S, engine=model_eng, rng="device", sync_host=False, seed=3)
    suff = _suff(ss[rows])
    suff["ss"] = suff["lpj"] = None
    data = {"y": np.ascontiguousarray(p.Y[rows]), "x_infr": np.ones_like(p.Y[rows], dtype=bool)}
    model.attach_resident_states(suff, data, [(0, np.packbits(ss[rows], axis=-1))])
    return model, suff, data


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def test_deterministic_streamed_and_write_free(model_eng):
    p = ap.problem("two_words")
    S = 12
    ss = seed_states_host("bsc", p.theta, p.Y, S, 3, 0)[0]
    model, suff, data = _resident_model(model_eng, p, S, ss)
    kw = dict(n_chains=ap.C, n_temps=ap.T, seed=9, keep_states=True)
    model.ais_log_likelihood(p.theta, suff, data, **kw)  # (configures the engine and installs Theta)
    model_eng.lpj_resident()
    model_eng.evolve_randflip(2, 2, 5, True)
    before = (model_eng.download_states_packed(), model_eng.download_lpj(), model_eng.download_candidates())
    for direction, s_start in (("forward", None), ("reverse", p.s_true)):
        La, a = model.ais_log_likelihood(p.theta, suff, data, direction=direction, s_start=s_start, **kw)
        Lb, b = model.ais_log_likelihood(p.theta, suff, data, direction=direction, s_start=s_start, **kw)
        assert La == Lb and _same(a, b), direction
        # chain c does not depend on n_chains
        _, pre = model.ais_log_likelihood(p.theta, suff, data, direction=direction, s_start=s_start,
                                          **dict(kw, n_chains=3))
        nb = (p.H + 7) // 8
        assert np.array_equal(pre["log_w"], a["log_w"][:, :3]) and np.array_equal(pre["chain_flips"], a["chain_flips"][:, :3])
        assert np.array_equal(pre["final"].reshape(p.N, 3, nb), a["final"].reshape(p.N, ap.C, nb)[:, :3])
    after = (model_eng.download_states_packed(), model_eng.download_lpj(), model_eng.download_candidates())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert suff["ss"] is None and suff["lpj"] is None
    # shards by first_index concatenate to the single call (each shard is a model of its own on the engine)
    _, full = model.ais_log_likelihood(p.theta, suff, data, **kw)
    cut = 8
    parts = []
    for rows, first in ((slice(0, cut), 0), (slice(cut, None), cut)):
        m, sf, d = _resident_model(model_eng, p, S, ss, rows)
        parts.append(m.ais_log_likelihood(p.theta, sf, d, first_index=first, **kw)[1])
    for k in full:
        assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]]), full[k]), k


# ---- 8. admit ------------------------------------------------------------------------------------------------------------------
def test_admit_equals_host_selection(eng):
    p = ap.problem("two_words")
    S, Cmax = 12, 4  # Cmax < C: the first four chains are taken
    ss = seed_states_host("bsc", p.theta, p.Y, S, 3, 0)[0]
    _install(eng, p, S, Cmax, ss)
    got = eng.ais_loglik(p.betas, ap.C, ap.STREAM_SEED, 0, keep_states=True, admit=True, Mprime=S)
    new_ss, new_lpj = eng.download_states(), eng.download_lpj()
    assert (got["F_after"] >= got["F_before"]).all()
    assert got["S_sub"] > 0.0, "no state of any chain entered K^n: the test shows nothing"
    oth = sp.oracle_theta("ebsc", p.theta, p.D, p.H)
    incl = np.zeros((0, p.H), dtype=bool)
    checked = 0
    for n in range(p.N):
        assert len({row.tobytes() for row in np.packbits(new_ss[n], axis=-1)}) == S, "datapoint %d lost a state" % n
        if not (p.forward["margin"][n, :Cmax] > ap.MARGIN_DECIDED).all():
            continue
        fin = p.forward["final_bool"][n, :Cmax]
        fin = fin[fin.any(axis=1)]  # the all-zero state is skipped
        old_lpj = sp.oracle_lpj("ebsc", oth, p.Y[n], ss[n])
        want_ss, want_lpj = ss[n].copy(), old_lpj.copy()
        if len(fin):
            cand_lpj = sp.oracle_lpj("ebsc", oth, p.Y[n], fin)
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
    plain = eng.ais_loglik(p.betas, ap.C, ap.STREAM_SEED, 0, keep_states=True)
    for k in plain:
        assert np.array_equal(plain[k], got[k]), k


def test_admit_through_the_model(model_eng):
    p = ap.problem("two_words")
    S = 12
    ss = seed_states_host("bsc", p.theta, p.Y, S, 3, 0)[0]
    model = BSC(p.D, p.H, S, engine=model_eng)
    suff = _suff(ss)
    data = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    suff["lpj"] = sp.rows_of("ebsc", p.theta, p.Y, ss, 0)
    F0 = model.posterior_scores(p.theta, suff, data)["F"]
    L, info = model.ais_log_likelihood(p.theta, suff, data, n_chains=ap.C, n_temps=ap.T, seed=4, admit=True)
    assert _close(info["F_before"], F0).all() and (info["F_after"] >= info["F_before"]).all() and info["S_sub"] > 0.0
    assert np.array_equal(suff["ss"], model_eng.download_states())  # sync_host: K^n came back
    assert _close(model.posterior_scores(p.theta, suff, data)["F"], info["F_after"]).all()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
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
    p = ap.problem("partial_chunk")
    S, Cmax = 6, 4
    ss = seed_states_host("bsc", p.theta, p.Y, S, 2, 0)[0]
    _install(eng, p, S, Cmax, ss)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    b = p.betas
    first = eng.ais_loglik(b, 3, 1, 0, keep_states=True)
    for call, match in (
            (lambda: eng.ais_loglik(b, 0, 1, 0), "n_chains"),
            (lambda: eng.ais_loglik(np.array([0.1, 1.0]), 3, 1, 0), "start at 0"),
            (lambda: eng.ais_loglik(np.array([0.0, 0.5, 0.9]), 3, 1, 0), "end at 1"),
            (lambda: eng.ais_loglik(np.array([0.0, 0.6, 0.5, 1.0]), 3, 1, 0), "descend"),
            (lambda: eng.ais_loglik(b, 3, 1, 0, reverse=True), "s_start"),
            (lambda: eng.ais_loglik(b, 3, 1, 0, reverse=True, s_start=p.s_true, admit=True, Mprime=S), "EVOAMD_AIS_ADMIT with"),
            (lambda: eng.ais_loglik(b, 3, 1, 0, admit=True, Mprime=S + 1), "Mprime"),
            (lambda: _lib.check(eng.lib.evoamd_ais_loglik(eng._h, 3, ap.T, _lib.dptr(b), 1, 0, 4, None, 1, None)), "unknown flag")):
        _refused(eng, call, match)
    eng.set_option("background_unit", 1)
    _refused(eng, lambda: eng.ais_loglik(b, 3, 1, 0), "background_unit")
    eng.set_option("background_unit", 0)
    eng.upload_masks(np.ones((p.N, p.D), dtype=bool))
    _refused(eng, lambda: eng.ais_loglik(b, 3, 1, 0), "incomplete data")
    eng.upload_masks(None)
    assert _same(eng.ais_loglik(b, 3, 1, 0, keep_states=True), first)
    # options that are read when Theta is installed or the context configured: each on a context of its own shape
    eng.set_option("bsc_direct", 1)
    try:
        _install(eng, p, S, Cmax, ss)
        with pytest.raises(EvoAmdError, match="bsc_direct"):
            eng.ais_loglik(b, 3, 1, 0)
    finally:
        eng.set_option("bsc_direct", 0)
    eng.set_option("ebsc_f32", 1)
    try:
        p4 = ap.build(9, 8, 16, 1)  # (the float32 mode asks for H % 4 == 0 and D % 4 == 0)
        _install(eng, p4)
        with pytest.raises(EvoAmdError, match="float32"):
            eng.ais_loglik(b, 3, 1, 0)
    finally:
        eng.set_option("ebsc_f32", 0)
    big = ap.build(2, 2, 1030, 1)
    _install(eng, big)
    with pytest.raises(EvoAmdError, match="at most 1024 latents"):
        eng.ais_loglik(b, 3, 1, 0)
    es3c = sp.problem("es3c", "ragged")
    eng.configure("sssc", es3c.N, es3c.D, es3c.H, es3c.S, 0, es3c.Cmax)
    eng.upload_data(es3c.Y)
    th = es3c.theta
    eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    with pytest.raises(EvoAmdError, match="ES3C is not supported"):
        eng.ais_loglik(b, 3, 1, 0)
    _install(eng, p, S, Cmax, ss)
    assert _same(eng.ais_loglik(b, 3, 1, 0, keep_states=True), first)


def test_kernel_class_is_named(eng):
    assert _lib.KERNEL_IDS_EXTRA["ais"] == 35
    assert eng.lib.evoamd_kernel_name(35) == b"ais"
    p = ap.problem("partial_chunk")
    _install(eng, p)
    eng.timing(("ais",))
    eng.timing_reset()
    eng.ais_loglik(p.betas, 2, 1, 0)
    ms, launches = eng.kernel_time_ms("ais")
    eng.timing(False)
    assert launches == 1 and ms > 0.0

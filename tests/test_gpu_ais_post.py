"""The posterior from AIS chains on the GPU (Engine.ais_posterior / Model.ais_posterior, csrc/kernels_ais_post.hpp) against its
NumPy mirror (evo_amd.models.ais_posterior_counter), the forward chains of Engine.ais_loglik and the exact marginals.

5. device against mirror at the shapes where the chunked scan and its Rao-Blackwell sum can go wrong, and once for each wide
   instantiation; 6. n_keep = 1 against Engine.ais_loglik, bit for bit; 7. Model.ais_posterior against
   Model.exact_log_likelihood(marginals=True); 8. write-freedom, determinism, the stream and the block size; 9. the refusals
   of the ABI, each with its text, the context usable afterwards; 10. the kernel class.
"""
import numpy as np
import pytest

import _ais_post_problems as pp
import _ais_problems as ap
import _sweep_problems as sp
from evo_amd import _lib
from evo_amd.engine import Engine, EvoAmdError
from evo_amd.models import BSC
from evo_amd.variational import init_states, seed_states_host

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


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


# ---- 5. device against mirror --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pp.CASES))
def test_device_equals_the_mirror(eng, name):
    p = pp.problem(name)
    want = p.want
    assert want["margin"].min() > pp.MARGIN_CPU, "the seed of the problems file no longer holds"
    _install(eng, p)
    got = eng.ais_posterior(p.betas, p.C, p.K, pp.STREAM_SEED, 0, mean=True, keep_chains=True)
    decided = want["margin"] > pp.MARGIN_DECIDED  # (N, C)
    same = (got["chain_flips"] == want["chain_flips"]) & (got["chain_map_state"] == want["chain_map_state"]).all(axis=2)
    err = {k: np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k])) for k in ("log_w", "rb", "chain_map_lpj")}
    print("%s: %d of %d chains undecided, smallest margin %.3g; against the mirror log_w %.3g, rb %.3g, chain_map_lpj %.3g; "
          "p %.3g, p_se %.3g; flips %d" % (name, (~decided).sum(), decided.size, want["margin"].min(), err["log_w"][decided].max(),
                                          err["rb"][decided].max(), err["chain_map_lpj"][decided].max(),
                                          np.abs(got["p"] - want["p"]).max(), np.abs(got["p_se"] - want["p_se"]).max(),
                                          got["n_flips"].sum()))
    assert same[decided].all(), np.argwhere(decided & ~same)
    for k, e in err.items():
        assert (e[decided] <= RTOL).all(), k
    assert (~decided).sum() <= pp.MAX_UNDECIDED * decided.size
    rows = decided.all(axis=1)
    for k in ("p", "p_se", "count", "map_lpj", "ll", "ess", "log_w_mean", "log_w_min", "log_w_max"):
        assert got[k].shape == want[k].shape and _close(got[k][rows], want[k][rows]).all(), k
    assert np.array_equal(got["map_state"][rows], want["map_state"][rows]) and got["map_state"].dtype == np.uint8
    assert np.array_equal(got["n_flips"][rows], want["n_flips"][rows]) and got["n_flips"].dtype == np.int64
    # mean = p W^T, through the GEMM
    assert _close(got["mean"], np.dot(got["p"], p.theta["W"].T)).all()
    assert _close(got["mean"][rows], want["mean"][rows]).all()


# ---- 6. the chains are those of ais_loglik -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_words", "nc16"])
def test_one_kept_scan_is_the_forward_chain(eng, name):
    p = pp.problem(name)
    _install(eng, p)
    fwd = eng.ais_loglik(p.betas, p.C, pp.STREAM_SEED, 0, keep_states=True)
    got = eng.ais_posterior(p.betas, p.C, 1, pp.STREAM_SEED, 0, keep_chains=True)
    for k in ("log_w", "ll", "ess", "n_flips", "log_w_mean", "log_w_min", "log_w_max", "chain_flips"):
        assert np.array_equal(got[k], fwd[k]), k
    # the state after the one kept scan is the chain's best state, and ais_loglik's `final`
    assert np.array_equal(got["chain_map_state"].reshape(-1), fwd["final"])
    more = eng.ais_posterior(p.betas, p.C, 3, pp.STREAM_SEED, 0, keep_chains=True)
    assert np.array_equal(more["log_w"], fwd["log_w"]) and np.array_equal(more["ll"], fwd["ll"])
    assert not np.array_equal(more["rb"], got["rb"]) and (more["chain_map_lpj"] >= got["chain_map_lpj"]).all()


# ---- 7. against the exact marginals on the GPU ---------------------------------------------------------------------------------
def _suff(ss):
    N, S, H = ss.shape
    suff = init_states(0, S, H, "fit", "randflip", 6, 5, 1)
    suff["ss"] = ss.copy()
    suff["lpj"] = np.zeros((N, S))
    return suff


def test_model_against_the_exact_marginals(model_eng):
    c = pp.EXACT
    p = pp.exact_problem()
    S = 8
    model = BSC(p.D, p.H, S, engine=model_eng)
    suff = _suff(seed_states_host("bsc", p.theta, p.Y, S, 2, 0)[0])
    data = {"y": p.Y, "x_infr": np.ones_like(p.Y, dtype=bool)}
    _, _, exact = model.exact_log_likelihood(data, dict(p.theta), suff, marginals=True)
    assert np.abs(exact - p.exact).max() <= 1e-9
    keys = (set(p.theta), set(suff), set(data))
    kw = dict(n_chains=c["C"], n_temps=c["T"], n_keep=c["K"], seed=pp.EXACT_STREAM)
    got = model.ais_posterior(p.theta, suff, data, mean=True, **kw)
    assert model.last_ais_seed == pp.EXACT_STREAM  # (one rank: the stream seed the problems file chose the data seed for)
    assert (set(p.theta), set(suff), set(data)) == keys, "the call wrote into a dict"
    assert set(got) == {"p", "p_se", "count", "map_lpj", "map_state", "ll", "ess", "log_w_mean", "log_w_min", "log_w_max",
                        "n_flips", "mean"}
    pp.check_bars(got, exact)
    assert _close(got["mean"], np.dot(got["p"], p.theta["W"].T)).all()
    # the forward bound of ais_log_likelihood is the same number
    _, lower = model.ais_log_likelihood(p.theta, suff, data, n_chains=c["C"], n_temps=c["T"], seed=pp.EXACT_STREAM,
                                        per_datapoint=True)
    assert np.array_equal(lower["ll"], got["ll"]) and np.array_equal(lower["ess"], got["ess"])
    # the mirror, where its chains are decided
    rows = (p.want["margin"] > pp.MARGIN_DECIDED).all(axis=1)
    assert rows.any()
    for k in ("p", "p_se", "map_lpj"):
        assert _close(got[k][rows], p.want[k][rows]).all(), k
    # seed=None draws one and leaves it behind
    model.ais_posterior(p.theta, suff, data, n_chains=2, n_temps=4, n_keep=1)
    assert isinstance(model.last_ais_seed, int)
    assert _same(model.ais_posterior(p.theta, suff, data, mean=True, **kw), got)


# ---- 8. write-free, deterministic, streamed, blocked ---------------------------------------------------------------------------
def test_write_free_deterministic_and_streamed(eng):
    p = pp.problem("two_words")
    S, Cmax = 12, 4
    ss = seed_states_host("bsc", p.theta, p.Y, S, 3, 0)[0]
    _install(eng, p, S, Cmax, ss)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    eng.stats()
    rec = eng.reconstruct()
    before = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.download_posterior()[0],
              eng.debug_validity())
    kw = dict(n_chains=p.C, n_keep=p.K, seed=9, mean=True, keep_chains=True)
    a = eng.ais_posterior(p.betas, **kw)
    b = eng.ais_posterior(p.betas, **kw)
    assert _same(a, b), "two calls differ"
    after = (eng.download_states_packed(), eng.download_lpj(), eng.download_candidates(), eng.download_posterior()[0],
             eng.debug_validity())
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[3], after[3])
    for x, y in zip(before[2], after[2]):
        assert np.array_equal(x, y, equal_nan=True)
    assert before[4] == after[4], {k: (before[4][k], after[4][k]) for k in before[4] if before[4][k] != after[4][k]}
    assert np.array_equal(eng.reconstruct(), rec), "reconstruct no longer returns what it did"
    # fewer chains are a prefix
    pre = eng.ais_posterior(p.betas, **dict(kw, n_chains=3))
    for k in ("log_w", "rb", "chain_map_lpj", "chain_map_state", "chain_flips"):
        assert np.array_equal(pre[k], a[k][:, :3]), k
    # the block size does not show: one datapoint per block, and a block that does not divide N
    for block in (1, 8):
        assert _same(eng.ais_posterior(p.betas, block=block, **kw), a), block
    # shards by first_index concatenate to the single call
    cut = 8
    parts = []
    for rows, first in ((slice(0, cut), 0), (slice(cut, None), cut)):
        eng.configure("bsc", p.N - cut if first else cut, p.D, p.H, S, 0, Cmax)
        eng.upload_data(np.ascontiguousarray(p.Y[rows]))
        eng.set_params_bsc(p.theta["W"], float(p.theta["pi"]), float(p.theta["sigma"]))
        parts.append(eng.ais_posterior(p.betas, first_index=first, **kw))
    for k in a:
        assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]]), a[k]), k


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
    p = pp.problem("partial_chunk")
    S, Cmax = 6, 4
    ss = seed_states_host("bsc", p.theta, p.Y, S, 2, 0)[0]
    _install(eng, p, S, Cmax, ss)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 5, True)
    b = p.betas
    first = eng.ais_posterior(b, 3, 2, 1, 0, keep_chains=True)
    for call, match in (
            (lambda: eng.ais_posterior(b, 0, 2, 1, 0), "evoamd_ais_posterior: n_chains"),
            (lambda: eng.ais_posterior(b, 3, 0, 1, 0), "evoamd_ais_posterior: n_keep"),
            (lambda: eng.ais_posterior(np.array([0.1, 1.0]), 3, 2, 1, 0), "evoamd_ais_posterior: betas must start at 0"),
            (lambda: eng.ais_posterior(np.array([0.0, 0.5, 0.9]), 3, 2, 1, 0), "evoamd_ais_posterior: betas must end at 1"),
            (lambda: eng.ais_posterior(np.array([0.0, 0.6, 0.5, 1.0]), 3, 2, 1, 0), "evoamd_ais_posterior: betas must not descend"),
            (lambda: eng.ais_posterior(b, 3, 2, 1, 0, block=-1), "evoamd_ais_posterior: block_datapoints"),
            (lambda: eng.ais_posterior(b, 3, 2, 1, 0, block=2 ** 40), "evoamd_ais_posterior: the per-chain rows of one block"),
            (lambda: _lib.check(eng.lib.evoamd_ais_posterior(eng._h, 3, pp.CASES["partial_chunk"][3], 2, None, 1, 0, 0, None)),
             "evoamd_ais_posterior: betas is NULL")):
        _refused(eng, call, match)
    eng.set_option("background_unit", 1)
    _refused(eng, lambda: eng.ais_posterior(b, 3, 2, 1, 0), "evoamd_ais_posterior: option background_unit")
    eng.set_option("background_unit", 0)
    eng.upload_masks(np.ones((p.N, p.D), dtype=bool))
    _refused(eng, lambda: eng.ais_posterior(b, 3, 2, 1, 0), "evoamd_ais_posterior: incomplete data")
    eng.upload_masks(None)
    assert _same(eng.ais_posterior(b, 3, 2, 1, 0, keep_chains=True), first)
    # options that are read when Theta is installed or the context configured: each on a context of its own shape
    eng.set_option("bsc_direct", 1)
    try:
        _install(eng, p, S, Cmax, ss)
        with pytest.raises(EvoAmdError, match="evoamd_ais_posterior: bsc_direct"):
            eng.ais_posterior(b, 3, 2, 1, 0)
    finally:
        eng.set_option("bsc_direct", 0)
    eng.set_option("ebsc_f32", 1)
    try:
        p4 = ap.build(9, 8, 16, 1)  # (the float32 mode asks for H % 4 == 0 and D % 4 == 0)
        _install(eng, p4)
        with pytest.raises(EvoAmdError, match="evoamd_ais_posterior is not available in the float32 mode"):
            eng.ais_posterior(b, 3, 2, 1, 0)
    finally:
        eng.set_option("ebsc_f32", 0)
    big = ap.build(2, 2, 1030, 1)
    _install(eng, big)
    with pytest.raises(EvoAmdError, match="evoamd_ais_posterior: H = 1030, at most 1024 latents"):
        eng.ais_posterior(b, 3, 2, 1, 0)
    es3c = sp.problem("es3c", "ragged")
    eng.configure("sssc", es3c.N, es3c.D, es3c.H, es3c.S, 0, es3c.Cmax)
    eng.upload_data(es3c.Y)
    th = es3c.theta
    eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    with pytest.raises(EvoAmdError, match="evoamd_ais_posterior: ES3C is not supported"):
        eng.ais_posterior(b, 3, 2, 1, 0)
    _install(eng, p, S, Cmax, ss)
    assert _same(eng.ais_posterior(b, 3, 2, 1, 0, keep_chains=True), first)


# ---- 10. the kernel class ------------------------------------------------------------------------------------------------------
def test_kernel_class_is_named(eng):
    assert _lib.KERNEL_IDS_EXTRA["ais_post"] == 36
    assert eng.lib.evoamd_kernel_name(36) == b"ais_post"
    p = pp.problem("partial_chunk")
    _install(eng, p)
    eng.timing(("ais_post", "gemm_f64"))
    eng.timing_reset()
    eng.ais_posterior(p.betas, 2, 2, 1, 0, mean=True, block=5)  # eight blocks, one span
    ms, launches = eng.kernel_time_ms("ais_post")
    _, gemms = eng.kernel_time_ms("gemm_f64")
    eng.timing(False)
    assert launches == 1 and ms > 0.0 and gemms == 1

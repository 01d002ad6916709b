"""The context and the memory it owns (csrc/evo_amd.hip: DevBuf / PinnedBuf, evoamd_configure, the option table): no buffer
outlives its context, a failed configure leaves the context unconfigured, a reconfigured context computes what a fresh
one does, and every option keeps its range and its message.  Tiny shapes; every test works on contexts of its own."""
import ctypes

import numpy as np
import pytest

import _estep_problems as ep

pytestmark = pytest.mark.gpu

N, S, CMAX = 64, 4, 4
ES_SMALL = ("es3c", N, 8, 6, S, 0, CMAX)
BSC_LARGE = ("bsc", N, 12, 8, S, 0, CMAX)
LEARN = {"es3c": ("W", "pies", "mus", "sigma2", "Psi"), "bsc": ("W", "pi", "sigma")}
# two device runs of the same statistics kernels: the bound test_gpu_models.py holds two such accumulators to
# (test_stats_flat_kernel_matches_wave_kernel)
ACC_RTOL, ACC_ATOL = 1e-11, 1e-13


def _live():
    from evo_amd import _lib
    out = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().evoamd_debug_live_buffers(out))
    return int(out[0]), int(out[1])


def _problem(geom, seed):
    model, n, D, H, s = geom[:5]
    rng = np.random.RandomState(seed)
    theta = ep.es3c_theta(rng, D, H) if model == "es3c" else ep.bsc_theta(rng, D, H)
    latents = (rng.random_sample((n, H)) < 0.3).astype(float)
    Y = latents @ theta["W"].T + 0.5 * rng.normal(size=(n, D))
    return {"geom": geom, "Y": Y, "ss": ep.make_kn(rng, n, s, H, kmax=4), "theta": theta}


def _set_params(eng, p):
    t = p["theta"]
    if p["geom"][0] == "es3c":
        eng.set_params_sssc(t["W"], t["pies"], t["mus"], t["Psi"], t["sigma2"])
    else:
        eng.set_params_bsc(t["W"], t["pi"], t["sigma"])


def _iteration(eng, p, configure=True, between=None):
    """One EM iteration through the public calls.  Returns (lpj, K^n, accumulator views); ``between`` runs after the
    statistics pass and before the Theta update."""
    if configure:
        eng.configure(*p["geom"])
    eng.upload_data(p["Y"])
    eng.upload_states(p["ss"])
    _set_params(eng, p)
    eng.lpj_resident()
    eng.evolve_randflip(2, 2, 11)
    eng.vary_kn(p["geom"][4])
    views = {k: np.array(v) for k, v in dict(eng.acc_views(eng.stats())).items()}
    lpj, kn = eng.download_lpj(), eng.download_states()
    if between:
        between()
    eng.mstep_device(LEARN[p["geom"][0]])
    return lpj, kn, views


def _touch_grown_on_demand(eng, p):
    """Every feature whose buffers are cut on first use, once, at the configured ES3C shape (after a statistics pass)."""
    _, n, D, H = p["geom"][:4]
    rng = np.random.RandomState(5)
    t = p["theta"]
    states = ep.make_kn(rng, 1, 5, H, kmax=4)[0]
    eng.posterior_codes(max_active=4)
    eng.download_posterior()
    eng.predictive_moments()
    eng.reconstruct_resident(rng.random_sample((n, D)) < 0.5)
    eng.download_reconstruction()
    eng.lpj_shared(states)
    eng.lpj_single(p["Y"][0], states)
    eng.generate("es3c", n, 3, t["W"].T.copy(), t["pies"], t["mus"], np.linalg.cholesky(t["Psi"]), sigma=0.5)
    eng.download_generated("y")
    eng.loglik_exact(marginals=True)
    eng.free_energy_sum(rng.normal(size=(n, 5)))
    eng.gemm_tn(rng.normal(size=(40, 6)), rng.normal(size=(40, 6)))
    img = rng.normal(size=(12, 12))
    Yp = eng.patches_extract(img, 3, 3)
    for method in ("mean", "median"):
        np.testing.assert_allclose(eng.patches_merge(Yp, img.shape, 3, 3, method=method), img, rtol=1e-12, atol=1e-12)
    eng.patches_merge(Yp, img.shape, 3, 3, method="precision", weights=np.ones_like(Yp))
    eng.evolve_states("randflip", 2, 2, 1, 13)  # the general EA's buffers


def test_no_buffer_outlives_its_context():
    from evo_amd.engine import Engine
    before = _live()
    eng = Engine()
    try:
        p = _problem(ES_SMALL, 1)
        _iteration(eng, p, between=lambda: _touch_grown_on_demand(eng, p))
        assert _live()[0] > before[0] and _live()[1] > before[1]
        eng.lpj_resident()  # (the pass the update prefetched)
        eng.init_states(0.3, 17)
        eng.lpj_resident()
        x_infr = np.random.RandomState(6).random_sample(p["Y"].shape) < 0.8
        eng.upload_masks(x_infr)  # incomplete data: a masked pass over K^n and a masked statistics pass
        eng.set_reliable_fraction(x_infr.sum() / float(N))
        _set_params(eng, p)
        eng.lpj_resident()
        eng.lpj_single(p["Y"][0], p["ss"][0], x_infr=x_infr[0])
        eng.set_option("reconstruct_in_stats", 1)
        eng.stats()
        eng.upload_masks(None)
        _iteration(eng, _problem(BSC_LARGE, 2))
        eng.set_option("ebsc_f32", 1)
        _iteration(eng, _problem(BSC_LARGE, 2))
    finally:
        eng.close()
    assert _live() == before


def test_failed_configure_leaves_the_context_unconfigured():
    from evo_amd.engine import Engine, EvoAmdError
    p = _problem(BSC_LARGE, 3)
    eng, fresh = Engine(), Engine()
    try:
        _iteration(eng, p)
        eng.set_option("ebsc_f32", 1)
        with pytest.raises(EvoAmdError, match="multiples of 4"):
            eng.configure("bsc", 64, 6, 6, 4, 0, 4)
        with pytest.raises(EvoAmdError, match="configure first"):
            eng.upload_data(p["Y"])
        with pytest.raises(EvoAmdError, match="configure first"):
            eng.upload_states(p["ss"])
        eng.set_option("ebsc_f32", 0)
        got = _iteration(eng, p)
        want = _iteration(fresh, p)
    finally:
        eng.close()
        fresh.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for k in want[2]:
        np.testing.assert_allclose(got[2][k], want[2][k], rtol=ACC_RTOL, atol=ACC_ATOL, err_msg=k)


def test_reconfigure_equals_fresh():
    from evo_amd.engine import Engine
    small, large = _problem(ES_SMALL, 4), _problem(BSC_LARGE, 5)
    eng, fresh = Engine(), Engine()
    try:
        first = _iteration(eng, small)
        _iteration(eng, large)
        third = _iteration(eng, small)
        want = _iteration(fresh, small)
    finally:
        eng.close()
        fresh.close()
    for got in (third, want):
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])


# name: (lowest, highest, default, message)
RANGED = {
    "codes_path": (-1, 2, -1, "codes_path: -1 (auto), 0 registers, 1 LDS, 2 global memory"),
    "pair_bins_scale": (1, 64, 3, "pair_bins_scale: 1 .. 64"),
    "lpj_singular_screen": (0, 2, 1, "lpj_singular_screen: 0 (never), 1 (automatic) or 2 (always)"),
    "init_states_home": (-1, 1, -1, "init_states_home: -1 (auto), 0 LDS, 1 global memory"),
    "sk_spare": (-1, 32, -1, "sk_spare: -1 (automatic) or 0 .. 32 workgroups per XCD"),
    "stats_chunks": (1, 16, 1, "stats_chunks: 1 .. 16"),
    "fused_estep": (0, 2, 0, "fused_estep: 0 (never), 1 (automatic) or 2 (whenever the shape allows it)"),
    "pair_bins_nwg": (256, 2048, 2048, "pair_bins_nwg: 256 .. 2048, multiple of 256"),
}
# name: (accepted, refused, default, message)
SETS = {
    "inverse_block": ((0, 16, 32), (-1, 8, 33), 0, "inverse_block: 0 (auto), 16 or 32"),
    "pair_bins_nwg": ((256, 1024, 2048), (257, 384), 2048, "pair_bins_nwg: 256 .. 2048, multiple of 256"),
    "sssc_precision": ((64, 32), (0, 16, 65), 64, "sssc_precision: 64 or 32"),
}


def test_options_keep_their_ranges_and_messages():
    import re
    from evo_amd.engine import Engine, EvoAmdError
    eng = Engine()
    try:
        for name, (lo, hi, default, msg) in RANGED.items():
            try:
                for bad in (lo - 1, hi + 1):
                    with pytest.raises(EvoAmdError, match=re.escape(msg)):
                        eng.set_option(name, bad)
                eng.set_option(name, lo)
                eng.set_option(name, hi)
            finally:
                eng.set_option(name, default)
        for name, (good, bad, default, msg) in SETS.items():
            try:
                for v in bad:
                    with pytest.raises(EvoAmdError, match=re.escape(msg)):
                        eng.set_option(name, v)
                for v in good:
                    eng.set_option(name, v)
            finally:
                eng.set_option(name, default)
        with pytest.raises(EvoAmdError, match="unknown option 'no_such_option'"):
            eng.set_option("no_such_option", 1)
        # bsc_direct changes what set_params derives: the next pass asks for the parameters again
        p = _problem(BSC_LARGE, 6)
        _iteration(eng, p)
        eng.lpj_resident()
        try:
            eng.set_option("bsc_direct", 1)
            with pytest.raises(EvoAmdError, match="set_params first"):
                eng.lpj_resident()
            _set_params(eng, p)
            eng.lpj_resident()
        finally:
            eng.set_option("bsc_direct", 0)
    finally:
        eng.close()

"""The kappa route of the ES3C statistics pass (option "stats_kappa", csrc/kernels_sssc.hpp: sssc_stats_wave_kernel<.., KAP>):
the lpj pass over K^n leaves kappa of every state with at most two active latents, the selection kernel carries the records
of the accepted candidates, and the statistics pass reads them instead of the B rows and the state-term tables; the Lam
terms of the second moments go back in once per active set (sssc_kappa_diag_body, sssc_finish_kernel).

Every problem is run with the option on and off: lpj must be bit-identical, every accumulator must agree with the float64
oracle to SUM_RTOL and with the option-off pass to ROUTE_RTOL (the bound tests/test_gpu_fused.py holds accumulators to
across routes), and the launch count of the nested timing class "stats_kappa" says which route the pass took."""
import functools

import numpy as np
import pytest

import _stats_problems as sp

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-9     # against the oracle (tests/test_gpu_stats_paths.py)
ROUTE_RTOL = 1e-11  # option on against option off
LPJ_RTOL = 1e-9
CMAX = sp.CMAX
ES_NAMES = ("xpt_s", "xpt_ss", "xpt_sz", "xpt_szsz", "Wp", "s_sz_outer", "sz_sz_outer", "y_outer_diag", "Fs")

# name -> (profile, N, D, H, S, seed, non-symmetric Psi); even H only: odd H never takes the route
PROBLEMS = {
    "mid": ("mid", 255, 33, 64, 64, 1, False),         # every level 0..9 present, as in es_mid
    "s200": ("sparse", 65, 33, 66, 200, 21, False),    # HW = 2
    "wide": ("wide", 129, 32, 130, 37, 22, False),     # HW = 3: word-loop instantiations of the lpj kernel
    "s300": ("sparse", 37, 33, 64, 300, 23, False),    # a second group of 256 states per datapoint
    "h512": ("sparse", 31, 32, 512, 37, 24, False),
    "h2": ("sparse", 513, 33, 2, 1, 6, False),
    "mid_nonsym": ("mid", 255, 33, 64, 64, 1, True),   # Lam_01 != Lam_10
    "dense": ("dense", 257, 32, 64, 64, 2, False),     # es_dense: the overflowing bin regions
}


def make_problem(name):
    """The recipe of _stats_problems.make_problem (same draws in the same order) for the shapes above."""
    profile, N, D, H, S, seed, nonsym = PROBLEMS[name]
    rng = np.random.RandomState(seed)
    Y = rng.normal(size=(N, D))
    W = rng.normal(size=(D, H)) * 0.4
    A = rng.normal(size=(H, 3)) * 0.2
    theta = {"W": W, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H), "Psi": np.eye(H) + A @ A.T,
             "sigma2": np.float64(1.3)}
    ss = sp.make_states(rng, N, S, H, profile)
    if nonsym:
        C = 0.05 * np.random.RandomState(seed + 1000).normal(size=(H, H))
        theta["Psi"] = theta["Psi"] + (C - C.T)
    return {"name": name, "algo": "es3c", "profile": profile, "N": N, "D": D, "H": H, "S": S, "S_perm": 0, "Y": Y,
            "theta": theta, "ss": ss}


@pytest.fixture(scope="module")
def engine():
    from evo_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.set_option("stats_kappa", 1)
    eng.close()


def _close(a, b, rtol, name=""):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, err_msg=name)


def _oracle(p, ss):
    from oracle import evo_oracle as orc
    N, H, S = p["N"], p["H"], p["S"]
    suff = {"ss": ss, "lpj": np.empty((N, S)), "S_perm": 0, "incl": np.zeros((0, H), dtype=bool), "Mprime": S}
    want = dict(orc.sssc_EM_accumulate(dict(p["theta"]), suff, p["Y"], use_storage=True, evolve=False))
    want["Fs"] = orc.free_energy_sum(suff["lpj"])
    return suff["lpj"], want


@functools.lru_cache(maxsize=None)
def _reference(name):
    p = make_problem(name)
    lpj, want = _oracle(p, p["ss"])
    return p, lpj, want


def _setup(engine, p, opts, kappa):
    for k, v in opts.items():
        engine.set_option(k, v)
    engine.set_option("stats_kappa", 2 if kappa else 0)  # 2: whatever the size (1 = automatic starts at 16 M resident states)
    engine.configure("sssc", p["N"], p["D"], p["H"], p["S"], 0, CMAX)
    engine.upload_data(p["Y"])
    engine.upload_states(p["ss"])
    th = p["theta"]
    engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))


def _restore(engine, opts):
    for k in opts:
        engine.set_option(k, sp.DEFAULTS[k])
    engine.set_option("stats_kappa", 1)


def _counted_stats(engine):
    """One statistics pass; returns (accumulator views, launches of the kappa-route kernel)."""
    engine.timing(("stats_kappa",))
    try:
        engine.timing_reset()
        v = {k: np.array(x) for k, x in engine.acc_views(engine.stats()).items()}
        n = engine.kernel_time_ms("stats_kappa")[1]
    finally:
        engine.timing(False)
    return v, n


def _pass(engine, p, opts, kappa, between=None):
    """lpj_resident + stats under `opts` with the option at `kappa`; `between` runs after the lpj pass."""
    try:
        _setup(engine, p, opts, kappa)
        engine.lpj_resident()
        lpj = engine.download_lpj()
        if between:
            between(engine, p)
        v, n = _counted_stats(engine)
    finally:
        _restore(engine, opts)
    return lpj, v, n


def _compare(label, p, want_lpj, want, on, off):
    lpj_on, v_on, n_on = on
    lpj_off, v_off, n_off = off
    assert n_on == 1, label + ": the kappa route did not run with the option on"
    assert n_off == 0, label + ": the kappa route ran with the option off"
    assert np.array_equal(lpj_on, lpj_off), label + ": lpj depends on the option"
    _close(lpj_on, want_lpj, LPJ_RTOL, label + ": lpj")
    for k in ES_NAMES:
        _close(v_on[k], want[k], SUM_RTOL, "%s: %s vs oracle" % (label, k))
        _close(v_off[k], want[k], SUM_RTOL, "%s: %s (option off) vs oracle" % (label, k))
        _close(v_on[k], v_off[k], ROUTE_RTOL, "%s: %s on vs off" % (label, k))


@pytest.mark.parametrize("name", ["mid", "s200", "wide", "s300", "h512", "h2", "mid_nonsym"])
@pytest.mark.parametrize("bins", [2, 0], ids=["bins", "atomics"])
def test_kappa_route_matches_oracle_and_table_route(engine, name, bins):
    """bins = 2: the pair states go through the pair bins (four planes); 0: through the atomics on xss / xszsz."""
    p, want_lpj, want = _reference(name)
    opts = {"pair_bins": bins}
    on = _pass(engine, p, opts, 1)
    off = _pass(engine, p, opts, 0)
    _compare("%s pair_bins=%d" % (name, bins), p, want_lpj, want, on, off)
    if name == "mid_nonsym":
        z = want["xpt_szsz"]
        assert np.abs(z - z.T).max() > 1e-3 * np.abs(z).max()  # the case exercises Lam_01 != Lam_10


def test_kappa_route_overflowing_bin_regions(engine):
    """More entries than all regions of all bins hold (pigeonhole, as in test_stats_path): the pair states of a full region
    fall back to the atomics on xss / xszsz, the quad levels' entries to the _o matrices."""
    p, want_lpj, want = _reference("dense")
    opts = dict(sp.OVF)
    on = _pass(engine, p, opts, 1)
    off = _pass(engine, p, opts, 0)
    _compare("dense overflow", p, want_lpj, want, on, off)
    g = sp.pair_bins_geometry(p["N"], p["H"], p["S"], opts["pair_bins_scale"], opts["pair_bins_nwg"])
    live = (on[0] - on[0].max(axis=1, keepdims=True)) > -700.0
    assert sp.bin_entries(p["ss"], "es3c", live) > g["capacity"]


def _device_flow(engine, p, kappa):
    opts = {"pair_bins": 2}
    try:
        _setup(engine, p, opts, kappa)
        engine.lpj_resident()
        engine.stats()
        n_parents, n_children, seed = sp.EVOLVE
        engine.evolve_randflip(n_parents, n_children, seed)
        engine.vary_kn(p["S"])
        v, n = _counted_stats(engine)
        return engine.download_states(), engine.download_lpj(), v, n
    finally:
        _restore(engine, opts)


@pytest.mark.parametrize("name", ["mid", "s200"])
def test_kappa_records_follow_the_selection(engine, name):
    """pass, then evolve_randflip + lpj of the children + vary_kn, then the statistics pass under test: the accepted
    candidates' records moved into K^n with them."""
    p = make_problem(name)
    ss_on, lpj_on, v_on, n_on = _device_flow(engine, p, 1)
    ss_off, lpj_off, v_off, n_off = _device_flow(engine, p, 0)
    assert not np.array_equal(ss_on, p["ss"]), "vary_kn changed nothing"
    assert np.array_equal(ss_on, ss_off), "K^n depends on the option"
    assert np.array_equal(lpj_on, lpj_off)
    assert (n_on, n_off) == (1, 0)
    want_lpj, want = _oracle(p, ss_on)
    _close(lpj_on, want_lpj, LPJ_RTOL, "lpj")
    for k in ES_NAMES:
        _close(v_on[k], want[k], SUM_RTOL, "%s vs oracle" % k)
        _close(v_on[k], v_off[k], ROUTE_RTOL, "%s on vs off" % k)


def _set_params_again(engine, p):
    # (the lpj rows of the pass before the install still describe this Theta: the same values are installed)
    th = p["theta"]
    engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))


def _upload_again(engine, p):
    engine.upload_states(p["ss"])


@pytest.mark.parametrize("what", ["set_params", "upload_states", "stats_stage0", "stats_flat", "waves8", "odd_H"])
def test_every_other_event_takes_the_table_route(engine, what):
    """The records count only for the Theta and the K^n they were written for, and only on the census route of the
    four-wave kernel with staging on: anything else takes today's kernel, and is still right."""
    if what == "odd_H":
        p = sp.make_problem("es_few4")
        want_lpj, want = _oracle(p, p["ss"])
    else:
        p, want_lpj, want = _reference("mid")
    opts = {"pair_bins": 2}
    between = None
    if what == "set_params":
        between = _set_params_again
    elif what == "upload_states":
        between = _upload_again
    elif what == "stats_stage0":
        opts["stats_stage"] = 0
    elif what == "stats_flat":
        opts["stats_flat"] = 1
    elif what == "waves8":
        opts["stats_waves"] = 8
    lpj, v, n = _pass(engine, p, opts, 1, between)
    assert n == 0, what + ": the kappa route ran"
    _close(lpj, want_lpj, LPJ_RTOL, what + ": lpj")
    for k in ES_NAMES:
        _close(v[k], want[k], SUM_RTOL, "%s: %s vs oracle" % (what, k))


def test_model_steps_agree_with_the_option_off(engine):
    """Three SSSC.step iterations of the device path (device generator, device Theta update): K^n identical, F and every
    Theta entry within 1e-9 of the option-off trajectory."""
    from evo_amd.models import SSSC
    from evo_amd.variational import init_states
    D, H, S, N = 16, 32, 24, 200
    Y = np.random.RandomState(9).normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    res = []
    try:
        for kappa in (1, 0):
            engine.set_option("stats_kappa", 2 if kappa else 0)
            np.random.seed(4)
            model = SSSC(D, H, S, rng="device", sync_host=False, engine=engine, seed=3, device_mstep=True)
            theta = model.check_params(model.standard_init(my_data))
            suff = init_states(N, S, H, "fit", "randflip", 6, 1, 1)
            engine.timing(("stats_kappa",))
            engine.timing_reset()
            Fs = []
            for _ in range(3):
                F, _, _, theta = model.step(theta, suff, my_data)
                Fs.append(F)
            n = engine.kernel_time_ms("stats_kappa")[1]
            engine.timing(False)
            res.append((engine.download_states(), Fs, {k: np.array(v) for k, v in theta.items()}, n))
    finally:
        engine.timing(False)
        engine.set_option("stats_kappa", 1)
    assert res[0][3] == 3 and res[1][3] == 0, (res[0][3], res[1][3])
    assert np.array_equal(res[0][0], res[1][0]), "K^n depends on the option"
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=1e-9)
    for k in ("W", "pies", "mus", "Psi", "sigma2"):
        np.testing.assert_allclose(res[0][2][k], res[1][2][k], rtol=1e-9, atol=1e-9, err_msg=k)


def test_automatic_setting_has_a_size_threshold(engine):
    """stats_kappa = 1 takes the route from stats_kappa_min x 1024 resident states on (measured: small shards lose):
    16 k states stay on the table route under the default threshold and take the kappa route with the threshold at 0."""
    p, want_lpj, want = _reference("mid")
    counts = []
    try:
        for kmin in (16384, 0):
            engine.set_option("stats_kappa_min", kmin)
            engine.set_option("stats_kappa", 1)
            engine.configure("sssc", p["N"], p["D"], p["H"], p["S"], 0, CMAX)
            engine.upload_data(p["Y"])
            engine.upload_states(p["ss"])
            th = p["theta"]
            engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
            engine.lpj_resident()
            v, n = _counted_stats(engine)
            counts.append(n)
            for k in ES_NAMES:
                _close(v[k], want[k], SUM_RTOL, "stats_kappa_min=%d: %s vs oracle" % (kmin, k))
    finally:
        engine.set_option("stats_kappa_min", 16384)
        engine.set_option("stats_kappa", 1)
    assert counts == [0, 1], counts

"""Statistics pass (evoamd_stats) against the float64 oracle across its routes: pair bins on / off / overflowing / re-cut,
census lists or the round-2 chains, the K = 4 / K = 8 register kernels, the flat and word-path kernels, bin counts from 1
to PB_MAX_BINS, the EBSC wave and one-shot kernels, and -- on a K^n the device evolved -- the merged 5..8 level.  Problems
are synthetic (_stats_problems.py); every case is also compared with the pair_bins = 0 result of the same problem, which
differs only in summation order."""
import functools

import numpy as np
import pytest

import _stats_problems as sp

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-9    # against the oracle
BASE_RTOL = 1e-12  # against pair_bins = 0 on the same device
LPJ_RTOL = 1e-9
CMAX = sp.CMAX
ES_NAMES = ("xpt_s", "xpt_ss", "xpt_sz", "xpt_szsz", "Wp", "s_sz_outer", "sz_sz_outer", "y_outer_diag", "Fs")
BSC_NAMES = ("Wp", "Wq", "pies", "sigma", "Fs")
CASE_IDS = [c[0] for c in sp.CASES]


@pytest.fixture(scope="module")
def engine():
    from evo_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.close()


def _close(a, b, rtol, name=""):
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * scale, err_msg=name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(problem, lpj, sums) of the float64 oracle; once per problem and module."""
    p = sp.make_problem(name)
    lpj, want = _oracle(p, p["ss"])
    return p, lpj, want


def _oracle(p, ss):
    """lpj and M-step sums of the float64 oracle for problem `p` with K^n `ss`."""
    from oracle import evo_oracle as orc
    N, D, H, S, S_perm, Y = p["N"], p["D"], p["H"], p["S"], p["S_perm"], p["Y"]
    if p["algo"] == "es3c":
        suff = {"ss": ss, "lpj": np.empty((N, S)), "S_perm": 0, "incl": np.zeros((0, H), dtype=bool), "Mprime": S}
        want = orc.sssc_EM_accumulate(dict(p["theta"]), suff, Y, use_storage=True, evolve=False)
        lpj = suff["lpj"]
    else:
        th = dict(p["theta"])
        cnt = orc.bsc_precompute(th, D, H)
        lpj = np.empty((N, S_perm + S))
        for n in range(N):
            if S_perm:
                lpj[n, 0] = orc.bsc_lpj_allzero(th, Y[n], cnt)[0]
            lpj[n, S_perm:] = orc.bsc_lpj(th, ss[n], Y[n], cnt)
        suff = {"ss": ss, "lpj": lpj, "S_perm": S_perm, "permanent": {"allzero": bool(S_perm), "background": False}}
        want = orc.bsc_accumulate(th, suff, Y)
    want = dict(want)
    want["Fs"] = orc.free_energy_sum(lpj)
    return lpj, want


def _set_options(engine, opts):
    for k, v in opts.items():
        engine.set_option(k, v)


def _restore(engine, opts):
    for k in opts:
        engine.set_option(k, sp.DEFAULTS[k])


def _run(engine, p, opts, passes):
    """Configure (options first: some are read there), upload, then `passes` x (lpj_resident, stats).  Returns a list of
    (lpj, accumulator views) per pass."""
    _set_options(engine, opts)
    engine.configure("sssc" if p["algo"] == "es3c" else "bsc", p["N"], p["D"], p["H"], p["S"], p["S_perm"], CMAX)
    engine.upload_data(p["Y"])
    engine.upload_states(p["ss"])
    th = p["theta"]
    if p["algo"] == "es3c":
        engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    else:
        engine.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))
    out = []
    for _ in range(passes):
        engine.lpj_resident()
        lpj = engine.download_lpj()
        out.append((lpj, {k: np.array(v) for k, v in engine.acc_views(engine.stats()).items()}))
    return out


_BASELINE = {}


def _baseline(engine, name):
    """pair_bins = 0 (every pair through the global atomics) on the device, default options otherwise."""
    if name not in _BASELINE:
        p, _, _ = _reference(name)
        opts = {"pair_bins": 0}
        try:
            _BASELINE[name] = _run(engine, p, opts, 1)[0][1]
        finally:
            _restore(engine, opts)
    return _BASELINE[name]


def _check(engine, name, lpj, v, label):
    p, want_lpj, want = _reference(name)
    names = ES_NAMES if p["algo"] == "es3c" else BSC_NAMES
    _close(lpj, want_lpj, LPJ_RTOL, label + ": lpj")
    base = _baseline(engine, name)
    for k in names:
        _close(v[k], want[k], SUM_RTOL, "%s: %s vs oracle" % (label, k))
        _close(v[k], base[k], BASE_RTOL, "%s: %s vs pair_bins = 0" % (label, k))


def _live(p, lpj):
    """States whose q = exp(lpj - max) is not zero (with a wide margin): only those append to the bins."""
    l = lpj[:, p["S_perm"]:]
    return (l - lpj.max(axis=1, keepdims=True)) > -700.0


@pytest.mark.parametrize("case", sp.CASES, ids=CASE_IDS)
def test_stats_path(engine, case):
    cid, name, opts, flow, overflow = case
    p, _, _ = _reference(name)
    try:
        runs = _run(engine, p, opts, 2 if flow == "twice" else 1)
    finally:
        _restore(engine, opts)
    for i, (lpj, v) in enumerate(runs):
        _check(engine, name, lpj, v, "%s pass %d" % (cid, i + 1))
    if overflow:
        # pigeonhole: more entries than all regions of all bins hold -> at least one region fell back to the atomics
        g = sp.pair_bins_geometry(p["N"], p["H"], p["S"], opts.get("pair_bins_scale", sp.PAIR_BINS_SCALE),
                                  opts.get("pair_bins_nwg", sp.PAIR_BINS_NWG))
        entries = sp.bin_entries(p["ss"], p["algo"], _live(p, runs[0][0]))
        assert entries > g["capacity"], (cid, entries, g)
        if opts.get("pair_bins_auto", 1) and p["algo"] == "es3c":  # ES3C only: the second pass ran on bins re-cut
            # from the first pass's census (ensure_bins_capacity never re-cuts the EBSC bins)
            g2 = sp.pair_bins_geometry(p["N"], p["H"], p["S"], sp.recut_scale(p["ss"]), g["nwg"])
            assert g2["capacity"] > entries, (cid, entries, g2)


def _run_device(engine, p, opts):
    """A K^n evolved on the device: lpj_resident + stats over the uploaded K^n (the census the next pass decides from),
    evolve_randflip + vary_kn, then the pass under test with the 5..8 quad launches counted.  Returns (K^n, lpj, views,
    5..8 quad launches)."""
    _run(engine, p, opts, 1)
    n_parents, n_children, seed = sp.EVOLVE
    engine.evolve_randflip(n_parents, n_children, seed)
    engine.vary_kn(p["S"])
    engine.timing(("stats_k5_8",))
    try:
        engine.timing_reset()
        v = {k: np.array(x) for k, x in engine.acc_views(engine.stats()).items()}
        n58 = engine.kernel_time_ms("stats_k5_8")[1]
    finally:
        engine.timing(False)
    return engine.download_states(), engine.download_lpj(), v, n58


_DEVICE_BASELINE = {}


@pytest.mark.parametrize("case", sp.DEVICE_CASES, ids=[c[0] for c in sp.DEVICE_CASES])
def test_stats_path_device_kn(engine, case):
    """The statistics pass after a device E-step: the census of the last pass is known and the candidates came from the
    device, so the pass may merge levels.  merge_small_levels = 1 on a K^n with few states above four latents must serve
    the 5..8 list from the wavefront kernel (no 5..8 quad launch); 0 must launch it.  The oracle runs on the K^n the device
    produced; the pair_bins = 0 run of the same flow must produce the same K^n."""
    cid, name, opts, k58 = case
    p = sp.make_problem(name)
    if name not in _DEVICE_BASELINE:
        base_opts = {"pair_bins": 0}
        try:
            _DEVICE_BASELINE[name] = _run_device(engine, p, base_opts)
        finally:
            _restore(engine, base_opts)
    try:
        ss, lpj, v, n58 = _run_device(engine, p, opts)
    finally:
        _restore(engine, opts)
    bss, _, base, _ = _DEVICE_BASELINE[name]
    assert not np.array_equal(ss, p["ss"]), cid + ": vary_kn changed nothing"
    assert np.array_equal(ss, bss), cid + ": the pair_bins = 0 flow evolved a different K^n"
    assert ((sp.level_census(ss) >= 5) & (sp.level_census(ss) <= 8)).any(), cid
    want_lpj, want = _oracle(p, ss)
    _close(lpj, want_lpj, LPJ_RTOL, cid + ": lpj")
    for k in ES_NAMES:
        _close(v[k], want[k], SUM_RTOL, "%s: %s vs oracle" % (cid, k))
        _close(v[k], base[k], BASE_RTOL, "%s: %s vs pair_bins = 0" % (cid, k))
    if k58 is not None:
        assert (n58 > 0) == k58, (cid, n58)


def test_pass_that_returns_early_leaves_clean_bins(engine):
    """A statistics pass that returns between the producers that append to the pair bins and the reduce that clears
    their region counters (census lists on: the next pass's first producers start from those counters) must not leak
    entries into the next pass."""
    from evo_amd._lib import EvoAmdError
    p, _, _ = _reference("es_mid")
    _baseline(engine, "es_mid")  # (configures the engine itself: before the sequence under test)
    opts = {"pair_bins": 2}
    try:
        _run(engine, p, opts, 1)  # a complete pass first: the counters start from zero below either way
        engine.lpj_resident()
        engine.set_option("debug_fail_stats", 1)
        with pytest.raises(EvoAmdError, match="debug_fail_stats"):
            engine.stats()
        for i in range(2):
            engine.lpj_resident()
            lpj = engine.download_lpj()
            v = {k: np.array(x) for k, x in engine.acc_views(engine.stats()).items()}
            _check(engine, "es_mid", lpj, v, "after the stopped pass, pass %d" % (i + 1))
    finally:
        engine.set_option("debug_fail_stats", 0)
        _restore(engine, opts)


def test_poisoned_list_with_pair_bins_then_stats_matches_reference(engine):
    """The out-of-range census entry of test_out_of_range_list_entry_is_an_error_not_a_fault with the pair bins on: the
    pass after the error gives the oracle's values, not just some values."""
    from evo_amd._lib import EvoAmdError
    p, _, _ = _reference("es_mid")
    _baseline(engine, "es_mid")  # (configures the engine itself: before the sequence under test)
    opts = {"pair_bins": 2}
    try:
        _run(engine, p, opts, 0)
        engine.set_option("debug_poison_list", 1)
        engine.lpj_resident()
        with pytest.raises(EvoAmdError, match="out of range"):
            engine.stats()
        engine.lpj_resident()  # fresh census
        lpj = engine.download_lpj()
        v = {k: np.array(x) for k, x in engine.acc_views(engine.stats()).items()}
        _check(engine, "es_mid", lpj, v, "after the poisoned pass")
    finally:
        engine.set_option("debug_poison_list", 0)
        _restore(engine, opts)

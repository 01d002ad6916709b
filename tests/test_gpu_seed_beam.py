"""Beam seeding of K^n on the GPU: Engine.seed_states_beam (csrc/kernels_seed_beam.hpp) and
Model.seed_resident_states(beam=B).

1. beam = 1 against the greedy kernel (Engine.seed_states) on every case of tests/_seed_problems.py, both models: packed
   states, path, lpj_path and the lpj rows of a pass afterwards (which read the digests) are equal bit for bit;
2. beam > 1 against the NumPy mirror (evo_amd.variational.seed_states_beam_host): the states of every slot, path, lpj_path
   and the lpj of every slot (1e-9 relative).  All datapoints must agree: tests/test_seed_beam_host.py holds the committed
   seeds to a margin of 1e-7;
3. the digests the kernel writes against digest_kernel's (same lpj bits before and after a re-upload of the same rows);
4. two calls give the same words, no stale rows or prefetched pass afterwards, refinement and sweeps run from the beam start;
5. every refusal leaves K^n, the lpj rows and the validity state as they were;
6. Model.seed_resident_states(beam=4) for both models, device-resident and host-synchronised; beam=None is today's call.
"""
import numpy as np
import pytest

import _beam_problems as bp
import _seed_problems as sdp
from evo_amd._lib import EvoAmdError
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC

pytestmark = pytest.mark.gpu

LPJ_RTOL = 1e-9
EA = ("fit", "randflip", 6, 1, 1)


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
    """The Model tests' own engine: Model._prepare keeps per-engine state that the engine-level tests do not maintain."""
    e = Engine(0)
    yield e
    e.close()


def _set_params(eng, algo, th):
    if algo == "ebsc":
        eng.set_params_bsc(th["W"], th["pi"], th["sigma"])
    else:
        eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], th["sigma2"])


def _install(eng, p):
    eng.configure("bsc" if p.algo == "ebsc" else "sssc", p.N, p.D, p.H, p.S, p.S_perm, 4)
    eng.upload_data(p.Y)
    _set_params(eng, p.algo, p.theta)


@pytest.mark.parametrize("name", sorted(sdp.CASES))
@pytest.mark.parametrize("algo", bp.ALGOS)
def test_beam_one_is_the_greedy_kernel(eng, algo, name):
    p = sdp.problem(algo, name)
    _install(eng, p)
    path_g, lpj_g = eng.seed_states(p.A, want_path=True)
    packed_g = eng.download_states_packed()
    eng.lpj_resident()
    rows_g = eng.download_lpj()
    eng.init_states(0.3, 5)  # something else in between
    path_b, lpj_b = eng.seed_states_beam(p.A, 1, want_path=True)
    assert path_b.dtype == np.int32 and path_b.shape == (p.N, p.A) and lpj_b.shape == (p.N, p.A)
    assert np.array_equal(eng.download_states_packed(), packed_g)
    assert np.array_equal(path_b, path_g)
    assert np.array_equal(lpj_b, lpj_g)
    eng.lpj_resident()
    assert np.array_equal(eng.download_lpj(), rows_g)  # the digests too


@pytest.mark.parametrize("name,beam", [("ragged", 3), ("ragged_perm", 3), ("tight", 4), ("tight", 6), ("s200", 4), ("s200", 16),
                                       ("large_h2", 2)])
@pytest.mark.parametrize("algo", bp.ALGOS)
def test_kernel_equals_mirror(eng, algo, name, beam):
    p = bp.problem(algo, name, beam)
    _install(eng, p)
    path, lpj_path = eng.seed_states_beam(p.A, beam, want_path=True)
    got = eng.download_states()
    assert got.shape == p.states.shape
    assert np.array_equal(eng.download_states_packed(), np.packbits(got, axis=-1))
    print("%s %s beam %d: smallest margin of the mirror %.3g" % (algo, name, beam, p.margin.min()))
    bad = [n for n in range(p.N) if not np.array_equal(got[n], p.states[n])]
    assert not bad, "datapoints whose states differ: %s" % bad[:8]
    assert np.array_equal(path, p.path)
    err = np.abs(lpj_path - p.lpj_path) / np.maximum(1.0, np.abs(p.lpj_path))
    assert err.max() <= LPJ_RTOL, err.max()
    eng.lpj_resident()
    rows = eng.download_lpj()
    assert rows.shape == (p.N, p.S_perm + p.S) and np.isfinite(rows).all()  # no clamp fired
    err = np.abs(rows[:, p.S_perm:] - p.lpj) / np.maximum(1.0, np.abs(p.lpj))
    print("%s %s beam %d: largest relative difference of a slot's lpj %.3g" % (algo, name, beam, err.max()))
    assert err.max() <= LPJ_RTOL


@pytest.mark.parametrize("algo,name,beam", [("es3c", "ragged", 3), ("ebsc", "s200", 16), ("ebsc", "large_h2", 2)])
def test_digests_equal_digest_kernel(eng, algo, name, beam):
    """The lpj kernels read the digests: the rows the beam kernel wrote must evaluate exactly like the same rows uploaded
    (upload_states_packed runs digest_kernel)."""
    p = bp.data(algo, name)
    _install(eng, p)
    eng.seed_states_beam(p.A, beam)
    eng.lpj_resident()
    before = eng.download_lpj()
    packed = eng.download_states_packed()
    eng.upload_states_packed(packed)
    eng.lpj_resident()
    assert np.isfinite(before).all()
    assert np.array_equal(before, eng.download_lpj())


@pytest.mark.parametrize("algo", bp.ALGOS)
def test_no_stale_state_after_seeding(eng, eng2, algo):
    p = bp.data(algo, "ragged_perm")
    _install(eng, p)
    eng.init_states(1.0 / p.H, 5)
    eng.lpj_resident()
    noise = eng.download_lpj()
    eng.seed_states_beam(p.A, 3)
    eng.lpj_resident()
    seeded = eng.download_lpj()
    packed = eng.download_states_packed()
    assert not np.array_equal(noise, seeded)
    _install(eng2, p)  # a fresh context that uploads the same states
    eng2.upload_states_packed(packed)
    eng2.lpj_resident()
    assert np.array_equal(seeded, eng2.download_lpj())
    eng.seed_states_beam(p.A, 3)
    assert np.array_equal(eng.download_states_packed(), packed)
    # the statistics rows of the old K^n are gone too: the codes are refused until a new pass has run
    eng.lpj_resident()
    eng.stats()
    eng.posterior_codes(4)
    eng.seed_states_beam(p.A, 3)
    with pytest.raises(EvoAmdError):
        eng.posterior_codes(4)


@pytest.mark.parametrize("algo", bp.ALGOS)
def test_refine_and_sweeps_run_from_the_beam_start(model_eng, algo):
    p = bp.data(algo, "correlated")
    cls = BSC if algo == "ebsc" else SSSC
    my_data = {"y": np.array(p.Y), "x_infr": np.ones(p.Y.shape, dtype=bool)}
    model = cls(p.D, p.H, p.S, engine=model_eng, rng="device", sync_host=False, seed=1)
    suff = model.seed_resident_states(dict(p.theta), my_data, *EA, max_active=p.A, beam=4)
    F0 = model_eng.ljc + model.posterior_scores(dict(p.theta), suff, my_data)["F"].mean()
    res = model.refine_resident_states(dict(p.theta), suff, my_data, 2)
    assert res.n_done == 2 and np.isfinite(res.F).all() and res.F[0] >= F0 - 1e-9 * abs(F0)
    sw = model.sweep_resident_states(dict(p.theta), suff, my_data, n_sweeps=2, neighbourhood="both", stop_when_quiet=False)
    assert sw.n_done == 2 and np.isfinite(sw.F).all()
    assert sw.F[0] >= res.F[-1] - 1e-9 * abs(res.F[-1]) and sw.F[1] >= sw.F[0] - 1e-9 * abs(sw.F[0])


def test_refusals_leave_everything_alone(eng):
    p = bp.data("ebsc", "tight")
    N, D, H, S = p.N, p.D, p.H, p.S
    rng = np.random.RandomState(2)

    def refused(match, A=p.A, beam=2):
        before = eng.download_states_packed(), eng.download_lpj(), eng.debug_validity()
        with pytest.raises(EvoAmdError, match=match):
            eng.seed_states_beam(A, beam, want_path=True)
        assert np.array_equal(eng.download_states_packed(), before[0])
        assert np.array_equal(eng.download_lpj(), before[1])
        assert eng.debug_validity() == before[2]

    for algo in bp.ALGOS:
        q = bp.data(algo, "tight")
        eng.configure("bsc" if algo == "ebsc" else "sssc", N, D, H, S, 0, 4)
        eng.upload_data(q.Y)
        eng.init_states(0.3, 9)
        with pytest.raises(EvoAmdError, match="no Theta"):
            eng.seed_states_beam(q.A, 2)
        _set_params(eng, algo, q.theta)
        eng.lpj_resident()
        refused("max_active = 0", 0)
        refused("max_active = 21", 21)  # > S
        refused("max_active = 9", 9)    # > Hv (and > 8 for ES3C)
        refused("quota q_1 = 10", 2)
        refused("beam = 0", beam=0)
        refused("beam = -3", beam=-3)
        refused("beam = 7", beam=7)     # > S / A = 6
        eng.seed_states_beam(q.A, 6)    # the bound itself is admitted
        eng.lpj_resident()
        eng.set_option("background_unit", 1)
        try:
            refused("background_unit")
        finally:
            eng.set_option("background_unit", 0)
        xi = np.ones((N, D), dtype=bool)
        xi[0, 0] = False
        eng.upload_masks(xi)
        try:
            _set_params(eng, algo, q.theta)
            eng.lpj_resident()
            refused("incomplete data")
        finally:
            eng.upload_masks(None)
            eng.upload_data(q.Y)
    # the caps: 8 steps for ES3C, 64 for EBSC, 16 beam members
    for algo, A, beam, match in (("es3c", 9, 2, "ES3C: at most 8"), ("ebsc", 65, 1, "EBSC: at most 64"), ("ebsc", 4, 17, "beam = 17"),
                                 ("es3c", 4, 17, "beam = 17")):
        Hc, Sc = 80, 80
        eng.configure("bsc" if algo == "ebsc" else "sssc", 3, D, Hc, Sc, 0, 4)
        eng.upload_data(rng.normal(size=(3, D)))
        _set_params(eng, algo, sdp.make_theta(rng, algo, D, Hc))
        eng.init_states(0.1, 9)
        eng.lpj_resident()
        refused(match, A, beam)
        if beam == 17:
            eng.seed_states_beam(A, 16)  # the cap itself is admitted
    # EBSC only: the direct residual kernel keeps no G; the float32 mode
    q = bp.data("ebsc", "tight")
    _install(eng, q)
    eng.init_states(0.3, 9)
    eng.set_option("bsc_direct", 1)
    try:
        _set_params(eng, "ebsc", q.theta)
        eng.lpj_resident()
        refused("bsc_direct")
    finally:
        eng.set_option("bsc_direct", 0)
    eng.set_option("ebsc_f32", 1)
    try:
        _install(eng, q)
        eng.init_states(0.3, 9)
        eng.lpj_resident()
        refused("float32")
    finally:
        eng.set_option("ebsc_f32", 0)
        _install(eng, q)


@pytest.mark.parametrize("sync_host", [False, True])
@pytest.mark.parametrize("algo", bp.ALGOS)
def test_model_seed_resident_states_beam(model_eng, algo, sync_host):
    eng = model_eng
    one, four = bp.problem(algo, "correlated", 1), bp.problem(algo, "correlated", 4)
    p = four
    cls = BSC if algo == "ebsc" else SSSC
    my_data = {"y": np.array(p.Y), "x_infr": np.ones(p.Y.shape, dtype=bool)}
    kw = dict(engine=eng, rng="device", sync_host=sync_host, seed=1)
    # beam=None is the call without the argument
    plain = cls(p.D, p.H, p.S, **kw)
    plain.seed_resident_states(dict(p.theta), my_data, *EA, max_active=p.A, want_path=True)
    words_plain, rows_plain, path_plain = eng.download_states_packed(), eng.download_lpj(), plain.last_seed_path
    none = cls(p.D, p.H, p.S, **kw)
    suff_none = none.seed_resident_states(dict(p.theta), my_data, *EA, max_active=p.A, want_path=True, beam=None)
    assert np.array_equal(eng.download_states_packed(), words_plain) and np.array_equal(eng.download_lpj(), rows_plain)
    assert np.array_equal(none.last_seed_path[0], path_plain[0]) and np.array_equal(none.last_seed_path[1], path_plain[1])
    assert np.array_equal(eng.download_states(), one.states)
    F_none = none.posterior_scores(dict(p.theta), suff_none, my_data)["F"].mean()
    # beam=4
    model = cls(p.D, p.H, p.S, **kw)
    suff = model.seed_resident_states(dict(p.theta), my_data, *EA, max_active=p.A, want_path=True, beam=4)
    path, lpj_path = model.last_seed_path
    assert np.array_equal(path, p.path) and path.dtype == np.int32 and lpj_path.shape == (p.N, p.A)
    if sync_host:
        assert suff["ss"].shape == (p.N, p.S, p.H) and suff["ss"].dtype == np.bool_
        assert suff["lpj"].shape == (p.N, p.S) and suff["lpj"].dtype == np.float64
        ss, rows = suff["ss"], suff["lpj"]
        assert np.array_equal(rows, eng.download_lpj())
    else:
        assert suff["ss"] is None and suff["lpj"] is None
        ss, rows = eng.download_states(), eng.download_lpj()
    assert suff["S_perm"] == 0
    assert np.array_equal(ss, p.states)
    err = np.abs(rows - p.lpj) / np.maximum(1.0, np.abs(p.lpj))
    assert err.max() <= LPJ_RTOL
    F_beam = model.posterior_scores(dict(p.theta), suff, my_data)["F"].mean()
    want = bp.mean_log_sum(four.lpj) - bp.mean_log_sum(one.lpj)
    print("%s sync_host=%s: mean F %.6f (beam 4) - %.6f (greedy) = %.6f, the mirror's difference %.6f"
          % (algo, sync_host, F_beam, F_none, F_beam - F_none, want))
    assert abs((F_beam - F_none) - want) <= 1e-9 * max(1.0, abs(want))
    model.seed_resident_states(dict(p.theta), my_data, *EA, max_active=p.A, beam=4)
    assert model.last_seed_path is None
    with pytest.raises(ValueError, match="beam = 9"):  # > S // A = 8
        model.seed_resident_states(dict(p.theta), my_data, *EA, max_active=p.A, beam=9)

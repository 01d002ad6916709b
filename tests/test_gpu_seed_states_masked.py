"""K^n seeded on the GPU from incomplete data: Engine.seed_states(incomplete=True) (csrc/kernels_seed.hpp:
seed_states_masked_kernel) and Model.seed_resident_states(incomplete=True).

1. kernel against its NumPy mirror (seed_states_host with x_infr) under the rule of tests/test_gpu_seed_states.py: a datapoint
   is decided when the mirror's margin exceeds 1e-7 -- equal states and path; an undecided one is compared up to the first
   near-tie; at most 2 % may be undecided (tests/test_seed_states_masked_host.py holds the committed seeds to 1e-6, so none
   is); lpj_path to 1e-9; the packed download equals np.packbits of the bool download;
2. lpj_path against lpj_resident() at the winners' slots (the masked lpj kernels), 1e-9 relative; winners lead their step;
3. the digests: the same lpj bits after a round trip of the packed states;
4. all-True masks go through the masked kernel: against the complete kernel on a second engine;
5. a row without any reliable entry and a row with exactly one;
6. two calls give the same bits; rows of the old K^n are refused after a seed call;
7. refusals leave K^n untouched;
8. the model method, both models, device-resident and host-synchronised.
"""
import numpy as np
import pytest

from _seed_masked_problems import ALGOS, all_problems, make_mask, problem
from _seed_problems import make_data, make_theta, quotas
from evo_amd._lib import EvoAmdError
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC

pytestmark = pytest.mark.gpu

ALLZERO = {"background": False, "allzero": True, "singletons": False}
LPJ_RTOL = 1e-9


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


def _install(eng, p, x_infr="own"):
    """Data with NaN under the mask's False entries, the masks, Theta."""
    eng.configure("bsc" if p.algo == "ebsc" else "sssc", p.N, p.D, p.H, p.S, p.S_perm, 4)
    eng.upload_data(p.Y)
    eng.upload_masks(p.x_infr if isinstance(x_infr, str) else x_infr)
    eng.set_reliable_fraction(p.x_infr.sum() / float(p.N))  # (enters ljc alone, which no score holds)
    _set_params(eng, p.algo, p.theta)


def _compare(p, got, path, lpj_path, rows=None):
    """The rule of test_kernel_equals_mirror over the datapoints ``rows`` (default: all)."""
    rows = np.arange(p.N) if rows is None else np.asarray(rows)
    decided = p.margin[rows] > 1e-7
    assert (~decided).mean() <= 0.02
    bad = [n for n in rows[decided] if not (np.array_equal(got[n], p.states[n]) and np.array_equal(path[n], p.path[n]))]
    assert not bad, "decided datapoints that differ: %s" % bad[:8]
    assert np.allclose(lpj_path[rows[decided]], p.lpj_path[rows[decided]], rtol=LPJ_RTOL, atol=LPJ_RTOL)
    q = quotas(p.S, p.A)
    for n in rows[~decided]:
        diff = np.nonzero(path[n] != p.path[n])[0]
        t = int(diff[0]) if len(diff) else p.A  # steps before t: the same active set, hence the same candidates
        assert np.array_equal(path[n, :t], p.path[n, :t])
        if t < p.A:  # they part at a near-tie
            assert abs(lpj_path[n, t] - p.lpj_path[n, t]) <= 1e-7 * max(1.0, abs(p.lpj_path[n, t]))
        for u in range(t):  # the slots of the steps before: the same sets of states
            lo = sum(q[:u])
            a = {r.tobytes() for r in got[n, lo:lo + q[u]]}
            assert len(a) == q[u] and all(r[p.path[n, :u]].all() for r in got[n, lo:lo + q[u]])


def _empty_ebsc_row(p, got, path, lpj_path, n=0):
    """A row without a reliable entry, EBSC: every score of a step is the same number, so the slots fill in ascending j."""
    assert np.array_equal(path[n], np.arange(p.A))
    slot = 0
    for t, qt in enumerate(quotas(p.S, p.A), start=1):
        want = np.zeros((qt, p.H), dtype=bool)
        want[:, :t - 1] = True
        want[np.arange(qt), t - 1 + np.arange(qt)] = True
        assert np.array_equal(got[n, slot:slot + qt], want)
        slot += qt
    assert np.allclose(lpj_path[n], p.lpj_path[n], rtol=LPJ_RTOL)


@pytest.mark.parametrize("algo,name,missing", all_problems())
def test_kernel_equals_mirror(eng, algo, name, missing):
    p = problem(algo, name, missing)
    _install(eng, p)
    path, lpj_path = eng.seed_states(p.A, want_path=True, incomplete=True)
    got = eng.download_states()
    packed = eng.download_states_packed()
    assert got.shape == p.states.shape and path.shape == p.path.shape and path.dtype == np.int32
    assert np.array_equal(packed, np.packbits(got, axis=-1))  # the packed download sees the same words
    rows = None
    if name == "empty_row" and algo == "ebsc":  # (its margin is 0: exact ties, decided by the tie rule)
        _empty_ebsc_row(p, got, path, lpj_path)
        rows = np.arange(1, p.N)
    print("%s %s %.1f: smallest margin of the mirror %.3g" % (algo, name, missing, p.margin[1:].min() if rows is not None
                                                               else p.margin.min()))
    _compare(p, got, path, lpj_path, rows)


@pytest.mark.parametrize("algo,name,missing", [("ebsc", "ragged", 0.3), ("es3c", "ragged", 0.6), ("es3c", "ragged_perm", 0.3),
                                               ("ebsc", "s200", 0.6), ("es3c", "s200", 0.3), ("es3c", "d130", 0.6),
                                               ("ebsc", "wide_d", 0.3), ("es3c", "rows_gmem", 0.3)])
def test_lpj_out_equals_lpj_resident(eng, algo, name, missing):
    p = problem(algo, name, missing)
    _install(eng, p)
    path, lpj_path = eng.seed_states(p.A, want_path=True, incomplete=True)
    eng.lpj_resident()
    lpj = eng.download_lpj()
    assert lpj.shape == (p.N, p.S_perm + p.S) and np.isfinite(lpj).all()  # no clamp fired
    slots = p.S_perm + np.concatenate(([0], np.cumsum(quotas(p.S, p.A))[:-1]))
    want = lpj[:, slots]
    err = np.abs(lpj_path - want) / np.maximum(1.0, np.abs(want))
    print("%s %s %.1f: largest relative difference %.3g" % (algo, name, missing, err.max()))
    assert err.max() <= LPJ_RTOL
    for t, (lo, q) in enumerate(zip(slots, quotas(p.S, p.A))):  # a winner has the largest lpj of its step
        assert (lpj[:, lo:lo + q].max(axis=1) <= lpj[:, lo] + 1e-9 * np.abs(lpj[:, lo])).all(), t


@pytest.mark.parametrize("algo,name,missing", [("es3c", "ragged", 0.3), ("ebsc", "s200", 0.6), ("ebsc", "large_h", 0.3)])
def test_digests_equal_digest_kernel(eng, algo, name, missing):
    p = problem(algo, name, missing)
    _install(eng, p)
    eng.seed_states(p.A, incomplete=True)
    eng.lpj_resident()
    before = eng.download_lpj()
    packed = eng.download_states_packed()
    eng.upload_states_packed(packed)
    eng.lpj_resident()
    after = eng.download_lpj()
    assert np.isfinite(before).all()
    assert np.array_equal(before, after)


@pytest.mark.parametrize("algo,name", [("ebsc", "ragged"), ("es3c", "ragged_perm"), ("es3c", "s200"), ("ebsc", "wide_d"),
                                       ("es3c", "d130")])
def test_all_true_masks_equal_the_complete_kernel(eng, eng2, algo, name):
    p = problem(algo, name, 0.3)
    Y = np.where(p.x_infr, p.Y, 0.5)  # complete data for both
    full = np.ones((p.N, p.D), dtype=bool)
    for e, masks in ((eng, True), (eng2, False)):
        e.configure("bsc" if algo == "ebsc" else "sssc", p.N, p.D, p.H, p.S, p.S_perm, 4)
        e.upload_data(Y)
        if masks:
            e.upload_masks(full)
        _set_params(e, algo, p.theta)
    path_m, lpj_m = eng.seed_states(p.A, want_path=True, incomplete=True)
    path_c, lpj_c = eng2.seed_states(p.A, want_path=True, incomplete=True)  # no masks: the flag changes nothing
    from evo_amd.variational import seed_states_host
    margin = seed_states_host("bsc" if algo == "ebsc" else "sssc", p.theta, Y, p.S, p.A, p.S_perm)[3]
    decided = margin > 1e-7
    assert (~decided).mean() <= 0.02
    assert np.array_equal(path_m[decided], path_c[decided])
    assert np.array_equal(eng.download_states()[decided], eng2.download_states()[decided])
    assert np.allclose(lpj_m[decided], lpj_c[decided], rtol=LPJ_RTOL, atol=LPJ_RTOL)


@pytest.mark.parametrize("algo", ALGOS)
def test_two_calls_same_bits_and_no_stale_rows(eng, algo):
    p = problem(algo, "ragged_perm", 0.6)
    _install(eng, p)
    eng.init_states(1.0 / p.H, 5)
    eng.lpj_resident()
    noise = eng.download_lpj()
    first = eng.seed_states(p.A, want_path=True, incomplete=True)
    eng.lpj_resident()
    seeded = eng.download_lpj()
    packed = eng.download_states_packed()
    assert not np.array_equal(noise, seeded)
    second = eng.seed_states(p.A, want_path=True, incomplete=True)
    assert np.array_equal(eng.download_states_packed(), packed)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    # the statistics rows of the old K^n are gone too: the codes are refused until a new pass has run
    eng.lpj_resident()
    eng.set_option("reconstruct_in_stats", 1)
    eng.stats()
    eng.posterior_codes(4)
    eng.seed_states(p.A, incomplete=True)
    with pytest.raises(EvoAmdError):
        eng.posterior_codes(4)


@pytest.mark.parametrize("algo", ALGOS)
def test_b_from_transposed_data_is_masked(eng, algo):
    """Large shapes form B = Y W from a transposed copy of Y (option b_transposed; 2 admits it from N = 8192, H = 128,
    D = 32): that copy has to carry the zeros of the missing entries too, or the NaN under them reach every score."""
    N, D, H, S, A = 8192, 32, 128, 6, 3
    rng = np.random.RandomState(41 if algo == "ebsc" else 42)
    theta = make_theta(rng, algo, D, H)
    Y, _ = make_data(rng, algo, theta, N)
    xi = make_mask(rng, N, D, 0.5)
    eng.set_option("b_transposed", 2)
    try:
        eng.configure("bsc" if algo == "ebsc" else "sssc", N, D, H, S, 0, 4)
        eng.upload_data(np.where(xi, Y, np.nan))
        eng.upload_masks(xi)
        eng.set_reliable_fraction(xi.sum() / float(N))
        _set_params(eng, algo, theta)
        path, lpj_path = eng.seed_states(A, want_path=True, incomplete=True)
        eng.lpj_resident()
        lpj = eng.download_lpj()
    finally:
        eng.set_option("b_transposed", 1)
        eng.configure("bsc", 4, 4, 8, 4, 0, 4)  # (the option is read by configure)
    slots = np.concatenate(([0], np.cumsum(quotas(S, A))[:-1]))
    assert np.isfinite(lpj_path).all() and np.isfinite(lpj).all()
    err = np.abs(lpj_path - lpj[:, slots]) / np.maximum(1.0, np.abs(lpj[:, slots]))
    print("%s: largest relative difference %.3g" % (algo, err.max()))
    assert err.max() <= LPJ_RTOL


def test_refusals_leave_kn_alone(eng):
    def refused(match, A, incomplete=True):
        before = eng.download_states_packed()
        with pytest.raises(EvoAmdError, match=match):
            eng.seed_states(A, want_path=True, incomplete=incomplete)
        assert np.array_equal(eng.download_states_packed(), before)
        eng.lpj_resident()  # K^n still counts as present

    for algo in ALGOS:
        q = problem(algo, "tight", 0.3)
        _install(eng, q)
        eng.init_states(0.3, 9)
        refused("incomplete data", q.A, incomplete=False)  # masks present and no permission: the old message
        refused("max_active = 0", 0)
        refused("max_active = 21", 21)
        refused("quota q_1 = 10", 2)
        eng.set_option("background_unit", 1)
        try:
            refused("background_unit", q.A)
        finally:
            eng.set_option("background_unit", 0)
        eng.seed_states(q.A, incomplete=True)  # admitted
    q = problem("ebsc", "tight", 0.3)
    _install(eng, q)
    eng.init_states(0.3, 9)
    eng.set_option("bsc_direct", 1)
    try:
        _set_params(eng, "ebsc", q.theta)
        refused("bsc_direct", q.A)
    finally:
        eng.set_option("bsc_direct", 0)
    # the float32 mode (it admits no masks at all: the flag alone must not open it)
    eng.set_option("ebsc_f32", 1)
    try:
        eng.configure("bsc", q.N, q.D, q.H, q.S, 0, 4)
        eng.upload_data(np.where(q.x_infr, q.Y, 0.0))
        _set_params(eng, "ebsc", q.theta)
        eng.init_states(0.3, 9)
        refused("float32", q.A)
    finally:
        eng.set_option("ebsc_f32", 0)
        _install(eng, q)


def _model_problem(algo):
    N, D, H, S = 64, 36, 48, 30
    rng = np.random.RandomState(27 if algo == "ebsc" else 28)
    theta = make_theta(rng, algo, D, H)  # pi H = 3
    Y, _ = make_data(rng, algo, theta, N)
    xi = make_mask(rng, N, D, 0.4)
    return N, D, H, S, theta, Y, {"y": np.where(xi, Y, np.nan), "x_infr": xi, "x": xi.copy()}


def _lse(lpj):
    m = lpj.max(axis=1, keepdims=True)
    return float((m[:, 0] + np.log(np.exp(lpj - m).sum(axis=1))).mean())


@pytest.mark.parametrize("sync_host", [False, True])
@pytest.mark.parametrize("algo,permanent", [("ebsc", None), ("es3c", ALLZERO)])
def test_model_seed_resident_states(model_eng, algo, permanent, sync_host):
    eng = model_eng
    N, D, H, S, theta, Y_full, my_data = _model_problem(algo)
    xi = my_data["x_infr"]
    cls = BSC if algo == "ebsc" else SSSC
    kw = dict(engine=eng, rng="device", sync_host=sync_host, seed=1)
    ea = ("fit", "randflip", 6, 1, 1)
    S_perm = 1 if permanent else 0
    # ---- from noise, on the same data
    other = cls(D, H, S, **kw)
    noise = other.init_resident_states(my_data, *ea, permanent=permanent, seed=3)
    other.E_step_precompute(dict(theta), dict(noise), my_data)
    eng.lpj_resident()
    lpj_noise = eng.download_lpj()
    if sync_host:
        noise["lpj"] = lpj_noise
    mean_noise = other.predictive_moments(dict(theta), noise, my_data)[0]
    # ---- seeded
    model = cls(D, H, S, **kw)
    suff = model.seed_resident_states(dict(theta), my_data, *ea, permanent=permanent, want_path=True, incomplete=True)
    assert set(suff) == set(noise)  # init_states' keys
    A = min(8, S, H)
    path, lpj_path = model.last_seed_path
    assert path.shape == (N, A) and lpj_path.shape == (N, A)
    if sync_host:
        assert suff["ss"].shape == (N, S, H) and suff["ss"].dtype == np.bool_
        assert suff["lpj"].shape == (N, S + S_perm) and suff["lpj"].dtype == np.float64
        ss, lpj = suff["ss"], suff["lpj"]
    else:
        assert suff["ss"] is None and suff["lpj"] is None
        ss, lpj = eng.download_states(), eng.download_lpj()
    assert suff["S_perm"] == S_perm
    for n in range(N):
        assert len({r.tobytes() for r in ss[n]}) == S
    # without any E-step: predictive moments and draws
    th = dict(theta)
    mean, var, info = model.predictive_moments(th, suff, my_data)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    draws = model.sample_posterior(th, suff, my_data, n_samples=2, fill="missing", seed=5)
    assert draws["y"].shape == (N, 2, D)
    rel = np.broadcast_to(xi[:, None, :], draws["y"].shape)
    assert np.array_equal(draws["y"][rel], np.broadcast_to(Y_full[:, None, :], draws["y"].shape)[rel])
    assert np.isfinite(draws["y"]).all()
    lse_seed, lse_noise = _lse(lpj), _lse(lpj_noise)
    mse_seed = float(np.nanmean(np.where(xi, np.nan, (mean - Y_full) ** 2)))
    mse_noise = float(np.nanmean(np.where(xi, np.nan, (mean_noise - Y_full) ** 2)))
    print("%s sync_host=%s: mean logsumexp lpj seeded %.4f, from noise %.4f; mse on the missing entries seeded %.5f, from "
          "noise %.5f" % (algo, sync_host, lse_seed, lse_noise, mse_seed, mse_noise))
    assert lse_seed > lse_noise
    assert mse_seed < mse_noise
    # EM follows as usual.  On incomplete data the statistics pass of an E-step reads y_reconstructed (ES3C refuses to run
    # without forming it in the same pass): the E-step is the one step(do_reconstruction=True) runs, which forms it first.
    F_seed = model.E_step(th, suff, my_data, _reconstruct=True)[0]
    assert np.isfinite(F_seed)
    F = model.step(th, suff, my_data, do_reconstruction=True)[0]
    assert np.isfinite(F)
    if algo == "ebsc":  # ... and a plain E_step reads the y_reconstructed that step left in my_data
        assert np.isfinite(model.E_step(th, suff, my_data)[0])

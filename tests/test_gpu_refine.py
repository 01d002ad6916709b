"""K^n refined at fixed Theta on the GPU (Engine.refine_states / Model.refine_resident_states, csrc/kernels_refine.hpp) and
the per-datapoint scores (Engine.posterior_scores / Model.posterior_scores).

1. the loop is the composition of the stages it is made of, bit for bit: lpj_resident, then per iteration evolve_randflip /
   evolve_states with seed0 + t stride, vary_kn -- K^n, lpj and the counts equal, Fs against the log-sum-exp of the rows;
2. one iteration is one E_step; 3. the rows it leaves are not stale, F never decreases; 4. a statistics pass, encode and the
   scores that follow see the new K^n; 5. early stop; 6. the score kernel against its NumPy mirror; 7. F_n against the exact
   log-likelihood per datapoint; 8. sync_host=False.
"""
import functools
import itertools

import numpy as np
import pytest

import _refine_problems as rp
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import posterior_scores_host

pytestmark = pytest.mark.gpu

LPJ_RTOL = 1e-9
SUM_RTOL = 1e-9  # (the constants of test_gpu_estep_paths.py)
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
    """The Model tests' own engine: Model._prepare keeps per-engine state that the engine-level tests do not maintain."""
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _problem(name):
    return rp.compose_problem(name)


class _installed:
    """The options of a problem set for the block, Theta / data / masks installed on entry, the options back on exit."""

    def __init__(self, eng, p):
        self.eng, self.p = eng, p

    def __enter__(self):
        eng, p = self.eng, self.p
        eng.set_option("state_digest", 0 if "digest0" in p.extras else 1)
        eng.set_option("ebsc_f32", 1 if "f32" in p.extras else 0)
        eng.set_option("background_unit", 1 if "bg" in p.extras else 0)
        eng.configure(p.model, p.N, p.D, p.H, p.S, p.S_perm, p.Cmax)
        eng.upload_data(p.Y)
        if p.x_infr is not None:  # (configure dropped the masks of the geometry before)
            eng.upload_masks(p.x_infr)
        eng.set_reliable_fraction(None if p.x_infr is None else p.x_infr.sum() / float(p.N))
        th = p.theta
        if p.model == "sssc":
            eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
        else:
            eng.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))
        return eng

    def __exit__(self, *exc):
        eng = self.eng
        eng.set_option("state_digest", 1)
        eng.set_option("ebsc_f32", 0)
        eng.set_option("background_unit", 0)  # (every test configures its own geometry: the defaults hold from there)
        return False


def _ea(p):
    return dict(mutation=p.mutation, n_parents=p.n_parents, n_children=p.n_children, n_generations=p.n_generations,
                sparseness=p.sparseness, bitflip_prob=p.bitflip_prob)


def _refine(eng, p, T, **kw):
    eng.upload_states(p.ss)
    trace, n_done = eng.refine_states(T, seed0=rp.SEED0, seed_stride=p.seed_stride, fit_parents=True, **_ea(p), **kw)
    assert trace.shape == (n_done, 3)
    return trace, n_done, eng.download_states(), eng.download_lpj()


def _separate(eng, p, T):
    """The same start through the calls the loop is made of; (sums (T, 2), lpj after every iteration, K^n, lpj)."""
    eng.upload_states(p.ss)
    eng.lpj_resident()
    sums, rows = [], []
    for t in range(T):
        seed = rp.SEED0 + t * p.seed_stride
        if p.mutation == "randflip" and p.n_generations == 1 and p.n_children <= 8:
            eng.evolve_randflip(p.n_parents, p.n_children, seed, True)
        else:
            eng.evolve_states(p.mutation, p.n_parents, p.n_children, p.n_generations, seed, True, p.sparseness, p.bitflip_prob)
        eng.set_estep_counts(0.0, 0.0)
        sums.append(eng.vary_kn(p.S))
        rows.append(eng.download_lpj())
    return np.array(sums), rows, eng.download_states(), eng.download_lpj()


@pytest.mark.parametrize("name", list(rp.COMPOSE))
def test_loop_is_the_composition_of_its_stages(eng, name):
    p = _problem(name)
    T = 5
    with _installed(eng, p):
        trace, n_done, ss_a, lpj_a = _refine(eng, p, T)
        sums, rows, ss_b, lpj_b = _separate(eng, p, T)
    assert n_done == T
    assert np.array_equal(ss_a, ss_b), "%s: K^n differs in datapoints %s" % (
        name, np.flatnonzero((ss_a != ss_b).any(axis=(1, 2))))
    assert np.array_equal(lpj_a, lpj_b), name
    assert np.array_equal(trace[:, 1:], sums), (name, trace[:, 1:], sums)
    assert (trace[:, 2] > 0).any(), name + ": no iteration swapped a state"
    assert not np.array_equal(ss_a, p.ss), name
    for t in range(T):
        want = rp.logsumexp_rows(rows[t]).sum()
        print("%s t=%d: Fs %.12g, rows %.12g" % (name, t, trace[t, 0], want))
        assert abs(trace[t, 0] - want) <= SUM_RTOL * max(1.0, abs(want)), (name, t, trace[t, 0], want)
    if "bg" in p.extras:
        assert ss_a[:, :, -1].all()


def _model_problem(algo, permanent=None, N=29, D=10, H=24, S=20, seed=3):
    rng = np.random.RandomState(seed + (0 if algo == "ebsc" else 1))
    theta = rp.bsc_theta(rng, D, H) if algo == "ebsc" else rp.es3c_theta(rng, D, H)
    Y = rng.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    return theta, my_data, rp.kn_nonzero(rng, N, S, H, kmax=4)


def _suff(ss, ea=("fit", "randflip", 4, 2, 1), permanent=None):
    """my_suff_stat around a given K^n: every key but the two arrays from init_states (no datapoint: nothing is drawn)."""
    from evo_amd.variational import init_states
    N, S, H = ss.shape
    suff = init_states(0, S, H, *ea, permanent=permanent)
    suff["ss"] = ss.copy()
    suff["lpj"] = np.zeros((N, S + suff["S_perm"]))
    return suff


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_one_iteration_is_one_estep(model_eng, algo):
    cls = BSC if algo == "ebsc" else SSSC
    theta, my_data, ss = _model_problem(algo)
    D, (N, S, H) = my_data["y"].shape[1], ss.shape
    a = cls(D, H, S, engine=model_eng, rng="device", sync_host=True, seed=7)
    b = cls(D, H, S, engine=model_eng, rng="device", sync_host=True, seed=7)
    suff_a, suff_b = _suff(ss), _suff(ss)
    res = a.refine_resident_states(dict(theta), suff_a, my_data, 1)
    F, nu, sub = b.E_step(dict(theta), suff_b, my_data)
    assert res.n_done == 1 and not res.stopped_early and res.F.shape == (1,)
    assert np.array_equal(suff_a["ss"], suff_b["ss"])
    assert not np.array_equal(suff_a["ss"], ss)
    for got, want in ((res.F[0], F), (res.S_nunique[0], nu), (res.S_sub[0], sub)):
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    np.testing.assert_allclose(suff_a["lpj"], suff_b["lpj"], rtol=LPJ_RTOL)
    assert a._n_steps == 1 and b._n_steps == 1


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_rows_are_not_stale(model_eng, algo):
    cls = BSC if algo == "ebsc" else SSSC
    theta, my_data, ss = _model_problem(algo)
    D, (N, S, H) = my_data["y"].shape[1], ss.shape
    model = cls(D, H, S, engine=model_eng, rng="device", sync_host=True, seed=2)
    suff = _suff(ss)
    res = model.refine_resident_states(dict(theta), suff, my_data, 6)
    assert res.n_done == 6 and model._n_steps == 6
    kept = model_eng.download_lpj()
    assert np.array_equal(kept, suff["lpj"])
    model_eng.lpj_resident()
    fresh = model_eng.download_lpj()
    err = np.abs(kept - fresh) / np.maximum(1.0, np.abs(fresh))
    print("%s: rows kept by the loop against a fresh pass: %.3g" % (algo, err.max()))
    assert err.max() <= LPJ_RTOL
    th = dict(theta)
    F = model.free_energy(my_data, th, suff, full=False, compute_lpj=True)
    assert abs(res.F[-1] - F) <= 1e-9 * abs(F), (res.F[-1], F)
    drops = res.F[:-1] - res.F[1:]
    assert (drops <= 1e-9 * np.abs(res.F[:-1])).all(), res.F
    assert res.F[-1] > res.F[0]
    assert (res.S_sub > 0).any()


@pytest.mark.parametrize("name", ["ebsc_n37", "es3c_perm"])
def test_statistics_pass_sees_the_new_kn(eng, eng2, name):
    p = _problem(name)
    with _installed(eng, p), _installed(eng2, p):
        trace, n_done, ss, lpj = _refine(eng, p, 3)
        acc = eng.stats()
        eng2.upload_states(ss)
        eng2.upload_lpj(lpj)
        acc2 = eng2.stats()
        va, vb = eng.acc_views(acc), eng2.acc_views(acc2)
    assert float(va["sum_nunique"]) == trace[-1, 1] and float(va["sum_sub"]) == trace[-1, 2], (name, trace[-1])
    assert float(va["N"]) == float(vb["N"]) == p.N
    for k in va:
        if k in ("sum_nunique", "sum_sub"):
            continue
        scale = max(1.0, float(np.abs(vb[k]).max()))
        assert np.abs(va[k] - vb[k]).max() <= 1e-12 * scale, (name, k)
    assert abs(float(va["Fs"]) - trace[-1, 0]) <= 1e-12 * max(1.0, abs(trace[-1, 0]))


@pytest.mark.parametrize("algo,permanent", [("ebsc", None), ("es3c", ALLZERO)])
def test_encode_names_the_best_state(model_eng, algo, permanent):
    cls = BSC if algo == "ebsc" else SSSC
    theta, my_data, ss = _model_problem(algo)
    D, (N, S, H) = my_data["y"].shape[1], ss.shape
    model = cls(D, H, S, engine=model_eng, rng="device", sync_host=True, seed=4)
    suff = _suff(ss, permanent=permanent)
    S_perm = suff["S_perm"]
    model.refine_resident_states(dict(theta), suff, my_data, 4)
    scores = model.posterior_scores(dict(theta), suff, my_data)
    codes = model.encode(dict(theta), suff, my_data, max_active=8)
    assert np.array_equal(codes.map_slot, scores["best"])
    full = np.concatenate((np.zeros((N, S_perm, H), dtype=bool), suff["ss"]), axis=1)
    assert np.array_equal(codes.map_states(), full[np.arange(N), scores["best"]])
    assert np.array_equal(scores["k_best"], codes.map_states().sum(axis=1))
    assert np.array_equal(scores["best"], suff["lpj"].argmax(axis=1))
    np.testing.assert_allclose(scores["n_eff"], np.exp(scores["entropy"]))


def test_early_stop(eng, model_eng):
    # every non-zero state of H = 4 is in K^n and the all-zero one is permanent: every child is a duplicate
    N, D, H, S = 9, 6, 4, 15
    rng = np.random.RandomState(8)
    table = np.array([s for s in itertools.product([False, True], repeat=H)][1:])
    ss = np.stack([table[rng.permutation(S)] for _ in range(N)])
    theta = rp.bsc_theta(rng, D, H)
    my_data = {"y": rng.normal(size=(N, D)), "x_infr": np.ones((N, D), dtype=bool)}
    model = BSC(D, H, S, engine=model_eng, rng="device", sync_host=True, seed=1)
    suff = _suff(ss, ea=("fit", "randflip", 3, 2, 1), permanent=ALLZERO)
    res = model.refine_resident_states(dict(theta), suff, my_data, 10, check_every=2, patience=2)
    assert res.n_done == 2 and res.n_done_local == 2 and res.stopped_early
    assert res.F.shape == (2,) and (res.S_nunique == 0).all() and (res.S_sub == 0).all()
    assert np.array_equal(suff["ss"], ss)
    assert model._n_steps == 10
    res = model.refine_resident_states(dict(theta), suff, my_data, 10, patience=None)
    assert res.n_done == 10 and not res.stopped_early and np.array_equal(suff["ss"], ss)
    assert (res.F == res.F[0]).all()
    # a problem that does move: whatever the stop, the result is that of a plain call of n_done iterations.  min_sub = 0
    # may not stop within 40 iterations; min_sub = 4 swaps per datapoint does
    p = _problem("ebsc_n37")
    for min_sub in (0.0, 4.0):
        with _installed(eng, p):
            trace, n_done, ss_a, lpj_a = _refine(eng, p, 40, check_every=2, patience=2, min_sub=min_sub)
            assert 2 <= n_done <= 40 and n_done % 2 == 0
            plain, n_plain, ss_b, lpj_b = _refine(eng, p, n_done)
            va = eng.acc_views(eng.stats())
        print("ebsc_n37 min_sub=%g: stopped after %d iterations, swaps %s" % (min_sub, n_done, trace[:, 2]))
        assert n_plain == n_done
        assert np.array_equal(trace, plain) and np.array_equal(ss_a, ss_b) and np.array_equal(lpj_a, lpj_b)
        quiet = trace[:, 2] / p.N <= min_sub
        if n_done < 40:  # the last two rows are quiet, no pair at an earlier boundary was
            assert quiet[-2:].all() and not quiet[:-2].reshape(-1, 2).all(axis=1).any()
        assert float(va["sum_sub"]) == plain[-1, 2]
    assert n_done < 40  # (min_sub = 4: 148 swaps over the 37 datapoints)


@pytest.mark.parametrize("H", [64, 130])
@pytest.mark.parametrize("S,S_perm", [(4, 0), (65, 1), (200, 0), (1024, 0)])
def test_scores_equal_the_mirror(eng, S, S_perm, H):
    N, D = 7, 4
    rng = np.random.RandomState(S + H)
    if S == 4:  # distinct states of a few latents; at H = 130 with latents in all three words
        ss = rp.kn_nonzero(rng, N, S, H, kmax=3)
    else:
        ss = rp.kn_nonzero(rng, N, S, H, kmax=9)
    ss[:, 0, :] = False
    ss[:, 0, [0, 63 if H == 64 else 64, H - 1]] = True  # word boundaries
    if S >= 65:
        ss[1, 1, :] = True  # every latent on: more than a digest counts at H = 130 ... and k_mean up to H
    lpj = rp.score_rows(rng, N, S + S_perm)  # ties for the maximum and a spread above 800 among its rows
    eng.configure("bsc", N, D, H, S, S_perm, 4)
    eng.upload_states(ss)
    eng.upload_lpj(lpj)
    got = eng.posterior_scores()
    again = eng.posterior_scores()
    assert np.array_equal(eng.download_lpj(), lpj) and np.array_equal(eng.download_states(), ss)
    want = posterior_scores_host(lpj, ss, S_perm)
    for k in ("F", "entropy"):
        err = np.abs(got[k] - want[k]) / np.maximum(1.0, np.abs(want[k]))
        print("S=%d H=%d %s: largest error %.3g" % (S, H, k, err.max()))
        assert np.isfinite(got[k]).all() and err.max() <= 1e-11, k
    err = np.abs(got["k_mean"] - want["k_mean"]).max()
    print("S=%d H=%d k_mean: largest error %.3g" % (S, H, err))
    assert err <= 1e-11 * H
    assert got["best"].dtype == np.int32 and np.array_equal(got["best"], want["best"])
    assert np.array_equal(got["k_best"], want["k_best"])
    ties = np.flatnonzero(lpj[1] == lpj[1].max())
    assert ties.size == 2 and got["best"][1] == ties[0]
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    part = eng.posterior_scores(what=("entropy", "k_best"))
    assert set(part) == {"entropy", "k_best"}
    assert np.array_equal(part["entropy"], got["entropy"]) and np.array_equal(part["k_best"], got["k_best"])
    with pytest.raises(ValueError):
        eng.posterior_scores(what=("F", "q"))


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_scores_against_the_exact_likelihood(model_eng, algo):
    cls = BSC if algo == "ebsc" else SSSC
    N, D, H, S = 20, 8, 10, 30
    rng = np.random.RandomState(21 if algo == "ebsc" else 22)
    theta = rp.bsc_theta(rng, D, H) if algo == "ebsc" else rp.es3c_theta(rng, D, H)
    my_data = {"y": rng.normal(size=(N, D)), "x_infr": np.ones((N, D), dtype=bool)}
    ss = rp.kn_nonzero(rng, N, S, H, kmax=3)
    model = cls(D, H, S, engine=model_eng, rng="device", sync_host=True, seed=5)
    suff = _suff(ss, permanent=ALLZERO)
    _, ll, _ = model.exact_log_likelihood(my_data, dict(theta), suff, per_datapoint=True)
    model.free_energy(my_data, dict(theta), suff, full=False, compute_lpj=True)  # (the rows of the start, on the device)
    suff["lpj"] = model_eng.download_lpj()
    before = model.posterior_scores(dict(theta), suff, my_data)["F"]
    model.refine_resident_states(dict(theta), suff, my_data, 20)
    after = model.posterior_scores(dict(theta), suff, my_data)["F"]
    for F in (before, after):
        assert (ll >= F - 1e-9 * np.maximum(1.0, np.abs(ll))).all(), (ll - F).min()
    print("%s: mean(ll - F) before %.6g, after 20 iterations %.6g" % (algo, (ll - before).mean(), (ll - after).mean()))
    assert (ll - after).mean() <= (ll - before).mean()
    # K^n = every non-zero state, the all-zero one permanent: the bound is the likelihood
    H6 = 6
    theta6 = rp.bsc_theta(rng, D, H6) if algo == "ebsc" else rp.es3c_theta(rng, D, H6)
    table = np.array([s for s in itertools.product([False, True], repeat=H6)][1:])
    full = cls(D, H6, 2 ** H6 - 1, engine=model_eng, rng="device", sync_host=True, seed=5)
    suff6 = _suff(np.stack([table] * N), permanent=ALLZERO)
    _, ll6, _ = full.exact_log_likelihood(my_data, dict(theta6), suff6, per_datapoint=True)
    full.free_energy(my_data, dict(theta6), suff6, full=False, compute_lpj=True)
    suff6["lpj"] = model_eng.download_lpj()
    F6 = full.posterior_scores(dict(theta6), suff6, my_data)["F"]
    np.testing.assert_allclose(F6, ll6, rtol=1e-9)


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_device_resident_refinement(model_eng, eng2, algo):
    cls = BSC if algo == "ebsc" else SSSC
    theta, my_data, ss = _model_problem(algo)
    D, (N, S, H) = my_data["y"].shape[1], ss.shape
    res_model = cls(D, H, S, engine=model_eng, rng="device", sync_host=False, seed=9)
    suff = _suff(ss)
    packed = np.packbits(ss, axis=-1)
    suff["ss"] = suff["lpj"] = None
    res_model.attach_resident_states(suff, my_data, [(0, packed)])
    res = res_model.refine_resident_states(dict(theta), suff, my_data, 5)
    scores = res_model.posterior_scores(dict(theta), suff, my_data)
    assert suff["ss"] is None and suff["lpj"] is None
    assert res.n_done == 5 and np.isfinite(scores["F"]).all()
    ljc = res_model.engine.ljc
    assert abs(ljc + scores["F"].mean() - res.F[-1]) <= 1e-9 * abs(res.F[-1])
    res_model.sync_to_host(suff)
    twin = cls(D, H, S, engine=eng2, rng="device", sync_host=True, seed=9)
    suff_t = _suff(ss)
    res_t = twin.refine_resident_states(dict(theta), suff_t, my_data, 5)
    assert np.array_equal(suff["ss"], suff_t["ss"]) and np.array_equal(suff["lpj"], suff_t["lpj"])
    assert np.array_equal(res.F, res_t.F) and np.array_equal(res.S_sub, res_t.S_sub)

"""K^n seeded on the GPU: Engine.seed_states (csrc/kernels_seed.hpp) and Model.seed_resident_states.

1. kernel against its NumPy mirror (evo_amd.variational.seed_states_host): K^n, the packed download and the path.  A
   datapoint is decided when the mirror's margin exceeds 1e-7: its states and path must be equal; an undecided one is
   compared up to the first step at which the two part, where the two scores must be a near-tie; at most 2 % may be
   undecided (tests/test_seed_states_host.py holds the committed seeds to a margin of 1e-6, so none is);
2. lpj_out against lpj_resident() at the winners' slots, 1e-9 relative;
3. the digests the kernel writes against digest_kernel's (same lpj bits before and after a re-upload of the same rows);
4. no stale rows or prefetched pass after a seed call; two seed calls give the same K^n;
5. every refusal leaves K^n as it was;
6. Model.seed_resident_states for both models, device-resident and host-synchronised;
7. evoamd_seed_states and evoamd_seed_states_ex without a flag give the same bits.
"""
import numpy as np
import pytest

from _seed_problems import ALGOS, CASES, make_data, make_theta, problem, quotas
from evo_amd._lib import EvoAmdError, check, dptr, i32ptr
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


def _install(eng, p):
    eng.configure("bsc" if p.algo == "ebsc" else "sssc", p.N, p.D, p.H, p.S, p.S_perm, 4)
    eng.upload_data(p.Y)
    _set_params(eng, p.algo, p.theta)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("algo", ALGOS)
def test_kernel_equals_mirror(eng, algo, name):
    p = problem(algo, name)
    _install(eng, p)
    path, lpj_path = eng.seed_states(p.A, want_path=True)
    got = eng.download_states()
    packed = eng.download_states_packed()
    assert got.shape == p.states.shape and path.shape == p.path.shape and path.dtype == np.int32
    assert np.array_equal(packed, np.packbits(got, axis=-1))  # the packed download sees the same words
    print("%s %s: smallest margin of the mirror %.3g" % (algo, name, p.margin.min()))
    decided = p.margin > 1e-7
    assert (~decided).mean() <= 0.02
    bad = [n for n in np.nonzero(decided)[0] if not (np.array_equal(got[n], p.states[n]) and np.array_equal(path[n], p.path[n]))]
    assert not bad, "decided datapoints that differ: %s" % bad[:8]
    assert np.allclose(lpj_path[decided], p.lpj_path[decided], rtol=LPJ_RTOL, atol=LPJ_RTOL)
    q = quotas(p.S, p.A)
    for n in np.nonzero(~decided)[0]:
        diff = np.nonzero(path[n] != p.path[n])[0]
        t = int(diff[0]) if len(diff) else p.A  # steps before t: the same active set, hence the same candidates
        assert np.array_equal(path[n, :t], p.path[n, :t])
        if t < p.A:  # they part at a near-tie
            assert abs(lpj_path[n, t] - p.lpj_path[n, t]) <= 1e-7 * max(1.0, abs(p.lpj_path[n, t]))
        for u in range(t):  # the slots of the steps before: the same sets of states
            lo = sum(q[:u])
            a = {r.tobytes() for r in got[n, lo:lo + q[u]]}
            assert len(a) == q[u] and all(r[p.path[n, :u]].all() for r in got[n, lo:lo + q[u]])


@pytest.mark.parametrize("algo,name", [("ebsc", "ragged"), ("es3c", "ragged"), ("es3c", "ragged_perm"), ("ebsc", "s200"),
                                       ("es3c", "s200")])
def test_lpj_out_equals_lpj_resident(eng, algo, name):
    p = problem(algo, name)
    _install(eng, p)
    path, lpj_path = eng.seed_states(p.A, want_path=True)
    eng.lpj_resident()
    lpj = eng.download_lpj()
    assert lpj.shape == (p.N, p.S_perm + p.S) and np.isfinite(lpj).all()  # no clamp fired
    slots = p.S_perm + np.concatenate(([0], np.cumsum(quotas(p.S, p.A))[:-1]))
    want = lpj[:, slots]
    err = np.abs(lpj_path - want) / np.maximum(1.0, np.abs(want))
    print("%s %s: largest relative difference %.3g" % (algo, name, err.max()))
    assert err.max() <= LPJ_RTOL
    # a winner has the largest lpj of its step
    for t, (lo, q) in enumerate(zip(slots, quotas(p.S, p.A))):
        assert (lpj[:, lo:lo + q].max(axis=1) <= lpj[:, lo] + 1e-9 * np.abs(lpj[:, lo])).all(), t


@pytest.mark.parametrize("algo,name", [("es3c", "ragged"), ("ebsc", "s200"), ("ebsc", "large_h")])
def test_digests_equal_digest_kernel(eng, algo, name):
    """The lpj kernels read the digests: the rows the seeding kernel wrote must evaluate exactly like the same rows
    uploaded (upload_states_packed runs digest_kernel)."""
    p = problem(algo, name)
    _install(eng, p)
    eng.seed_states(p.A)
    eng.lpj_resident()
    before = eng.download_lpj()
    packed = eng.download_states_packed()
    eng.upload_states_packed(packed)
    eng.lpj_resident()
    after = eng.download_lpj()
    assert np.isfinite(before).all()
    assert np.array_equal(before, after)


@pytest.mark.parametrize("algo", ALGOS)
def test_no_stale_rows_after_seeding(eng, eng2, algo):
    p = problem(algo, "ragged_perm")
    _install(eng, p)
    eng.init_states(1.0 / p.H, 5)
    eng.lpj_resident()
    noise = eng.download_lpj()
    eng.seed_states(p.A)
    eng.lpj_resident()
    seeded = eng.download_lpj()
    packed = eng.download_states_packed()
    assert not np.array_equal(noise, seeded)
    _install(eng2, p)  # a fresh context that uploads the same states
    eng2.upload_states_packed(packed)
    eng2.lpj_resident()
    assert np.array_equal(seeded, eng2.download_lpj())
    eng.seed_states(p.A)
    assert np.array_equal(eng.download_states_packed(), packed)
    # the statistics rows of the old K^n are gone too: the codes are refused until a new pass has run
    eng.lpj_resident()
    eng.stats()
    eng.posterior_codes(4)
    eng.seed_states(p.A)
    with pytest.raises(EvoAmdError):
        eng.posterior_codes(4)


def test_refusals_leave_kn_alone(eng):
    p = problem("ebsc", "tight")
    N, D, H, S = p.N, p.D, p.H, p.S
    rng = np.random.RandomState(2)

    def refused(match, A=p.A):
        before = eng.download_states_packed()
        with pytest.raises(EvoAmdError, match=match):
            eng.seed_states(A, want_path=True)
        assert np.array_equal(eng.download_states_packed(), before)
        eng.lpj_resident()  # K^n still counts as present

    for algo in ALGOS:
        q = problem(algo, "tight")
        eng.configure("bsc" if algo == "ebsc" else "sssc", N, D, H, S, 0, 4)
        eng.upload_data(q.Y)
        eng.init_states(0.3, 9)
        with pytest.raises(EvoAmdError, match="no Theta"):
            eng.seed_states(q.A)
        _set_params(eng, algo, q.theta)
        assert np.array_equal(eng.download_states_packed(), eng.download_states_packed())
        refused("max_active = 0", 0)
        refused("max_active = 21", 21)  # > S
        refused("max_active = 9", 9)    # > Hv (and > 8 for ES3C)
        refused("quota q_1 = 10", 2)
        eng.seed_states(q.A)            # quotas 7, 7, 6 of 8, 7, 6 latents: admitted
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
            refused("incomplete data")
        finally:
            eng.upload_masks(None)
            eng.upload_data(q.Y)
    # the caps: 8 for ES3C, 64 for EBSC
    for algo, A, match in (("es3c", 9, "ES3C: at most 8"), ("ebsc", 65, "EBSC: at most 64")):
        Hc, Sc = 80, 80
        eng.configure("bsc" if algo == "ebsc" else "sssc", 3, D, Hc, Sc, 0, 4)
        eng.upload_data(rng.normal(size=(3, D)))
        _set_params(eng, algo, make_theta(rng, algo, D, Hc))
        eng.init_states(0.1, 9)
        refused(match, A)
    # EBSC only: the direct residual kernel keeps no G; the float32 mode
    q = problem("ebsc", "tight")
    _install(eng, q)
    eng.init_states(0.3, 9)
    eng.set_option("bsc_direct", 1)
    try:
        _set_params(eng, "ebsc", q.theta)
        refused("bsc_direct")
    finally:
        eng.set_option("bsc_direct", 0)
    eng.set_option("ebsc_f32", 1)
    try:
        _install(eng, q)
        eng.init_states(0.3, 9)
        refused("float32")
    finally:
        eng.set_option("ebsc_f32", 0)
        _install(eng, q)


def _model_problem(algo):
    N, D, H, S = 64, 36, 48, 30
    rng = np.random.RandomState(17 if algo == "ebsc" else 18)
    theta = make_theta(rng, algo, D, H)  # pi H = 3
    Y, _ = make_data(rng, algo, theta, N)
    return N, D, H, S, theta, {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}


def _check_map_state(model, eng, theta, suff, my_data, S_perm, A, sync_host):
    """encode() on a freshly seeded K^n; returns the number of datapoints whose path's last state has the largest lpj."""
    path, _ = model.last_seed_path
    N, S, H = path.shape[0], model.S, model.H
    ss, lpj = (suff["ss"], suff["lpj"]) if sync_host else (eng.download_states(), eng.download_lpj())
    codes = model.encode(theta, suff, my_data, max_active=8)
    last = S_perm + sum(quotas(S, A)[:-1])
    top = lpj.argmax(axis=1) == last
    full = np.zeros((N, H), dtype=bool)
    np.put_along_axis(full, path.astype(np.int64), True, axis=1)
    assert np.array_equal(ss[:, last - S_perm], full)
    assert np.array_equal(codes.map_slot[top], np.full(top.sum(), last))
    assert np.array_equal(codes.map_states()[top], full[top])
    return int(top.sum())


@pytest.mark.parametrize("sync_host", [False, True])
@pytest.mark.parametrize("algo,permanent", [("ebsc", None), ("es3c", ALLZERO)])
def test_model_seed_resident_states(model_eng, algo, permanent, sync_host):
    eng = model_eng
    N, D, H, S, theta, my_data = _model_problem(algo)
    cls = BSC if algo == "ebsc" else SSSC
    kw = dict(engine=eng, rng="device", sync_host=sync_host, seed=1)
    ea = ("fit", "randflip", 6, 1, 1)
    S_perm = 1 if permanent else 0
    model = cls(D, H, S, **kw)
    suff = model.seed_resident_states(dict(theta), my_data, *ea, permanent=permanent, want_path=True)
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
    # the MAP state of encode() is the path's last state wherever that state has the largest lpj
    th = dict(theta)
    _check_map_state(model, eng, th, suff, my_data, S_perm, A, sync_host)
    # ... which, with as many steps as latents generated the data (three: each explains |W_h|^2 / (2 sigma^2) ~ 100 nats
    # against a prior cost of log(pi / (1 - pi)) ~ -2.7), is the case for some datapoint at least
    three = cls(D, H, S, **kw)
    suff3 = three.seed_resident_states(dict(theta), my_data, *ea, max_active=3, permanent=permanent, want_path=True)
    assert _check_map_state(three, eng, dict(theta), suff3, my_data, S_perm, 3, sync_host) >= 1
    model.invalidate()  # the engine holds the other model's K^n
    suff = model.seed_resident_states(dict(theta), my_data, *ea, permanent=permanent)
    # the first E-step from the seeded K^n against the first from Bernoulli(1 / H) states on the same data
    F_seed = model.E_step(th, suff, my_data)[0]
    F, _, _, th = model.step(th, suff, my_data)  # the dict feeds step()
    assert np.isfinite(F)
    other = cls(D, H, S, **kw)
    th2 = dict(theta)
    noise = other.init_resident_states(my_data, *ea, permanent=permanent, seed=3)
    F_noise = other.E_step(th2, noise, my_data)[0]
    print("%s sync_host=%s: first free energy seeded %.4f, init_resident_states %.4f" % (algo, sync_host, F_seed, F_noise))
    assert np.isfinite(F_seed) and np.isfinite(F_noise)
    assert F_seed > F_noise


def test_plain_and_ex_calls_agree(eng):
    """evoamd_seed_states against evoamd_seed_states_ex with no flag, on the smallest problem: K^n, path and lpj bit for bit."""
    p = problem("ebsc", "tight")
    _install(eng, p)
    got = []
    for call in ("plain", "ex"):
        eng.upload_states(np.zeros((p.N, p.S, p.H), dtype=bool))
        path, lpj = np.full((p.N, p.A), -7, dtype=np.int32), np.full((p.N, p.A), -7.0)
        if call == "plain":
            check(eng.lib.evoamd_seed_states(eng._h, p.A, i32ptr(path), dptr(lpj)))
        else:
            check(eng.lib.evoamd_seed_states_ex(eng._h, p.A, 0, i32ptr(path), dptr(lpj)))
        got.append((eng.download_states_packed(), path, lpj))
    assert np.array_equal(got[0][1], p.path) and got[0][0].any()
    assert all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))

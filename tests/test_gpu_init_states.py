"""K^n(0) drawn on the GPU: Engine.init_states (csrc/kernels_init.hpp) and Model.init_resident_states.

1. kernel against its NumPy mirror (evo_amd.variational.init_states_counter), np.array_equal, both homes of the round state;
2. the digests the kernel writes against digest_kernel's (same lpj bits before and after a re-upload of the same rows);
3. Model.init_resident_states for both models, device-resident and host-synchronised;
4. the round cap on the device; 5. a learning smoke on the bars.
"""
import numpy as np
import pytest

from evo_amd._lib import EvoAmdError
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC
from evo_amd.variational import init_states, init_states_counter
from evo_amd.variational.utils import enumerate_states

pytestmark = pytest.mark.gpu

ALLZERO = {"background": False, "allzero": True, "singletons": False}
BACKGROUND = {"background": True, "allzero": False, "singletons": False}

# name -> (algo, N, D, H, S, S_perm, background, home)
SHAPES = {
    "es3c": ("es3c", 37, 8, 70, 12, 0, False, -1),       # HW = 2, ragged last word, N no multiple of the waves per workgroup
    "es3c_perm": ("es3c", 37, 8, 70, 12, 1, False, -1),  # ... with the permanent all-zero state
    "ebsc_s200": ("ebsc", 9, 4, 130, 200, 0, False, -1),  # more than 64 states per wave, HW = 3
    "ebsc_dups": ("ebsc", 33, 4, 8, 50, 0, False, -1),    # ~11 rounds, almost all candidates duplicates, HW = 1
    "ebsc_bg": ("ebsc", 16, 4, 9, 20, 0, True, -1),       # background unit
    "ebsc_large_h": ("ebsc", 5, 4, 1100, 4, 0, False, -1),  # HW = 18
    "ebsc_exact": ("ebsc", 6, 4, 5, 32, 0, False, -1),    # exact mode
    "ebsc_s1024": ("ebsc", 3, 4, 64, 1024, 0, False, -1),  # the largest S configure admits (LDS home: 32 KB per wave)
    "ebsc_s1024_gmem": ("ebsc", 3, 4, 64, 1024, 0, False, 1),  # ... and the same in the global-memory home
    "es3c_gmem": ("es3c", 37, 8, 70, 12, 1, False, 1),
}
SEED = 20240607


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.set_option("init_states_home", -1)
    e.set_option("background_unit", 0)
    e.close()


@pytest.fixture(scope="module")
def model_eng():
    """The Model tests' own engine: Model._prepare keeps per-engine state that the engine-level tests do not maintain."""
    e = Engine(0)
    yield e
    e.close()


def _permanent(S_perm, background):
    return BACKGROUND if background else (ALLZERO if S_perm else None)


def _configure(eng, name):
    algo, N, D, H, S, S_perm, background, home = SHAPES[name]
    eng.set_option("background_unit", 1 if background else 0)
    eng.set_option("init_states_home", home)
    eng.configure("bsc" if algo == "ebsc" else "sssc", N, D, H, S, S_perm, 4)
    return algo, N, D, H, S, S_perm, background


_mirror_cache = {}


def _mirror(N, S, H, S_perm, background, seed=SEED):
    key = (N, S, H, S_perm, background, seed)
    if key not in _mirror_cache:
        _mirror_cache[key] = init_states_counter(N, S, H, seed, permanent=_permanent(S_perm, background))
        _mirror_cache[key].setflags(write=False)
    return _mirror_cache[key]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_kernel_equals_mirror(eng, name):
    algo, N, D, H, S, S_perm, background = _configure(eng, name)
    Hv = H - 1 if background else H
    table = enumerate_states(Hv) if S == 2 ** Hv else None
    eng.init_states(1.0 / H, SEED, table=table)
    got = eng.download_states()
    want = _mirror(N, S, H, S_perm, background)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert np.array_equal(got, want), "datapoints that differ: %s" % bad[:8]
    # the packed download sees the same words
    assert np.array_equal(eng.download_states_packed(), np.packbits(want, axis=-1))


def _theta(rng, algo, D, H):
    W = rng.normal(size=(D, H)) * 0.4
    if algo == "ebsc":
        return {"W": W, "pi": 0.1, "sigma": 1.1}
    A = rng.normal(size=(H, 3)) * 0.2
    return {"W": W, "pies": rng.uniform(0.1, 0.4, H), "mus": rng.normal(size=H) * 0.5, "Psi": np.eye(H) + A @ A.T,
            "sigma2": np.float64(1.3)}


@pytest.mark.parametrize("name", ["es3c", "ebsc_s200"])
def test_digests_equal_digest_kernel(eng, name):
    """The lpj kernels read the digests: the rows the sampler wrote must evaluate exactly like the same rows uploaded
    (upload_states_packed runs digest_kernel)."""
    algo, N, D, H, S, S_perm, background = _configure(eng, name)
    rng = np.random.RandomState(3)
    eng.upload_data(rng.normal(size=(N, D)))
    th = _theta(rng, algo, D, H)
    if algo == "ebsc":
        eng.set_params_bsc(th["W"], th["pi"], th["sigma"])
    else:
        eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], th["sigma2"])
    eng.init_states(1.0 / H, SEED)
    eng.lpj_resident()
    before = eng.download_lpj()
    packed = eng.download_states_packed()
    eng.upload_states_packed(packed)
    eng.lpj_resident()
    after = eng.download_lpj()
    assert np.isfinite(before).all()
    assert np.array_equal(before, after)


def _model_problem(algo, seed=0):
    rng = np.random.RandomState(seed)
    N, D, H, S = 37, 8, 70, 12
    Y = rng.normal(size=(N, D))
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    return N, D, H, S, my_data


@pytest.mark.parametrize("algo", ["ebsc", "es3c"])
def test_model_resident(model_eng, algo):
    eng = model_eng
    N, D, H, S, my_data = _model_problem(algo)
    cls = BSC if algo == "ebsc" else SSSC
    model = cls(D, H, S, engine=eng, rng="device", sync_host=False)
    theta = model.check_params(model.standard_init(my_data))
    suff = model.init_resident_states(my_data, "fit", "randflip", 6, 1, 1, seed=11)
    assert suff["ss"] is None and suff["lpj"] is None
    assert np.array_equal(eng.download_states(), _mirror(N, S, H, 0, False, model.last_init_seed))
    for _ in range(3):
        F, _, _, theta = model.step(theta, suff, my_data)
        assert np.isfinite(F)
    model.sync_to_host(suff)
    assert suff["ss"].shape == (N, S, H) and suff["ss"].dtype == np.bool_
    assert suff["lpj"].shape == (N, S) and np.isfinite(suff["lpj"]).all()
    for n in range(N):
        assert len({r.tobytes() for r in suff["ss"][n]}) == S
    codes = model.encode(theta, suff, my_data, max_active=8)
    assert codes.idx.shape == (N, 8) and np.isfinite(codes.p).all() and np.isfinite(codes.map_q).all()


@pytest.mark.parametrize("algo,permanent", [("ebsc", None), ("es3c", ALLZERO)])
def test_model_host_synchronised(model_eng, algo, permanent):
    eng = model_eng
    N, D, H, S, my_data = _model_problem(algo)
    cls = BSC if algo == "ebsc" else SSSC
    model = cls(D, H, S, engine=eng)
    args = ("fit", "cross_randflip", 4, 2, 1)
    np.random.seed(5)
    suff = model.init_resident_states(my_data, *args, permanent=permanent)
    S_perm = 1 if permanent else 0
    assert np.array_equal(suff["ss"], _mirror(N, S, H, S_perm, False, model.last_init_seed))
    np.random.seed(5)
    again = model.init_resident_states(my_data, *args, permanent=permanent)
    assert np.array_equal(again["ss"], suff["ss"])
    host = init_states(N, S, H, *args, permanent=permanent)
    assert set(suff) == set(host)
    for k, v in host.items():
        if isinstance(v, np.ndarray):
            assert suff[k].dtype == v.dtype and suff[k].shape == v.shape, k
            if k not in ("ss", "lpj"):
                assert np.array_equal(suff[k], v), k
        else:
            assert suff[k] == v and type(suff[k]) is type(v), k
    assert suff["n_children"] == 3  # the cross rule
    theta = model.check_params(model.standard_init(my_data))
    np.random.seed(6)
    F, _, _, theta = model.step(theta, suff, my_data)
    assert np.isfinite(F)


def test_round_cap_on_the_device(eng):
    algo, N, D, H, S, S_perm, background = _configure(eng, "es3c")
    rng = np.random.RandomState(3)
    eng.upload_data(rng.normal(size=(N, D)))
    th = _theta(rng, algo, D, H)
    eng.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], th["sigma2"])
    with pytest.raises(EvoAmdError, match="max_rounds = 1 "):
        eng.init_states(1.0 / H, SEED, max_rounds=1)
    with pytest.raises(EvoAmdError, match="K\\^n is not on the device"):
        eng.lpj_resident()
    with pytest.raises(EvoAmdError, match="K\\^n is not on the device"):
        eng.stats()
    eng.init_states(1.0 / H, SEED)
    assert np.array_equal(eng.download_states(), _mirror(N, S, H, S_perm, background))
    eng.lpj_resident()
    assert np.isfinite(eng.download_lpj()).all()


def test_learning_smoke_bars(model_eng):
    """The bars set-up of tests/test_gpu_models.py (test_kat_bars_from_seed: H = 10, D = 25, N = 500, S = 32, data and
    Theta^init from np.random.seed(42), fit / randflip 10 x 1 x 1), BSC only, 30 EM iterations with the device EA from a
    device-initialised K^n and from two host-initialised ones (np.random seeds 1 and 2 for K^n(0)); data, Theta^init
    and EA stream are the same in all three.  Every run ends finite and higher than it started; the device-initialised
    final F does not lie below the first host run's by more than the spread between the two host runs.

    Observed on one MI355X with bars data from RandomState(42) instead (eight K^n(0) seeds per side, final F after 30
    iterations): N = 500 host -41.23 .. -42.59 and one run at -57.06, device-initialised -40.53 .. -43.13; N = 200 (this
    test's first form, which failed: host -42.04 / -44.73, device-initialised -55.70) both sides bimodal, -40 .. -44 or
    -55 .. -60.  The two initialisations give the same distribution, but the margin of this test is the difference of two
    draws from it."""
    eng = model_eng
    H, D, N, S = 10, 25, 500, 32
    R = H // 2
    W = np.zeros((R, R, H))
    for i in range(R):
        W[i, :, i] = 1.0
        W[:, i, R + i] = 1.0
    gen = {"W": 10.0 * W.reshape(D, H), "pi": 2.0 / H, "sigma": 1.0}
    ea = ("fit", "randflip", 10, 1, 1)

    def run(kind, seed):
        model = BSC(D, H, S, engine=eng, rng="device", sync_host=False, seed=1)
        np.random.seed(42)
        Y = model.generate_data(gen, N)["y"]
        my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
        theta = model.check_params(model.standard_init(my_data))
        np.random.seed(seed)
        if kind == "device":
            suff = model.init_resident_states(my_data, *ea)
        else:
            suff = init_states(N, S, H, *ea)
        Fs = []
        for _ in range(30):
            F, _, _, theta = model.step(theta, suff, my_data)
            Fs.append(F)
        Fs = np.array(Fs)
        assert np.isfinite(Fs).all()
        assert Fs[-5:].mean() > Fs[:5].mean()
        return Fs[-1]

    F_host_a, F_host_b, F_dev = run("host", 1), run("host", 2), run("device", 1)
    spread = abs(F_host_a - F_host_b)
    print("final F: host %.6f / %.6f (spread %.3g), device-initialised %.6f" % (F_host_a, F_host_b, spread, F_dev))
    assert F_dev >= F_host_a - spread

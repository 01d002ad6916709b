"""Samples from the model on the GPU: Engine.generate / Model.generate_data_device (csrc/kernels_generate.hpp) against the
NumPy mirror evo_amd.models.generate_counter.

1. s bit for bit, z / y_mean / y to 1e-9 max(1, max |mirror|) at the word edges of H, the lane-stride tails of D and a
   partly filled last workgroup; 2. given s; 3. shards; 4. determinism; 5. keep; 6. the law on the device; 7. a resident
   training run is not disturbed.
"""
import numpy as np
import pytest

import _generate_problems as gp
from evo_amd._lib import EvoAmdError
from evo_amd.engine import Engine
from evo_amd.models import BSC, SSSC, generate_counter

pytestmark = pytest.mark.gpu

N = 257  # 64 full workgroups of four waves and one wave of a 65th
SEED = 0x1234567890ABCDEF
RTOL = 1e-9  # of max(1, max |mirror|): the parity tolerance of the project's sums

# name -> (model, H, D, Psi ("dense", "singular", "diag"; None for BSC), prior)
#   prior, ES3C: "edges" = per-latent pies from U(0.05, 0.6) with pies[0] = 0 and pies[-1] = 1 (H = 1: 0.5); BSC: the scalar pi
CASES = {
    "es3c_h1_d1": ("sssc", 1, 1, "dense", "edges"),
    "es3c_h63_d37": ("sssc", 63, 37, "dense", "edges"),
    "es3c_h64_d64": ("sssc", 64, 64, "diag", "edges"),
    "es3c_h70_d200": ("sssc", 70, 200, "singular", "edges"),
    "es3c_h130_d37": ("sssc", 130, 37, "dense", "edges"),
    "es3c_h70_d600": ("sssc", 70, 600, "dense", "edges"),  # D above 512: a second walk over the active latents
    "ebsc_h1_d1": ("bsc", 1, 1, None, 0.5),
    "ebsc_h63_d37": ("bsc", 63, 37, None, 0.1),
    "ebsc_h64_d64": ("bsc", 64, 64, None, 0.05),
    "ebsc_h70_d200": ("bsc", 70, 200, None, 0.03),
    "ebsc_h130_d37": ("bsc", 130, 37, None, 0.02),
    "ebsc_h70_d600": ("bsc", 70, 600, None, 0.03),
    "ebsc_pi0": ("bsc", 70, 37, None, 0.0),
    "ebsc_pi1": ("bsc", 70, 37, None, 1.0),
}


def _theta(name):
    model_name, H, D, psi, prior = CASES[name]
    if model_name == "bsc":
        return gp.bsc_theta(H, D, 21, pi=prior)
    theta = gp.sssc_theta(H, D, 22, rank=max(1, H - 6) if psi == "singular" else None, diagonal=psi == "diag")
    theta["pies"] = np.random.RandomState(23).uniform(0.05, 0.6, size=H)
    if H > 1:
        theta["pies"][0], theta["pies"][-1] = 0.0, 1.0
    return theta


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _model(eng, name_or_model, H=None, D=None, **kw):
    if name_or_model in CASES:
        name_or_model, H, D = CASES[name_or_model][:3]
    return (BSC if name_or_model == "bsc" else SSSC)(D, H, 8, engine=eng, **kw)


_mirror_cache = {}


def _mirror(name, n=N, seed=SEED):
    key = (name, n, seed)
    if key not in _mirror_cache:
        out = generate_counter(CASES[name][0], _theta(name), n, seed)
        for v in out.values():
            v.setflags(write=False)
        _mirror_cache[key] = out
    return _mirror_cache[key]


def _assert_close(got, want, label):
    for key in want:
        if key == "s":
            assert got["s"].dtype == np.bool_ and np.array_equal(got["s"], want["s"]), label + ": s"
            continue
        bound = RTOL * max(1.0, float(np.abs(want[key]).max()))
        err = float(np.abs(got[key] - want[key]).max())
        print("%s %s: max |device - mirror| = %.3g (bound %.3g)" % (label, key, err, bound))
        assert got[key].shape == want[key].shape and err <= bound, (label, key, err, bound)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_against_mirror(eng, name):
    model = _model(eng, name)
    got = model.generate_data_device(_theta(name), N, seed=SEED)
    want = _mirror(name, seed=model.last_generate_seed)
    assert model.last_generate_seed == SEED and sorted(got) == sorted(want)
    _assert_close(got, want, name)
    if CASES[name][0] == "sssc":
        assert np.array_equal(got["z"] != 0.0, got["s"])
        if CASES[name][1] > 1:
            assert not got["s"][:, 0].any() and got["s"][:, -1].all()  # pies of 0 and of 1
    elif name in ("ebsc_pi0", "ebsc_pi1"):
        assert got["s"].all() if name == "ebsc_pi1" else not got["s"].any()


@pytest.mark.parametrize("model_name", ["bsc", "sssc"])
def test_given_s(eng, model_name):
    name = "es3c_h130_d37" if model_name == "sssc" else "ebsc_h130_d37"
    H, D = CASES[name][1:3]
    theta = _theta(name)
    s = np.random.RandomState(31).random_sample((N, H)) < 0.1
    s[:40] = False
    s[40:80] = True  # k = H = 130
    s[255] = False   # a wave of the last full workgroup, and the lone wave behind it
    s[256] = True
    model = _model(eng, name)
    got = model.generate_data_device(theta, N, seed=SEED, my_hdata={"s": s})
    want = generate_counter(model_name, theta, N, SEED, s=s)
    assert np.array_equal(got["s"], s)
    _assert_close(got, want, name + " given s")
    zero = ~s.any(axis=1)
    assert zero.sum() >= 41
    assert not got["y_mean"][zero].any()
    sigma = theta["sigma"] if model_name == "bsc" else np.sqrt(theta["sigma2"])
    noise = (want["y"] - want["y_mean"])[zero]  # sigma g of the mirror
    assert np.abs(got["y"][zero] - noise).max() <= RTOL * max(1.0, np.abs(noise).max())
    assert abs(noise.std() / sigma - 1.0) < 5.0 / np.sqrt(2.0 * noise.size)  # five standard errors of a sample deviation
    if model_name == "sssc":
        assert not got["z"][zero].any()
        assert (got["z"][40:80] != 0.0).all()


def test_shards_concatenate(eng):
    for name in ("es3c_h70_d200", "ebsc_h130_d37"):
        model = _model(eng, name)
        theta = _theta(name)
        full = model.generate_data_device(theta, N, seed=SEED)
        a = model.generate_data_device(theta, 100, seed=SEED)
        b = model.generate_data_device(theta, N - 100, seed=SEED, first_index=100)
        for key in full:
            assert np.array_equal(np.concatenate((a[key], b[key])), full[key]), (name, key)
    # ... and with s given
    name = "es3c_h70_d200"
    model, theta = _model(eng, name), _theta(name)
    s = np.random.RandomState(32).random_sample((N, 70)) < 0.2
    full = model.generate_data_device(theta, N, seed=SEED, my_hdata={"s": s})
    a = model.generate_data_device(theta, 100, seed=SEED, my_hdata={"s": s[:100]})
    b = model.generate_data_device(theta, N - 100, seed=SEED, first_index=100, my_hdata={"s": s[100:]})
    for key in full:
        assert np.array_equal(np.concatenate((a[key], b[key])), full[key]), key


def test_determinism_and_seeds(eng):
    name = "es3c_h130_d37"
    model, theta = _model(eng, name), _theta(name)
    one = model.generate_data_device(theta, N, seed=SEED)
    two = model.generate_data_device(theta, N, seed=SEED)
    other = model.generate_data_device(theta, N, seed=SEED + 1)
    for key in one:
        assert np.array_equal(one[key], two[key]), key
    assert not np.array_equal(one["s"], other["s"]) and not np.array_equal(one["y"], other["y"])
    np.random.seed(9)
    drawn = model.generate_data_device(theta, 5)
    np.random.seed(9)
    assert model.last_generate_seed == int(np.random.randint(0, 2 ** 31 - 1))
    assert np.array_equal(drawn["y"], model.generate_data_device(theta, 5, seed=model.last_generate_seed)["y"])


def test_keep(eng):
    name = "es3c_h70_d200"
    model, theta = _model(eng, name), _theta(name)
    full = model.generate_data_device(theta, N, seed=SEED)
    only_y = model.generate_data_device(theta, N, seed=SEED, keep=("y",))
    assert sorted(only_y) == ["y"] and np.array_equal(only_y["y"], full["y"])
    for what in ("s", "z", "y_mean"):
        with pytest.raises(EvoAmdError, match="%s was not kept" % what):
            eng.download_generated(what)
    some = model.generate_data_device(theta, N, seed=SEED, keep=("z", "y_mean"))
    assert sorted(some) == ["y_mean", "z"]
    assert np.array_equal(some["z"], full["z"]) and np.array_equal(some["y_mean"], full["y_mean"])
    with pytest.raises(ValueError):
        model.generate_data_device(theta, N, seed=SEED, keep=("y", "lpj"))
    bsc = _model(eng, "ebsc_h70_d200")
    assert sorted(bsc.generate_data_device(_theta("ebsc_h70_d200"), 9, seed=SEED)) == ["s", "y", "y_mean"]
    with pytest.raises(EvoAmdError, match="z was not kept"):
        eng.download_generated("z")


def test_refusals(eng):
    th = gp.bsc_theta(4, 3, 0)
    par = dict(Wt=np.ascontiguousarray(th["W"].T), pies=np.full(4, 0.5))
    with pytest.raises(EvoAmdError, match="sigma"):
        eng.generate("bsc", 5, 1, sigma=float("nan"), **par)
    with pytest.raises(EvoAmdError, match="positive"):
        eng.generate("bsc", 0, 1, sigma=1.0, **par)
    H = 8200  # one wave's eps values: more than 64 KB
    with pytest.raises(EvoAmdError, match="64 KB"):
        eng.generate("sssc", 1, 1, np.zeros((H, 1)), np.zeros(H), np.zeros(H), np.zeros((H, H)), 1.0)
    fresh = Engine(0)
    try:
        with pytest.raises(EvoAmdError, match="no evoamd_generate call has completed"):
            fresh.download_generated("y")
    finally:
        fresh.close()


@pytest.mark.parametrize("model_name", ["bsc", "sssc"])
def test_law_on_the_device(eng, model_name):
    """The problem and the bounds of tests/test_generate_counter.py::test_law, which shows that the mirror alone meets them."""
    theta = gp.law_theta(model_name)
    model = _model(eng, model_name, 8, 6)
    out = model.generate_data_device(theta, gp.LAW_N, seed=gp.LAW_SEED)
    gp.assert_law(model_name, theta, out, "device")


@pytest.mark.parametrize("device_mstep", [False, True])
@pytest.mark.parametrize("model_name", ["bsc", "sssc"])
def test_resident_run_is_not_disturbed(model_name, device_mstep):
    """generate_data_device between the step() calls of a resident run (rng="device", sync_host=False) on the SAME engine,
    compared with the same run without the calls.

    A learning run does not repeat bit for bit by itself: the statistics are summed with f64 atomics ("not
    bit-reproducible run to run"), and on one MI355X two runs WITHOUT any generate call differed in Theta by 4e-16 ..
    5e-14 from the first iteration on (both models, host and device Theta update), in F in the last place now and then,
    never in K^n.  So the bit-for-bit comparison is made where the run is deterministic -- with Theta held fixed
    (to_learn = ()): F, the counters, K^n and the lpj rows of every step --, and the learning run is compared in what it
    repeats exactly (K^n, the counters) and to the parity tolerance of the project's sums in F and Theta."""
    Nr, D, H, S = 150, 12, 20, 10
    gen = gp.sssc_theta(H, D, 41, diagonal=True) if model_name == "sssc" else gp.bsc_theta(H, D, 41)
    e = Engine(0)
    try:
        cls = BSC if model_name == "bsc" else SSSC
        Y = cls(D, H, S, engine=e).generate_data_device(gen, Nr, seed=77, keep=("y",))["y"]
        assert Y.shape == (Nr, D) and np.isfinite(Y).all()

        def run(interleave, **kw):
            model = cls(D, H, S, engine=e, rng="device", sync_host=False, seed=3, device_mstep=device_mstep, **kw)
            my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
            np.random.seed(4)
            theta = model.check_params(model.standard_init(my_data))
            suff = model.init_resident_states(my_data, "fit", "randflip", 4, 1, 1, seed=5)
            trace = []
            for it in range(4):
                if interleave and it in (1, 3):
                    extra = model.generate_data_device(gen, 300, seed=it)
                    assert np.isfinite(extra["y"]).all()
                F, nu, nsub, theta = model.step(theta, suff, my_data)
                assert np.isfinite(F)  # step() on generated my_data
                trace.append((F, nu, nsub))
            model.sync_to_host(suff)
            return trace, {k: np.array(v) for k, v in theta.items()}, suff["ss"].copy(), suff["lpj"].copy()

        plain, disturbed = run(False, to_learn=()), run(True, to_learn=())
        assert plain[0] == disturbed[0], (plain[0], disturbed[0])
        for key in plain[1]:
            assert np.array_equal(plain[1][key], disturbed[1][key]), key
        assert np.array_equal(plain[2], disturbed[2]) and np.array_equal(plain[3], disturbed[3])

        plain, disturbed = run(False), run(True)
        assert [t[1:] for t in plain[0]] == [t[1:] for t in disturbed[0]]
        assert np.array_equal(plain[2], disturbed[2])
        for a, b in zip(plain[0], disturbed[0]):
            assert abs(a[0] - b[0]) <= RTOL * abs(a[0]), (a, b)
        for key in plain[1]:
            scale = max(1.0, float(np.abs(plain[1][key]).max()))
            assert np.abs(plain[1][key] - disturbed[1][key]).max() <= RTOL * scale, key
        scale = max(1.0, float(np.abs(plain[3]).max()))
        assert np.abs(plain[3] - disturbed[3]).max() <= RTOL * scale
    finally:
        e.close()

"""evo_amd.variational.init_states_counter: the NumPy mirror of the device K^n(0) sampler (csrc/kernels_init.hpp).

1. the law: the mirror's assembly function fed NumPy's own stream reproduces init_states exactly;
2. the stream: bit frequencies of the counter-based draw within 5 sigma (fixed seed: deterministic), different
   (n, round, seed) give different draws, same arguments the same;
3. invariants of the result; 4. the round cap.
"""
import numpy as np
import pytest

from evo_amd.variational import init_states, init_states_counter
from evo_amd.variational.utils import assemble_states, counter_draw

ALLZERO = {"background": False, "allzero": True, "singletons": False}
BACKGROUND = {"background": True, "allzero": False, "singletons": False}

# (H, S asked of init_states, permanent, rows of K^n)
LAW_CASES = {
    "s_perm0": (70, 12, None, 12),
    "s_perm1": (70, 12, ALLZERO, 12),
    "many_rounds": (8, 50, None, 50),        # 50 of 256 states at p0 = 1/8: ~10 rounds, almost all candidates duplicates
    "background": (9, 20, BACKGROUND, 20),
    "exact": (5, 32, None, 32),
    # exact mode with the permanent all-zero state, as the host function lays it out: asked for 2^5 states it returns
    # the table's other 31 rows ...
    "exact_allzero": (5, 32, ALLZERO, 31),
    # ... and asked for 31 it SAMPLES all 31 non-zero states (hundreds of rounds: the reference has no cap)
    "s31_allzero_sampled": (5, 31, ALLZERO, 31),
}


@pytest.mark.parametrize("name", sorted(LAW_CASES))
def test_law_is_init_states(name):
    H, S, permanent, rows = LAW_CASES[name]
    N = 9
    Hv = H - 1 if (permanent and permanent["background"]) else H
    p0 = 1.0 / H
    for k in (0, 1):
        np.random.seed(k)
        want = init_states(N, S, H, "fit", "randflip", 2, 1, 1, permanent=permanent)["ss"]
        np.random.seed(k)
        got = assemble_states(N, S, H, lambda n, r: np.random.random((S, Hv)) < p0, permanent, max_rounds=10 ** 6)
        assert want.shape == (N, rows, H)
        assert got.dtype == np.bool_ and np.array_equal(got, want)


def test_law_with_p_init():
    H, S, N, p0 = 70, 12, 9, 0.08
    np.random.seed(3)
    want = init_states(N, S, H, "fit", "randflip", 2, 1, 1, p_init_Kn=p0)["ss"]
    np.random.seed(3)
    got = assemble_states(N, S, H, lambda n, r: np.random.random((S, H)) < p0)
    assert np.array_equal(got, want)


def test_stream_frequencies():
    N, S, H = 64, 64, 256
    p0 = 1.0 / H
    draw = counter_draw(1234, S, H, p0)
    bits = np.stack([draw(n, 0) for n in range(N)])
    assert bits.shape == (N, S, H) and bits.dtype == np.bool_
    M = N * S * H
    print("bits set", int(bits.sum()), "expected", M * p0, "+-", 5 * np.sqrt(M * p0 * (1 - p0)))
    assert abs(bits.sum() - M * p0) <= 5 * np.sqrt(M * p0 * (1 - p0))
    M = N * S
    per_latent = bits.sum(axis=(0, 1))
    print("largest per-latent deviation", np.abs(per_latent - M * p0).max(), "bound", 5 * np.sqrt(M * p0 * (1 - p0)))
    assert (np.abs(per_latent - M * p0) <= 5 * np.sqrt(M * p0 * (1 - p0))).all()


def test_stream_depends_on_every_argument():
    S, H, p0 = 64, 256, 0.05
    a = counter_draw(7, S, H, p0)
    b = counter_draw(8, S, H, p0)
    base = a(3, 0)
    assert np.array_equal(base, counter_draw(7, S, H, p0)(3, 0))
    assert not np.array_equal(base, a(4, 0))
    assert not np.array_equal(base, a(3, 1))
    assert not np.array_equal(base, b(3, 0))
    x, y = init_states_counter(5, 12, 70, 99), init_states_counter(5, 12, 70, 99)
    assert np.array_equal(x, y)
    assert not np.array_equal(x, init_states_counter(5, 12, 70, 100))
    assert not np.array_equal(x[0], x[1])


def _keys(rows):
    return [r.tobytes() for r in np.packbits(rows, axis=1)]


@pytest.mark.parametrize("H,S,permanent", [(70, 12, None), (70, 12, ALLZERO), (8, 50, None), (9, 20, BACKGROUND)])
def test_invariants(H, S, permanent):
    N, seed = 21, 5
    ss = init_states_counter(N, S, H, seed, permanent=permanent)
    assert ss.shape == (N, S, H) and ss.dtype == np.bool_
    background = bool(permanent and permanent["background"])
    Hv = H - 1 if background else H
    draw = counter_draw(seed, S, Hv, 1.0 / H)
    for n in range(N):
        keys = _keys(ss[n])
        assert len(set(keys)) == S
        if permanent is ALLZERO:
            assert ss[n].any(axis=1).all()
        if background:
            assert ss[n, :, -1].all()
        first = len({r.tobytes() for r in draw(n, 0) if permanent is not ALLZERO or r.any()})
        block = keys[:min(first, S)]
        assert block == sorted(block), "the first round's block is not ascending"


def test_round_cap():
    with pytest.raises(RuntimeError, match="max_rounds = 1 "):
        init_states_counter(37, 12, 70, 1, max_rounds=1)
    assert init_states_counter(37, 12, 70, 1, max_rounds=256).shape == (37, 12, 70)

"""evo_amd.variational.posterior_scores_host, the NumPy mirror of the score kernel (csrc/kernels_refine.hpp), against a
brute-force evaluation in np.longdouble, and the refusal of Model.refine_resident_states that needs no device.

Tolerance for F and entropy: 1e-12 per unit of max(1, |value|) -- the longdouble evaluation is the yardstick, and a
double-precision sum of L <= 1025 terms is bounded by about L 2^-53 = 1.1e-13 relative.  best and k_best are exact."""
import numpy as np
import pytest

from _refine_problems import score_rows, scores_longdouble
from evo_amd.variational import posterior_scores_host

TOL = 1e-12


def _close(got, want, tol, name):
    want = np.asarray(want, dtype=np.longdouble)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - want) / np.maximum(1.0, np.abs(want))
    assert np.isfinite(np.asarray(got)).all(), name
    assert float(err.max()) <= tol, (name, float(err.max()))


@pytest.mark.parametrize("L,S_perm", [(L, p) for L in (1, 4, 66, 200, 1025) for p in (0, 1) if L - p >= 1])
def test_mirror_against_longdouble(L, S_perm):
    rng = np.random.RandomState(100 + L + S_perm)
    N, H = 7, 70
    lpj = score_rows(rng, N, L)
    ss = rng.uniform(size=(N, L - S_perm, H)) < 0.1
    got = posterior_scores_host(lpj, ss, S_perm)
    want = scores_longdouble(lpj, ss, S_perm)
    _close(got["F"], want["F"], TOL, "F")
    _close(got["entropy"], want["entropy"], TOL, "entropy")
    assert got["best"].dtype == np.int32 and got["k_best"].dtype == np.int32
    assert np.array_equal(got["best"], want["best"])
    assert np.array_equal(got["k_best"], want["k_best"])
    _close(got["k_mean"] / H, want["k_mean"] / H, TOL, "k_mean")
    # the planted rows: equal values -> entropy log L; two equal maxima -> the lower column; spread > 800 -> finite
    assert abs(got["entropy"][0] - np.log(L)) <= TOL * max(1.0, np.log(L))
    assert abs(got["F"][0] - (lpj[0, 0] + np.log(L))) <= TOL * abs(lpj[0, 0])
    if L >= 2:
        ties = np.flatnonzero(lpj[1] == lpj[1].max())
        assert ties.size == 2 and got["best"][1] == ties[0]
        assert lpj[2].max() - lpj[2].min() > 800 and np.isfinite(got["entropy"][2]) and got["entropy"][2] >= 0
        assert (np.exp(lpj[2] - lpj[2].max()) == 0).any()  # weights do underflow in this row


def test_permanent_column_as_the_maximum():
    rng = np.random.RandomState(5)
    N, S, H = 5, 9, 12
    lpj = rng.normal(size=(N, S + 1)) - 20.0
    lpj[:, 0] = lpj.max(axis=1) + 1.0
    ss = rng.uniform(size=(N, S, H)) < 0.4
    got = posterior_scores_host(lpj, ss, S_perm=1)
    assert (got["best"] == 0).all() and (got["k_best"] == 0).all()
    want = scores_longdouble(lpj, ss, 1)
    _close(got["k_mean"] / H, want["k_mean"] / H, TOL, "k_mean")


def test_without_states_only_the_row_scores():
    lpj = np.array([[0.0, -1.0, -2.0]])
    got = posterior_scores_host(lpj)
    assert set(got) == {"F", "entropy", "best"}
    q = np.exp(lpj[0]) / np.exp(lpj[0]).sum()
    assert abs(got["entropy"][0] + (q * np.log(q)).sum()) <= 1e-14


def test_refine_needs_device_rng():
    """rng="reference" draws candidates on the host: refused before an engine exists."""
    from evo_amd.models import BSC, SSSC
    for cls in (BSC, SSSC):
        model = cls(8, 6, 5, rng="reference")
        with pytest.raises(ValueError, match="rng='device'"):
            model.refine_resident_states({}, {}, {}, 3)
        assert model._engine is None and model._n_steps == 0

"""evo_amd.models.sample_posterior_counter: the NumPy mirror of Model.sample_posterior (csrc/kernels_posterior_sample.hpp).

1. the law in distribution, with fixed seeds (deterministic): slot frequencies over 20 000 draws against q_ns, every
   |f - q| <= 6 sqrt(q (1 - q) / T); with fill="all", the sample mean of y per entry against predictive_moments_host's mean
   within 6 standard errors sqrt(var / T), and the sample variance against its var within 6 sqrt((m4 - var^2) / T);
2. the rules of the law: fewer draws are a prefix, shards concatenate, fill="missing" keeps the reliable entries bit for
   bit, a slot of weight zero is never drawn, the top-end rule, an indefinite Psi is counted in n_not_pd, an all -inf lpj
   row in n_bad_weights; the stream against a scalar Python-int restatement.
No GPU: the mirror never touches the engine."""
import numpy as np
import pytest

import _generate_problems as gp
import _posterior_sample_problems as pp
from _predictive_problems import problem
from evo_amd._lib import EvoAmdError
from evo_amd.models import sample_posterior_counter
from evo_amd.models.posterior_sample import PSAMP_PURPOSE, posterior_weights, slots_of_targets

T_STAT = 20000
STAT_CASES = {"es3c": ("es3c", 6, 25, 10, True, 1, False), "ebsc": ("ebsc", 6, 25, 10, False, 1, False)}


def test_the_gpu_shapes_are_those_of_the_predictive_tests():
    from test_gpu_predictive import CASES
    assert [c[:3] for c in pp.CASES] == CASES


def test_purpose_is_its_own():
    assert PSAMP_PURPOSE == int.from_bytes(b"PSAM\0\0\0\0", "big")
    assert len({PSAMP_PURPOSE >> 32, gp.GEN_PURPOSE >> 32, 0x494E4954}) == 3  # (INIT_PURPOSE; the evolve purposes are < 2^32)


@pytest.mark.parametrize("algo", ["es3c", "ebsc"])
def test_frequencies_mean_and_variance(algo):
    p = problem(*STAT_CASES[algo])
    out = pp.draws(STAT_CASES[algo], "all", True, T_STAT)
    ok = ~np.isnan(p.mean).any(axis=1)
    assert out["info"] == {"n_singular": 0, "n_skipped": int((~ok).sum()), "n_not_pd": 0, "n_bad_weights": 0}
    assert (out["slot"][~ok] == -1).all() and (out["slot"][ok] >= 0).all()
    q = pp.q_of(p.lpj)
    f = np.stack([np.bincount(row, minlength=q.shape[1]) for row in out["slot"][ok]]) / float(T_STAT)
    dev = np.abs(f - q[ok]) / np.sqrt(q[ok] * (1.0 - q[ok]) / T_STAT)
    zm, zv = pp.moment_bounds(out["y"], *pp.moments(p))
    print("%s: frequencies %.2f, mean %.2f, variance %.2f standard errors at most" % (algo, dev.max(), zm, zv))
    assert dev.max() <= 6.0
    assert zm <= 6.0
    assert zv <= 6.0


def test_slot_and_s_follow_the_stream():
    """slot against a scalar restatement on Python ints / floats; s is the drawn state."""
    case = ("es3c", 30, 25, 10, True, 0, True)
    p = problem(*case)
    out = pp.draws(case, "missing", True)
    ss = np.array(p.ss)
    ss[:, :, -1] = True  # the background unit
    for n in (0, 3, 29):
        e, c, bad = posterior_weights(p.lpj[n])
        assert not bad
        for t in (0, 1, 63, 64, 69):
            target = gp.rng_u01_int(pp.SEED, n, PSAMP_PURPOSE, t) * c[-1]
            run, want = 0.0, None
            for j in range(e.size):
                run = run + float(e[j])
                if run > target:
                    want = j
                    break
            assert out["slot"][n, t] == want, (n, t)
            assert np.array_equal(out["s"][n, t], ss[n, want])
    assert (out["slot"][5] == -1).all() and not out["s"][5].any() and np.isnan(out["y"][5]).all() and np.isnan(out["z"][5]).all()
    assert out["info"]["n_skipped"] == 1


@pytest.mark.parametrize("case,noise,fill", [(c[0], c[1], c[3]) for c in pp.CASES[3:5] + pp.CASES[7:8]])
def test_prefix_and_shards(case, noise, fill):
    p = problem(*case)
    full = pp.draws(case, fill, noise)
    few = pp.mirror(p, 5, fill, noise)
    a = 11
    lo = pp.mirror(p, pp.T_MAX, fill, noise, rows=slice(0, a))
    hi = pp.mirror(p, pp.T_MAX, fill, noise, rows=slice(a, None), first_index=a)
    for k in full:
        if k == "info":
            assert {i: lo[k][i] + hi[k][i] for i in lo[k]} == full[k] == few[k]
            continue
        assert np.array_equal(few[k], full[k][:, :5], equal_nan=True), k
        assert np.array_equal(np.concatenate((lo[k], hi[k])), full[k], equal_nan=True), k


def test_fill_missing_keeps_the_reliable_entries():
    case = ("es3c", 37, 70, 70, True, 1, False)
    p = problem(*case)
    miss, every = pp.draws(case, "missing", True), pp.draws(case, "all", True)
    ok = p.x_infr.any(axis=1)
    rel = np.broadcast_to((p.x_infr & ok[:, None])[:, None, :], miss["y"].shape)
    assert np.array_equal(miss["y"][rel], np.broadcast_to(p.Y[:, None, :], miss["y"].shape)[rel])  # bit for bit
    other = np.broadcast_to((~p.x_infr & ok[:, None])[:, None, :], miss["y"].shape)
    assert np.array_equal(miss["y"][other], every["y"][other]) and not np.isnan(every["y"][ok]).any()
    for k in ("slot", "s", "z"):
        assert np.array_equal(miss[k], every[k], equal_nan=True)
    # complete data: every entry is reliable
    case = ("ebsc", 37, 25, 70, False, 1, False)
    full = pp.draws(case, "missing", True)
    assert np.array_equal(full["y"], np.broadcast_to(problem(*case).Y[:, None, :], full["y"].shape))


def test_zero_weight_slots_and_the_top_end():
    p = problem("ebsc", 30, 70, 10, True, 0, False)
    lpj = np.array(p.lpj)
    lpj[:, [0, 3]] = -np.inf
    lpj[:, 7] -= 800.0  # exp underflows: weight exactly 0 in the LAST slot, where the top end would fall
    out = pp.mirror(p, 2000, lpj=lpj)
    drawn = out["slot"][out["slot"][:, 0] >= 0]
    assert drawn.size and not np.isin(drawn, (0, 3, 7)).any()
    e, c, bad = posterior_weights(lpj[0])
    assert not bad and e[7] == 0.0 and e[0] == 0.0 and c[-1] == c[6]
    # target = C (u = 1, or rounding): no c_j exceeds it; the rule names the last slot of positive weight
    assert slots_of_targets(e, c, np.array([c[-1], np.nextafter(c[-1], np.inf), np.nextafter(c[-1], 0.0), 0.0])).tolist() == [6, 6, 6, 1]


def test_indefinite_psi_and_bad_weights_are_counted():
    case = ("es3c", 30, 25, 10, False, 1, False)
    p = problem(*case)
    clean = pp.draws(case, "all", True)
    theta = dict(p.theta)
    Psi = np.array(theta["Psi"])
    h = 4
    Psi[h, :] = Psi[:, h] = 0.0
    Psi[h, h] = -0.05  # 1 / Psi_hh = -20 on the diagonal of Lam^-1 = Psi_AA^-1 + G_A / sigma2 (G_hh / sigma2 ~ 3): not PD
    theta["Psi"] = Psi
    lpj = np.array(p.lpj)
    lpj[2] = -np.inf
    lpj[9, 1] = np.nan
    lpj[11, 0] = np.inf
    out = pp.mirror(p, pp.T_MAX, theta=theta, lpj=lpj)
    hit = np.array([(clean["s"][n, :, h]).any() for n in range(p.N)])  # (the slots do not depend on Psi)
    hit[[2, 9, 11]] = False
    assert 0 < hit.sum() < p.N - 3
    assert out["info"] == {"n_singular": 0, "n_skipped": 0, "n_not_pd": int(hit.sum()), "n_bad_weights": 3}
    gone = hit.copy()
    gone[[2, 9, 11]] = True
    assert (out["slot"][gone] == -1).all() and not out["s"][gone].any()
    assert np.isnan(out["y"][gone]).all() and np.isnan(out["z"][gone]).all()
    keep = ~gone
    assert np.array_equal(out["slot"][keep], clean["slot"][keep]) and not np.isnan(out["y"][keep]).any()


def test_more_than_32_active_latents_raise():
    p = problem("es3c", 37, 64, 70, True, 0, False)
    ss = np.array(p.ss)
    ss[1, 2, np.flatnonzero(~ss[1, 2])[0]] = True
    with pytest.raises(EvoAmdError, match=r"n = 1 .*k = 33"):
        sample_posterior_counter("sssc", p.theta, ss, p.lpj, p.Y, p.x_infr)

"""Time the importance-draw estimate of the log-likelihood (Model.estimate_log_likelihood, evoamd_loglik_estimate) at
the north-star shape (ES3C D = 256, H = 512, S = 200, N = 100k) and at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k) on
one MI355X.  Data and Theta as in tools/time_refine.py; the start is the seeded K^n (seed_resident_states) after
``--refine`` iterations of refine_resident_states.  For T = 64, 256, 1024 draws per datapoint:

  wall     host clock around each of ``--repeat`` estimate_log_likelihood calls (each ends in a device synchronise) after
           one warm-up: median (min - max); posterior_scores likewise;
  kernels  a second call with Engine.timing on (HIP events cost stream time: not the call the wall time is from): the
           proposal kernel, the lpj launches over the outside draws and the fold, summed over the passes of the call;
  beside   posterior_scores and a refine iteration of the same run (wall; one refine call of ``--refine`` iterations);
  mirror   estimate_log_likelihood_counter (NumPy, lpj of the draws from the oracle) on the first 30 datapoints,
           extrapolated to N, and the largest |ll - ll_mirror| over those datapoints;
  result   L^ - F (mean gap in nats), the quartiles of ess and of n_outside / T, the mean share of Z^ from outside K^n.

    python tools/time_loglik_estimate.py [--config c4|c5|both] [--n N] [--refine 20] [--draws 64,256,1024] [--repeat 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, SSSC, estimate_log_likelihood_counter  # noqa: E402
from oracle import evo_oracle as orc  # noqa: E402  (the mirror's lpj: the package itself never imports it)
from time_refine import CONFIGS, EA, sparse_theta  # noqa: E402

KERNELS = ("loglik_proposal", "loglik_lpj", "loglik_fold")
N_MIRROR = 30


def oracle_lpj_fn(algo, theta, Y):
    th = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in theta.items()}
    D, H = th["W"].shape
    counters = orc.bsc_precompute(th, D, H) if algo == "ebsc" else orc.sssc_precompute(th, D)

    def fn(n, states):
        out = np.empty(states.shape[0])
        nz = states.any(axis=1)
        zero = orc.bsc_lpj_allzero(th, Y[n], counters) if algo == "ebsc" else orc.sssc_lpj_allzero(th, Y[n], counters)
        out[~nz] = zero[0]
        if nz.any():
            out[nz] = (orc.bsc_lpj(th, states[nz], Y[n], counters) if algo == "ebsc"
                       else orc.sssc_lpj(th, states[nz], Y[n], counters, {}))
        return out

    return fn


def quartiles(a):
    return "%.3g / %.3g / %.3g" % tuple(np.percentile(a, (25, 50, 75)))


def run(name, args):
    algo, D, H, S, N = CONFIGS[name]
    N = args.n or N
    rng = np.random.RandomState(0)
    theta = sparse_theta(rng, algo, D, H)
    cls = BSC if algo == "ebsc" else SSSC
    model = cls(D, H, S, rng="device", sync_host=False, seed=1)
    theta = model.check_params(theta)
    Y = model.generate_data_device(theta, N, seed=7, keep=("y",))["y"]
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    eng = model.engine
    tag = "%s %s D=%d H=%d S=%d N=%d Cmax=%d" % (name, algo, D, H, S, N, EA[2] * EA[3] * EA[4])
    suff = model.seed_resident_states(dict(theta), my_data, *EA)
    model.refine_resident_states(dict(theta), suff, my_data, 2)  # warm-up
    eng.synchronize()
    t0 = time.perf_counter()
    res = model.refine_resident_states(dict(theta), suff, my_data, args.refine)
    ms_refine = (time.perf_counter() - t0) * 1e3 / max(1, args.refine)
    model.posterior_scores(theta, suff, my_data)  # warm-up
    t_scores = []
    for _ in range(args.repeat):
        eng.synchronize()
        t0 = time.perf_counter()
        scores = model.posterior_scores(theta, suff, my_data)
        t_scores.append((time.perf_counter() - t0) * 1e3)
    ms_scores = float(np.median(t_scores))
    print("start %s: F after %d refine iterations %.4f; refine %.3f ms per iteration (one call of %d), posterior_scores "
          "%.3f ms per call (median of %d, %.3f - %.3f)" % (tag, args.refine, res.F[-1], ms_refine, args.refine, ms_scores,
                                                            args.repeat, min(t_scores), max(t_scores)), flush=True)
    model.estimate_log_likelihood(theta, suff, my_data, n_samples=16, seed=1)  # warm-up: code objects, buffers
    states = lpj = None
    for T in args.draws:
        walls = []
        for _ in range(args.repeat):
            eng.synchronize()
            t0 = time.perf_counter()
            L, info = model.estimate_log_likelihood(theta, suff, my_data, n_samples=T, seed=1, per_datapoint=True)
            walls.append((time.perf_counter() - t0) * 1e3)
        ms = float(np.median(walls))
        eng.timing(KERNELS)
        eng.timing_reset()
        model.estimate_log_likelihood(theta, suff, my_data, n_samples=T, seed=1)
        parts = []
        for k in KERNELS:
            avg, n = eng.kernel_time_ms(k)
            parts.append("%s %.3f ms (%d spans)" % (k, avg * n, n))
        eng.timing(False)
        print("T=%d %s: wall %.2f ms per call (median of %d, %.2f - %.2f; %.1f x a refine iteration, %.1f x posterior_scores); "
              "%s" % (T, tag, ms, args.repeat, min(walls), max(walls), ms / ms_refine, ms / ms_scores, "; ".join(parts)),
              flush=True)
        print("T=%d %s: L^ - F = %.4f nats (F %.4f); ess quartiles %s; n_outside / T quartiles %s; mean mass outside %.4f; "
              "no estimate for %d datapoints" % (T, tag, np.nanmean(info["gap"]), np.nanmean(scores["F"]), quartiles(info["ess"]),
                                                 quartiles(info["n_outside"] / T), np.nanmean(info["mass_outside"]),
                                                 info["n_bad_weights"] + info["n_skipped"]), flush=True)
        if args.mirror:
            m = min(N_MIRROR, N)
            if states is None:  # (bit-packed rows of the first datapoints only: K^n as bool is 10 GB at c4)
                states = np.unpackbits(eng.download_states_packed(0, m), axis=-1)[..., :H].astype(bool)
                lpj = eng.download_lpj()[:m]
            t0 = time.perf_counter()
            ref = estimate_log_likelihood_counter("bsc" if algo == "ebsc" else "sssc", theta, states[:m], lpj[:m],
                                                  oracle_lpj_fn(algo, theta, Y), n_samples=T, seed=model.last_estimate_seed)
            s_m = time.perf_counter() - t0
            print("T=%d %s: mirror %.2f s for %d datapoints = %.0f s for N (%.0f x the call); max |ll - ll_mirror| %.3g, "
                  "n_outside equal: %s" % (T, tag, s_m, m, s_m * N / m, s_m * N / m / (ms * 1e-3),
                                           np.abs(info["ll"][:m] - ref["ll"]).max(),
                                           np.array_equal(info["n_outside"][:m], ref["n_outside"])), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--refine", type=int, default=20)
    ap.add_argument("--draws", default="64,256,1024")
    ap.add_argument("--repeat", type=int, default=5, help="timed calls per figure (median, min - max)")
    ap.add_argument("--no-mirror", dest="mirror", action="store_false")
    args = ap.parse_args()
    args.draws = [int(t) for t in args.draws.split(",")]
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

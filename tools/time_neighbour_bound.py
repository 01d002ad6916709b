"""Time the neighbourhood bound (Model.neighbourhood_bound, evoamd_neighbour_bound) and read its tightness at the north-star
shape (ES3C D = 256, H = 512, S = 200, N = 100k) and at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k) on one MI355X.  Data and
Theta as in tools/time_refine.py; the start is the seeded K^n (seed_resident_states) after ``--refine`` iterations of
refine_resident_states.  For P = 1, 8 and S parents per datapoint:

  wall     host clock around each of ``--repeat`` neighbourhood_bound calls (each ends in a device synchronise) after one
           warm-up: median (min - max);
  kernel   one more call with Engine.timing on (HIP events cost stream time: not the call the wall time is from): the span
           "neighbour_bound" -- the neighbourhood kernel, ES3C with the transpose of GP, and the bound of the rows;
  result   F (ljc + mean F_n), L+ - F in nats, the quartiles of gap, how many datapoints gain more than 0.01 nats and the
           largest gap, the quartiles of n_states, the datapoints with a capped parent.

Beside that, from the same K^n in the same run, estimate_log_likelihood at T = 256 draws: wall (median of ``--repeat``),
L^ - F and the quartiles of ess -- the yardstick for both time and tightness.  ``--missing FRACTION`` (default 0: complete
data only): the same on data with an i.i.d. mask hiding that fraction of the entries, in the same run on the same engine.

    python tools/time_neighbour_bound.py [--config c4|c5|both] [--n N] [--refine 20] [--repeat 5] [--missing 0.5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, SSSC  # noqa: E402
from time_refine import CONFIGS, EA, sparse_theta  # noqa: E402

T_DRAWS = 256


def quartiles(a):
    return "%.3g / %.3g / %.3g" % tuple(np.nanpercentile(a, (25, 50, 75)))


def timed(eng, repeat, call):
    call()  # warm-up: code objects, buffers
    walls, out = [], None
    for _ in range(repeat):
        eng.synchronize()
        t0 = time.perf_counter()
        out = call()
        walls.append((time.perf_counter() - t0) * 1e3)
    return "%.2f ms per call (median of %d, %.2f - %.2f)" % (float(np.median(walls)), repeat, min(walls), max(walls)), out


def measure(args, cls, eng, S, theta, my_data, incomplete, tag):
    (N, D), H = my_data["y"].shape, theta["W"].shape[1]
    model = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
    theta = model.check_params(dict(theta))
    suff = model.seed_resident_states(dict(theta), my_data, *EA, incomplete=incomplete)
    res = model.refine_resident_states(dict(theta), suff, my_data, args.refine)
    print("start %s: F after %d refine iterations %.4f" % (tag, args.refine, res.F[-1]), flush=True)
    for P in (1, 8, S):
        wall, (L, info) = timed(eng, args.repeat, lambda: model.neighbourhood_bound(
            theta, suff, my_data, n_parents=P, per_datapoint=True, incomplete=incomplete))
        eng.timing(("neighbour_bound",))
        eng.timing_reset()
        model.neighbourhood_bound(theta, suff, my_data, n_parents=P, incomplete=incomplete)
        avg, n = eng.kernel_time_ms("neighbour_bound")
        eng.timing(False)
        F = L - np.nanmean(info["gap"])
        print("P=%d %s: wall %s; span neighbour_bound %.3f ms (%d spans)" % (P, tag, wall, avg * n, n), flush=True)
        print("P=%d %s: F %.4f, L+ - F = %.4f nats; gap quartiles %s, above 0.01 nats at %d datapoints, largest %.4g; n_states "
              "quartiles %s; datapoints with a capped parent %d; no estimate for %d datapoints" % (
                  P, tag, F, L - F, quartiles(info["gap"]), int((info["gap"] > 0.01).sum()), np.nanmax(info["gap"]),
                  quartiles(info["n_states"]), int((info["n_capped"] > 0).sum()), info["n_bad_weights"]), flush=True)
    wall, (L, info) = timed(eng, args.repeat, lambda: model.estimate_log_likelihood(
        theta, suff, my_data, n_samples=T_DRAWS, seed=1, per_datapoint=True))
    print("T=%d %s: estimate_log_likelihood wall %s; L^ - F = %.4f nats; ess quartiles %s" % (
        T_DRAWS, tag, wall, np.nanmean(info["gap"]), quartiles(info["ess"])), flush=True)


def run(name, args):
    algo, D, H, S, N = CONFIGS[name]
    N = args.n or N
    rng = np.random.RandomState(0)
    theta = sparse_theta(rng, algo, D, H)
    cls = BSC if algo == "ebsc" else SSSC
    first = cls(D, H, S, rng="device", sync_host=False, seed=1)
    theta = first.check_params(theta)
    Y = first.generate_data_device(theta, N, seed=7, keep=("y",))["y"]
    eng = first.engine
    measure(args, cls, eng, S, theta, {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}, False,
            "%s %s D=%d H=%d S=%d N=%d" % (name, algo, D, H, S, N))
    if args.missing > 0:  # the same run, the same engine: the masked calls beside the complete ones
        x_infr = np.random.RandomState(11).random_sample(Y.shape) >= args.missing
        measure(args, cls, eng, S, theta, {"y": np.where(x_infr, Y, np.nan), "x_infr": x_infr, "x": x_infr.copy()}, True,
                "%s %s D=%d H=%d S=%d N=%d missing=%.2f" % (name, algo, D, H, S, N, args.missing))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--refine", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls per figure (median, min - max)")
    ap.add_argument("--missing", type=float, default=0.0, help="fraction of entries hidden by an i.i.d. mask (0: complete data)")
    args = ap.parse_args()
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

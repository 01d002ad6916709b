"""Time annealed importance sampling (Model.ais_log_likelihood, evoamd_ais_loglik) at c5 (EBSC D = 256, H = 1024, S = 256)
on one MI355X and print the bracket it gives around the log-likelihood.  Data are drawn from a sparse Theta (pi H = 3,
tools/time_refine.py) with generate_data_device and their s is kept: the exact posterior sample the reverse chains start
from.  The start of K^n is the seeded one (seed_resident_states) after ``--refine`` iterations of refine_resident_states,
as in tools/time_loglik_estimate.py.  For T = 32, 128, 512 temperatures and C = ``--chains`` chains, each figure the median
of ``--repeat`` calls with (min - max):

  wall     host clock around a forward and around a reverse call (each ends in a device synchronise) after one warm-up;
  kernel   the "ais" span (chain kernel + fold) of a further call with Engine.timing on;
  result   L_lower, L_upper and their difference (seed r of the r-th repeat: the spread is the estimator's), the quartiles
           of ess in both directions, flips per chain and temperature;
  beside   F (posterior_scores), L^ of estimate_log_likelihood (T = 256 draws) in the same run: L_lower - F next to L^ - F;
  admit    once, at the largest T: F before and after admit=True and S_sub;
  masked   with ``--missing F[,F]``: the same forward and reverse calls with that share of the entries hidden (i.i.d. mask,
           NaN under False, incomplete=True; K^n seeded and swept on the incomplete data, for F alone) beside the complete
           calls of this run: wall, the "ais" span of ``--repeat`` calls, their ratio, n_flips per chain, the bracket width.

    python tools/time_ais.py [--n-data 20000] [--refine 20] [--temps 32,128,512] [--chains 16] [--repeat 5] [--missing 0.5,0.1]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC  # noqa: E402
from time_refine import CONFIGS, EA, sparse_theta  # noqa: E402


def quartiles(a):
    return "%.3g / %.3g / %.3g" % tuple(np.percentile(a, (25, 50, 75)))


def mmm(v):
    return "%.4f (%.4f - %.4f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-data", type=int, default=20000)
    ap.add_argument("--refine", type=int, default=20)
    ap.add_argument("--temps", default="32,128,512")
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls per figure (median, min - max)")
    ap.add_argument("--missing", default="", help="fractions of hidden entries, e.g. 0.5,0.1: the masked calls (incomplete=True) "
                                                  "beside the complete calls of the same run")
    args = ap.parse_args()
    args.missing = [float(f) for f in args.missing.split(",") if f]
    temps = [int(t) for t in args.temps.split(",")]
    algo, D, H, S, _ = CONFIGS["c5"]
    N, C = args.n_data, args.chains
    rng = np.random.RandomState(0)
    model = BSC(D, H, S, rng="device", sync_host=False, seed=1)
    theta = model.check_params(sparse_theta(rng, algo, D, H))
    gen = model.generate_data_device(theta, N, seed=7, keep=("y", "s"))
    Y, s_true = gen["y"], gen["s"]
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    eng = model.engine
    tag = "c5 ebsc D=%d H=%d S=%d N=%d C=%d" % (D, H, S, N, C)
    suff = model.seed_resident_states(dict(theta), my_data, *EA)
    res = model.refine_resident_states(dict(theta), suff, my_data, args.refine)
    scores = model.posterior_scores(theta, suff, my_data)
    F = float(res.F[-1])
    model.estimate_log_likelihood(theta, suff, my_data, n_samples=16, seed=1)  # warm-up
    L_hat, est = [], None
    for r in range(args.repeat):
        L, est = model.estimate_log_likelihood(theta, suff, my_data, n_samples=256, seed=1 + r, per_datapoint=True)
        L_hat.append(L)
    print("start %s: F after %d refine iterations %.4f (mean F_n %.4f); estimate_log_likelihood T=256: L^ %s, L^ - F %.4f, "
          "ess quartiles %s" % (tag, args.refine, F, float(np.mean(scores["F"])), mmm(L_hat), float(np.median(L_hat)) - F,
                                quartiles(est["ess"])), flush=True)
    model.ais_log_likelihood(theta, suff, my_data, n_chains=2, n_temps=4, seed=1)  # warm-up: code objects, buffers
    model.ais_log_likelihood(theta, suff, my_data, n_chains=2, n_temps=4, seed=1, direction="reverse", s_start=s_true)
    complete = {}  # T -> direction -> (median wall, the spans of --repeat further calls): what --missing is held against
    for T in temps:
        complete[T] = {}
        rows = {"forward": ([], [], None), "reverse": ([], [], None)}
        for direction in ("forward", "reverse"):
            walls, Ls, info = [], [], None
            for r in range(args.repeat):
                eng.synchronize()
                t0 = time.perf_counter()
                L, info = model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1 + r, direction=direction,
                                                   s_start=s_true if direction == "reverse" else None, per_datapoint=True)
                walls.append((time.perf_counter() - t0) * 1e3)
                Ls.append(L)
            spans = []
            for r in range(args.repeat):
                eng.timing(("ais",))
                eng.timing_reset()
                model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1 + r, direction=direction,
                                         s_start=s_true if direction == "reverse" else None)
                span, n_spans = eng.kernel_time_ms("ais")
                spans.append(span * n_spans)
                eng.timing(False)
            rows[direction] = (walls, Ls, info)
            complete[T][direction] = (float(np.median(walls)), spans)
            print("T=%d %s %s: wall %s ms per call (median of %d), kernel span %s ms; ess quartiles %s; flips per chain and "
                  "temperature %.3f, per chain %.3f" % (T, direction, tag, mmm(walls), args.repeat, mmm(spans), quartiles(info["ess"]),
                                                        info["n_flips"].mean() / (C * T), info["n_flips"].mean() / C), flush=True)
        lo, up = rows["forward"][1], rows["reverse"][1]
        gap = [u - l for u, l in zip(up, lo)]
        print("T=%d %s: L_lower %s, L_upper %s, L_upper - L_lower %s; L_lower - F %.4f beside L^ - F %.4f" % (
            T, tag, mmm(lo), mmm(up), mmm(gap), float(np.median(lo)) - F, float(np.median(L_hat)) - F), flush=True)
    T = temps[-1]
    L, info = model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1, admit=True)
    after = model.posterior_scores(theta, suff, my_data)
    print("admit T=%d %s: mean F_n before %.4f, after %.4f (posterior_scores after: %.4f), S_sub %.4f, datapoints improved %d "
          "of %d" % (T, tag, float(info["F_before"].mean()), float(info["F_after"].mean()), float(np.mean(after["F"])),
                     info["S_sub"], int((info["F_after"] > info["F_before"]).sum()), N), flush=True)
    for missing in args.missing:
        masked(args, temps, theta, Y, s_true, missing, complete, tag)
    eng.close()


def masked(args, temps, theta, Y, s_true, missing, complete, tag):
    """The same calls with ``missing`` of the entries hidden (an i.i.d. mask, NaN under False) and incomplete=True, on a
    model of its own, beside the complete figures of this run (``complete``: T -> direction -> (wall, span))."""
    algo, D, H, S, _ = CONFIGS["c5"]
    N, C = args.n_data, args.chains
    x_infr = np.random.RandomState(11).random_sample(Y.shape) >= missing
    my_data = {"y": np.where(x_infr, Y, np.nan), "x_infr": x_infr, "x": x_infr.copy()}
    model = BSC(D, H, S, rng="device", sync_host=False, seed=1)
    eng = model.engine
    suff = model.seed_resident_states(dict(theta), my_data, *EA, incomplete=True)
    sweep = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=8, incomplete=True)
    F = float(model.posterior_scores(theta, suff, my_data)["F"].mean())
    tag = "%s missing=%.2f" % (tag, missing)
    print("masked start %s: mean F_n of the seeded and swept K^n %.4f (%d sweeps ran)" % (tag, F, sweep.n_done), flush=True)
    kw = dict(incomplete=True)
    model.ais_log_likelihood(theta, suff, my_data, n_chains=2, n_temps=4, seed=1, **kw)  # warm-up: code objects, buffers
    model.ais_log_likelihood(theta, suff, my_data, n_chains=2, n_temps=4, seed=1, direction="reverse", s_start=s_true, **kw)
    for T in temps:
        Ls = {}
        for direction in ("forward", "reverse"):
            start = s_true if direction == "reverse" else None
            walls, Ls[direction], info = [], [], None
            for r in range(args.repeat):
                eng.synchronize()
                t0 = time.perf_counter()
                L, info = model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1 + r, direction=direction,
                                                   s_start=start, per_datapoint=True, **kw)
                walls.append((time.perf_counter() - t0) * 1e3)
                Ls[direction].append(L)
            spans = []
            for r in range(args.repeat):
                eng.timing(("ais",))
                eng.timing_reset()
                model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1 + r, direction=direction, s_start=start,
                                         **kw)
                ms, n = eng.kernel_time_ms("ais")
                spans.append(ms * n)
                eng.timing(False)
            wall_c, span_c = complete[T][direction]
            print("masked T=%d %s %s: wall %s ms per call, kernel span %s ms; complete call of this run: wall %.4f ms, span %s ms; "
                  "span ratio %.2f; ess quartiles %s; n_flips per chain %.3f" % (
                      T, direction, tag, mmm(walls), mmm(spans), wall_c, mmm(span_c), float(np.median(spans)) / float(np.median(span_c)),
                      quartiles(info["ess"]), info["n_flips"].mean() / C), flush=True)
        gap = [u - l for u, l in zip(Ls["reverse"], Ls["forward"])]
        print("masked T=%d %s: L_lower %s, L_upper %s, L_upper - L_lower %s; L_lower - (ljc + mean F_n) %.4f" % (
            T, tag, mmm(Ls["forward"]), mmm(Ls["reverse"]), mmm(gap), float(np.median(Ls["forward"])) - (eng.ljc + F)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()

"""Time the log predictive score (Model.predictive_log_score, evoamd_predictive_score) and read what it says about a seeded
K^n at the north-star shape (ES3C D = 256, H = 512, S = 200, N = 100k) and at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k) on
one MI355X.  Data (Model.generate_data_device) and Theta as in tools/time_refine.py.  Three masks per shape: an i.i.d. mask
hiding 10 % and 50 % of the entries, and one hiding 50 % of the entries of 10 % of the datapoints (the others keep all
of theirs and are not visited).  K^n is seeded on the reliable entries (seed_resident_states, incomplete=True) and swept
4 times (sweep_resident_states); the hidden entries are scored at their true values.

  wall     host clock around each of ``--repeat`` predictive_log_score calls (per_entry=False; each ends synchronised; the
           upload of y_true and of the query is inside) after one warm-up: median (min - max); one per_entry=True call
           beside it (it downloads logp and pit, 16 N D bytes);
  kernel   one more call with Engine.timing on: the span "predictive_score" (transpose, score kernel, the reductions);
  yardstick  predictive_moments in the same run on the same K^n: wall of the call (it downloads mean and var) and the
           span "misc" of its kernels;
  host     the NumPy mirror (evo_amd.models.predictive_log_score_host) on the first ``--host-n`` datapoints on one core,
           scaled to N and labelled as extrapolated; the device's logp_n of the slice is compared with it;
  result   the score, the score of the moment-matched Gaussian N(mean, var) of predictive_moments at the same entries,
           and pit_summary (coverage of the central 50 % and 90 % intervals, KS distance to uniform).

    python tools/time_predictive_score.py [--config c4|c5|both] [--n N] [--repeat 5] [--host-n 30] [--sweeps 4]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, SSSC, pit_summary, predictive_log_score_host  # noqa: E402
from time_refine import CONFIGS, EA, sparse_theta  # noqa: E402


def timed(eng, repeat, call):
    call()  # warm-up: code objects, buffers
    walls, out = [], None
    for _ in range(repeat):
        eng.synchronize()
        t0 = time.perf_counter()
        out = call()
        walls.append((time.perf_counter() - t0) * 1e3)
    return "%.2f ms per call (median of %d, %.2f - %.2f)" % (float(np.median(walls)), repeat, min(walls), max(walls)), out


def span(eng, name, call):
    eng.timing((name,))
    eng.timing_reset()
    call()
    avg, n = eng.kernel_time_ms(name)
    eng.timing(False)
    return avg * n, n


def masks(shape, rng):
    yield "10 % of the entries hidden", rng.random_sample(shape) >= 0.1
    yield "50 % of the entries hidden", rng.random_sample(shape) >= 0.5
    rows = rng.random_sample(shape[0]) < 0.1
    yield "50 % of the entries of 10 % of the datapoints hidden", (rng.random_sample(shape) >= 0.5) | ~rows[:, None]


def measure(args, cls, eng, algo, S, theta, Y, x_infr, tag):
    (N, D), H = Y.shape, theta["W"].shape[1]
    x_infr[~x_infr.any(axis=1), 0] = True  # every datapoint keeps a reliable entry
    my_data = {"y": np.where(x_infr, Y, np.nan), "x_infr": x_infr, "x": x_infr.copy()}
    model = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
    theta = model.check_params(dict(theta))
    suff = model.seed_resident_states(dict(theta), my_data, *EA, incomplete=True)
    model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=args.sweeps, incomplete=True)
    hidden = ~x_infr
    print("%s: %d entries scored in %d of %d datapoints" % (tag, hidden.sum(), hidden.any(axis=1).sum(), N), flush=True)
    wall, (score, info) = timed(eng, args.repeat, lambda: model.predictive_log_score(theta, suff, my_data, Y))
    ms, n = span(eng, "predictive_score", lambda: model.predictive_log_score(theta, suff, my_data, Y))
    print("%s: predictive_log_score wall %s; span predictive_score %.3f ms (%d spans)" % (tag, wall, ms, n), flush=True)
    t0 = time.perf_counter()
    score_e, info_e = model.predictive_log_score(theta, suff, my_data, Y, per_entry=True)
    print("%s: predictive_log_score with per_entry=True, one call: %.2f ms; same score bits: %s"
          % (tag, (time.perf_counter() - t0) * 1e3, score_e == score), flush=True)
    wall_m, (mean, var, minfo) = timed(eng, args.repeat, lambda: model.predictive_moments(theta, suff, my_data))
    ms_m, n_m = span(eng, "misc", lambda: model.predictive_moments(theta, suff, my_data))
    print("%s: predictive_moments (the yardstick, same run) wall %s; span misc %.3f ms (%d spans)" % (tag, wall_m, ms_m, n_m),
          flush=True)
    ok = hidden & ~np.isnan(info_e["logp"])
    gauss = float((-0.5 * (np.log(2.0 * np.pi * var[ok]) + (Y[ok] - mean[ok]) ** 2 / var[ok])).mean())
    summ = pit_summary(info_e["pit"])
    print("%s: score %.4f nats per entry over %d entries (moment-matched Gaussian of predictive_moments: %.4f); PIT coverage "
          "of the central 50 %% / 90 %% intervals %.3f / %.3f, KS distance %.4f (0.1 %% critical value %.4f); counters: "
          "n_singular %d, n_skipped %d, n_not_queried %d, n_bad_values %d"
          % (tag, score, int(info["count"].sum()), gauss, summ["coverage"][0.5], summ["coverage"][0.9], summ["ks"],
             1.95 / np.sqrt(max(1, summ["n"])), info["n_singular"], info["n_skipped"], info["n_not_queried"],
             info["n_bad_values"]), flush=True)
    if args.host_n > 0:
        n = min(args.host_n, N)
        ss = np.unpackbits(eng.download_states_packed(0, n), axis=-1)[..., :H].astype(bool)
        lpj = eng.download_lpj()[:n]
        t0 = time.perf_counter()
        _, hinfo = predictive_log_score_host("bsc" if algo == "ebsc" else "sssc", theta, ss, lpj, my_data["y"][:n], Y[:n],
                                             hidden[:n], x_infr[:n], S_perm=lpj.shape[1] - S)
        dt = time.perf_counter() - t0
        visited = max(1, int(hidden[:n].any(axis=1).sum()))
        print("%s: host mirror on one core: %.2f s for %d datapoints (%d visited); extrapolated to the %d visited of N=%d: %.0f s; "
              "device against the mirror on the slice: max |logp_n| diff %.3g"
              % (tag, dt, n, visited, hidden.any(axis=1).sum(), N, dt * hidden.any(axis=1).sum() / visited,
                 np.abs(hinfo["logp_n"] - info["logp_n"][:n]).max()), flush=True)


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
    for what, x_infr in masks(Y.shape, np.random.RandomState(11)):
        measure(args, cls, eng, algo, S, theta, Y, x_infr, "%s %s D=%d H=%d S=%d N=%d, %s" % (name, algo, D, H, S, N, what))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--repeat", type=int, default=5, help="timed calls per figure (median, min - max)")
    ap.add_argument("--host-n", type=int, default=30, help="datapoints of the NumPy mirror (0: none)")
    ap.add_argument("--sweeps", type=int, default=4)
    args = ap.parse_args()
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

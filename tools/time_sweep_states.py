"""Time the local search on K^n (Model.sweep_resident_states, evoamd_sweep_states) from the seeded start beside
Model.refine_resident_states over the same wall time, at the north-star shape (ES3C D = 256, H = 512, S = 200, N = 100k) and
at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k) on one MI355X.  Data and Theta as tools/time_refine.py; the start is the
seeded K^n (seed_resident_states is deterministic: every route re-seeds and so starts from the same states).

  wall    host clock around one sweep_resident_states call of ``--sweeps`` sweeps (stop_when_quiet off, one warm-up call
          first), ms per sweep, median (min - max) of ``--repeats`` calls from the same start; the proposal kernel's own
          time from a further run with Engine.timing on the class "sweep";
  F       the free energy before and after each sweep;
  refine  refine_resident_states is run with growing iteration counts until one call takes at least the sweeps' wall
          time: its iterations, wall time and F -- the yardstick, untouched by the sweep;
  L^ - F  estimate_log_likelihood's L^ - F and mean ess at the seeded start and after the sweeps (same seed).

``--missing FRACTION`` (default 0: all of the above on complete data, nothing else): an i.i.d. mask hides that fraction of
the entries (NaN in the data); after the complete measurement the same lines are printed for the masked data
(seed_resident_states and sweep_resident_states with incomplete=True: evoamd_sweep_states_ex, EVOAMD_SWEEP_INCOMPLETE), in
the same run on the same engine, with refine_resident_states on the masked data as the yardstick.

``--neighbourhood flip|swap|both`` (default flip: the lines above, nothing else; several may be named): the wall, F and
L^ - F lines once per neighbourhood in the same run, in the order given, with the class times "sweep" and "sweep_swap" and the
counts of gain <= 0 and swap_gain <= 0; the refine yardstick runs over the slowest route's wall time.  Complete data only
(swaps on incomplete data are refused).  ``--alternate``: for comparison, flips until quiet, then swaps until quiet,
repeated until a round of both swaps nothing (at most ``--sweeps`` sweeps per stage and 16 rounds), from the same start.

    python tools/time_sweep_states.py [--config c4|c5|both] [--n N] [--sweeps 4] [--parents 1] [--repeats 5] [--missing 0.5]
                                      [--neighbourhood flip swap both] [--alternate]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, SSSC  # noqa: E402
from time_refine import CONFIGS, EA, sparse_theta  # noqa: E402


def run(name, args):
    algo, D, H, S, N = CONFIGS[name]
    N = args.n or N
    rng = np.random.RandomState(0)
    theta = sparse_theta(rng, algo, D, H)
    cls = BSC if algo == "ebsc" else SSSC
    first = cls(D, H, S, rng="device", sync_host=False, seed=1)
    Y = first.generate_data_device(theta, N, seed=7, keep=("y",))["y"]
    eng = first.engine
    measure(args, cls, eng, S, theta, {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}, False,
            "%s %s D=%d H=%d S=%d N=%d" % (name, algo, D, H, S, N), algo)
    if args.missing > 0:  # the same run, the same engine: the masked calls beside the complete ones
        x_infr = np.random.RandomState(11).random_sample(Y.shape) >= args.missing
        measure(args, cls, eng, S, theta, {"y": np.where(x_infr, Y, np.nan), "x_infr": x_infr, "x": x_infr.copy()},
                True,
                "%s %s D=%d H=%d S=%d N=%d missing=%.2f" % (name, algo, D, H, S, N, args.missing), algo)
    eng.close()


def measure(args, cls, eng, S, theta, my_data, incomplete, tag, algo):
    (N, D), H = my_data["y"].shape, theta["W"].shape[1]
    T, P = args.sweeps, args.parents

    def seeded():
        model = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
        return model, model.seed_resident_states(dict(theta), my_data, *EA, incomplete=incomplete)

    def bound(model, suff):
        th = dict(theta)
        model.E_step_precompute(th, dict(suff), my_data)
        return th["ljc"] + model.posterior_scores(theta, suff, my_data)["F"].mean()

    def tightness(model, suff):
        L, info = model.estimate_log_likelihood(dict(theta), suff, my_data, n_samples=256, seed=11, per_datapoint=True)
        return L - bound(model, suff), float(np.nanmean(info["ess"]))

    def sweep_route(sweeps, timed_class=False, nb="flip"):
        model, suff = seeded()
        before = bound(model, suff)
        if timed_class:
            eng.timing(("sweep",))
            eng.timing_reset()
        eng.synchronize()
        t0 = time.perf_counter()
        kw = {} if nb == "flip" else {"neighbourhood": nb}
        res = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=sweeps, n_parents=P, stop_when_quiet=False,
                                          incomplete=incomplete, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        kernel = eng.kernel_time_ms("sweep") if timed_class else None
        if timed_class:
            eng.timing(False)
        return ms, before, res, model, suff, kernel

    def alternate_route():
        """flips until quiet, then swaps until quiet, repeated until a round of both swaps nothing"""
        model, suff = seeded()
        before = bound(model, suff)
        eng.synchronize()
        t0 = time.perf_counter()
        n_flip = n_swap = rounds = 0
        F = before
        while rounds < 16:
            a = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=T, n_parents=P, stop_when_quiet=True)
            b = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=T, n_parents=P, stop_when_quiet=True,
                                            neighbourhood="swap")
            n_flip, n_swap, rounds, F = n_flip + a.n_done, n_swap + b.n_done, rounds + 1, b.F[-1]
            if a.S_sub.sum() + b.S_sub.sum() == 0.0:
                break
        ms = (time.perf_counter() - t0) * 1e3
        last = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=1, n_parents=P, neighbourhood="both")
        return ms, before, F, n_flip, n_swap, rounds, last, model, suff

    def refine_route(iters):
        model, suff = seeded()
        eng.synchronize()
        t0 = time.perf_counter()
        res = model.refine_resident_states(dict(theta), suff, my_data, iters)
        return (time.perf_counter() - t0) * 1e3, res.F

    nbs = ["flip"] if incomplete else list(args.neighbourhood)
    if nbs == ["flip"] and not (args.alternate and not incomplete):
        measure_flip(args, tag, algo, N, T, P, sweep_route, refine_route, seeded, tightness)
        return
    sweep_route(1)  # warm-up: code objects, buffers
    for nb in nbs:
        sweep_route(1, nb=nb)
    refine_route(2)
    model, suff = seeded()
    gap0, ess0 = tightness(model, suff)
    slowest, F_best = 0.0, -np.inf
    for nb in nbs:
        walls = []
        for _ in range(args.repeats):
            ms, before, res, model, suff, _ = sweep_route(T, nb=nb)
            walls.append(ms)
        gap1, ess1 = tightness(model, suff)
        ms = float(np.median(walls))
        slowest, F_best = max(slowest, ms), max(F_best, res.F[-1])
        eng.timing(("sweep", "sweep_swap"))
        eng.timing_reset()
        model, suff = seeded()
        kw = {} if nb == "flip" else {"neighbourhood": nb}
        model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=T, n_parents=P, stop_when_quiet=False, **kw)
        (kf_ms, kf_n), (ks_ms, ks_n) = eng.kernel_time_ms("sweep"), eng.kernel_time_ms("sweep_swap")
        eng.timing(False)
        print("wall %s %s: sweep_resident_states %.3f ms per sweep (%d sweeps, n_parents %d, one call; median of %d calls, "
              "%.3f - %.3f); class sweep %.3f ms per span (%d spans%s), class sweep_swap %.3f ms per span (%d spans), events on"
              % (tag, nb, ms / T, T, P, len(walls), min(walls) / T, max(walls) / T, kf_ms, kf_n,
                 "; one of them the transpose of GP" if algo == "es3c" else "", ks_ms, ks_n), flush=True)
        counts = ""
        if res.gain is not None:
            counts += "; gain <= 0: %d of %d" % (int((res.gain <= 0).sum()), N)
        if res.swap_gain is not None:
            counts += "; swap_gain <= 0: %d of %d, parents above the cap %d" % (int((res.swap_gain <= 0).sum()), N,
                                                                                int(res.n_capped_swap.sum()))
        print("F %s %s: seeded %.4f; after each sweep %s; swapped per datapoint %s%s"
              % (tag, nb, before, " ".join("%.4f" % f for f in res.F), " ".join("%.3f" % s for s in res.S_sub), counts),
              flush=True)
        print("L^ - F %s %s (256 draws): seeded %.4f nats (mean ess %.2f); after %d sweeps %.4f nats (mean ess %.2f)"
              % (tag, nb, gap0, ess0, T, gap1, ess1), flush=True)
    if args.alternate:
        alternate_route()  # warm-up
        ms_a, before, F_a, n_flip, n_swap, rounds, last, model, suff = alternate_route()
        gap1, ess1 = tightness(model, suff)
        slowest, F_best = max(slowest, ms_a), max(F_best, F_a)
        print("alternate %s: flips until quiet, then swaps until quiet: %d rounds, %d flip and %d swap sweeps, %.3f ms in all; F "
              "seeded %.4f, at the end %.4f; gain <= 0: %d, swap_gain <= 0: %d of %d; L^ - F %.4f nats (mean ess %.2f)"
              % (tag, rounds, n_flip, n_swap, ms_a, before, F_a, int((last.gain <= 0).sum()), int((last.swap_gain <= 0).sum()),
                 N, gap1, ess1), flush=True)
    iters, ms_r, F_r = 1, 0.0, None
    while True:
        ms_r, F_r = refine_route(iters)
        if ms_r >= slowest or iters >= 4096:
            break
        iters = max(iters + 1, int(iters * min(4.0, 1.2 * slowest / max(ms_r, 1e-3))))
    print("refine %s: refine_resident_states needs %d iterations for the slowest route's wall time (%.3f ms against %.3f ms): "
          "F %.4f against the routes' best %.4f" % (tag, iters, ms_r, slowest, F_r[-1], F_best), flush=True)


def measure_flip(args, tag, algo, N, T, P, sweep_route, refine_route, seeded, tightness):
    """The one-flip lines alone (the default)."""
    sweep_route(1)  # warm-up: code objects, buffers
    refine_route(2)
    model, suff = seeded()
    gap0, ess0 = tightness(model, suff)
    walls = []
    for _ in range(args.repeats):
        ms, before, res, model, suff, _ = sweep_route(T)
        walls.append(ms)
    gap1, ess1 = tightness(model, suff)
    ms = float(np.median(walls))
    _, _, _, _, _, (k_ms, k_n) = sweep_route(T, timed_class=True)
    print("wall %s: sweep_resident_states %.3f ms per sweep (%d sweeps, n_parents %d, one call; median of %d calls, %.3f - "
          "%.3f); proposal kernel class %.3f ms per span (%d spans, events on%s)"
          % (tag, ms / T, T, P, len(walls), min(walls) / T, max(walls) / T, k_ms, k_n,
             "; one of them the transpose of GP" if algo == "es3c" else ""), flush=True)
    print("F %s: seeded %.4f; after each sweep %s; swapped per datapoint %s; gain > 0 at the end: %d, gain <= 0: %d of %d "
          "datapoints" % (tag, before, " ".join("%.4f" % f for f in res.F), " ".join("%.3f" % s for s in res.S_sub),
                          int((res.gain > 0).sum()), int((res.gain <= 0).sum()), N), flush=True)
    iters, ms_r, F_r = 1, 0.0, None
    while True:
        ms_r, F_r = refine_route(iters)
        if ms_r >= ms or iters >= 4096:
            break
        iters = max(iters + 1, int(iters * min(4.0, 1.2 * ms / max(ms_r, 1e-3))))
    print("refine %s: refine_resident_states needs %d iterations for the sweeps' wall time (%.3f ms against %.3f ms): "
          "F %.4f against the sweeps' %.4f" % (tag, iters, ms_r, ms, F_r[-1], res.F[-1]), flush=True)
    print("L^ - F %s (256 draws): seeded %.4f nats (mean ess %.2f); after %d sweeps %.4f nats (mean ess %.2f)"
          % (tag, gap0, ess0, T, gap1, ess1), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--parents", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5, help="timed calls of the sweep route (the median is reported)")
    ap.add_argument("--missing", type=float, default=0.0, help="fraction of entries hidden by an i.i.d. mask (0: complete data)")
    ap.add_argument("--neighbourhood", nargs="+", default=["flip"], choices=["flip", "swap", "both"],
                    help="the neighbourhoods to measure, in this order (complete data)")
    ap.add_argument("--alternate", action="store_true", help="also: flips until quiet, then swaps until quiet, repeated")
    args = ap.parse_args()
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

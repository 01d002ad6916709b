"""Time K^n refinement at fixed Theta (Model.refine_resident_states, evoamd_refine_states) beside the training E-step
(Model.E_step) from the same start, at the north-star shape (ES3C D = 256, H = 512, S = 200, N = 100k) and at c5 (EBSC
D = 256, H = 1024, S = 256, N = 200k) on one MI355X.  Data is drawn by generate_data_device from a sparse Theta (pi H = 3,
Gaussian W * 0.8, noise 0.3; ES3C: SPD Psi = I + low rank); the start is the seeded K^n (seed_resident_states, which is
deterministic: every route re-seeds and so starts from the same states).

  wall    host clock around ``--iters`` iterations of each route, both ending in a device synchronise: one
          refine_resident_states call, and that many E_step calls (rng="device", sync_host=False); one warm-up of each
          route first; ms per iteration;
  F       the free energy before, after 10 and after ``--iters`` iterations, both routes (same seeds: same K^n);
  stages  a second run of each route with Engine.timing on (HIP events around every kernel class; the events cost stream
          time, so this run is not the one the wall times come from): ms per launch and launches per class.

The yardstick is E_step.  A refine iteration runs a strict subset of its launches.

    python tools/time_refine.py [--config c4|c5|both] [--n N] [--iters 50]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd import _lib  # noqa: E402
from evo_amd.models import BSC, SSSC  # noqa: E402

CONFIGS = {"c4": ("es3c", 256, 512, 200, 100000), "c5": ("ebsc", 256, 1024, 256, 200000)}
EA = ("fit", "randflip", 10, 1, 1)
STAGES = ("lpj_pass", "lpj_resident", "lpj_candidates", "lpj_overflow", "evolve", "vary_kn", "estep_fused", "row_lse",
          "stats_pass", "gemm_f64", "misc")


def sparse_theta(rng, algo, D, H):
    W = rng.normal(size=(D, H)) * 0.8
    if algo == "ebsc":
        return {"W": W, "pi": 3.0 / H, "sigma": 0.3}
    L = rng.normal(size=(H, 2)) * 0.3
    return {"W": W, "pies": np.full(H, 3.0 / H), "mus": np.full(H, 1.0), "Psi": np.eye(H) + L @ L.T,
            "sigma2": np.float64(0.09)}


def run(name, args):
    algo, D, H, S, N = CONFIGS[name]
    N = args.n or N
    T = args.iters
    rng = np.random.RandomState(0)
    theta = sparse_theta(rng, algo, D, H)
    cls = BSC if algo == "ebsc" else SSSC
    first = cls(D, H, S, rng="device", sync_host=False, seed=1)
    Y = first.generate_data_device(theta, N, seed=7, keep=("y",))["y"]
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    eng = first.engine
    tag = "%s %s D=%d H=%d S=%d N=%d" % (name, algo, D, H, S, N)

    def seeded():
        """A fresh model on the shared engine with the seeded K^n resident: every route starts from the same states and,
        with _n_steps = 0 and the same model seed, draws the same children."""
        model = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
        return model, model.seed_resident_states(dict(theta), my_data, *EA)

    def refine_route(iters):
        model, suff = seeded()
        F0 = dict(theta)
        model.E_step_precompute(F0, dict(suff), my_data)
        before = F0["ljc"] + model.posterior_scores(theta, suff, my_data)["F"].mean()
        eng.synchronize()
        t0 = time.perf_counter()
        res = model.refine_resident_states(dict(theta), suff, my_data, iters)  # (returns after its one synchronise)
        return (time.perf_counter() - t0) * 1e3, before, res.F

    def estep_route(iters):
        model, suff = seeded()
        th = dict(theta)
        eng.synchronize()
        t0 = time.perf_counter()
        F = [model.E_step(th, suff, my_data)[0] for _ in range(iters)]  # (each returns after the accumulator arrived)
        return (time.perf_counter() - t0) * 1e3, np.array(F), bool(getattr(model, "last_estep_fused", False))

    def stages(route, iters):
        eng.timing(True)
        eng.timing_reset()
        route(iters)
        out = []
        for k in STAGES:
            ms, n = eng.kernel_time_ms(k)
            if n:
                out.append("%s %.4f ms x %d" % (k, ms, n))
        eng.timing(False)
        return "; ".join(out)

    refine_route(2)  # warm-up: code objects, buffers
    estep_route(2)
    ms_r, F_before, F_r = refine_route(T)
    ms_e, F_e, fused = estep_route(T)
    ten = min(10, T) - 1
    print("wall %s: refine_resident_states %.3f ms per iteration (%d iterations, one call), E_step %.3f ms per call "
          "(%d calls%s); E_step / refine = %.2f" % (tag, ms_r / T, T, ms_e / T, T, ", fused kernel" if fused else "",
                                                  ms_e / ms_r), flush=True)
    print("F %s: before %.4f; refine after %d %.4f, after %d %.4f; E_step after %d %.4f, after %d %.4f"
          % (tag, F_before, ten + 1, F_r[ten], T, F_r[-1], ten + 1, F_e[ten], T, F_e[-1]), flush=True)
    print("stages %s refine (%d iterations, events on): %s" % (tag, T, stages(refine_route, T)), flush=True)
    print("stages %s E_step (%d calls, events on): %s" % (tag, T, stages(estep_route, T)), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    assert set(STAGES) <= set(_lib.KERNEL_IDS)
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

"""Time the greedy K^n seeding (evoamd_seed_states) at the north-star shape (ES3C D = 256, H = 512, S = 200, N = 100k) and
at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k) with max_active = 8 on one MI355X.  Data is drawn by
generate_data_device from a sparse Theta (pi H = 3, Gaussian W * 0.8, noise 0.3; ES3C: SPD Psi = I + low rank).

  device  HIP events around the kernel (kernel class "seed_states"; B = Y W and transfers excluded), one warm-up, then
          ``--reps`` launches; mean / median / min / max;
  mirror  wall time of evo_amd.variational.seed_states_host for ``--host-n`` datapoints on one core, scaled to N and
          labelled as extrapolated;
  start   the first free energy of an E-step (rng="device") from the seeded K^n, and the number of E-steps a start from
          init_resident_states needs on the same data and Theta before its free energy passes it (at most ``--esteps``).

    python tools/time_seed_states.py [--config c4|c5|both] [--n N] [--reps 5] [--host-n 30] [--esteps 60]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, SSSC  # noqa: E402
from evo_amd.variational import seed_states_host  # noqa: E402

CONFIGS = {"c4": ("es3c", 256, 512, 200, 100000), "c5": ("ebsc", 256, 1024, 256, 200000)}
EA = ("fit", "randflip", 10, 1, 1)


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
    A = args.max_active
    rng = np.random.RandomState(0)
    theta = sparse_theta(rng, algo, D, H)
    cls = BSC if algo == "ebsc" else SSSC
    model = cls(D, H, S, rng="device", sync_host=False, seed=1)
    Y = model.generate_data_device(theta, N, seed=7, keep=("y",))["y"]
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    tag = "%s %s D=%d H=%d S=%d N=%d A=%d" % (name, algo, D, H, S, N, A)
    # ---- device
    suff = model.seed_resident_states(dict(theta), my_data, *EA, max_active=A)  # warm-up
    eng = model.engine
    eng.timing(["seed_states"])
    t = []
    for _ in range(args.reps):
        eng.timing_reset()
        eng.seed_states(A)
        t.append(eng.kernel_time_ms("seed_states")[0])
    eng.timing(False)
    t = np.array(t)
    print("device seed_states %s: mean %.3f ms, median %.3f, min %.3f, max %.3f (%d launches)"
          % (tag, t.mean(), np.median(t), t.min(), t.max(), t.size), flush=True)
    # ---- the start it gives
    if args.esteps > 0:
        eng.lpj_resident()
        th = dict(theta)
        F_seed = model.E_step(th, suff, my_data)[0]
        other = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
        noise = other.init_resident_states(my_data, *EA, seed=3)
        th2, n_steps, F = dict(theta), 0, -np.inf
        F_first = None
        while n_steps < args.esteps and not F > F_seed:
            F = other.E_step(th2, noise, my_data)[0]
            n_steps += 1
            if F_first is None:
                F_first = F
        print("start %s: first free energy seeded %.3f, from init_resident_states %.3f; %s%d E-steps (rng=device) from "
              "init_resident_states to pass the seeded start's first free energy (last F %.3f)"
              % (tag, F_seed, F_first, "" if F > F_seed else "more than ", n_steps, F), flush=True)
    eng.close()
    # ---- mirror
    if args.host_n > 0:
        n = min(args.host_n, N)
        t0 = time.perf_counter()
        seed_states_host("bsc" if algo == "ebsc" else "sssc", theta, Y[:n], S, A)
        dt = time.perf_counter() - t0
        print("mirror seed_states_host %s on one core: %.2f s for %d datapoints; extrapolated to N=%d: %.0f s"
              % (tag, dt, n, N, dt * N / n), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--max-active", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=30)
    ap.add_argument("--esteps", type=int, default=60)
    args = ap.parse_args()
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

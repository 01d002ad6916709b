"""Time K^n(0) initialisation at the north-star shape (N = 100k, S = 200, H = 512) on one MI355X:

  device  evoamd_init_states, HIP events around the kernel (kernel class "init_states"), for p0 = 1/H and p0 = 8/H,
          one warm-up each, then the two settings interleaved ``--reps`` times; mean / median / min / max;
  host    wall time of evo_amd.variational.init_states for ``--host-n`` datapoints at the same S and H on one core,
          scaled to N and labelled as extrapolated.

    python tools/time_init_states.py [--n 100000] [--s 200] [--h 512] [--reps 7] [--host-n 2000]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.engine import Engine  # noqa: E402
from evo_amd.variational import init_states  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--s", type=int, default=200)
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=2000)
    ap.add_argument("--home", type=int, default=-1, help="option init_states_home")
    args = ap.parse_args()
    N, S, H = args.n, args.s, args.h
    eng = Engine(0)
    eng.set_option("init_states_home", args.home)
    eng.configure("bsc", N, 4, H, S, 0, 4)
    settings = {"1/H": 1.0 / H, "8/H": 8.0 / H}
    for p0 in settings.values():
        eng.init_states(p0, 1)
    eng.timing(["init_states"])
    times = {k: [] for k in settings}
    for rep in range(args.reps):
        for name, p0 in settings.items():
            eng.timing_reset()
            eng.init_states(p0, 100 + rep)
            times[name].append(eng.kernel_time_ms("init_states")[0])
    eng.timing(False)
    for name, t in times.items():
        t = np.array(t)
        print("device init_states N=%d S=%d H=%d p0=%s: mean %.3f ms, median %.3f, min %.3f, max %.3f (%d launches)"
              % (N, S, H, name, t.mean(), np.median(t), t.min(), t.max(), t.size))
    eng.close()
    if args.host_n > 0:
        np.random.seed(0)
        t0 = time.perf_counter()
        init_states(args.host_n, S, H, "fit", "randflip", 10, 1, 1)
        dt = time.perf_counter() - t0
        print("host init_states N=%d S=%d H=%d on one core: %.2f s measured; extrapolated to N=%d: %.1f s"
              % (args.host_n, S, H, dt, N, dt * N / args.host_n))


if __name__ == "__main__":
    main()

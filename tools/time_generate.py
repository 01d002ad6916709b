"""Time sampling from the model at the north-star size (D = 256, H = 512, N = 100k, ES3C) on one MI355X:

  device  evoamd_generate for pi H = 1 and pi H = 5 (y only kept): HIP events around the kernel (kernel class "misc"), the
          wall time of the call (upload of Theta, kernel, synchronisation) and of the download of y; one warm-up each,
          then the two settings interleaved ``--reps`` times; median / min / max;
  host    wall time of SSSC.generate_data for ``--host-n`` datapoints at pi H = 5 on one core, scaled to N and labelled as
          extrapolated.

    python tools/time_generate.py [--n 100000] [--d 256] [--h 512] [--reps 5] [--host-n 500]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.engine import Engine  # noqa: E402
from evo_amd.models import SSSC  # noqa: E402
from evo_amd.models.generate import generate_params  # noqa: E402


def theta(D, H, piH, rng):
    A = rng.normal(size=(H, H))
    return {"W": rng.normal(size=(D, H)), "pies": np.full(H, piH / H), "mus": rng.normal(size=H),
            "Psi": np.dot(A, A.T) / H, "sigma2": 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--h", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=500)
    args = ap.parse_args()
    N, D, H = args.n, args.d, args.h
    rng = np.random.RandomState(0)
    thetas = {piH: theta(D, H, piH, rng) for piH in (1.0, 5.0)}
    pars = {piH: generate_params("sssc", th) for piH, th in thetas.items()}
    eng = Engine(0)

    def call(piH, seed):
        p = pars[piH]
        t0 = time.perf_counter()
        eng.generate("sssc", N, seed, p["Wt"], p["pies"], p["mus"], p["F"], p["sigma"], keep=())
        t1 = time.perf_counter()
        y = eng.download_generated("y")
        return t1 - t0, time.perf_counter() - t1, y

    for piH in pars:
        call(piH, 1)
    eng.timing(["misc"])
    times = {piH: [] for piH in pars}
    for rep in range(args.reps):
        for piH in pars:
            eng.timing_reset()
            t_call, t_down, y = call(piH, 100 + rep)
            times[piH].append((eng.kernel_time_ms("misc")[0], 1e3 * t_call, 1e3 * t_down))
            assert np.isfinite(y).all()
    eng.timing(False)
    for piH, t in times.items():
        t = np.array(t)
        for col, what in enumerate(("kernel", "call (upload of Theta + kernel + sync)", "download of y")):
            print("device generate ES3C N=%d D=%d H=%d pi H=%g, %s: median %.3f ms, min %.3f, max %.3f (%d calls)"
                  % (N, D, H, piH, what, np.median(t[:, col]), t[:, col].min(), t[:, col].max(), t.shape[0]))
    eng.close()
    if args.host_n > 0:
        np.random.seed(0)
        t0 = time.perf_counter()
        SSSC(D, H, 8).generate_data(thetas[5.0], args.host_n)
        dt = time.perf_counter() - t0
        print("host generate_data ES3C N=%d D=%d H=%d pi H=5 on one core: %.2f s measured; extrapolated to N=%d: %.1f s"
              % (args.host_n, D, H, dt, N, dt * N / args.host_n))


if __name__ == "__main__":
    main()

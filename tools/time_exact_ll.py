"""Time the exact log-likelihood on one MI355X, EBSC and ES3C at N = 500, D = 64:

  H = 11            Model.free_energy(full=True) (state table, N x 2^H lpj through the host) beside
                    Model.exact_log_likelihood (states enumerated and folded on the device): the only shape both can run;
  H = 16, H = 20    Model.exact_log_likelihood alone (the table path stops at H = 12).

Wall time of the whole call, data and Theta resident from a warm-up call at H = 11; ``--reps`` calls each, median / min /
max.  Every line is printed as soon as it is measured.  ``--budget`` seconds: a shape is skipped, and said to be, when the
time of the previous shape of the same model times 2^(difference in H) exceeds what is left.

    python tools/time_exact_ll.py [--n 500] [--d 64] [--hs 16,20] [--reps 3] [--budget 600] [--models ebsc,es3c]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.engine import Engine  # noqa: E402
from evo_amd.models import BSC, SSSC  # noqa: E402
from evo_amd.variational import init_states  # noqa: E402


def problem(algo, N, D, H, rng):
    """Theta with a sparse W and a non-diagonal SPD Psi, and data generated from it."""
    W = rng.normal(size=(D, H)) * (rng.random_sample((D, H)) < 0.3) + 0.1 * rng.normal(size=(D, H))
    s = rng.random_sample((N, H)) < 2.0 / H
    if algo == "ebsc":
        theta = {"W": W, "pi": np.float64(2.0 / H), "sigma": np.float64(0.5)}
        Y = s.astype(float) @ W.T + 0.5 * rng.normal(size=(N, D))
    else:
        A = rng.normal(size=(H, 3)) * 0.3
        theta = {"W": W, "pies": np.full(H, 2.0 / H), "mus": np.ones(H), "Psi": 0.5 * np.eye(H) + A @ A.T,
                 "sigma2": np.float64(0.25)}
        z = theta["mus"] + rng.normal(size=(N, H)) @ np.linalg.cholesky(theta["Psi"]).T
        Y = (s * z) @ W.T + 0.5 * rng.normal(size=(N, D))
    return theta, {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, np.array(ts)


def report(what, ts):
    print("%s: median %.3f ms, min %.3f, max %.3f (%d calls)"
          % (what, 1e3 * np.median(ts), 1e3 * ts.min(), 1e3 * ts.max(), ts.size), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--hs", default="16,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget", type=float, default=600.0)
    ap.add_argument("--models", default="ebsc,es3c")
    args = ap.parse_args()
    N, D, S = args.n, args.d, 16
    t_start = time.perf_counter()
    eng = Engine(0)
    for algo in args.models.split(","):
        last = None  # (H, seconds) of the previous exact call of this model
        for H in [11] + [int(h) for h in args.hs.split(",") if h]:
            tag = "%s N=%d D=%d H=%d" % (algo.upper(), N, D, H)
            left = args.budget - (time.perf_counter() - t_start)
            if last is not None and last[1] * 2.0 ** (H - last[0]) * (args.reps + 1) > left:
                print("%s exact_log_likelihood: not measured (about %.0f s per call expected, %.0f s of the budget left)"
                      % (tag, last[1] * 2.0 ** (H - last[0]), left), flush=True)
                continue
            rng = np.random.RandomState(H)
            np.random.seed(H)
            theta, my_data = problem(algo, N, D, H, rng)
            model = (BSC if algo == "ebsc" else SSSC)(D, H, S, engine=eng)
            theta = model.check_params(theta)
            suff = init_states(N, S, H, "fit", "randflip", 4, 1, 1)
            L, _ = timed(lambda: model.exact_log_likelihood(my_data, theta, suff, max_H=H), 1)  # warm-up: uploads, buffers
            L, ts = timed(lambda: model.exact_log_likelihood(my_data, theta, suff, max_H=H), args.reps)
            report("%s exact_log_likelihood (L = %.6f)" % (tag, L), ts)
            last = (H, float(np.median(ts)))
            if H == 11:
                Lt, _ = timed(lambda: model.free_energy(my_data, dict(theta), suff, full=True), 1)
                Lt, ts = timed(lambda: model.free_energy(my_data, dict(theta), suff, full=True), args.reps)
                report("%s free_energy(full=True) (L = %.6f)" % (tag, Lt), ts)
                assert abs(L - Lt) <= 1e-11 * abs(Lt), (L, Lt)
    eng.close()


if __name__ == "__main__":
    main()

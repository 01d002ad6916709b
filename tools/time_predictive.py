"""Time the predictive moments (evoamd_predictive_moments, csrc/kernels_predictive.hpp) on one MI355X at the north-star
shape (ES3C D = 256, H = 512, S = 200, N = 100k) and at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k):

  device  HIP events around the kernels of the call (kernel class "misc": the W^T transpose and the moments kernel), the
          wall time of the call (kernels, status scan) and of the download of mean and var; one warm-up, then ``--reps``
          calls; median / min / max.  For scale, the statistics pass of the same build on the same K^n (kernel class
          "stats_pass" plus its contraction, "gemm_f64").
  host    wall time of the NumPy mirror (evo_amd.models.predictive_moments_host) on the first ``--host-n`` datapoints on
          one core, scaled to N and labelled as extrapolated; the device rows of the slice are compared with it.

K^n is drawn on the device (Engine.init_states, p = ``--pih`` / H) and its lpj rows come from one pass over it.

    python tools/time_predictive.py [--shapes c4,c5] [--scale 1.0] [--pih 2] [--reps 3] [--host-n 40]

``--merge``: the whole user-visible operation, from the call to the precision-merged image and to the uncertainty map, on
the image-shaped problems of tools/merge_timing.py (``--geometries g16,g8``), both ways: the default path downloads mean
and var (N, D) and ``set_and_merge(mean.T, precision_merger(var.T))`` uploads both again; with ``resident=True`` the two
stay on the device and only the image comes back.  Wall times around calls that end synchronised, one warm-up and five
repeats each (median, min, max: the spread); the images of the two paths are compared bit for bit.

    python tools/time_predictive.py --merge [--geometries g16,g8]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd._lib import check, dptr  # noqa: E402
from evo_amd.engine import Engine  # noqa: E402
from evo_amd.models import predictive_moments_host  # noqa: E402

SHAPES = {"c4": ("es3c", 100000, 256, 512, 200), "c5": ("ebsc", 200000, 256, 1024, 256)}


def theta_of(algo, D, H, piH, rng):
    W = rng.normal(size=(D, H)) * 0.3
    if algo == "ebsc":
        return {"W": W, "pi": piH / H, "sigma": np.float64(1.0)}
    A = rng.normal(size=(H, 3)) * 0.2
    return {"W": W, "pies": np.full(H, piH / H), "mus": rng.normal(size=H) * 0.5 + 1.0, "Psi": np.eye(H) + A @ A.T,
            "sigma2": np.float64(1.0)}


def stat(what, v, unit="ms"):
    v = np.asarray(v)
    print("%s: median %.3f %s, min %.3f, max %.3f (%d calls)" % (what, np.median(v), unit, v.min(), v.max(), v.size), flush=True)


def merge_mode(args):
    import merge_timing as mt
    from evo_amd.utils.prepost import mean_merger, precision_merger
    eng = Engine(0)
    for name in args.geometries.split(","):
        ovp, tag = mt.setup(eng, name, args.pih)

        def precision(resident):
            mean, var, _ = eng.predictive_moments(resident=resident)
            return ovp.set_and_merge(mean.T, merge_method=precision_merger(var.T))

        def both(resident):
            mean, var, _ = eng.predictive_moments(resident=resident)
            return (ovp.set_and_merge(mean.T, merge_method=precision_merger(var.T)),
                    ovp.set_and_merge(var.T, merge_method=mean_merger))

        t_d, img_d = mt.timed(lambda: precision(False))
        t_r, img_r = mt.timed(lambda: precision(True))
        t_db, both_d = mt.timed(lambda: both(False))
        t_rb, both_r = mt.timed(lambda: both(True))
        mt.stat(tag + " to the precision-merged image, default path", t_d)
        mt.stat(tag + " to the precision-merged image, resident path", t_r)
        mt.stat(tag + " to the image and the uncertainty map, default path", t_db)
        mt.stat(tag + " to the image and the uncertainty map, resident path", t_rb)
        print("%s images of the two paths equal bit for bit: %s, uncertainty maps: %s"
              % (tag, np.array_equal(img_d, img_r, equal_nan=True), np.array_equal(both_d[1], both_r[1], equal_nan=True)), flush=True)
        mean, var, _ = eng.predictive_moments(resident=True)
        mt.stat(tag + " precision merge of the resident moments, device",
                mt.kernel_ms(eng, lambda: ovp.set_and_merge(mean.T, merge_method=precision_merger(var.T))))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,c5")
    ap.add_argument("--scale", type=float, default=1.0, help="N is multiplied by this")
    ap.add_argument("--pih", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=40)
    ap.add_argument("--merge", action="store_true", help="time moments -> merged image, default against resident")
    ap.add_argument("--geometries", default="g16,g8")
    args = ap.parse_args()
    if args.merge:
        return merge_mode(args)
    eng = Engine(0)
    for name in args.shapes.split(","):
        algo, N, D, H, S = SHAPES[name]
        N = max(64, int(N * args.scale))
        tag = "%s %s N=%d D=%d H=%d S=%d pi H=%g" % (name, algo.upper(), N, D, H, S, args.pih)
        rng = np.random.RandomState(1)
        theta = theta_of(algo, D, H, args.pih, rng)
        Y = rng.normal(size=(N, D))
        eng.set_option("ebsc_f32", 0)
        eng.f32 = False
        eng.configure("bsc" if algo == "ebsc" else "sssc", N, D, H, S, 0, 4)
        eng.upload_data(Y)
        eng.set_reliable_fraction(None)
        if algo == "ebsc":
            eng.set_params_bsc(theta["W"], theta["pi"], theta["sigma"])
        else:
            eng.set_params_sssc(theta["W"], theta["pies"], theta["mus"], theta["Psi"], theta["sigma2"])
        eng.init_states(args.pih / H, 7)
        eng.lpj_resident()
        counters = (ctypes.c_int64 * 2)()
        mean, var = np.empty((N, D)), np.empty((N, D))

        def call():
            t0 = time.perf_counter()
            check(eng.lib.evoamd_predictive_moments(eng._h, 1, counters))
            t1 = time.perf_counter()
            check(eng.lib.evoamd_download_predictive(eng._h, dptr(mean), dptr(var)))
            return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)

        call()
        eng.timing(["misc"])
        rows = []
        for _ in range(args.reps):
            eng.timing_reset()
            t_call, t_down = call()
            eng.synchronize()
            rows.append((eng.kernel_time_ms("misc")[0], t_call, t_down))
        eng.timing(False)
        rows = np.array(rows)
        stat(tag + " predictive moments, kernels", rows[:, 0])
        stat(tag + " predictive moments, call (kernels + status scan)", rows[:, 1])
        stat(tag + " predictive moments, download of mean and var (%.0f MB)" % (2 * N * D * 8 / 1e6), rows[:, 2])
        print("%s counters: n_singular %d, n_skipped %d" % (tag, counters[0], counters[1]), flush=True)
        # the statistics pass of the same build on the same K^n, for scale
        eng.stats()
        eng.timing(["stats_pass", "gemm_f64"])
        ts = []
        for _ in range(args.reps):
            eng.timing_reset()
            eng.stats()
            eng.synchronize()
            a, na = eng.kernel_time_ms("stats_pass")
            b, nb = eng.kernel_time_ms("gemm_f64")
            ts.append(a * na + b * nb)
        eng.timing(False)
        stat(tag + " statistics pass (scatter kernels + contraction)", ts)
        if args.host_n > 0:
            n = min(args.host_n, N)
            ss = eng.download_states_packed(0, n)
            ss = np.unpackbits(ss, axis=-1)[..., :H].astype(bool)
            lpj = eng.download_lpj()[:n]
            t0 = time.perf_counter()
            hm, hv, _ = predictive_moments_host("bsc" if algo == "ebsc" else "sssc", theta, ss, lpj, Y[:n])
            dt = time.perf_counter() - t0
            print("%s host mirror on one core: %.2f s for %d datapoints; extrapolated to N=%d: %.0f s"
                  % (tag, dt, n, N, dt * N / n), flush=True)
            print("%s device against the mirror on the slice: max |mean| diff %.3g, max |var| diff %.3g"
                  % (tag, np.abs(hm - mean[:n]).max(), np.abs(hv - var[:n]).max()), flush=True)
    eng.close()


if __name__ == "__main__":
    main()

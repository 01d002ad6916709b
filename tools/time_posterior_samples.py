"""Time the posterior sampler (evoamd_posterior_sample, csrc/kernels_posterior_sample.hpp) on one MI355X at the north-star
shape (ES3C D = 256, H = 512, S = 200, N = 100k) and at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k), for T = 1, 8 and
64 draws per datapoint (``--draws``), fill "all", with the noise:

  device  HIP events around the kernels of the call (kernel class "posterior_sample": the W^T transpose and the sampling
          kernel), the wall time of the call (kernels, status scan) and of the download of slot, packed s and y; one warm-up, then
          ``--reps`` calls; median / min / max.  Draws whose outputs do not fit the device are refused by the library:
          the refusal is printed and the next T is tried.
  host    wall time of the NumPy mirror (evo_amd.models.sample_posterior_counter) on the first ``--host-n`` datapoints on
          one core, scaled to N and labelled as extrapolated; the device rows of the slice are compared with it.

K^n is drawn on the device (Engine.init_states, p = ``--pih`` / H) and its lpj rows come from one pass over it.

    python tools/time_posterior_samples.py [--shapes c4,c5] [--scale 1.0] [--pih 2] [--reps 3] [--draws 1,8,64] [--host-n 30]

``--merge``: the whole user-visible operation, from the call to the T merged images and to their pixelwise (mean, std), on
the image-shaped problems of tools/merge_timing.py (``--geometries g16,g8``), both ways:

  default   sample_posterior downloads y (N, T, D); every draw is merged by Engine.patches_merge (an upload of its (N, D)
            slice each); np.mean / np.std over the images;
  resident  sample_posterior(resident=True); ResidentDraws.merge / merge_moments: one launch, only the images (or only the
            two moment images) come back.

Wall times around calls that end synchronised, one warm-up and five repeats each (median, min, max: the spread), and the
device time of the batched merge per draw next to one patches_merge_resident at the same geometry.  The images of the two
paths are compared bit for bit.

    python tools/time_posterior_samples.py --merge [--geometries g16,g8] [--draws 1,8,64]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd._lib import PSAMP_KEEP, PSAMP_WHAT, EvoAmdError, check  # noqa: E402
from evo_amd.engine import Engine  # noqa: E402
from evo_amd.models import sample_posterior_counter  # noqa: E402
from evo_amd.models.generate import unpack_words  # noqa: E402
from evo_amd.utils.prepost import median_merger  # noqa: E402

SHAPES = {"c4": ("es3c", 100000, 256, 512, 200), "c5": ("ebsc", 200000, 256, 1024, 256)}
KEEP = ("slot", "s", "y")


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
    eng = Engine(0)
    for name in args.geometries.split(","):
        ovp, tag = mt.setup(eng, name, args.pih)
        geom = (ovp.shape, ovp.ph, ovp.pw, ovp.shift)
        # one resident merge of the reconstruction at this geometry, for scale (select kernel + mean merge)
        eng.stats()
        eng.reconstruct_resident()
        mt.stat(tag + " patches_merge_resident (mean), device", mt.kernel_ms(eng, lambda: eng.patches_merge_resident(*geom)))
        mt.stat(tag + " patches_merge_resident (mean), call", mt.timed(lambda: eng.patches_merge_resident(*geom))[0])
        eng.lpj_resident()
        for T in (int(t) for t in args.draws.split(",")):
            tt = "%s T=%d" % (tag, T)

            def default_images():
                y = eng.sample_posterior(T, seed=5, keep=("y",), fill="all")["y"]
                return np.stack([eng.patches_merge(y[:, t], *geom) for t in range(T)])

            def default_moments():
                imgs = default_images()
                return np.mean(imgs, axis=0), np.std(imgs, axis=0)

            def resident_images():
                return eng.sample_posterior(T, seed=5, keep=("y",), fill="all", resident=True)["y"].merge(ovp)

            def resident_moments():
                return eng.sample_posterior(T, seed=5, keep=("y",), fill="all", resident=True)["y"].merge_moments(ovp)

            try:
                t_di, imgs_d = mt.timed(default_images)
            except (EvoAmdError, MemoryError) as e:
                print("%s refused: %s" % (tt, e), flush=True)
                continue
            t_ri, imgs_r = mt.timed(resident_images)
            t_dm, mom_d = mt.timed(default_moments)
            t_rm, mom_r = mt.timed(resident_moments)
            mt.stat(tt + " to the T images, default path", t_di)
            mt.stat(tt + " to the T images, resident path", t_ri)
            mt.stat(tt + " to (mean, std), default path", t_dm)
            mt.stat(tt + " to (mean, std), resident path", t_rm)
            print("%s images of the two paths equal bit for bit: %s; max |mean| diff %.3g, max |std| diff %.3g"
                  % (tt, np.array_equal(imgs_d, imgs_r, equal_nan=True), np.abs(mom_d[0] - mom_r[0]).max(),
                     np.abs(mom_d[1] - mom_r[1]).max()), flush=True)
            h = eng.sample_posterior(T, seed=5, keep=("y",), fill="all", resident=True)["y"]
            mt.stat(tt + " batched mean merge to images, device, per draw", mt.kernel_ms(eng, lambda: h.merge(ovp)) / T)
            mt.stat(tt + " batched mean merge to moments, device, per draw", mt.kernel_ms(eng, lambda: h.merge_moments(ovp)) / T)
            mt.stat(tt + " batched median merge to images, device, per draw",
                    mt.kernel_ms(eng, lambda: h.merge(ovp, median_merger)) / T)
            del imgs_d, imgs_r, h
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,c5")
    ap.add_argument("--scale", type=float, default=1.0, help="N is multiplied by this")
    ap.add_argument("--pih", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--draws", default="1,8,64")
    ap.add_argument("--host-n", type=int, default=30)
    ap.add_argument("--merge", action="store_true", help="time sample -> merged images / moments, default against resident")
    ap.add_argument("--geometries", default="g16,g8")
    args = ap.parse_args()
    if args.merge:
        return merge_mode(args)
    eng = Engine(0)
    for name in args.shapes.split(","):
        algo, N, D, H, S = SHAPES[name]
        N = max(64, int(N * args.scale))
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
        n = min(args.host_n, N)
        ss = np.unpackbits(eng.download_states_packed(0, n), axis=-1)[..., :H].astype(bool) if n > 0 else None
        lpj = eng.download_lpj()[:n]
        for T in (int(t) for t in args.draws.split(",")):
            tag = "%s %s N=%d D=%d H=%d S=%d pi H=%g T=%d" % (name, algo.upper(), N, D, H, S, args.pih, T)
            counters = (ctypes.c_int64 * 4)()
            bits = sum(PSAMP_KEEP[k] for k in KEEP)
            out = {"slot": np.empty((N, T), dtype=np.int32), "s": np.empty((N * T, (H + 63) // 64), dtype=np.uint64),
                   "y": np.empty((N, T, D))}

            def call():
                t0 = time.perf_counter()
                check(eng.lib.evoamd_posterior_sample(eng._h, T, 5, 0, bits, 1, 1, counters))
                t1 = time.perf_counter()
                for k in KEEP:
                    check(eng.lib.evoamd_download_posterior_samples(eng._h, PSAMP_WHAT[k], out[k].ctypes.data_as(ctypes.c_void_p)))
                return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)

            try:
                call()  # warm-up: the buffers are cut here
            except EvoAmdError as e:
                print("%s refused: %s" % (tag, e), flush=True)
                continue
            eng.timing(["posterior_sample"])
            rows = []
            for _ in range(args.reps):
                eng.timing_reset()
                t_call, t_down = call()
                eng.synchronize()
                rows.append((eng.kernel_time_ms("posterior_sample")[0], t_call, t_down))
            eng.timing(False)
            rows = np.array(rows)
            mb = N * T * (4 + 8 * ((H + 63) // 64) + 8 * D) / 1e6
            stat(tag + " posterior samples, kernels", rows[:, 0])
            stat(tag + " posterior samples, call (kernels + status scan)", rows[:, 1])
            stat(tag + " posterior samples, download of slot, s and y (%.0f MB)" % mb, rows[:, 2])
            print("%s counters: n_singular %d, n_skipped %d, n_not_pd %d, n_bad_weights %d" % ((tag,) + tuple(counters)), flush=True)
            if n > 0:
                t0 = time.perf_counter()
                ref = sample_posterior_counter("bsc" if algo == "ebsc" else "sssc", theta, ss, lpj, Y[:n], n_samples=T, seed=5,
                                               fill="all")
                dt = time.perf_counter() - t0
                print("%s host mirror on one core: %.2f s for %d datapoints; extrapolated to N=%d: %.0f s"
                      % (tag, dt, n, N, dt * N / n), flush=True)
                print("%s device against the mirror on the slice: slot equal %s, s equal %s, max |y| diff %.3g"
                      % (tag, np.array_equal(ref["slot"], out["slot"][:n]), np.array_equal(ref["s"], unpack_words(out["s"][:n * T], H).reshape(n, T, H)),
                         np.nanmax(np.abs(ref["y"] - out["y"][:n]))), flush=True)
            del out
    eng.close()


if __name__ == "__main__":
    main()

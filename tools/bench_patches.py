"""Overlapping-patch merge on the GPU against the NumPy merge: prints ONE JSON line.

Per shape (H x W x C image, ph x pw patches, shift 1) and NaN fraction of the estimates:
  kernel_ms_{mean,median}  device time of the merge kernel (kernel class "patches", HIP events; transfers excluded)
  call_ms_{mean,median}    Engine.patches_merge end to end: upload of Y (N x D), kernel, download of the image
  numpy_ms_{mean,median}   np.nanmean / np.nanmedian over the NaN-padded estimate stack, stacking included
  bytes                    algorithmic bytes: N D 8 read + H W C 8 written
  hbm_frac_{mean,median}   bytes / kernel time over the 6.29 TB/s achievable HBM rate (8 TB/s spec)
Rounds are interleaved (mean, median, mean, ...); each number is reported as median and minimum over the rounds.

    python tools/bench_patches.py [--rounds 7] [--numpy-rounds 2] [--quick]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from evo_amd.engine import Engine  # noqa: E402
from evo_amd.utils.prepost import estimate_stack, mean_merger, median_merger, patch_geometry  # noqa: E402

HBM_BPS = 6.29e12


def _stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4)}


def run_shape(eng, name, shape, ph, pw, nan_frac, rounds, numpy_rounds):
    H, W = shape[:2]
    C = shape[2] if len(shape) == 3 else 1
    N, D = patch_geometry(H, W, C, ph, pw, 1)
    rng = np.random.RandomState(0)
    Y = rng.normal(size=(N, D))
    if nan_frac:
        Y[rng.random_sample(Y.shape) < nan_frac] = np.nan
    res = {"shape": name, "N": N, "D": D, "nan": nan_frac, "bytes": N * D * 8 + H * W * C * 8}
    if eng is None:
        rounds = 0
    kern = {"mean": [], "median": []}
    call = {"mean": [], "median": []}
    for m in ("mean", "median") if rounds else ():  # warm-up (code objects, scratch growth)
        eng.patches_merge(Y, shape, ph, pw, 1, m)
    for _ in range(rounds):
        for m in ("mean", "median"):
            eng.timing(["patches"])
            eng.timing_reset()
            t0 = time.perf_counter()
            eng.patches_merge(Y, shape, ph, pw, 1, m)
            call[m].append((time.perf_counter() - t0) * 1e3)
            kern[m].append(eng.kernel_time_ms("patches")[0])
            eng.timing(False)
    nbytes = res["bytes"]
    for m in ("mean", "median") if rounds else ():
        res["kernel_ms_" + m] = _stats(kern[m])
        res["call_ms_" + m] = _stats(call[m])
        res["hbm_frac_" + m] = round(nbytes / (np.min(kern[m]) * 1e-3) / HBM_BPS, 4)
    if numpy_rounds:
        npt = {"mean": [], "median": []}
        for _ in range(numpy_rounds):
            for m, f in (("mean", mean_merger), ("median", median_merger)):
                t0 = time.perf_counter()
                f(estimate_stack(Y, H, W, C, ph, pw, 1), axis=0)
                npt[m].append((time.perf_counter() - t0) * 1e3)
        for m in ("mean", "median"):
            res["numpy_ms_" + m] = _stats(npt[m])
    else:
        for m in ("mean", "median"):
            res["numpy_ms_" + m] = "not measured"
    if not rounds:
        for m in ("mean", "median"):
            res["kernel_ms_" + m] = res["call_ms_" + m] = res["hbm_frac_" + m] = "not measured"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--numpy-rounds", type=int, default=1)
    ap.add_argument("--numpy-only", action="store_true", help="the NumPy merges alone (no GPU needed)")
    ap.add_argument("--quick", action="store_true", help="one small shape (rehearsal)")
    a = ap.parse_args()
    shapes = [("512x512_5x5", (512, 512), 5, 5), ("512x512_8x8", (512, 512), 8, 8),
              ("512x512_16x16", (512, 512), 16, 16), ("1024x1024_8x8", (1024, 1024), 8, 8),
              ("castle_481x321x3_8x8", (481, 321, 3), 8, 8)]
    if a.quick:
        shapes = [("64x64_8x8", (64, 64), 8, 8)]
    eng = None if a.numpy_only else Engine()
    out = []
    for name, shape, ph, pw in shapes:
        for nan_frac in (0.0, 0.3):
            out.append(run_shape(eng, name, shape, ph, pw, nan_frac, a.rounds, a.numpy_rounds))
            print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    if eng is not None:
        eng.close()
    print(json.dumps({"tool": "bench_patches", "hbm_Bps": HBM_BPS, "results": out}))


if __name__ == "__main__":
    main()

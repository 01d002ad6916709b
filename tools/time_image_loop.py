"""Time the inpainting loop of the reference's examples/image-inpainting/main.py epoch by epoch: EM step, hand-over of the
reconstruction, merge into an image -- with the default N x D round trip and with the reconstruction kept on the device.

    python tools/time_image_loop.py [--modes default,resident,resident_fused] [--repeats 3] [--out FILE]

A 256 x 256 synthetic grey image (generated here from a seed), 20 % of the pixels missing, overlapping 5 x 5 and 8 x 8
patches (N = 63 504 / 62 001), EBSC and ES3C with H = 32 and H = 256, S = 20, device_mstep=True, rng="device"; every
epoch runs step(do_reconstruction=True) and set_and_merge(y_reconstructed.T, mean_merger).  30 timed epochs after 5
warm-up epochs per run; the modes of one row alternate inside one process and every run is repeated (--repeats), so the
spread between repeats of the same code stands beside the difference between the modes.

Per epoch (host clock; every part ends in a device synchronise -- the step in its mailbox poll, the merge in the copy of
the image):
  em        model.step minus the hand-over inside it
  handover  Model._write_reconstruction: default = download of y_hat + the host selection; resident = one library call
  merge     OverlappingPatches.set_and_merge: default = upload of N x D + kernel + image back; resident = kernel + image back
  epoch     em + handover + merge

Modes: default (resident_reconstruction=False), resident (=True), resident_fused (=True with option
"merge_select_fused" = 1: the merge kernel selects while it gathers instead of reading rows a select kernel wrote).
--modes default runs on a tree that lacks the feature.  Prints one JSON line per row and mode, then a table.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.engine import Engine  # noqa: E402
from evo_amd.models import BSC, SSSC  # noqa: E402
from evo_amd.utils.prepost import OverlappingPatches, mean_merger  # noqa: E402
from evo_amd.variational import init_states  # noqa: E402

S = 20


def synthetic_image(side=256, seed=0):
    """Smooth gradients, a few edges and texture, 0..255."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:side, 0:side] / float(side)
    img = 120 + 60 * np.sin(6.0 * x + 2.0 * y) + 40 * np.cos(9.0 * y * x)
    img += 50 * ((x > 0.3) & (x < 0.6) & (y > 0.2) & (y < 0.7))
    img += rng.normal(scale=8.0, size=img.shape)
    return np.clip(img, 0, 255)


def run(algo, H, patch, mode, eng, epochs, warmup, seed):
    clean = synthetic_image()
    rng = np.random.RandomState(seed)
    incomplete = clean.copy()
    incomplete[rng.random_sample(clean.shape) < 0.2] = np.nan
    ovp = OverlappingPatches(incomplete, patch, patch, patch_shift=1, engine=eng)
    Y = ovp.get().T
    N, D = Y.shape
    xi = np.logical_not(np.isnan(Y))
    my_data = {"y": Y, "x_infr": xi, "x": xi.copy()}
    np.random.seed(seed)
    kw = dict(engine=eng, device_mstep=True, rng="device", sync_host=False, seed=seed)
    if mode != "default":
        kw["resident_reconstruction"] = True
    if algo == "es3c":
        model = SSSC(D, H, S, to_learn=["W", "pies", "sigma2"], **kw)
    else:
        model = BSC(D, H, S, **kw)
    if mode != "default":
        eng.set_option("merge_select_fused", 1 if mode == "resident_fused" else 0)
    theta = model.check_params(model.standard_init(my_data))
    suff = init_states(N, S, H, "fit", "randflip", 10, 1, 1)
    spent = [0.0]
    inner = model._write_reconstruction

    def timed_handover(md):
        t = time.perf_counter()
        inner(md)
        spent[0] += time.perf_counter() - t

    model._write_reconstruction = timed_handover
    rows = []
    img = None
    for epoch in range(warmup + epochs):
        spent[0] = 0.0
        t0 = time.perf_counter()
        F, _, _, theta = model.step(theta, suff, my_data, do_reconstruction=True)
        t1 = time.perf_counter()
        img = ovp.set_and_merge(my_data["y_reconstructed"].T, merge_method=mean_merger)
        t2 = time.perf_counter()
        if epoch >= warmup:
            rows.append(((t1 - t0 - spent[0]) * 1e3, spent[0] * 1e3, (t2 - t1) * 1e3))
    assert img.shape == clean.shape and np.isfinite(F)
    assert not np.isnan(img).any()  # 20 % missing, patches of >= 25 pixels: every pixel has a valid estimate
    em, ho, mg = (float(np.median(c)) for c in zip(*rows))
    return {"em": em, "handover": ho, "merge": mg, "epoch": float(np.median([sum(r) for r in rows])),
            "N": int(N), "D": int(D)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="default,resident")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--algos", default="ebsc,es3c")
    ap.add_argument("--H", default="32,256")
    ap.add_argument("--patches", default="5,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = a.modes.split(",")
    eng = Engine(0)
    results = []
    for algo in a.algos.split(","):
        for H in (int(v) for v in a.H.split(",")):
            for patch in (int(v) for v in a.patches.split(",")):
                per_mode = {m: [] for m in modes}
                for rep in range(a.repeats):
                    for m in modes:  # alternate the modes inside one repeat
                        per_mode[m].append(run(algo, H, patch, m, eng, a.epochs, a.warmup, seed=rep))
                for m in modes:
                    rs = per_mode[m]
                    ep = [r["epoch"] for r in rs]
                    rec = {"algo": algo, "H": H, "patch": patch, "mode": m, "N": rs[0]["N"], "D": rs[0]["D"],
                           "epochs": a.epochs, "warmup": a.warmup, "repeats": a.repeats,
                           "epoch_ms": float(np.median(ep)), "epoch_ms_min": min(ep), "epoch_ms_max": max(ep),
                           "em_ms": float(np.median([r["em"] for r in rs])),
                           "handover_ms": float(np.median([r["handover"] for r in rs])),
                           "merge_ms": float(np.median([r["merge"] for r in rs]))}
                    results.append(rec)
                    print(json.dumps(rec), flush=True)
    print("\n%-5s %4s %5s %-17s %9s %9s %9s %9s  %s" % ("algo", "H", "patch", "mode", "em", "handover", "merge", "epoch",
                                                       "epoch min..max over repeats [ms]"))
    for r in results:
        print("%-5s %4d %2dx%-2d %-17s %9.3f %9.3f %9.3f %9.3f  %.3f..%.3f" % (
            r["algo"], r["H"], r["patch"], r["patch"], r["mode"], r["em_ms"], r["handover_ms"], r["merge_ms"],
            r["epoch_ms"], r["epoch_ms_min"], r["epoch_ms_max"]))
    if a.out:
        with open(a.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")
    eng.close()


if __name__ == "__main__":
    main()

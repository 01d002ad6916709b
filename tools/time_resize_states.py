"""Time K^n resized (evoamd_resize_states, Model.resize_states) at the two large shapes on one MI355X: ES3C D = 256, H = 512,
N = 100k, S 200 -> 100 and 100 -> 200 (c4) and EBSC D = 256, H = 1024, N = 200k, S 256 -> 128 and 128 -> 256 (c5).  Data is
drawn by generate_data_device from a sparse Theta (pi H = 3, Gaussian W * 0.8, noise 0.3; ES3C: SPD Psi = I + low rank), K^n
is seeded (seed_resident_states) and refined for ``--refine`` iterations (refine_resident_states).

  kernel  HIP events around the resize kernel (kernel class "resize"; downloads excluded), one warm-up, then ``--reps``
          launches; median (min - max), and the share of the traffic bound N (S + S') HW 8 + N S 8 + N S' 12 bytes at
          ``--peak-gbs`` that the median achieves;
  call    wall time of the whole Model.resize_states call, with the configure and the data upload inside it listed apart;
  host    the route without the kernel -- download of K^n and its rows, evo_amd.variational.resize_states_host, upload -- for
          ``--host-n`` datapoints on one core, scaled to N and labelled as extrapolated;
  grow    mean F_after - F_before per datapoint, then the free energy after ``--sweeps`` flip sweeps from the grown K^n
          against the same number of flip sweeps at the old S (from a copy of the old K^n).

    python tools/time_resize_states.py [--config c4|c5|both] [--direction shrink|grow|both] [--n N] [--reps 5]
                                       [--host-n 200] [--refine 20] [--sweeps 4] [--peak-gbs 8000]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, SSSC  # noqa: E402
from evo_amd.variational import resize_states_host  # noqa: E402

from time_remap_latents import EA, _Stopwatch, sparse_theta  # noqa: E402

# name -> (algo, D, H, the larger S, N); a shrink halves S, a grow doubles S / 2
CONFIGS = {"c4": ("es3c", 256, 512, 200, 100000), "c5": ("ebsc", 256, 1024, 256, 200000)}


def run(name, direction, args):
    algo, D, H, S_big, N = CONFIGS[name]
    N = args.n or N
    S, S2 = (S_big, S_big // 2) if direction == "shrink" else (S_big // 2, S_big)
    rng = np.random.RandomState(0)
    theta = sparse_theta(rng, algo, D, H)
    cls = BSC if algo == "ebsc" else SSSC
    model = cls(D, H, S, rng="device", sync_host=False, seed=1)
    Y = model.generate_data_device(theta, N, seed=7, keep=("y",))["y"]
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    tag = "%s %s D=%d H=%d N=%d S=%d->%d" % (name, algo, D, H, N, S, S2)
    suff = model.seed_resident_states(dict(theta), my_data, *EA)
    eng = model.engine
    th = model.check_params(dict(theta))
    res = model.refine_resident_states(th, suff, my_data, args.refine)
    print("start %s: F after seeding and %d refine iterations %.6f" % (tag, res.n_done, res.F[-1]), flush=True)
    # ---- kernel
    eng.resize_states(S2)  # warm-up (and the scratch buffers)
    eng.timing(["resize"])
    t = []
    for _ in range(args.reps):
        eng.timing_reset()
        eng.resize_states(S2)
        t.append(eng.kernel_time_ms("resize")[0])
    eng.timing(False)
    t = np.array(t)
    HW = (H + 63) // 64
    bound = N * (S + S2) * HW * 8 + N * S * 8 + N * S2 * 12
    at_peak = bound / (args.peak_gbs * 1e9) * 1e3
    print("kernel resize %s: median %.3f ms (%.3f - %.3f), %d launches; traffic bound %.2f GB = %.3f ms at %.0f GB/s: the "
          "median achieves %.1f %% of it (%.0f GB/s)"
          % (tag, np.median(t), t.min(), t.max(), t.size, bound / 1e9, at_peak, args.peak_gbs, 100.0 * at_peak / np.median(t),
             bound / np.median(t) / 1e6), flush=True)
    # ---- host route on a slice (before the call below invalidates the model)
    host_line = None
    if args.host_n > 0:
        n = min(args.host_n, N)
        t0 = time.perf_counter()
        ss = np.unpackbits(eng.download_states_packed(0, n), axis=-1)[..., :H].astype(bool)
        rows = eng.download_lpj()
        t_down = time.perf_counter() - t0
        t0 = time.perf_counter()
        ss2, src2 = resize_states_host(ss, rows[:n], suff["S_perm"], S2)
        t_host = time.perf_counter() - t0
        host_line = (n, t_down, t_host, np.packbits(ss2, axis=-1), src2)
    old_packed = eng.download_states_packed() if direction == "grow" and args.sweeps > 0 else None
    # ---- the whole call
    with _Stopwatch(eng, "configure") as t_conf, _Stopwatch(eng, "upload_data") as t_data:
        t0 = time.perf_counter()
        new_model, new_suff, info = model.resize_states(th, suff, my_data, S2)
        eng.synchronize()
        t_call = time.perf_counter() - t0
    print("call Model.resize_states %s: %.1f ms in all, of which configure %.1f ms and data upload %.1f ms (wall time)"
          % (tag, 1e3 * t_call, 1e3 * t_conf.seconds, 1e3 * t_data.seconds), flush=True)
    if host_line is not None:
        n, t_down, t_host, packed, src2 = host_line
        same = np.array_equal(packed, eng.download_states_packed(0, n)) and np.array_equal(src2, info["src_slot"][:n])
        t0 = time.perf_counter()
        fresh = cls(D, H, S2, rng="device", sync_host=False, seed=1, engine=eng)  # (construct: nothing on the device yet)
        eng.upload_states_packed(packed, 0)
        eng.synchronize()
        t_up = time.perf_counter() - t0
        del fresh
        dt = t_down * n / N + t_host + t_up  # (the rows came down for all N: their share)
        print("host route %s on one core: download %.3f s + resize_states_host %.3f s + construct and upload %.3f s = %.3f s "
              "for %d datapoints (rows equal the kernel's: %s); extrapolated to N=%d: %.1f s"
              % (tag, t_down * n / N, t_host, t_up, dt, n, same, N, dt * N / n), flush=True)
    if direction == "grow":
        d = info["F_after"] - info["F_before"]
        print("grow %s: mean F_after - F_before %.6g per datapoint (min %.3g, max %.3g); %.1f %% of the datapoints gain more "
              "than 1e-6" % (tag, d.mean(), d.min(), d.max(), 100.0 * (d > 1e-6).mean()), flush=True)
        if args.sweeps > 0:
            sw = new_model.sweep_resident_states(th, new_suff, my_data, n_sweeps=args.sweeps, stop_when_quiet=False)
            old = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
            old_suff = dict(suff)
            old.attach_resident_states(old_suff, my_data, [(0, old_packed)])
            sw_old = old.sweep_resident_states(th, old_suff, my_data, n_sweeps=args.sweeps, stop_when_quiet=False)
            print("grow %s: F after %d flip sweeps from the grown K^n %.6f, after %d flip sweeps at the old S %.6f "
                  "(difference %.6g)" % (tag, sw.n_done, sw.F[-1], sw_old.n_done, sw_old.F[-1], sw.F[-1] - sw_old.F[-1]),
                  flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--direction", default="both", choices=["shrink", "grow", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=200)
    ap.add_argument("--refine", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="memory bandwidth the traffic bound is priced at (GB/s)")
    args = ap.parse_args()
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        for direction in (["shrink", "grow"] if args.direction == "both" else [args.direction]):
            run(name, direction, args)


if __name__ == "__main__":
    main()

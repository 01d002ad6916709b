"""Time the dictionary resize (evoamd_remap_latents, Model.remap_latents) at the two large shapes on one MI355X: ES3C D = 256,
H = 512 -> 384, S = 200, N = 100k (c4) and EBSC D = 256, H = 1024 -> 768, S = 256, N = 200k (c5).  Data is drawn by
generate_data_device from a sparse Theta (pi H = 3, Gaussian W * 0.8, noise 0.3; ES3C: SPD Psi = I + low rank), K^n is seeded
(seed_resident_states) and the kept latents are the most used ones (latent_usage -> prune_index).

  kernel  HIP events around the remap kernel (kernel class "remap_latents"; index upload and downloads excluded), one
          warm-up, then ``--reps`` launches; mean / median / min / max, and the share of the word traffic bound
          N S (HW + HW') 8 + N S 8 bytes at ``--peak-gbs`` that the median achieves;
  call    wall time of the whole Model.remap_latents call, with the configure and the data upload inside it listed apart;
  fills   sum_replaced / (N S);
  host    the route without the kernel -- download of K^n, evo_amd.variational.remap_states_host, upload -- for ``--host-n``
          datapoints on one core, scaled to N and labelled as extrapolated.

    python tools/time_remap_latents.py [--config c4|c5|both] [--n N] [--reps 5] [--host-n 200] [--peak-gbs 8000]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, SSSC  # noqa: E402
from evo_amd.variational import prune_index, remap_states_host  # noqa: E402

CONFIGS = {"c4": ("es3c", 256, 512, 384, 200, 100000), "c5": ("ebsc", 256, 1024, 768, 256, 200000)}
EA = ("fit", "randflip", 10, 1, 1)


def sparse_theta(rng, algo, D, H):
    W = rng.normal(size=(D, H)) * 0.8
    if algo == "ebsc":
        return {"W": W, "pi": 3.0 / H, "sigma": 0.3}
    L = rng.normal(size=(H, 2)) * 0.3
    return {"W": W, "pies": np.full(H, 3.0 / H), "mus": np.full(H, 1.0), "Psi": np.eye(H) + L @ L.T,
            "sigma2": np.float64(0.09)}


class _Stopwatch:
    """Wall time spent inside one method of the engine (synchronised), while the block runs."""

    def __init__(self, eng, name):
        self.eng, self.name, self.seconds = eng, name, 0.0

    def __enter__(self):
        inner = getattr(self.eng, self.name)

        def timed(*a, **kw):
            t0 = time.perf_counter()
            out = inner(*a, **kw)
            self.eng.synchronize()
            self.seconds += time.perf_counter() - t0
            return out

        setattr(self.eng, self.name, timed)
        return self

    def __exit__(self, *exc):
        delattr(self.eng, self.name)
        return False


def run(name, args):
    algo, D, H, H2, S, N = CONFIGS[name]
    N = args.n or N
    rng = np.random.RandomState(0)
    theta = sparse_theta(rng, algo, D, H)
    cls = BSC if algo == "ebsc" else SSSC
    model = cls(D, H, S, rng="device", sync_host=False, seed=1)
    Y = model.generate_data_device(theta, N, seed=7, keep=("y",))["y"]
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    tag = "%s %s D=%d H=%d->%d S=%d N=%d" % (name, algo, D, H, H2, S, N)
    suff = model.seed_resident_states(dict(theta), my_data, *EA)
    eng = model.engine
    usage = model.latent_usage(dict(theta), suff, my_data)
    index = prune_index(usage["usage"], n_keep=H2)
    print("usage %s: %d latents with usage > 0, %d with a MAP count > 0; kept usage from %.3g up"
          % (tag, int((usage["usage"] > 0).sum()), int((usage["map_count"] > 0).sum()), np.sort(usage["usage"])[H - H2]),
          flush=True)
    # ---- kernel
    eng.remap_latents(index)  # warm-up (and the scratch buffers)
    eng.timing(["remap_latents"])
    t = []
    for _ in range(args.reps):
        eng.timing_reset()
        n_rep, total = eng.remap_latents(index)
        t.append(eng.kernel_time_ms("remap_latents")[0])
    eng.timing(False)
    t = np.array(t)
    HW, HW2 = (H + 63) // 64, (H2 + 63) // 64
    bound = N * S * (HW + HW2) * 8 + N * S * 8
    at_peak = bound / (args.peak_gbs * 1e9) * 1e3
    print("kernel remap_latents %s: mean %.3f ms, median %.3f, min %.3f, max %.3f (%d launches); traffic bound %.2f GB = "
          "%.3f ms at %.0f GB/s: the median achieves %.1f %% of it (%.0f GB/s)"
          % (tag, t.mean(), np.median(t), t.min(), t.max(), t.size, bound / 1e9, at_peak, args.peak_gbs,
             100.0 * at_peak / np.median(t), bound / np.median(t) / 1e6), flush=True)
    print("fills %s: sum_replaced / (N S) = %d / %d = %.3g" % (tag, total, N * S, total / float(N * S)), flush=True)
    # ---- host route on a slice (before the call below invalidates the model)
    host_line = None
    if args.host_n > 0:
        n = min(args.host_n, N)
        t0 = time.perf_counter()
        ss = np.unpackbits(eng.download_states_packed(0, n), axis=-1)[..., :H].astype(bool)
        t_down = time.perf_counter() - t0
        t0 = time.perf_counter()
        ss2, _ = remap_states_host(ss, index, suff["S_perm"])
        t_host = time.perf_counter() - t0
        host_line = (n, t_down, t_host, np.packbits(ss2, axis=-1))
    # ---- the whole call
    with _Stopwatch(eng, "configure") as t_conf, _Stopwatch(eng, "upload_data") as t_data:
        t0 = time.perf_counter()
        new_model, new_theta, new_suff, info = model.remap_latents(dict(theta), suff, my_data, index)
        eng.synchronize()
        t_call = time.perf_counter() - t0
    print("call Model.remap_latents %s: %.1f ms in all, of which configure %.1f ms and data upload %.1f ms (wall time)"
          % (tag, 1e3 * t_call, 1e3 * t_conf.seconds, 1e3 * t_data.seconds), flush=True)
    if host_line is not None:
        n, t_down, t_host, packed = host_line
        same = np.array_equal(packed, eng.download_states_packed(0, n))  # the kernel's rows of the same datapoints
        t0 = time.perf_counter()
        eng.upload_states_packed(packed, 0)
        eng.synchronize()
        t_up = time.perf_counter() - t0
        dt = t_down + t_host + t_up
        print("host route %s on one core: download %.3f s + remap_states_host %.3f s + upload %.3f s = %.3f s for %d "
              "datapoints (rows equal the kernel's: %s); extrapolated to N=%d: %.1f s"
              % (tag, t_down, t_host, t_up, dt, n, same, N, dt * N / n), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["c4", "c5", "both"])
    ap.add_argument("--n", type=int, default=0, help="datapoints (0: the configuration's)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-n", type=int, default=200)
    ap.add_argument("--peak-gbs", type=float, default=8000.0, help="memory bandwidth the traffic bound is priced at (GB/s)")
    args = ap.parse_args()
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

"""Time the greedy K^n seeding (evoamd_seed_states) at the north-star shape (ES3C D = 256, H = 512, S = 200, N = 100k) and
at c5 (EBSC D = 256, H = 1024, S = 256, N = 200k) with max_active = 8 on one MI355X.  Data is drawn by
generate_data_device from a sparse Theta (pi H = 3, Gaussian W * 0.8, noise 0.3; ES3C: SPD Psi = I + low rank).

  device  HIP events around the kernel (kernel class "seed_states"; B = Y W and transfers excluded), one warm-up, then
          ``--reps`` launches; mean / median / min / max;
  mirror  wall time of evo_amd.variational.seed_states_host for ``--host-n`` datapoints on one core, scaled to N and
          labelled as extrapolated;
  start   the first free energy of an E-step (rng="device") from the seeded K^n, and the number of E-steps a start from
          init_resident_states needs on the same data and Theta before its free energy passes it (at most ``--esteps``).

``--missing FRACTION`` (default 0: all of the above on complete data, nothing else): an i.i.d. mask hides that fraction of
the entries (NaN in the data); the masked call (evoamd_seed_states_ex, EVOAMD_SEED_INCOMPLETE) is timed beside the
complete call in the same run, and ``mirror`` and ``start`` run on the masked data.

``--beam B [B ...]`` (complete data only): the beam kernel (evoamd_seed_states_beam) is timed for every B beside the greedy
kernel of the same run, same engine, same data; per B the free energy of the seeded K^n (ljc + mean posterior_scores F), for
the first and the last B the estimate L^ of the log-likelihood (estimate_log_likelihood, ``--samples`` draws), L^ - F and the
mean effective sample size; then the greedy start is followed by neighbourhood="both" sweeps (one call each, wall time
with the host wait) until they have used at least the slowest beam kernel's time, F after each.

    python tools/time_seed_states.py [--config c4|c5|both] [--n N] [--reps 5] [--host-n 30] [--esteps 60] [--missing 0.5]
                                     [--beam 1 2 4 8] [--samples 256]
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
    masked = args.missing > 0
    x_infr = None

    def time_device(what, incomplete, beam=None):
        eng.timing(["seed_states"])
        t = []
        for _ in range(args.reps):
            eng.timing_reset()
            if beam is None:
                eng.seed_states(A, incomplete=incomplete)
            else:
                eng.seed_states_beam(A, beam)
            t.append(eng.kernel_time_ms("seed_states")[0])
        eng.timing(False)
        t = np.array(t)
        print("device seed_states %s %s: mean %.3f ms, median %.3f, min %.3f, max %.3f (%d launches)"
              % (what, tag, t.mean(), np.median(t), t.min(), t.max(), t.size), flush=True)
        return np.median(t)

    # ---- device
    suff = model.seed_resident_states(dict(theta), my_data, *EA, max_active=A)  # warm-up
    eng = model.engine
    t_complete = time_device("complete", False)
    if masked:  # the same run, the same engine: the masked call beside the complete one
        x_infr = np.random.RandomState(11).random_sample(Y.shape) >= args.missing
        my_data = {"y": np.where(x_infr, Y, np.nan), "x_infr": x_infr, "x": x_infr.copy()}
        tag += " missing=%.2f" % args.missing
        model = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
        suff = model.seed_resident_states(dict(theta), my_data, *EA, max_active=A, incomplete=True)  # warm-up
        t_masked = time_device("masked", True)
        print("device seed_states %s: masked / complete = %.2f (medians)" % (tag, t_masked / t_complete), flush=True)
    # ---- the beam beside the greedy kernel: time, the bound of the start, its tightness, and sweeps for the same time
    if args.beam and not masked:
        def bound(m, sf):
            return eng.ljc + m.posterior_scores(dict(theta), sf, my_data)["F"].mean()

        eng.lpj_resident()  # (the timed launches wrote K^n again: its rows are due)
        F_greedy = bound(model, suff)
        print("beam %s: greedy kernel median %.3f ms, F of its K^n %.4f" % (tag, t_complete, F_greedy), flush=True)
        t_slowest = 0.0
        for B in args.beam:
            bm = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
            sf = bm.seed_resident_states(dict(theta), my_data, *EA, max_active=A, beam=B)  # warm-up
            t_b = time_device("beam %d" % B, False, beam=B)
            eng.lpj_resident()
            F_b = bound(bm, sf)
            t_slowest = max(t_slowest, t_b)
            print("beam %s B=%d: kernel / greedy kernel = %.2f (medians), F of its K^n %.4f (greedy %+.4f)"
                  % (tag, B, t_b / t_complete, F_b, F_b - F_greedy), flush=True)
            if B in (args.beam[0], args.beam[-1]):
                L_hat, info = bm.estimate_log_likelihood(dict(theta), sf, my_data, n_samples=args.samples, seed=5,
                                                         per_datapoint=True)
                print("beam %s B=%d: L^ %.4f at T=%d, L^ - F %.4f, mean ess %.2f"
                      % (tag, B, L_hat, args.samples, L_hat - F_b, info["ess"].mean()), flush=True)
        gm = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
        sf = gm.seed_resident_states(dict(theta), my_data, *EA, max_active=A)
        gm.sweep_resident_states(dict(theta), sf, my_data, n_sweeps=1, neighbourhood="both", stop_when_quiet=False)  # warm-up
        sf = gm.seed_resident_states(dict(theta), my_data, *EA, max_active=A)
        used, n_sw = 0.0, 0
        while used < t_slowest and n_sw < 64:
            t0 = time.perf_counter()
            res = gm.sweep_resident_states(dict(theta), sf, my_data, n_sweeps=1, neighbourhood="both", stop_when_quiet=False)
            used += 1e3 * (time.perf_counter() - t0)
            n_sw += 1
            print("beam %s: greedy start + %d \"both\" sweep(s), %.1f ms wall so far (slowest beam kernel %.1f ms): F %.4f "
                  "(greedy %+.4f)" % (tag, n_sw, used, t_slowest, res.F[-1], res.F[-1] - F_greedy), flush=True)
        suff = model.seed_resident_states(dict(theta), my_data, *EA, max_active=A)
    # ---- the start it gives
    if args.esteps > 0:
        eng.lpj_resident()
        th = dict(theta)
        # (incomplete data: the statistics pass of an E-step reads y_reconstructed, which _reconstruct forms first, as
        # step(do_reconstruction=True) does; each model gets its own dict to write it into)
        F_seed = model.E_step(th, suff, my_data, _reconstruct=masked)[0]
        my_data = dict(my_data)
        other = cls(D, H, S, rng="device", sync_host=False, seed=1, engine=eng)
        noise = other.init_resident_states(my_data, *EA, seed=3)
        th2, n_steps, F = dict(theta), 0, -np.inf
        F_first = None
        while n_steps < args.esteps and not F > F_seed:
            F = other.E_step(th2, noise, my_data, _reconstruct=masked)[0]
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
        seed_states_host("bsc" if algo == "ebsc" else "sssc", theta, Y[:n], S, A, x_infr=x_infr[:n] if masked else None)
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
    ap.add_argument("--missing", type=float, default=0.0, help="fraction of entries hidden by an i.i.d. mask (0: complete data)")
    ap.add_argument("--beam", type=int, nargs="*", default=[], help="beam widths to time beside the greedy kernel (complete data)")
    ap.add_argument("--samples", type=int, default=256, help="draws of estimate_log_likelihood for the first and last --beam")
    args = ap.parse_args()
    for name in (["c4", "c5"] if args.config == "both" else [args.config]):
        run(name, args)


if __name__ == "__main__":
    main()

"""Time the posterior from AIS chains (Model.ais_posterior, evoamd_ais_posterior) at c5 (EBSC D = 256, H = 1024, S = 256) on
one MI355X and print what the call is for.  The setting is that of tools/time_ais.py: data drawn from a sparse Theta (pi H =
3, tools/time_refine.py) with generate_data_device, ``s`` and ``y_mean`` kept; the start of K^n is the seeded one
(seed_resident_states) after ``--refine`` iterations of refine_resident_states.  For T = 128, 512 temperatures, n_keep = 1, 4
and C = ``--chains`` chains, each figure the median of ``--repeat`` calls with (min - max):

  wall     host clock around a call with mean=True (it ends in a device synchronise) after one warm-up, and beside it in the
           same run around ais_log_likelihood forward at the same T and C;
  kernel   the "ais_post" span (chains + fold of every block) of a further call with Engine.timing on, beside the "ais" span;
  p        mean |p - E_q[s]| with E_q[s] = encode(dense=True).Es, the marginals under K^n; the quartiles of ess and of p_se;
  mean     the mean squared error of ``mean`` against the generator's y_mean, next to that of E_q[s] W^T, the reconstruction
           from K^n (what reconstruct forms);
  map      the share of datapoints whose map_lpj is above the best lpj in K^n by more than MAP_TOL nats (c_j is kept
           current by adds and subtractions in the order of the chain's flips, so two chains at the SAME state differ in
           the last digits of lpj: without the tolerance the comparison counts rounding), the share whose map_state is
           the generator's s, and the same share for the best state of K^n;
  blocks   once, at the first T and n_keep: the span with --block datapoints per block beside the automatic block;
  masked   with ``--missing F[,F]``: the same calls with that share of the entries hidden (i.i.d. mask, NaN under False,
           incomplete=True) beside the complete calls of this run: wall, the "ais_post" span of ``--repeat`` calls and its
           ratio to the complete span, n_flips per chain, ess, and the squared error of ``mean`` on the MISSING entries
           against the generator's y_mean beside that of ``reconstruct`` from a seeded and swept K^n on the same data.

    python tools/time_ais_posterior.py [--n-data 20000] [--refine 20] [--temps 128,512] [--keeps 1,4] [--chains 16] [--repeat 5]
                                        [--block 512] [--missing 0.5,0.1]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC, sigmoid_schedule  # noqa: E402
from time_refine import CONFIGS, EA, sparse_theta  # noqa: E402


MAP_TOL = 1e-6


def quartiles(a):
    return "%.3g / %.3g / %.3g" % tuple(np.percentile(a, (25, 50, 75)))


def mmm(v):
    return "%.4g (%.4g - %.4g)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-data", type=int, default=20000)
    ap.add_argument("--refine", type=int, default=20)
    ap.add_argument("--temps", default="128,512")
    ap.add_argument("--keeps", default="1,4")
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls per figure (median, min - max)")
    ap.add_argument("--block", type=int, default=512, help="datapoints per block of the block-size line")
    ap.add_argument("--missing", default="", help="fractions of hidden entries, e.g. 0.5,0.1: the masked calls (incomplete=True) "
                                                  "beside the complete calls of the same run")
    args = ap.parse_args()
    args.missing = [float(f) for f in args.missing.split(",") if f]
    temps = [int(t) for t in args.temps.split(",")]
    keeps = [int(k) for k in args.keeps.split(",")]
    algo, D, H, S, _ = CONFIGS["c5"]
    N, C = args.n_data, args.chains
    rng = np.random.RandomState(0)
    model = BSC(D, H, S, rng="device", sync_host=False, seed=1)
    theta = model.check_params(sparse_theta(rng, algo, D, H))
    gen = model.generate_data_device(theta, N, seed=7, keep=("y", "s", "y_mean"))
    Y, y_mean, s_true = gen["y"], gen["y_mean"], np.asarray(gen["s"], dtype=bool)
    s_packed = np.packbits(s_true, axis=-1)
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    eng = model.engine
    tag = "c5 ebsc D=%d H=%d S=%d N=%d C=%d" % (D, H, S, N, C)
    suff = model.seed_resident_states(dict(theta), my_data, *EA)
    res = model.refine_resident_states(dict(theta), suff, my_data, args.refine)
    codes = model.encode(theta, suff, my_data, dense=True)
    Es = codes.Es
    lpj_kn = eng.download_lpj()
    best_kn = lpj_kn.max(axis=1)
    kn_true = float((codes.map_state == s_packed).all(axis=1).mean())
    rec_kn = np.dot(Es, theta["W"].T)
    mse_kn = float(((rec_kn - y_mean) ** 2).mean())
    print("start %s: F after %d refine iterations %.4f; reconstruction from K^n (E_q[s] W^T) against y_mean: mse %.6g "
          "(data against y_mean: %.6g); mean |E_q[s] - s| %.4g; best state of K^n is the generator's s for %.4f of the datapoints" % (
              tag, args.refine, float(res.F[-1]), mse_kn, float(((Y - y_mean) ** 2).mean()), float(np.abs(Es - s_true).mean()),
              kn_true), flush=True)
    model.ais_posterior(theta, suff, my_data, n_chains=2, n_temps=4, n_keep=2, seed=1, mean=True)  # warm-up: code objects, buffers
    model.ais_log_likelihood(theta, suff, my_data, n_chains=2, n_temps=4, seed=1)
    complete = {}  # (T, n_keep) -> (median wall, the spans of --repeat further calls): what --missing is held against
    for T in temps:
        walls = []
        for r in range(args.repeat):
            eng.synchronize()
            t0 = time.perf_counter()
            model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1 + r)
            walls.append((time.perf_counter() - t0) * 1e3)
        eng.timing(("ais",))
        eng.timing_reset()
        model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1)
        span_fwd, n_fwd = eng.kernel_time_ms("ais")
        eng.timing(False)
        wall_fwd = float(np.median(walls))
        print("T=%d %s ais_log_likelihood forward: wall %s ms per call (median of %d), kernel span %.2f ms (%d span)" % (
            T, tag, mmm(walls), args.repeat, span_fwd * n_fwd, n_fwd), flush=True)
        for K in keeps:
            walls, d_p, d_s, mses, shares, trues, out = [], [], [], [], [], [], None
            for r in range(args.repeat):
                eng.synchronize()
                t0 = time.perf_counter()
                out = model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r, mean=True)
                walls.append((time.perf_counter() - t0) * 1e3)
                d_p.append(float(np.abs(out["p"] - Es).mean()))
                mses.append(float(((out["mean"] - y_mean) ** 2).mean()))
                d_s.append(float(np.abs(out["p"] - s_true).mean()))
                shares.append(float((out["map_lpj"] > best_kn + MAP_TOL).mean()))
                trues.append(float((out["map_state"] == s_packed).all(axis=1).mean()))
            spans = []
            for r in range(args.repeat):
                eng.timing(("ais_post", "gemm_f64"))
                eng.timing_reset()
                model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r, mean=True)
                span, n_spans = eng.kernel_time_ms("ais_post")
                gemm, n_gemm = eng.kernel_time_ms("gemm_f64")
                eng.timing(False)
                spans.append(span * n_spans)
            complete[(T, K)] = (float(np.median(walls)), spans)
            span, n_spans = float(np.median(spans)), 1
            print("T=%d n_keep=%d %s ais_posterior: ais_post span over %d calls %s ms; n_flips per chain %.3f" % (
                T, K, tag, args.repeat, mmm(spans), out["n_flips"].mean() / C), flush=True)
            print("T=%d n_keep=%d %s ais_posterior: wall %s ms per call, %.3f of forward (cost model (T + n_keep - 1) / T = %.3f); "
                  "ais_post span %.2f ms (%d span), %.3f of the ais span; mean GEMM %.3f ms" % (
                      T, K, tag, mmm(walls), float(np.median(walls)) / wall_fwd, (T + K - 1) / T, span * n_spans, n_spans,
                      span * n_spans / (span_fwd * n_fwd), gemm * n_gemm), flush=True)
            print("T=%d n_keep=%d %s: mean |p - E_q[s]| %s, mean |p - s| %s; mse of mean against y_mean %s beside %.6g from K^n; "
                  "share of datapoints with map_lpj above the best lpj in K^n %s, with map_state = s %s (K^n: %.4f); ess quartiles "
                  "%s; p_se quartiles %s, mean %.3g, largest %.3g, share above 1e-3 %.3g; count quartiles %s" % (
                      T, K, tag, mmm(d_p), mmm(d_s), mmm(mses), mse_kn, mmm(shares), mmm(trues), kn_true, quartiles(out["ess"]),
                      quartiles(out["p_se"]), float(out["p_se"].mean()), float(out["p_se"].max()),
                      float((out["p_se"] > 1e-3).mean()), quartiles(out["count"])), flush=True)
    # the block size: the engine still holds this Theta and the data
    T, K = temps[0], keeps[0]
    spans = {}
    for block in (0, args.block):
        eng.ais_posterior(sigmoid_schedule(T), C, K, 1, 0, block=block)
        eng.timing(("ais_post",))
        eng.timing_reset()
        eng.ais_posterior(sigmoid_schedule(T), C, K, 1, 0, block=block)
        ms, n = eng.kernel_time_ms("ais_post")
        eng.timing(False)
        spans[block] = ms * n
    print("T=%d n_keep=%d %s blocks: ais_post span %.2f ms with the automatic block, %.2f ms with %d datapoints per block" % (
        T, K, tag, spans[0], spans[args.block], args.block), flush=True)
    for missing in args.missing:
        masked(args, temps, keeps, theta, Y, y_mean, missing, complete, tag)
    eng.close()


def masked(args, temps, keeps, theta, Y, y_mean, missing, complete, tag):
    """The same calls with ``missing`` of the entries hidden (an i.i.d. mask, NaN under False) and incomplete=True, on a
    model of its own, beside the complete figures of this run and beside ``reconstruct`` from a seeded and swept K^n."""
    algo, D, H, S, _ = CONFIGS["c5"]
    N, C = args.n_data, args.chains
    x_infr = np.random.RandomState(11).random_sample(Y.shape) >= missing
    my_data = {"y": np.where(x_infr, Y, np.nan), "x_infr": x_infr, "x": x_infr.copy()}
    hidden = ~x_infr
    model = BSC(D, H, S, rng="device", sync_host=False, seed=1)
    eng = model.engine
    suff = model.seed_resident_states(dict(theta), my_data, *EA, incomplete=True)
    sweep = model.sweep_resident_states(dict(theta), suff, my_data, n_sweeps=8, incomplete=True)
    model.reconstruct(my_data, suff, dict(theta))
    rec_kn = np.asarray(my_data.pop("y_reconstructed"))
    mse_kn = float(((rec_kn - y_mean)[hidden] ** 2).mean())
    tag = "%s missing=%.2f" % (tag, missing)
    print("masked start %s: K^n seeded and swept (%d sweeps ran); reconstruct from K^n against y_mean on the %d missing entries: "
          "mse %.6g (y_mean itself: mean square %.6g)" % (tag, sweep.n_done, int(hidden.sum()), mse_kn,
                                                         float((y_mean[hidden] ** 2).mean())), flush=True)
    kw = dict(incomplete=True)
    model.ais_posterior(theta, suff, my_data, n_chains=2, n_temps=4, n_keep=2, seed=1, mean=True, **kw)  # warm-up
    for T in temps:
        for K in keeps:
            walls, mses, mses_rel, out = [], [], [], None
            for r in range(args.repeat):
                eng.synchronize()
                t0 = time.perf_counter()
                out = model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r, mean=True, **kw)
                walls.append((time.perf_counter() - t0) * 1e3)
                mses.append(float(((out["mean"] - y_mean)[hidden] ** 2).mean()))
                mses_rel.append(float(((out["mean"] - y_mean)[x_infr] ** 2).mean()))
            spans = []
            for r in range(args.repeat):
                eng.timing(("ais_post",))
                eng.timing_reset()
                model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r, **kw)
                ms, n = eng.kernel_time_ms("ais_post")
                eng.timing(False)
                spans.append(ms * n)
            wall_c, span_c = complete[(T, K)]
            print("masked T=%d n_keep=%d %s ais_posterior: wall %s ms per call (complete: %.4g), ais_post span %s ms (complete: %s), "
                  "span ratio %.2f; n_flips per chain %.3f; ess quartiles %s; p_se quartiles %s; mse of mean against y_mean on the "
                  "missing entries %s beside %.6g from K^n (on the reliable entries %s)" % (
                      T, K, tag, mmm(walls), wall_c, mmm(spans), mmm(span_c), float(np.median(spans)) / float(np.median(span_c)),
                      out["n_flips"].mean() / C, quartiles(out["ess"]), quartiles(out["p_se"]), mmm(mses), mse_kn, mmm(mses_rel)),
                  flush=True)
    eng.close()


if __name__ == "__main__":
    main()

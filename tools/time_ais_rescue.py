"""Time the AIS rescue (Model.ais_posterior(index=..., admit=True), evoamd_ais_posterior_sel) at c5 (EBSC D = 256, H = 1024,
S = 256) on one MI355X and print what it does to K^n.  The setting is that of tools/time_ais_posterior.py: data drawn from a
sparse Theta (pi H = 3) with generate_data_device, ``s`` kept; K^n is the seeded one (seed_resident_states) after ``--refine``
iterations of refine_resident_states; C = ``--chains`` chains, n_keep = 1.

The list is the worst ``--share`` of the datapoints by F_n (Model.posterior_scores).  For T = 128, 512, each timing the median
of ``--repeat`` calls with (min - max), every admitted call from the SAME K^n (restored before it):

  span     the "ais_post" span (chains, fold, emission, tally) of the listed call beside that of the call over all N
           datapoints in the same run, and their ratio beside ``--share``; the wall clock of the listed call;
  caught   the share of the datapoints whose K^n misses the chains' best state (map_lpj of the full call above the best lpj
           in K^n by more than MAP_TOL nats) that the list holds;
  counts   the totals of n_distinct, n_new, n_proposed and n_admitted, map_held before and after; the listed datapoints
           whose map_state is the all-zero state (never proposed; K^n holds it only as the permanent state);
  F        mean F over the listed datapoints before and after, F over ALL datapoints (with ljc) after, beside the bracket of
           ais_log_likelihood (forward, and reverse from the generator's s);
  s        the share of datapoints whose best state in K^n is the generator's s, before and after;
  loglik   once: ais_log_likelihood(admit=True) from the same K^n with the same T, its S_sub and F after, for comparison.

``--missing F``: the same on incomplete data (that share of the entries hidden, incomplete=True).

    python tools/time_ais_rescue.py [--n-data 20000] [--refine 20] [--temps 128,512] [--chains 16] [--repeat 5] [--share 0.1]
                                    [--missing 0.5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from evo_amd.models import BSC  # noqa: E402
from time_ais_posterior import MAP_TOL, mmm  # noqa: E402
from time_refine import CONFIGS, EA, sparse_theta  # noqa: E402


def span_of(eng, call):
    eng.timing(("ais_post",))
    eng.timing_reset()
    out = call()
    ms, n = eng.kernel_time_ms("ais_post")
    eng.timing(False)
    return ms * n, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-data", type=int, default=20000)
    ap.add_argument("--refine", type=int, default=20)
    ap.add_argument("--temps", default="128,512")
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5, help="timed calls per figure (median, min - max)")
    ap.add_argument("--share", type=float, default=0.1, help="the share of the datapoints, worst F_n first, that is listed")
    ap.add_argument("--missing", type=float, default=0.0, help="share of hidden entries: the masked route (incomplete=True)")
    args = ap.parse_args()
    temps = [int(t) for t in args.temps.split(",")]
    algo, D, H, S, _ = CONFIGS["c5"]
    N, C, K = args.n_data, args.chains, 1
    rng = np.random.RandomState(0)
    model = BSC(D, H, S, rng="device", sync_host=False, seed=1)
    theta = model.check_params(sparse_theta(rng, algo, D, H))
    gen = model.generate_data_device(theta, N, seed=7, keep=("y", "s"))
    Y, s_true = gen["y"], np.asarray(gen["s"], dtype=bool)
    s_packed = np.packbits(s_true, axis=-1)
    inc = args.missing > 0.0
    if inc:
        x_infr = np.random.RandomState(11).random_sample(Y.shape) >= args.missing
        my_data = {"y": np.where(x_infr, Y, np.nan), "x_infr": x_infr, "x": x_infr.copy()}
    else:
        my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    kw = dict(incomplete=True) if inc else {}
    eng = model.engine
    tag = "c5 ebsc D=%d H=%d S=%d N=%d C=%d n_keep=%d%s" % (D, H, S, N, C, K, " missing=%.2f" % args.missing if inc else "")
    suff = model.seed_resident_states(dict(theta), my_data, *EA, **kw)
    res = model.refine_resident_states(dict(theta), suff, my_data, args.refine)
    kn0 = eng.download_states_packed()  # every admitted call starts here

    def restore():
        eng.upload_states_packed(kn0)
        eng.lpj_resident()

    def best_is_s():
        sc = eng.posterior_scores(("best",))["best"]
        st = eng.download_states_packed()
        return float((st[np.arange(N), sc] == s_packed).all(axis=1).mean())

    scores = model.posterior_scores(theta, suff, my_data)
    F_n = scores["F"]
    ljc = float(res.F[-1]) - float(F_n.mean())
    n_list = max(1, int(round(args.share * N)))
    index = np.sort(np.argsort(F_n, kind="stable")[:n_list]).astype(np.int64)
    best_kn = eng.download_lpj().max(axis=1)
    true0 = best_is_s()
    print("start %s: F after %d refine iterations %.4f (mean F_n %.4f + ljc); the list: the %d datapoints of lowest F_n (share %.3f), "
          "mean F_n %.4f on it; best state of K^n is the generator's s for %.4f of the datapoints" % (
              tag, args.refine, float(res.F[-1]), float(F_n.mean()), n_list, args.share, float(F_n[index].mean()), true0), flush=True)
    model.ais_posterior(theta, suff, my_data, n_chains=2, n_temps=4, n_keep=1, seed=1, index=index[:8], admit=True, **kw)  # warm-up
    model.ais_posterior(theta, suff, my_data, n_chains=2, n_temps=4, n_keep=1, seed=1, **kw)
    model.ais_log_likelihood(theta, suff, my_data, n_chains=2, n_temps=4, seed=1, **kw)
    restore()
    for T in temps:
        full_spans, list_spans, admit_spans, walls = [], [], [], []
        full = info = None
        for r in range(args.repeat):
            ms, full = span_of(eng, lambda: model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r, **kw))
            full_spans.append(ms)
            ms, _ = span_of(eng, lambda: model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r,
                                                             index=index, **kw))
            list_spans.append(ms)
        for r in range(args.repeat):
            restore()
            ms, _ = span_of(eng, lambda: model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r,
                                                             index=index, admit=True, **kw))
            admit_spans.append(ms)
            restore()
            eng.synchronize()
            t0 = time.perf_counter()
            info = model.ais_posterior(theta, suff, my_data, n_chains=C, n_temps=T, n_keep=K, seed=1 + r, index=index, admit=True, **kw)
            walls.append((time.perf_counter() - t0) * 1e3)
        ratio = float(np.median(list_spans)) / float(np.median(full_spans))
        print("T=%d %s span: ais_post of the listed call %s ms beside %s ms over all N: ratio %.4f against share %.4f (%.2f x); "
              "with admit (emission and tally in the span) %s ms; wall of the admitted call %s ms" % (
                  T, tag, mmm(list_spans), mmm(full_spans), ratio, n_list / float(N), ratio * N / n_list, mmm(admit_spans), mmm(walls)),
              flush=True)
        # (full and info are those of the last repeat: the same seed)
        missed = full["map_lpj"] > best_kn + MAP_TOL
        listed = np.zeros(N, dtype=bool)
        listed[index] = True
        print("T=%d %s caught: K^n misses the chains' best state at %d datapoints (%.4f); the list holds %d of them (%.4f)" % (
            T, tag, int(missed.sum()), float(missed.mean()), int((missed & listed).sum()),
            float((missed & listed).sum()) / max(1, int(missed.sum()))), flush=True)
        tot = {k: int(info[k].sum()) for k in ("n_distinct", "n_new", "n_proposed", "n_admitted", "map_held_before", "map_held_after")}
        zero = ~info["map_state"].any(axis=1)
        print("T=%d %s counts over the %d listed datapoints: n_distinct %d, n_new %d, n_proposed %d, n_admitted %d; map_state held "
              "before %d, after %d; datapoints with n_new > 0: %d, with n_admitted > 0: %d; S_sub %.5f; map_state is the all-zero "
              "state (never proposed) at %d listed datapoints, %d of them among the missed, n_distinct = 0 at %d; the generator's s "
              "is all-zero at %d of all datapoints" % (
                  T, tag, n_list, tot["n_distinct"], tot["n_new"], tot["n_proposed"], tot["n_admitted"], tot["map_held_before"],
                  tot["map_held_after"], int((info["n_new"] > 0).sum()), int((info["n_admitted"] > 0).sum()), info["S_sub"],
                  int(zero.sum()), int((zero & missed[index]).sum()), int((info["n_distinct"] == 0).sum()),
                  int((~s_true.any(axis=1)).sum())), flush=True)
        F_all = eng.posterior_scores(("F",))["F"]
        true1 = best_is_s()
        lo = model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1, **kw)
        up = model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1, direction="reverse", s_start=s_true, **kw)
        print("T=%d %s F: mean F_n on the list before %.4f, after %.4f; F over all datapoints before %.4f, after %.4f; "
              "ais_log_likelihood bracket [%.4f, %.4f]; best state of K^n is s: before %.4f, after %.4f" % (
                  T, tag, float(info["F_before"].mean()), float(info["F_after"].mean()), float(res.F[-1]), ljc + float(F_all.mean()),
                  lo, up, true0, true1), flush=True)
        # the call this one is held against: the final states of the first chains of ais_log_likelihood, all N datapoints
        restore()
        _, adm = model.ais_log_likelihood(theta, suff, my_data, n_chains=C, n_temps=T, seed=1 + args.repeat - 1, admit=True, **kw)
        improved = int((adm["F_after"] > adm["F_before"] + MAP_TOL).sum())
        print("T=%d %s ais_log_likelihood(admit=True) from the same K^n: F over all datapoints after %.4f, %d datapoints improved, "
              "S_sub %.5f, best state of K^n is s %.4f" % (T, tag, ljc + float(adm["F_after"].mean()), improved, adm["S_sub"],
                                                           best_is_s()), flush=True)
        restore()
    eng.close()


if __name__ == "__main__":
    main()

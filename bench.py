#!/usr/bin/env python3
"""bench.py -- EM-iteration throughput of the EVO hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c4] [--dump-outputs DIR] [--full]

`--gpus N` with N > 1 may be called bare: the parent starts N fresh child processes (one per GPU,
RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set) before anything touches the GPU, waits
for them and prints rank 0's JSON line.  Under a launcher (torch.distributed.run sets WORLD_SIZE) the
process is one of the ranks.  No PyTorch anywhere: ranks share the RCCL id through a file
(evo_amd.utils.parallel) and all-reduce through librccl inside libevo_amd.

Workload (default): BASELINE.json's north-star shape, configs[3] -- ES3C D=256 H=512 S=200 N=100k, float64
-- on ONE GPU for --gpus 1 and split like np.array_split over the ranks for --gpus N (strong scaling: the
job is the same 100k datapoints whatever N is).  --config c2 | c3 | c5 select the other BASELINE shapes.

A *step* is `--em-per-step` (default 10) full EM iterations of the product path (evo_amd.models,
rng="device", K^n resident on the GPU, device Theta update): per iteration lpj of all N x S resident states,
device candidate generation + their lpj, vary_Kn, sufficient statistics + free energy, ONE RCCL all-reduce of
the packed accumulator when N > 1, Theta update, dense precompute for the next E-step.  Ten iterations per
step keep the timed region of the driver's 20 steps above one second of GPU time.
Metric = candidate-state evaluations per second counted as N x S per EM iteration (BASELINE.json's headline;
the candidate evaluations are done but not counted), whole job, all ranks.

A plain run sets up, warms up, times the steps, writes the outputs if asked to and prints the JSON line:
metric / value / unit / higher_is_better / dtype, ms_per_step (milliseconds per timed step) and the workload.

--full adds, after the timed region (and HIP-event spans of the two passes inside it):
  roofline        the WHOLE pass over the resident K^n (main kernel + every overflow level it spawns, one
                  HIP-event span on the library's stream inside the timed region) against the HBM roof
  roofline_stats  the whole statistics pass (scatter kernels + overflow levels + column sums) likewise
  mfma, levels    the contractions against the MFMA peak; the overflow levels by number of active latents
  config          + kernel_ms (per-class times of extra instrumented iterations), the eager-Theta loop, E-step counters
  per_rank        (N > 1) every rank's view of the timed loop
  cpu_baseline    the loop-faithful NumPy restatement of the reference (oracle/, "port") timed on every host
                  core this process may use, on a bounded sample of the same workload (N=1 only; --no-cpu-baseline)

--dump-outputs DIR writes what the last timed step handed its caller (dump_outputs) as DIR/<name>.npy.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CONFIGS = {  # BASELINE.json "configs": the whole job (N_total is split over the ranks)
    "c1": dict(algo="ebsc", D=25, H=10, S=32, N=500, name="bars-test EBSC D=25 H=10 S=32 N=500"),
    "c2": dict(algo="es3c", D=256, H=128, S=64, N=10000, name="ES3C synthetic Gaussian D=256 H=128 S=64 N=10k f64"),
    "c3": dict(algo="ebsc", D=64, H=256, S=128, N=50000, name="EBSC 8x8 patches D=64 H=256 S=128 N=50k f64"),
    "c4": dict(algo="es3c", D=256, H=512, S=200, N=100000, name="ES3C D=256 H=512 S=200 N=100k f64 (north-star shape)"),
    "c4shard": dict(algo="es3c", D=256, H=512, S=200, N=12500, name="ES3C D=256 H=512 S=200 N=12.5k (one eighth of c4) f64"),
    "c4half": dict(algo="es3c", D=256, H=512, S=200, N=50000, name="ES3C D=256 H=512 S=200 N=50k (half of c4) f64"),
    "c4quarter": dict(algo="es3c", D=256, H=512, S=200, N=25000, name="ES3C D=256 H=512 S=200 N=25k (a quarter of c4) f64"),
    "c5": dict(algo="ebsc", D=256, H=1024, S=256, N=200000, name="EBSC D=256 H=1024 S=256 N=200k (f64; the reference has no f32)"),
    "c5shard": dict(algo="ebsc", D=256, H=1024, S=256, N=25000, name="EBSC D=256 H=1024 S=256 N=25k (one eighth of c5) f64"),
    "c5f32": dict(algo="ebsc", D=256, H=1024, S=256, N=200000, f32=True,
                  name="EBSC D=256 H=1024 S=256 N=200k float32 mode (data / B / E_q[s] rows and the long contractions in f32; "
                       "lpj arithmetic, sums, Theta f64)"),
}
CONFIGS["c4full"] = CONFIGS["c4"]  # round-1 name
EA = dict(parent_selection="fit", mutation="randflip", n_parents=10, n_children=1, n_generations=1)  # examples' defaults
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
F64_MFMA_PEAK_TFLOPS = 78.6  # MI355X FP64 matrix = FP64 vector peak
F32_MFMA_PEAK_TFLOPS = 157.3  # f32-input MFMA (v_mfma_f32_16x16x4_f32), MI355X_MICROARCH.md
# oracle (the timed "port") vs the imported reference, same container, same inputs, 1 core:
# ES3C c2 shape 32.7 vs 37.4 ms per datapoint, EBSC c3 shape 2.33 vs 2.50 -- the port is 7-13 % FASTER
ORACLE_VS_REFERENCE = "oracle is 7-13 % faster than the imported reference (ES3C c2 shape 32.7 vs 37.4 ms per " \
                      "datapoint, EBSC c3 shape 2.33 vs 2.50; build container, 1 core), i.e. inside the +-15 % band"


def log(msg):
    """Progress on stderr (rank 0): a silent run of several minutes is taken for a hang by the job runner."""
    if os.environ.get("RANK", "0") == "0":
        sys.stderr.write("[bench %6.1fs] %s\n" % (time.perf_counter() - _T0, msg))
        sys.stderr.flush()


_T0 = time.perf_counter()


def host_cores():
    """Cores this process may really use: the scheduler affinity, capped by the cgroup CPU quota (the GPU box
    shows all 256 hardware threads of the host but grants a share of 16 through cpu.max)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                quota, period = parts[0], float(parts[1])
            else:
                quota = parts[0]
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                    period = float(f.read().split()[0])
            if quota not in ("max", "-1"):
                n = min(n, max(1, int(round(float(quota) / period))))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def pass_kernels(cfg):
    """Kernels of the pass over all N x S resident states, as rocprofv3 names them (TAG 0 = the pass over K^n)."""
    hw = (cfg["H"] + 63) // 64
    if cfg["algo"] == "es3c":  # census lists (round 3): main kernel (|s| <= 2), quad levels 3..4 / 5..8, wavefront kernel
        return ["void sssc_main_lpj_kernel<0, 512, %d, 2, false, true>" % (hw if hw in (1, 2, 4, 8, 16) else 0),
                "void sssc_quad_kernel<1, 0, 0>", "void sssc_quad_kernel<2, 0, 0>", "void sssc_big_kernel<0, 0>"]
    return ["void bsc_lpj_gram2_kernel<0, %d>" % (hw if hw in (1, 2, 4, 8) else 16)]


def stats_kernels(cfg):
    hw = (cfg["H"] + 63) // 64
    hwt = hw if hw in (1, 2, 4, 8, 16) else 0
    if cfg["algo"] == "es3c":
        # (the census of a new K^n runs at the head of the first pass that needs it: the statistics pass behind vary_Kn)
        return ["void sssc_stats_wave_kernel<%d, 4, true>" % hwt, "census_kernel", "pair_bins_reduce_kernel", "void sssc_quad_kernel<1, 1, 2>",
                "void sssc_quad_kernel<2, 1, 2>", "void sssc_big_kernel<1, 2>", "sssc_finish_kernel"]
    sr = (cfg["S"] + 63) // 64
    if sr <= 4:  # wave-per-datapoint kernel + pair bins (evo_amd.hip: bsc_wave)
        return ["void bsc_stats_wave_kernel<%d>" % (sr if sr in (1, 2) else 4), "pair_bins_reduce_kernel", "bsc_finish_kernel"]
    return ["void bsc_stats_kernel<%d>" % hwt, "colsum_partial_kernel", "bsc_finish_kernel"]


def traffic_key(args):
    """profiles/rNN_<key>_pmc_traffic.json: the counters belong to a workload, i.e. config + state variant."""
    return args.config + ("dense" if args.dense_states else "")


def pmc_traffic(config, kernels):
    """HBM bytes per pass = sum over `kernels` of (bytes per launch x launches per pass) from the committed
    rocprofv3 counter passes (profiles/r02_<config>_pmc_traffic.json, written by tools/profile_bench.sh: separate
    --pmc FETCH_SIZE / WRITE_SIZE runs, read side doubled as MI355X_MICROARCH.md prescribes for gfx950).  A pass is
    one launch of the first kernel of the list; the conditional overflow levels count with their own launch
    frequency.  None if the file is absent."""
    d = None
    for rnd in ("r04", "r03", "r02"):
        path = os.path.join(ROOT, "profiles", "%s_%s_pmc_traffic.json" % (rnd, config))
        try:
            with open(path) as f:
                d = json.load(f)
            pmc_traffic.source = os.path.relpath(path, ROOT)
            break
        except Exception:
            continue
    if d is None:
        return None

    def find(k):
        return [rec for name, rec in d.items() if name.startswith(k)]

    main = find(kernels[0])
    if not main:
        return None
    passes = float(main[0].get("launches", 1)) or 1.0
    total = 0.0
    for k in kernels:
        for rec in find(k):
            total += float(rec["traffic_bytes_2xfetch_plus_write"]) * float(rec.get("launches", passes)) / passes
    return total


def algorithmic_bytes_pass(cfg, N):
    """lpj pass and statistics pass alike, per datapoint D*w + C*(ceil(H/8) + w) with w = 8, C = S."""
    w_y = 4 if cfg.get("f32") else 8  # float32 mode: y_n is float, lpj stays double
    return N * (cfg["D"] * w_y + cfg["S"] * ((cfg["H"] + 7) // 8 + 8))


def layout_bytes_lpj(cfg, N):
    """Compulsory bytes of the lpj pass in THIS implementation's HBM layout: per datapoint the row of
    B = Y W (H doubles, replaces y_n in the Gram form) and per state one 8-byte digest (count + first
    active latents, replaces the ceil(H/8) bit words) plus the 8-byte lpj written."""
    return N * (cfg["H"] * (4 if cfg.get("f32") else 8) + cfg["S"] * (8 + 8))


def layout_bytes_stats(cfg, N):
    """Compulsory bytes of the statistics pass in THIS layout: per datapoint the B row, per state digest + lpj (16 bytes),
    and the dense moment rows it writes for the contraction ([Es | Ez] for ES3C, Es -- float in the float32 mode -- for EBSC)."""
    w = 4 if cfg.get("f32") else 8
    rows = 2 * cfg["H"] * 8 if cfg["algo"] == "es3c" else cfg["H"] * w
    return N * (cfg["H"] * w + cfg["S"] * 16 + rows)


def gemm_flops_per_iteration(cfg, N, executed=False):
    """Dense f64 contractions of one EM iteration in steady state (the launches timed under
    kernel class "gemm_f64"): the K = N statistics contraction, G = W^T W and B = Y W.
    executed=True: what the kernels really multiply -- the symmetric block Ez^T Ez of the ES3C contraction runs its
    upper 128 x 128 tiles only (H = 512: 10 of 16), and G = W^T W likewise where the tile kernel serves it."""
    D, H = cfg["D"], cfg["H"]
    if cfg["algo"] == "es3c":
        nominal = 2.0 * N * (D + 2 * H) * H + 2.0 * D * H * H + 2.0 * N * D * H
        if not executed:
            return nominal
        T = 128
        ts = (H + T - 1) // T
        sym_done = ts * (ts + 1) / 2.0 / (ts * ts) if (D + H) % T == 0 else 1.0  # fraction of the Ez^T Ez tiles computed
        return 2.0 * N * (D + H) * H + sym_done * 2.0 * N * H * H + 2.0 * D * H * H + 2.0 * N * D * H
    return 2.0 * N * H * D + 2.0 * D * H * H + 2.0 * N * D * H


# ---------------------------------------------------------------------------------------------
# K^n(0): init_states (variational/utils.py:155-228) per chunk on the host cores, handed over bit-packed
# ---------------------------------------------------------------------------------------------
def _init_chunk(args):
    n, S, H, seed, p_init = args
    import numpy as np  # noqa: F811
    from evo_amd.variational import init_states
    np.random.seed(seed)
    suff = init_states(n, S, H, EA["parent_selection"], EA["mutation"], EA["n_parents"], EA["n_children"],
                       EA["n_generations"], p_init_Kn=p_init)
    return np.packbits(suff["ss"], axis=-1)


def _bernoulli_rows_packed(rs, n_rows, H, p):
    """(n_rows, ceil(H/8)) uint8: iid Bernoulli(p) bits in np.packbits layout, drawn through the gaps between
    successive ones (geometric), i.e. ~n_rows H p random numbers instead of n_rows H."""
    PB = (H + 7) // 8
    total = n_rows * H
    out = np.zeros(n_rows * PB, dtype=np.uint8)
    pos = -1
    while pos < total:
        m = int(1.2 * (total - pos) * p) + 64
        where = pos + np.cumsum(rs.geometric(p, size=m))
        pos = int(where[-1])
        where = where[where < total]
        r, h = np.divmod(where, H)
        np.bitwise_or.at(out, r * PB + (h >> 3), (0x80 >> (h & 7)).astype(np.uint8))
    return out.reshape(n_rows, PB)


def init_states_inprocess(cfg, n_rows, seed, dense=False, chunk=1000):
    """init_states' construction (variational/utils.py:100-138: S Bernoulli(p) rows, sorted-unique; while fewer than S,
    S more rows whose new unique ones are appended in sorted order; first S kept) from a private generator IN THIS
    PROCESS, bits drawn sparsely: for runs under rocprofv3, where starting worker processes is not an option.
    Same law as init_states, not the same np.random stream."""
    H, S = cfg["H"], cfg["S"]
    p = (8.0 / H) if dense else 1.0 / H
    rs = np.random.RandomState(seed)
    PB = (H + 7) // 8
    void = np.dtype((np.void, PB))
    R = 6  # rounds of S rows drawn ahead per datapoint
    for n0 in range(0, n_rows, chunk):
        n = min(chunk, n_rows - n0)
        pool = _bernoulli_rows_packed(rs, n * R * S, H, p).reshape(n, R * S, PB)
        out = np.zeros((n, S, PB), dtype=np.uint8)
        for i in range(n):
            first_rows = np.ascontiguousarray(pool[i, :S])
            _, first = np.unique(first_rows.view(void), return_index=True)
            have = first_rows[first]
            r = 1
            while have.shape[0] < S:
                more = pool[i, r * S:(r + 1) * S] if r < R else _bernoulli_rows_packed(rs, S, H, p)
                conc = np.ascontiguousarray(np.concatenate((have, more)))
                _, first = np.unique(conc.view(void), return_index=True)
                have = np.concatenate((have, conc[first[first >= have.shape[0]]]))
                r += 1
            out[i] = have[:S]
        yield n0, out


def init_states_packed(cfg, n_rows, seed, workers, dense=False, chunk=2000):
    """Yields (n0, packed uint8 (n, S, ceil(H/8))): the reference's init_states run chunk by chunk in a process
    pool (the bool form of the north-star K^n would be 10 GB, and one core needs minutes for 100k datapoints)."""
    import multiprocessing as mp
    p_init = (8.0 / cfg["H"]) if dense else None  # SURVEY 8d dense-state stress variant
    jobs, n0 = [], 0
    while n0 < n_rows:
        n = min(chunk, n_rows - n0)
        jobs.append((n0, (n, cfg["S"], cfg["H"], seed + 7919 * len(jobs), p_init)))
        n0 += n
    if workers <= 1 or len(jobs) == 1:
        for n0, a in jobs:
            yield n0, _init_chunk(a)
        return
    with mp.get_context("spawn").Pool(min(workers, len(jobs))) as pool:
        for (n0, _), packed in zip(jobs, pool.imap(_init_chunk, [a for _, a in jobs])):
            yield n0, packed


def ea_suff(cfg):
    """my_suff_stat without the K^n arrays (they live on the device): the EA knobs init_states stores."""
    from evo_amd.variational import eas
    return {"ss": None, "lpj": None, "S_perm": 0, "incl": np.zeros((0, cfg["H"]), dtype=bool), "sm": None,
            "permanent": {"background": False, "allzero": False, "singletons": False},
            "n_parents": EA["n_parents"], "n_children": EA["n_children"], "n_generations": EA["n_generations"],
            "parent_selection": eas.fitparents, "mutation_algorithm": eas.randflip, "bitflip_prob": None,
            "Mprime": cfg["S"]}


# ---------------------------------------------------------------------------------------------
# CPU baseline: the oracle (NumPy restatement of the reference loops), one process per core
# ---------------------------------------------------------------------------------------------
def _cpu_worker(args):
    algo, D, H, S, n, seed, reps = args
    os.environ["OPENBLAS_NUM_THREADS"] = "1"
    import numpy as np  # noqa: F811
    from oracle import evo_oracle as orc
    np.random.seed(seed)
    Y = np.random.randn(n, D)
    if algo == "ebsc":
        theta = orc.check_params(orc.bsc_standard_init(Y, H), orc.BSC_POLICY)
    else:
        theta = orc.check_params(orc.sssc_standard_init(Y, H), orc.SSSC_POLICY)
    suff = orc.init_states(n, S, H, "fit", "randflip", 10, 1, 1)
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        # the per-datapoint loops (E-step + sufficient statistics); the Theta solve is timed apart
        # (_cpu_theta_solve): a sample with N < H would make it singular
        if algo == "ebsc":
            orc.bsc_E_step(theta, suff, Y)
            orc.bsc_accumulate(theta, suff, Y)
        else:
            # use_storage=False: the reference's only memory-scalable mode
            orc.sssc_EM_accumulate(theta, suff, Y, use_storage=False)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def _cpu_theta_solve(cfg):
    """The once-per-iteration H x H part of the reference's Theta update (bsc.py:237 lstsq; sssc.py:693,738
    two inverses + W = Wp inv), timed on well-conditioned stand-ins of the same sizes, one process,
    BLAS threads as the reference would have them (unrestricted)."""
    rng = np.random.RandomState(0)
    H, D = cfg["H"], cfg["D"]
    A = rng.normal(size=(H, H))
    A = A @ A.T + H * np.eye(H)
    t0 = time.perf_counter()
    if cfg["algo"] == "ebsc":
        np.linalg.lstsq(A, rng.normal(size=(H, D)), rcond=-1)
    else:
        np.dot(rng.normal(size=(D, H)), np.linalg.inv(A))
        np.linalg.inv(A + 1e-5 * np.eye(H))
    return time.perf_counter() - t0


def cpu_baseline(cfg, budget_s=20.0):
    """Time the oracle on a bounded sample (about budget_s seconds of wall time): every core this process may
    use runs the reference-style per-datapoint loop on its own shard, like one MPI rank per core."""
    import multiprocessing as mp
    cores = host_cores()
    # probe one datapoint-step cost on one core, then size the sample
    t_probe = _cpu_worker((cfg["algo"], cfg["D"], cfg["H"], cfg["S"], 2, 99, 1)) / 2
    per_core = int(max(2, min(2048, (budget_s / 2.0) / max(t_probe, 1e-4))))  # two timed steps per worker
    os.environ["OPENBLAS_NUM_THREADS"] = "1"
    ctx = mp.get_context("spawn")
    jobs = [(cfg["algo"], cfg["D"], cfg["H"], cfg["S"], per_core, 1234 + i, 2) for i in range(cores)]
    with ctx.Pool(cores) as pool:
        times = pool.map(_cpu_worker, jobs)
    os.environ.pop("OPENBLAS_NUM_THREADS", None)
    t = max(times)
    n_sub = per_core * cores
    t_solve = _cpu_theta_solve(cfg)
    t_full = cfg["N"] * t / n_sub
    return {
        "value": n_sub * cfg["S"] / t, "unit": "N*S state evals/s", "cores": cores, "kind": "port",
        "cpu_model": cpu_model(),
        "sample": "oracle EM iteration (reference loop structure: E-step + sufficient statistics, use_storage=False) "
                  "on %d datapoints (%d per core, %d processes = every core of this process's CPU share: affinity "
                  "capped by the cgroup quota), OPENBLAS_NUM_THREADS=1, best of 2, %.2f s; cost is linear in N"
                  % (n_sub, per_core, cores, t),
        "ms_per_datapoint_per_core": 1e3 * t / per_core,
        "theta_solve_s": t_solve,
        "theta_solve_note": "the H x H solves of the Theta update (once per iteration, every rank redundantly) are not "
                            "in `value`: %.3f s against %.0f s of loops for the full N on these cores" % (t_solve, t_full),
        "extrapolated_s_per_iteration_full_N": t_full + t_solve,
        "port_vs_reference": ORACLE_VS_REFERENCE,
    }


# ---------------------------------------------------------------------------------------------
# --gpus N without a launcher: one fresh child per GPU, started before anything touches the GPU
# ---------------------------------------------------------------------------------------------
def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv, worker=None, timeout_s=None, poll_s=0.05, grace_s=5.0):
    """Start `n` ranks of this script (or of `worker`, a command list, for the CPU test of this logic) and watch ALL of
    them: returns (rc, rank-0 stdout).  Like `mpirun`, the job dies with its first failing rank -- the first child that
    exits non-zero gets the others terminated (killed after `grace_s`) and its code returned at once, so a rank that
    dies before or inside an RCCL collective cannot leave rank 0 (and this parent) blocked.  Rank 0's stdout is drained
    by a thread so that a full pipe never stalls it.  The parent never touches the GPU."""
    import threading
    port = free_port()
    nonce = "%d_%d" % (os.getpid(), int(time.time() * 1e3))
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), EVO_AMD_LAUNCH_NONCE=nonce,
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = (worker or [sys.executable, os.path.abspath(__file__)]) + list(argv)
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    chunks = []

    def drain():
        for line in iter(procs[0].stdout.readline, b""):
            chunks.append(line)

    reader = threading.Thread(target=drain, daemon=True)
    reader.start()
    rc, t0 = 0, time.time()
    try:
        while True:
            codes = [p.poll() for p in procs]
            bad = [c for c in codes if c not in (None, 0)]
            if bad:
                rc = bad[0]
                break
            if all(c == 0 for c in codes):
                break
            if timeout_s is not None and time.time() - t0 > timeout_s:
                rc = 124
                break
            time.sleep(poll_s)
    finally:
        alive = [p for p in procs if p.poll() is None]
        for p in alive:
            p.terminate()
        t1 = time.time()
        for p in alive:
            try:
                p.wait(timeout=max(0.1, grace_s - (time.time() - t1)))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    reader.join(timeout=2.0)
    return rc, b"".join(chunks).decode(errors="replace")


# ---------------------------------------------------------------------------------------------
# --dump-outputs: what the timed path computed in its last step
# ---------------------------------------------------------------------------------------------
DUMP_MAX_BYTES = 64 * 10 ** 6
DUMP_SAMPLE_BYTES = 32 * 10 ** 6  # K^n / lpj sample
DUMP_MAX_ROWS = 256  # datapoints of the K^n / lpj sample
DUMP_SEED = 8191


def dump_outputs(path, eng, F, nu, nsub, theta):
    """Write what step() handed its caller in the last timed step, as <path>/<name>.npy (float64; float32 where Theta
    is float32), at most DUMP_MAX_BYTES in all:
      free_energy, S_nunique, S_sub    step()'s three scalars
      theta_<key>                      every numeric entry of Theta^new (a LazyTheta downloads here)
      Kn_sample, lpj_sample            my_suff_stat["ss"] / ["lpj"] as sync_to_host would hand them over, for a fixed
                                       seeded sample of this rank's datapoints (Kn_sample_rows): K^n as 0/1 floats
                                       (rows, S, H), the S states of each datapoint sorted by their bits (K^n is a
                                       set) and lpj permuted alike
    The sample takes DUMP_SAMPLE_BYTES at most, DUMP_MAX_ROWS datapoints at most."""
    os.makedirs(path, exist_ok=True)
    out = {"free_energy": F, "S_nunique": nu, "S_sub": nsub}
    for k in sorted(theta.keys()):
        v = np.asarray(theta[k])
        if v.dtype.kind in "biuf":
            out["theta_" + k] = v
    out = {k: np.asarray(v, dtype=np.float32 if np.asarray(v).dtype == np.float32 else np.float64) for k, v in out.items()}
    N, S, H = eng.N, eng.S, eng.H
    per_row = S * H * 4 + eng.L * 8 + 8
    n_rows = max(1, min(N, DUMP_MAX_ROWS, DUMP_SAMPLE_BYTES // per_row))
    rows = np.sort(np.random.RandomState(DUMP_SEED).choice(N, n_rows, replace=False))
    lpj = eng.download_lpj()[rows]
    packed = np.concatenate([eng.download_states_packed(int(r), 1) for r in rows])  # (rows, S, ceil(H/8))
    ss = np.unpackbits(packed, axis=-1)[..., :H]
    for i in range(n_rows):
        order = np.lexsort(packed[i].T[::-1])  # states by their bit words, first byte most significant
        ss[i] = ss[i][order]
        lpj[i, eng.S_perm:] = lpj[i, eng.S_perm:][order]
    out["Kn_sample"] = ss.astype(np.float32)
    out["lpj_sample"] = lpj
    out["Kn_sample_rows"] = rows.astype(np.float64)
    assert sum(v.nbytes for v in out.values()) <= DUMP_MAX_BYTES
    for k, v in out.items():
        np.save(os.path.join(path, k + ".npy"), v)
    return sorted(out)


def full_measurements(args, cfg, eng, comm, model, theta, suff, my_data, barrier, world, rank, n_loc, iters, dt_own):
    """--full, after the timed region: the roofline spans recorded inside it, the per-rank view, the eager-Theta loop and
    the instrumented iterations.  Rank 0 gets what it adds to the JSON line ("config" entries apart), the others None."""
    lpj_ms, lpj_n = eng.kernel_time_ms("lpj_pass")
    st_ms, st_n = eng.kernel_time_ms("stats_pass")
    # per-rank view of the timed loop in rank 0's line (a first multi-GPU run must be diagnosable from it): every rank fills
    # its slot of a zero vector, the sum is the gather
    per_rank = None
    if world > 1:
        ar_ms, ar_n = eng.kernel_time_ms("allreduce")
        mine = np.zeros((world, 5))
        mine[rank] = [1e3 * dt_own / (args.steps * iters), lpj_ms, st_ms, ar_ms * (ar_n / max(1.0, float(st_n))), n_loc]
        allr = comm.allreduce_array(mine)
        per_rank = {"ms_per_em_iteration_own_queue": [round(v, 5) for v in allr[:, 0]],
                    "lpj_pass_ms": [round(v, 5) for v in allr[:, 1]], "stats_pass_ms": [round(v, 5) for v in allr[:, 2]],
                    "allreduce_ms_per_iteration": [round(v, 5) for v in allr[:, 3]], "datapoints": [int(v) for v in allr[:, 4]],
                    "note": "allreduce_ms_per_iteration = HIP-event span(s) around the RCCL all-reduce(s) of the packed accumulator "
                            "on each rank's stream: from the rank's own statistics being done to the sum being delivered, i.e. "
                            "waiting for the slowest rank + the collective; the SMALLEST entry is the closest to the collective "
                            "itself (the last rank to arrive waits for nobody)"}
    # the reference's step() returns Theta^new as host arrays every epoch: the same loop with the per-iteration download
    eager_ms = None
    if not args.eager_theta and not args.host_mstep:
        eager_iters = max(10, min(50, args.steps * iters // 4))
        model.lazy_theta = False
        for _ in range(3):
            F2, nu2, nsub2, theta = model.step(theta, suff, my_data)
        barrier()
        t1 = time.perf_counter()
        for _ in range(eager_iters):
            F2, nu2, nsub2, theta = model.step(theta, suff, my_data)
        barrier()
        eager_ms = 1e3 * (time.perf_counter() - t1) / eager_iters
        if world > 1:
            eager_ms = comm.allreduce_max(eager_ms)
        model.lazy_theta = True
        F2, nu2, nsub2, theta = model.step(theta, suff, my_data)
    n_gt2 = float(getattr(model, "last_dpar", {}).get("n_gt2", float("nan")))
    # instrumented pass (not part of `value`): per-class device time of a few more iterations
    prof_iters = 5
    eng.timing(True)
    eng.timing_reset()
    for _ in range(prof_iters):
        _F, _nu, _nsub, theta = model.step(theta, suff, my_data)
    barrier()
    kernel_ms = {}
    for name in ("lpj_resident", "lpj_candidates", "lpj_overflow", "row_lse", "vary_kn", "stats", "stats_overflow",
                 "gemm_f64", "evolve", "misc", "mstep_device", "lpj_pass", "stats_pass", "lpj_k3_4", "lpj_k5_8", "lpj_k9plus",
                 "stats_k3_4", "stats_k5_8", "stats_k9plus", "estep_fused", "allreduce"):
        avg, n = eng.kernel_time_ms(name)
        if n:
            kernel_ms[name] = {"avg_ms": round(avg, 6), "launches_per_iteration": n / prof_iters}
    # the contractions once more with ONLY their own class timed: the K = N product then runs forked beside the
    # Theta-update chain exactly as in the timed loop (the fully instrumented pass above runs it alone on the main stream,
    # between event records that idle the GPU), its span recorded on the stream it runs on
    eng.timing(["gemm_f64"])
    eng.timing_reset()
    for _ in range(prof_iters):
        _F, _nu, _nsub, theta = model.step(theta, suff, my_data)
    barrier()
    g_avg, g_n = eng.kernel_time_ms("gemm_f64")
    gemm_loop = {"avg_ms": round(g_avg, 6), "launches_per_iteration": g_n / prof_iters} if g_n else None
    eng.timing(False)

    estep_diag = eng.estep_counters() if cfg["algo"] == "es3c" else None
    if rank != 0:
        return None
    alg_bytes = algorithmic_bytes_pass(cfg, n_loc)  # per launch = this rank's shard
    lay_bytes = layout_bytes_lpj(cfg, n_loc)

    def roof(ms, launches, kernels, what):
        ach = (alg_bytes / (ms * 1e-3) / 1e9) if ms > 0 else 0.0
        return {"bound": "hbm", "kernel": what, "kernels_in_span": kernels,
                "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                "traffic": pmc_traffic(traffic_key(args), kernels),
                "traffic_note": "HBM bytes per pass, rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, read "
                                "side corrected for gfx950 (2 x FETCH_SIZE: an upper bound for kernels whose loads are 8 bytes per lane), "
                                "summed over the kernels of the span; counters of this workload from "
                                + str(getattr(pmc_traffic, "source", None)),
                "algorithmic_bytes_per_launch": alg_bytes,
                "algorithmic_bytes_note": "SURVEY 8d: N_rank x (D*8 + S*(ceil(H/8) + 8)), states priced bit-packed",
                "avg_launch_ms": ms, "launches_timed": launches}

    r_lpj = roof(lpj_ms, lpj_n, pass_kernels(cfg), "whole pass over the resident K^n: lpj of all N x S states "
                 "(main kernel + every overflow level it spawns), one HIP-event span per pass")
    r_lpj["states_in_main_kernel"] = (1.0 - n_gt2 / (float(n_loc) * cfg["S"])) if n_gt2 == n_gt2 else None
    ld = getattr(model, "last_dpar", {})
    r_lpj["overflow_census"] = {k: ld.get(k) for k in ("n_gt2", "n_gt4", "n_gt8") if k in ld}
    r_lpj["layout_bytes_per_launch"] = lay_bytes
    r_lpj["frac_of_layout_bytes"] = (lay_bytes / (lpj_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if lpj_ms > 0 else 0.0
    r_lpj["layout_note"] = ("`achieved` / `frac` price SURVEY 8d's algorithmic bytes (bit-packed states + y_n); the kernels "
                            "read an 8-byte digest per state and the row of B = Y W instead: frac_of_layout_bytes prices that")
    if r_lpj["frac"] > 1.0:
        # at large H the digest layout moves fewer bytes than SURVEY 8d prices: a fraction above 1 says nothing
        # about the kernel, so the headline fraction becomes the layout one and the other keeps its own name
        r_lpj["frac_algorithmic_bytes_over_roof"] = r_lpj["frac"]
        r_lpj["frac"] = r_lpj["frac_of_layout_bytes"]
        r_lpj["frac_basis"] = "layout bytes (algorithmic-byte pricing exceeds the roof for this layout)"
    r_st = roof(st_ms, st_n, stats_kernels(cfg), "whole statistics pass over the resident K^n (scatter kernel + overflow "
                "levels + column sums + finish; the MFMA contraction is priced under `mfma`)")
    tr = r_st.get("traffic")
    lay_st = layout_bytes_stats(cfg, n_loc)
    r_st["layout_bytes_per_launch"] = lay_st
    r_st["frac_of_layout_bytes"] = (lay_st / (st_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if st_ms > 0 else 0.0
    if tr is None and lay_st < alg_bytes:
        # no counters for this workload and the layout moves fewer bytes than SURVEY 8d prices: the algorithmic-byte
        # fraction would flatter the kernel (c5 float32 mode: 0.99) -- the headline fraction prices the layout bytes
        r_st["frac_algorithmic_bytes_over_roof"] = r_st["frac"]
        r_st["frac"] = r_st["frac_of_layout_bytes"]
        r_st["frac_basis"] = "layout bytes (no PMC counters committed for this workload; below the algorithmic bytes of SURVEY 8d)"
    if tr is not None and tr < alg_bytes:
        # the digest layout moves fewer bytes than SURVEY 8d prices (H = 1024: 8-byte digests for 128-byte bit words):
        # a fraction of algorithmic bytes then flatters the kernel -- the headline fraction prices the measured traffic
        r_st["frac_algorithmic_bytes_over_roof"] = r_st["frac"]
        r_st["frac"] = (tr / (st_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if st_ms > 0 else 0.0
        r_st["frac_basis"] = "measured HBM traffic (below the algorithmic bytes of SURVEY 8d for this layout)"
    # states above two active latents, level by level (census of the last statistics pass) and what the levels cost
    lv = {}
    if all(k in ld for k in ("n_gt2", "n_gt4", "n_gt8")):
        cnt = {"k3_4": ld["n_gt2"] - ld["n_gt4"], "k5_8": ld["n_gt4"] - ld["n_gt8"], "k9plus": ld["n_gt8"]}
        for name, n_states in cnt.items():
            e = {"states": n_states, "fraction_of_K": n_states / (float(n_loc) * cfg["S"])}
            for pas in ("lpj", "stats"):
                km = kernel_ms.get("%s_%s" % (pas, name))
                if km:
                    e["%s_ms_per_pass" % pas] = km["avg_ms"] * km["launches_per_iteration"]
            lv[name] = e
    above2 = {}
    for pas, span in (("lpj", "lpj_pass"), ("stats", "stats_pass")):
        tot = kernel_ms.get(span)
        if tot and lv:
            t_lv = sum(e.get("%s_ms_per_pass" % pas, 0.0) for e in lv.values())
            above2[pas] = {"ms_levels": t_lv, "ms_pass": tot["avg_ms"] * tot["launches_per_iteration"],
                           "fraction_of_pass_above_k2": t_lv / max(1e-12, tot["avg_ms"] * tot["launches_per_iteration"])}
    out = {
        "config": {"ms_per_em_iteration_eager_theta": eager_ms,
                   "eager_theta_note": "the same loop with Theta^new copied to host arrays every iteration, as the reference's "
                                       "step() returns it (a short second loop after the timed region; not `value`)",
                   "estep": estep_diag,
                   "kernel_ms": kernel_ms,
                   "kernel_ms_note": "per-class HIP-event times from %d extra instrumented iterations after the timed region" % prof_iters},
        "roofline": r_lpj, "roofline_stats": r_st,
        "levels": {"by_active_latents": lv, "above_two_latents": above2,
                   "note": "ES3C states by number of active latents (census lists, one pass over the digests per K^n): "
                           "per-level HIP-event times from the instrumented iterations after the timed region"},
    }
    g = gemm_loop or kernel_ms.get("gemm_f64")
    if g:
        t_ms = g["avg_ms"] * g["launches_per_iteration"]
        gi = kernel_ms.get("gemm_f64")
        fl_nom = gemm_flops_per_iteration(cfg, n_loc)
        fl = gemm_flops_per_iteration(cfg, n_loc, executed=True)
        f32 = bool(cfg.get("f32"))
        peak = F32_MFMA_PEAK_TFLOPS if f32 else F64_MFMA_PEAK_TFLOPS
        out["mfma"] = {"kernels": ("gemm_tn128_gk<float> (grouped split-K) / gemm_tn128_sk_f32 / gemm_tn128_store_f32 (v_mfma_f32_16x16x4_f32)" if f32 else
                                   "gemm_tn128_gk (grouped split-K; gemm_tn128_sk_f64 where chunks do not fill the grid) / gemm_tn128_rows_f64 / gemm_tn_f64 / gemm_nn_f64 (v_mfma_f64_16x16x4_f64)"),
                       "flops_per_iteration": fl,
                       "flops_note": "EXECUTED flops: 2 M N K of every product, the symmetric block of the ES3C contraction "
                                     "counted with the upper tiles it really runs (34 of 40 tiles at H = 512); "
                                     "`frac_nominal` prices all tiles",
                       "slots_note": "the K = N contraction, forked beside the Theta-update chain, runs on 14 (30 at H = 1024) of the 15 (32) K "
                                     "chunks per tile a full resident grid would hold (option sk_spare, automatic): the product takes ~6 % "
                                     "longer, the chain hides inside it and the iteration is 2-6 % shorter (DESIGN 3); on all slots "
                                     "the same kernels reach 0.87 of the peak at the north-star shape",
                       "ms_per_iteration": t_ms,
                       "ms_note": "HIP-event spans of the products on the streams they run on, %d iterations after the timed region "
                                  "with only this class timed (the K = N product forked beside the Theta-update chain as in the "
                                  "timed loop); `ms_per_iteration_instrumented`: the same products in the fully instrumented "
                                  "iterations of `kernel_ms` (alone on the main stream between event records)" % prof_iters,
                       "ms_per_iteration_instrumented": (gi["avg_ms"] * gi["launches_per_iteration"]) if gi else None,
                       "achieved": fl / (t_ms * 1e-3) / 1e12, "peak": peak, "unit": "TFLOP/s",
                       "frac": fl / (t_ms * 1e-3) / 1e12 / peak,
                       "flops_per_iteration_nominal": fl_nom,
                       "frac_nominal": fl_nom / (t_ms * 1e-3) / 1e12 / peak}
    if per_rank is not None:
        out["per_rank"] = per_rank
    return out


# ---------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c4", choices=sorted(CONFIGS))
    ap.add_argument("--em-per-step", type=int, default=10, help="EM iterations per step (default 10)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--host-mstep", action="store_true", help="Theta update with host NumPy (reference formulas)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--eager-theta", action="store_true",
                    help="step() copies Theta^new to the host every iteration (3 MB over PCIe + a host copy) like the reference's "
                         "return value; default: LazyTheta, downloaded when it is read (the timed loop never reads it)")
    ap.add_argument("--dense-states", action="store_true",
                    help="SURVEY 8d stress variant: K^n initialised with p_init_Kn = 8/H (mean |s| = 8)")
    ap.add_argument("--inprocess-init", action="store_true",
                    help="draw K^n(0) in this process instead of a worker pool (runs under rocprofv3)")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="evoamd_set_option before the run (A/B of a kernel path, e.g. overlap_gemm=0)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: CPU baseline, roofline spans, per-class kernel "
                         "times, eager-Theta loop, per-rank view")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # bare `bench.py --gpus N`: this parent never initialises HIP; it only starts the ranks and relays rank 0
        stub = os.environ.get("EVO_AMD_BENCH_WORKER")  # tests: a stand-in rank program (no GPU)
        rc, out = launch_ranks(args.gpus, sys.argv[1:], worker=[sys.executable, stub] if stub else None)
        sys.stdout.write(out)
        sys.stdout.flush()
        sys.exit(rc)
    cfg = dict(CONFIGS[args.config])
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    args.gpus = world  # under a launcher the world it built is what runs
    iters = max(1, args.em_per_step)

    # CPU baseline first: it forks worker processes and must run before HIP is initialised
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        log("CPU baseline (oracle on %d cores, ~%.0f s) ..." % (host_cores(), args.cpu_seconds))
        cpu = cpu_baseline(cfg, args.cpu_seconds)
        log("CPU baseline: %.3g evals/s" % cpu["value"])

    from evo_amd.utils import parallel
    b = parallel.shard_bounds(cfg["N"], world)  # np.array_split order (evo/utils/parallel.py:102-112)
    n_loc = int(b[rank + 1] - b[rank])
    # the same job whatever the number of ranks: one dataset, each rank keeps its block
    t_setup = time.perf_counter()
    np.random.seed(1234 + 2)
    Y = np.ascontiguousarray(np.random.randn(cfg["N"], cfg["D"])[b[rank]:b[rank + 1]])
    my_data = {"y": Y, "x_infr": np.ones_like(Y, dtype=bool)}
    workers = max(1, host_cores() // world)
    log("data ready (%d x %d); init_states for %d datapoints on %d workers ..." % (n_loc, cfg["D"], n_loc, workers))
    if args.inprocess_init:
        chunks = list(init_states_inprocess(cfg, n_loc, 4321 + 100003 * rank, dense=args.dense_states))
    else:
        chunks = list(init_states_packed(cfg, n_loc, 4321 + 100003 * rank, workers, dense=args.dense_states))
    log("K^n(0) ready")

    from evo_amd.engine import Engine
    from evo_amd.models import BSC, SSSC

    eng = Engine()  # LOCAL_RANK selects the GPU
    for kv in args.option:
        name, _, val = kv.partition("=")
        eng.set_option(name, int(val))
    comm = parallel.init_rccl_from_env(eng)
    cls = BSC if cfg["algo"] == "ebsc" else SSSC
    kw = {"dtype": np.float32} if cfg.get("f32") else {}
    model = cls(cfg["D"], cfg["H"], cfg["S"], comm=comm, rng="device", sync_host=False, engine=eng, seed=17,
                device_mstep=not args.host_mstep, lazy_theta=not args.eager_theta, **kw)
    np.random.seed(99)
    theta = model.check_params(model.standard_init(my_data))  # data moments all-reduced, W noise broadcast from rank 0
    suff = ea_suff(cfg)
    model.attach_resident_states(suff, my_data, chunks)
    del chunks
    t_setup = time.perf_counter() - t_setup
    log("device resident; warm-up %d + timed %d EM iterations ..." % (args.warmup * iters, args.steps * iters))

    def barrier():
        eng.synchronize()
        comm.Barrier()
        eng.synchronize()

    F = nu = nsub = None
    for _ in range(args.warmup * iters):
        F, nu, nsub, theta = model.step(theta, suff, my_data)
    if args.full:
        # Timed region: HIP events only around the two roofline spans (every timed span costs ~10 us of stream
        # time, so the per-kernel classes are measured in a separate instrumented pass afterwards).
        eng.timing(["lpj_pass", "stats_pass"] + (["allreduce"] if world > 1 else []))
        eng.timing_reset()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps * iters):
        F, nu, nsub, theta = model.step(theta, suff, my_data)
    eng.synchronize()
    dt_own = time.perf_counter() - t0  # this rank alone (its queue drained), before it waits for the others
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        dt = comm.allreduce_max(dt)
    log("timed region %.3f s" % dt)
    if args.dump_outputs and rank == 0:
        names = dump_outputs(args.dump_outputs, eng, F, nu, nsub, theta)
        log("outputs of the last timed step: %d arrays in %s" % (len(names), args.dump_outputs))
    full = None
    if args.full:
        full = full_measurements(args, cfg, eng, comm, model, theta, suff, my_data, barrier, world, rank, n_loc, iters,
                                 dt_own)

    if rank == 0:
        total_iters = args.steps * iters
        evals = float(cfg["N"]) * cfg["S"] * total_iters
        out = {
            "metric": "E-step candidate-state evals/sec (NxS), full EM iteration", "value": evals / dt,
            "unit": "state evals/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32 data + contractions, f64 lpj / sums" if cfg.get("f32") else "f64",
            "data": "synthetic",
            "config": {"workload": cfg["name"], "algo": cfg["algo"], "N_total": cfg["N"], "N_rank0": n_loc,
                       "D": cfg["D"], "H": cfg["H"], "S": cfg["S"],
                       "step": "%d full EM iterations" % iters, "em_iterations_per_step": iters,
                       "em_iterations_timed": total_iters, "ms_per_em_iteration": 1e3 * dt / total_iters,
                       "timed_region_s": dt, "world_size_rccl": comm.size,
                       "ea": "fit/randflip 10 parents x 1 child x 1 gen",
                       "states": "p_init_Kn=8/H (dense stress variant)" if args.dense_states else "p_init_Kn=1/H (init_states default)",
                       "rng": "device", "mstep": "host" if args.host_mstep else "device", "parallelism": "dp%d" % world,
                       "theta": "eager (host copy every iteration)" if args.eager_theta else
                                "lazy view (resident on the device; downloaded when read, never in the timed loop)",
                       "sharding": "np.array_split over N (evo/utils/parallel.py:102-112), one packed RCCL all-reduce per iteration",
                       "free_energy_last": F, "S_nunique_last": nu, "S_sub_last": nsub, "setup_s": round(t_setup, 1)},
        }
        if full is not None:
            out["config"].update(full.pop("config"))
            out.update(full)
        if cpu is not None:
            out["cpu_baseline"] = cpu
        print(json.dumps(out))
        sys.stdout.flush()
    if world > 1:
        comm.Barrier()
        comm.close()
    eng.close()

if __name__ == "__main__":
    main()

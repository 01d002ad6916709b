"""The image-shaped problems of the ``--merge`` modes of tools/time_posterior_samples.py and tools/time_predictive.py:

  g16  a grey 323 x 323 image, 16 x 16 patches, shift 1: N = 94 864, D = 256
  g8   a grey 512 x 512 image, 8 x 8 patches, shift 1:   N = 255 025, D = 64

both ES3C with H = 512 and S = 200, K^n drawn on the device (Engine.init_states, p = pi H / H) and its lpj rows from one
pass over it.  The patch rows are random numbers: the times do not depend on them."""
import time

import numpy as np

from evo_amd.utils.prepost import OverlappingPatches

GEOMETRIES = {"g16": ((323, 323), 16, 16, 1), "g8": ((512, 512), 8, 8, 1),
              "tiny": ((40, 40), 8, 8, 1)}  # (tiny: a rehearsal of the tool, not a measurement)
H_LATENTS, S_STATES = 512, 200
REPEATS = 5  # per figure: the run-to-run spread is printed with every median


def setup(eng, name, piH=2.0):
    """Configure ``eng`` for geometry ``name``; returns (ovp, tag)."""
    shape, ph, pw, shift = GEOMETRIES[name]
    ovp = OverlappingPatches(np.zeros(shape), ph, pw, shift, engine=eng)
    N, D, H, S = ovp.N, ovp.D, H_LATENTS, S_STATES
    rng = np.random.RandomState(1)
    W = rng.normal(size=(D, H)) * 0.3
    A = rng.normal(size=(H, 3)) * 0.2
    eng.set_option("ebsc_f32", 0)
    eng.f32 = False
    eng.configure("sssc", N, D, H, S, 0, 4)
    eng.upload_data(rng.normal(size=(N, D)))
    eng.set_reliable_fraction(None)
    eng.set_params_sssc(W, np.full(H, piH / H), rng.normal(size=H) * 0.5 + 1.0, np.eye(H) + A @ A.T, np.float64(1.0))
    eng.init_states(piH / H, 7)
    eng.lpj_resident()
    return ovp, "%s ES3C %dx%d image, %dx%d patches: N=%d D=%d H=%d S=%d" % (name, shape[0], shape[1], ph, pw, N, D, H, S)


def timed(fn, reps=REPEATS):
    """Wall times in ms of ``reps`` calls of fn (which ends synchronised) after one warm-up, and the last result."""
    out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return np.array(ts), out


def stat(what, v, unit="ms"):
    v = np.asarray(v, dtype=np.float64)
    print("%s: median %.3f %s, min %.3f, max %.3f (%d calls)" % (what, np.median(v), unit, v.min(), v.max(), v.size), flush=True)


def kernel_ms(eng, fn, reps=REPEATS):
    """Device time in ms (HIP events, kernel class "patches": all its launches of one call summed) of ``reps`` calls of fn."""
    fn()
    eng.timing(["patches"])
    ts = []
    for _ in range(reps):
        eng.timing_reset()
        fn()
        eng.synchronize()
        avg, n = eng.kernel_time_ms("patches")
        ts.append(avg * n)
    eng.timing(False)
    return np.array(ts)

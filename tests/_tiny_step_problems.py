"""step() at the lower edge of the latent space (H = 1 ... 4) for test_tiny_latent_space_against_oracle
(test_gpu_models.py), with the CPU checks in test_tiny_step_problems.py.

A case is (algo, D, H, S): N = 23 datapoints from the oracle's own generator, the standard initialisation, K^n from
init_states(N, S, H, "fit", "randflip", parents, children, 1), three chained steps on the reference rng.  oracle_run()
is the float64 reference (oracle/evo_oracle.py: bsc_step / sssc_step), computed once per case and shared by both
device_mstep values; it keeps the condition numbers of the H x H systems every step's update solved."""
import functools
import warnings

import numpy as np

N = 23
STEPS = 3
SHAPES = ((3, 1, 2), (4, 2, 3), (5, 3, 5), (6, 4, 7))  # (D, H, S)
EA = {1: (1, 1), 2: (2, 1), 3: (2, 2), 4: (3, 2)}      # H -> (parents, children); one generation
ALGOS = ("ebsc", "es3c")
SEED_DATA, SEED_INIT, SEED_STATES, SEED_STEP = 31, 32, 33, 200


def generating_theta(algo, D, H):
    rng = np.random.RandomState(1000 + 10 * D + H)
    W = rng.normal(size=(D, H)) * 2.0
    if algo == "ebsc":
        return {"W": W, "pi": 0.5 if H == 1 else 1.5 / H, "sigma": 0.7}
    return {"W": W, "pies": np.full(H, 0.5 if H == 1 else 1.5 / H), "mus": rng.normal(size=H) + 2.0, "Psi": np.eye(H),
            "sigma2": np.float64(0.5)}


@functools.lru_cache(maxsize=None)
def make_case(algo, D, H, S):
    """(Y, theta0): data of the oracle's generator and the oracle's standard initialisation, both seeded."""
    from oracle import evo_oracle as orc
    gen = generating_theta(algo, D, H)
    np.random.seed(SEED_DATA)
    Y = (orc.bsc_generate if algo == "ebsc" else orc.sssc_generate)(gen, N)[0]
    np.random.seed(SEED_INIT)
    theta0 = orc.bsc_standard_init(Y, H) if algo == "ebsc" else orc.sssc_standard_init(Y, H)
    return Y, theta0


def copy_theta(theta):
    th = {k: np.array(v) for k, v in theta.items()}
    for k in ("sigma2", "pi", "sigma"):
        if k in th:
            th[k] = np.float64(th[k])
    return th


def init_args(H, S):
    parents, children = EA[H]
    return (N, S, H, "fit", "randflip", parents, children, 1)


@functools.lru_cache(maxsize=None)
def oracle_run(algo, D, H, S):
    """Per step: {"F", "nu", "nsub", "theta", "ss", "conds", "skipped"}; conds are those of the systems the update solved
    (ES3C: xpt_szsz, xpt_ss + eps I; EBSC: Wq), skipped = the EA of some datapoint found no new state."""
    from oracle import evo_oracle as orc
    Y, theta0 = make_case(algo, D, H, S)
    np.random.seed(SEED_STATES)
    suff = orc.init_states(*init_args(H, S))
    ss0 = suff["ss"].copy()
    th = copy_theta(theta0)
    out = []
    for t in range(STEPS):
        np.random.seed(SEED_STEP + t)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            F, nu, nsub, th, acc = (orc.bsc_step if algo == "ebsc" else orc.sssc_step)(th, suff, Y)
        if algo == "ebsc":
            conds = {"Wq": float(np.linalg.cond(acc["Wq"]))}
        else:
            conds = {"xpt_szsz": float(np.linalg.cond(acc["xpt_szsz"])),
                     "xpt_ss": float(np.linalg.cond(acc["xpt_ss"] + orc.EPS_PSI * np.eye(H)))}
        out.append({"F": float(F), "nu": nu, "nsub": nsub, "theta": copy_theta(th), "ss": suff["ss"].copy(), "conds": conds,
                    "skipped": any("No new and unique states" in str(w.message) for w in seen)})
    return ss0, out

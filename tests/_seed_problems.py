"""Problems for the K^n seeding tests (tests/test_seed_states_host.py, tests/test_gpu_seed_states.py): Gaussian W * 0.8, data
from three active latents plus noise of 0.3, ES3C with an SPD Psi = I + low rank.  The NumPy mirror of a case is computed
once and handed out read-only."""
from functools import lru_cache

import numpy as np

from evo_amd.variational import seed_states_host

# name -> (N, D, H, S, A, S_perm)
CASES = {
    "ragged": (37, 8, 70, 12, 4, 0),     # HW = 2 with a ragged last word; N is no multiple of the waves per workgroup
    "ragged_perm": (37, 8, 70, 12, 4, 1),  # ... with the permanent all-zero state
    "s200": (9, 16, 130, 200, 8, 0),     # 25 states per step, more than 64 states per wave, HW = 3
    "tight": (33, 4, 8, 20, 3, 0),       # quotas 7, 7, 6 close to Hv - t + 1
    "large_h": (5, 8, 1100, 6, 6, 0),    # HW = 18, q_t = 1: the path only
    "wpw2": (5, 4, 2500, 6, 3, 0),       # Hp = 2560: four wavefronts' shares of LDS (41 KB each) exceed 150 KiB, two fit
}
ALGOS = ("ebsc", "es3c")
SEEDS = {name: 100 + i for i, name in enumerate(sorted(CASES))}


def make_theta(rng, algo, D, H):
    W = rng.normal(size=(D, H)) * 0.8
    pi = min(0.4, 3.0 / H)
    if algo == "ebsc":
        return {"W": W, "pi": pi, "sigma": 0.3}
    L = rng.normal(size=(H, 2)) * 0.3
    return {"W": W, "pies": np.full(H, pi) * rng.uniform(0.8, 1.2, H), "mus": rng.normal(size=H) * 0.3 + 1.0,
            "Psi": np.eye(H) + L @ L.T, "sigma2": np.float64(0.09)}


def make_data(rng, algo, theta, N, k=3):
    W = theta["W"]
    D, H = W.shape
    s = np.zeros((N, H), dtype=bool)
    for n in range(N):
        s[n, rng.choice(H, size=min(k, H), replace=False)] = True
    if algo == "ebsc":
        z = np.ones((N, H))
    else:
        z = theta["mus"] + rng.normal(size=(N, H)) @ np.linalg.cholesky(theta["Psi"]).T
    return (s * z) @ W.T + 0.3 * rng.normal(size=(N, D)), s


class SeedProblem:
    pass


@lru_cache(maxsize=None)
def problem(algo, name):
    N, D, H, S, A, S_perm = CASES[name]
    rng = np.random.RandomState(SEEDS[name] + (0 if algo == "ebsc" else 1000))
    p = SeedProblem()
    p.algo, p.N, p.D, p.H, p.S, p.A, p.S_perm = algo, N, D, H, S, A, S_perm
    p.theta = make_theta(rng, algo, D, H)
    p.Y, p.s_true = make_data(rng, algo, p.theta, N)
    p.states, p.path, p.lpj_path, p.margin = seed_states_host("bsc" if algo == "ebsc" else "sssc", p.theta, p.Y, S, A, S_perm)
    for a in (p.Y, p.states, p.path, p.lpj_path, p.margin):
        a.setflags(write=False)
    return p


def quotas(S, A):
    return [S // A + (1 if t <= S % A else 0) for t in range(1, A + 1)]

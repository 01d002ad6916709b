"""Problems for test_gpu_refine.py / test_refine_host.py: K^n refined at fixed Theta (Engine.refine_states,
Model.refine_resident_states) and the per-datapoint scores (Engine.posterior_scores, posterior_scores_host).

The smallest shapes at which the loop and the score kernel can go wrong: N no multiple of the 4 datapoints per workgroup of
the selection and score kernels, S below / above one wavefront, H of one and of three words, both models, the permanent
all-zero column, masks, the float32 mode, the background unit, the general operators with two generations.  K^n and Theta
come from the helpers of _estep_problems.py."""
import numpy as np

from _estep_problems import bsc_theta, es3c_theta, make_kn

# name: (model, N, D, H, S, S_perm, n_parents, n_children, mutation, n_generations, seed_stride, extras)
# extras: "masked" (30 % of the entries missing), "f32" (EBSC float32 mode), "bg" (background unit), "digest0" (word
# de-duplication instead of digests)
COMPOSE = {
    "ebsc_n37": ("bsc", 37, 10, 64, 65, 0, 5, 2, "randflip", 1, 1, ()),
    "es3c_perm": ("sssc", 21, 12, 64, 40, 1, 4, 2, "randflip", 1, 3, ()),
    "ebsc_hw3": ("bsc", 13, 10, 130, 72, 0, 4, 2, "randflip", 1, 1, ()),
    "ebsc_hw3_digest0": ("bsc", 13, 10, 130, 72, 0, 4, 2, "randflip", 1, 1, ("digest0",)),
    "ebsc_masked": ("bsc", 37, 10, 64, 65, 0, 5, 2, "randflip", 1, 1, ("masked",)),
    "es3c_sparseflip_2gen": ("sssc", 21, 12, 64, 40, 0, 4, 2, "sparseflip", 2, 1, ()),
    "ebsc_cross_randflip": ("bsc", 13, 10, 64, 40, 0, 4, 1, "cross_randflip", 1, 3, ()),
    "ebsc_f32": ("bsc", 37, 12, 64, 65, 0, 5, 2, "randflip", 1, 1, ("f32",)),  # (float rows of 16 bytes: D, H multiples of 4)
    "es3c_background": ("sssc", 21, 12, 64, 40, 0, 4, 2, "randflip", 1, 1, ("bg",)),
}
SEED0 = 1234567


class Problem:
    pass


def kn_nonzero(rng, N, S, H, kmax=6):
    """make_kn without the all-zero state (the permanent column holds it when S_perm = 1)."""
    ss = make_kn(rng, N, S + 1, H, kmax=kmax)
    out = np.empty((N, S, H), dtype=bool)
    for n in range(N):
        keep = np.flatnonzero(ss[n].any(axis=1))[:S]
        out[n] = ss[n, keep]
    return out


def cmax(mutation, n_parents, n_children, n_generations):
    per_gen = n_parents * (n_parents - 1) if mutation.startswith("cross") else n_parents * n_children
    return per_gen * n_generations


def compose_problem(name):
    model, N, D, H, S, S_perm, npar, nch, mut, ngen, stride, extras = COMPOSE[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    p = Problem()
    p.name, p.model, p.N, p.D, p.H, p.S, p.S_perm = name, model, N, D, H, S, S_perm
    p.n_parents, p.n_children, p.mutation, p.n_generations, p.seed_stride = npar, nch, mut, ngen, stride
    p.Cmax = cmax(mut, npar, nch, ngen)
    p.extras = extras
    p.bitflip_prob = 1.0 / H if "sparseflip" in mut else None
    p.theta = es3c_theta(rng, D, H) if model == "sssc" else bsc_theta(rng, D, H)
    p.sparseness = float(np.sum(p.theta["pies"])) if model == "sssc" else float(p.theta["pi"]) * H
    p.Y = rng.normal(size=(N, D))
    p.x_infr = (rng.uniform(size=(N, D)) >= 0.3) if "masked" in extras else None
    if "bg" in extras:  # the last latent is on in every state; the others vary
        body = kn_nonzero(rng, N, S, H - 1)
        p.ss = np.concatenate((body, np.ones((N, S, 1), dtype=bool)), axis=2)
    else:
        p.ss = kn_nonzero(rng, N, S, H)
    return p


def logsumexp_rows(lpj):
    m = lpj.max(axis=1)
    return m + np.log(np.exp(lpj - m[:, None]).sum(axis=1))


# ---- score rows ------------------------------------------------------------------------------------------------------
def score_rows(rng, N, L):
    """(N, L) lpj rows with the cases the score kernel must get right: row 0 all equal (entropy log L), row 1 two equal
    maxima (the lower column wins), row 2 a spread above 800 (weights underflow to 0), row 3 the maximum in column 0, row 4
    the maximum in the last column; the others random."""
    lpj = rng.normal(size=(N, L)) * 3.0 - 50.0
    lpj[0] = -7.25
    if L >= 2:
        a, b = sorted(rng.choice(L, 2, replace=False))
        lpj[1, a] = lpj[1, b] = lpj[1].max() + 1.0
        lpj[2] = np.linspace(-900.0, 0.0, L)[rng.permutation(L)]
    if N > 3:
        lpj[3, 0] = lpj[3].max() + 2.0
    if N > 4:
        lpj[4, L - 1] = lpj[4].max() + 2.0
    return lpj


def scores_longdouble(lpj, ss=None, S_perm=0):
    """The definitions of the score kernel evaluated row by row in np.longdouble, first maximum by a plain loop."""
    N, L = lpj.shape
    F, ent, best = np.empty(N, dtype=np.longdouble), np.empty(N, dtype=np.longdouble), np.empty(N, dtype=np.int64)
    k_best, k_mean = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.longdouble)
    for n in range(N):
        row = lpj[n].astype(np.longdouble)
        m, b = row[0], 0
        for s in range(1, L):
            if row[s] > m:
                m, b = row[s], s
        d = row - m
        w = np.exp(d)
        z = w.sum()
        F[n] = m + np.log(z)
        ent[n] = np.log(z) - sum((w[s] * d[s] for s in range(L) if w[s] > 0), np.longdouble(0)) / z
        best[n] = b
        if ss is not None:
            k = np.concatenate((np.zeros(S_perm, dtype=np.int64), ss[n].sum(axis=1)))
            k_best[n] = k[b]
            k_mean[n] = (w * k).sum() / z
    return {"F": F, "entropy": ent, "best": best, "k_best": k_best, "k_mean": k_mean}

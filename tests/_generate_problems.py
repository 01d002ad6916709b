"""Problems and checks shared by test_generate_counter.py (the NumPy mirror, CPU) and test_gpu_generate.py (the kernel):
the law problems with their analytic moments, and the scalar restatement of the stream."""
import numpy as np

LAW_N = 20000
LAW_SEED = 7
LAW_BOUND = 5.0  # standard errors

_M64 = (1 << 64) - 1
GEN_PURPOSE = 0x47454E0000000000


def mix64_int(x):
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & _M64
    return x ^ (x >> 31)


def rng_u01_int(seed, n, purpose, index):
    """rng_u01 of csrc/kernels_evolve.hpp on Python ints."""
    x = mix64_int((seed + 0x9e3779b97f4a7c15 * (n + 1)) & _M64)
    x = mix64_int(x ^ ((purpose * 0xd1b54a32d192ed03 + index + 0x632be59bd9b4e019) & _M64))
    return (float(x >> 11) + 0.5) * (1.0 / 9007199254740992.0)


def sssc_theta(H, D, seed, rank=None, diagonal=False):
    """A Theta from a fixed RandomState.  ``rank`` < H: Psi = A A^T is singular; ``diagonal``: Psi diagonal."""
    rng = np.random.RandomState(seed)
    A = rng.normal(size=(H, H if rank is None else rank))
    Psi = np.diag(rng.uniform(0.5, 2.0, size=H)) if diagonal else np.dot(A, A.T) / A.shape[1]
    return {"W": rng.normal(size=(D, H)), "pies": rng.uniform(0.1, 0.6, size=H), "mus": rng.normal(size=H),
            "Psi": Psi, "sigma2": 0.49}


def bsc_theta(H, D, seed, pi=None):
    rng = np.random.RandomState(seed)
    return {"W": rng.normal(size=(D, H)), "pi": 2.0 / H if pi is None else pi, "sigma": 0.7}


def law_theta(model_name):
    """The law problems: ES3C with H = 8, D = 6 and a Psi of rank 6 (singular); BSC with the same shape."""
    return sssc_theta(8, 6, 11, rank=6) if model_name == "sssc" else bsc_theta(8, 6, 12, pi=0.3)


def analytic_moments(model_name, theta):
    """(E[s], E[y], Cov[y]) of the generative model."""
    W = theta["W"]
    D, H = W.shape
    if model_name == "bsc":
        pi, sigma2 = theta["pi"], theta["sigma"] ** 2
        pies = np.full(H, pi)
        return pies, pi * W.sum(axis=1), pi * (1.0 - pi) * np.dot(W, W.T) + sigma2 * np.eye(D)
    pies, mus, Psi = theta["pies"], theta["mus"], theta["Psi"]
    m = pies * mus
    M2 = np.outer(pies, pies) * (Psi + np.outer(mus, mus))        # h != h'
    M2[np.diag_indices(H)] = pies * (np.diag(Psi) + mus ** 2)     # the diagonal
    return pies, np.dot(W, m), np.dot(W, np.dot(M2 - np.outer(m, m), W.T)) + theta["sigma2"] * np.eye(D)


def law_zscores(model_name, theta, out):
    """Worst |deviation| / SE of the mean of s, the mean of y and the covariance of y from their analytic values:
    analytic SEs for the means, the sample SE of the centred products for the covariance."""
    pies, Ey, Cy = analytic_moments(model_name, theta)
    s, y = out["s"], out["y"]
    N = y.shape[0]
    z_s = np.abs(s.mean(axis=0) - pies) / np.sqrt(pies * (1.0 - pies) / N)
    z_mean = np.abs(y.mean(axis=0) - Ey) / np.sqrt(np.diag(Cy) / N)
    yc = y - y.mean(axis=0)
    prod = yc[:, :, None] * yc[:, None, :]
    z_cov = np.abs(prod.mean(axis=0) - Cy) / (prod.std(axis=0) / np.sqrt(N))
    return float(z_s.max()), float(z_mean.max()), float(z_cov.max())


def assert_law(model_name, theta, out, label):
    z_s, z_mean, z_cov = law_zscores(model_name, theta, out)
    print("%s %s: worst z-scores s %.2f, mean(y) %.2f, cov(y) %.2f (bound %.1f)" % (label, model_name, z_s, z_mean, z_cov,
                                                                                   LAW_BOUND))
    assert z_s <= LAW_BOUND and z_mean <= LAW_BOUND and z_cov <= LAW_BOUND, (z_s, z_mean, z_cov)

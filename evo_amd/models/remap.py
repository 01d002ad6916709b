"""Theta in a new latent numbering (host; the arrays are small).  The counterpart for K^n runs on the device:
Model.remap_latents / Engine.remap_latents, mirrored by evo_amd.variational.remap_states_host."""
import numpy as np

# keys the models derive from Theta (E_step_precompute, update_params): dropped, so that they are rebuilt for H'
_DERIVED = ("piH", "pre1", "pil_bar", "ljc", "sigma2_inv")


def remap_theta(model_name, theta, index, W_new=None, pies_new=None, mus_new=None, Psi_diag_new=None, rng=None):
    """``theta`` with its latents renumbered by ``index`` (int (H',): a source latent, or -1 for a new one): a new dict.
    W' = W[:, index]; ES3C pies' = pies[index], mus' = mus[index], Psi' = Psi[np.ix_(index, index)], sigma2 unchanged;
    EBSC pi and sigma unchanged -- pi is PER LATENT, so the expected number of active latents pi H' changes with H' (the
    optional key "pies" of a trained EBSC Theta is gathered too).  Derived keys (piH, pre1, pil_bar, ljc, sigma2_inv) are
    dropped: check_params / E_step_precompute rebuild them.
    The columns of the -1 entries: ``W_new`` (D, n_new) or, None, the mean of the kept columns plus N(0, (sigma / 4)^2)
    noise from ``rng`` (standard_init's rule with the current sigma; ``rng`` a np.random.RandomState / Generator, None:
    np.random); ``pies_new``, ``mus_new``, ``Psi_diag_new`` (n_new,) or, None, the mean of the kept entries (of the kept
    diagonal for Psi); new off-diagonal entries of Psi are 0.  Gathered entries are copied bit for bit."""
    sssc = model_name not in ("bsc", "BSC", "ebsc")
    W = np.asarray(theta["W"], dtype=np.float64)
    D, H = W.shape
    idx = np.asarray(index)
    if idx.ndim != 1 or idx.size < 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("remap_theta: index must be a one-dimensional integer array with at least one entry")
    idx = idx.astype(np.intp)
    if ((idx < -1) | (idx >= H)).any():
        raise ValueError("remap_theta: index entries must be -1 or in [0, %d)" % H)
    old = idx >= 0
    if np.unique(idx[old]).size != old.sum():
        raise ValueError("remap_theta: a source latent is named twice")
    new = ~old
    n_new, H2 = int(new.sum()), idx.size
    if n_new and not old.any():
        raise ValueError("remap_theta: no latent is kept: the defaults of the new columns are means of the kept ones")
    rng = np.random if rng is None else rng

    def column_values(given, kept, name):
        if given is None:
            return np.full(n_new, kept.mean())
        given = np.asarray(given, dtype=np.float64)
        if given.shape != (n_new,):
            raise ValueError("remap_theta: %s must have shape (%d,)" % (name, n_new))
        return given

    out = {k: v for k, v in theta.items() if k not in _DERIVED}
    sigma = np.sqrt(float(theta["sigma2"])) if sssc else float(theta["sigma"])
    W2 = np.empty((D, H2))
    W2[:, old] = W[:, idx[old]]
    if n_new:
        if W_new is None:
            W2[:, new] = W[:, idx[old]].mean(axis=1)[:, None] + rng.normal(scale=sigma / 4.0, size=(D, n_new))
        else:
            W_new = np.asarray(W_new, dtype=np.float64)
            if W_new.shape != (D, n_new):
                raise ValueError("remap_theta: W_new must have shape (%d, %d)" % (D, n_new))
            W2[:, new] = W_new
    out["W"] = W2
    if sssc:
        for key, given in (("pies", pies_new), ("mus", mus_new)):
            v = np.asarray(theta[key], dtype=np.float64)
            v2 = np.empty(H2)
            v2[old] = v[idx[old]]
            if n_new:
                v2[new] = column_values(given, v[idx[old]], key + "_new")
            out[key] = v2
        Psi = np.asarray(theta["Psi"], dtype=np.float64)
        Psi2 = np.zeros((H2, H2))
        Psi2[np.ix_(old, old)] = Psi[np.ix_(idx[old], idx[old])]
        if n_new:
            Psi2[new, new] = column_values(Psi_diag_new, np.diag(Psi)[idx[old]], "Psi_diag_new")
        out["Psi"] = Psi2
    elif "pies" in theta:
        v = np.asarray(theta["pies"], dtype=np.float64)
        v2 = np.empty(H2)
        v2[old] = v[idx[old]]
        if n_new:
            v2[new] = column_values(pies_new, v[idx[old]], "pies_new")
        out["pies"] = v2
    return out

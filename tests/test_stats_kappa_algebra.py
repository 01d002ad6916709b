"""The algebra of the kappa route of the ES3C statistics pass, in NumPy on the oracle's own per-state quantities: the Lam
terms of the second moments of the states with one or two active latents depend on the active set only, so they factor out
of the sum over the datapoints -- the pass may collect sum q (P1 per singleton, P per pair), sum q kappa_i kappa_j and
sum q kappa^2 and put Lam back once per active set (csrc/kernels_sssc.hpp: sssc_kappa_diag_body, sssc_finish_kernel),
while the states above two latents keep their Lam-complete contributions.  Psi is made non-symmetric, so Lam_01 != Lam_10."""
import os
import re

import numpy as np

import _stats_problems as sp
from oracle import evo_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem():
    p = sp.make_problem("es_mid")
    H = p["H"]
    C = 0.05 * np.random.RandomState(77).normal(size=(H, H))
    p["theta"] = dict(p["theta"], Psi=p["theta"]["Psi"] + (C - C.T))
    return p


def test_lam_terms_factor_out_of_the_sum_over_datapoints():
    p = _problem()
    N, D, H, S, Y, ss = p["N"], p["D"], p["H"], p["S"], p["Y"], p["ss"]
    suff = {"ss": ss, "lpj": np.empty((N, S)), "S_perm": 0, "incl": np.zeros((0, H), dtype=bool), "Mprime": S}
    want = orc.sssc_EM_accumulate(dict(p["theta"]), suff, Y, use_storage=True, evolve=False)
    z = want["xpt_szsz"]
    assert np.abs(z - z.T).max() > 1e-3 * np.abs(z).max()  # visibly asymmetric: the case exercises Lam_01 != Lam_10

    theta = dict(p["theta"])
    orc.sssc_precompute(theta, D)
    mus = theta["mus"]
    cache = {}
    xs = np.zeros(H)
    P1 = np.zeros(H)               # sum q over the singleton states {i}
    P = np.zeros((H, H))           # sum q over the pair states {i, j}, i < j
    K = np.zeros((H, H))           # sum q kappa_i kappa_j over them, i < j
    kd = np.zeros(H)               # sum q kappa_i^2 over the states with one or two latents
    Q = np.zeros((H, H))           # states above two latents, Lam-complete: sum q (i < j) ...
    UL = np.zeros((H, H))          # ... sum q (Lam + kappa kappa^T), both triangles ...
    Dg = np.zeros(H)               # ... and its diagonal
    for n in range(N):
        lpj = suff["lpj"][n]
        q = np.exp(lpj + np.minimum(orc.B_MAX - lpj.max(), orc.B_MAX_SHFT))
        qn = q / (q.sum() + orc.F64_TINY)
        for s in range(S):
            st = ss[n, s]
            idx = np.flatnonzero(st)
            if idx.size == 0:
                continue
            key = st.tobytes()
            if key not in cache:
                cache[key] = orc.sssc_state_terms(theta, st)
            t = cache[key]
            kappa = np.dot(t["lam_Wt"], Y[n] - t["Wmu"]) + mus[st]
            xs[idx] += qn[s]
            if idx.size == 1:
                P1[idx[0]] += qn[s]
                kd[idx[0]] += qn[s] * kappa[0] ** 2
            elif idx.size == 2:
                i, j = idx
                P[i, j] += qn[s]
                K[i, j] += qn[s] * kappa[0] * kappa[1]
                kd[i] += qn[s] * kappa[0] ** 2
                kd[j] += qn[s] * kappa[1] ** 2
            else:
                sec = qn[s] * (t["lam"] + np.outer(kappa, kappa))
                for a in range(idx.size):
                    Dg[idx[a]] += sec[a, a]
                    for b in range(a + 1, idx.size):
                        Q[idx[a], idx[b]] += qn[s]
                        UL[idx[a], idx[b]] += sec[a, b]
                        UL[idx[b], idx[a]] += sec[b, a]
    assert P1.any() and P.any() and Q.any()

    def lam_of(*latents):
        st = np.zeros(H, dtype=bool)
        st[list(latents)] = True
        return orc.sssc_state_terms(theta, st)["lam"]

    # the finish kernels' formulas
    xss = np.zeros((H, H))
    xszsz = np.zeros((H, H))
    diag = kd + Dg
    for i in range(H):
        if P1[i] != 0.0:
            diag[i] += lam_of(i)[0, 0] * P1[i]
        for j in range(i + 1, H):
            xss[i, j] = xss[j, i] = Q[i, j] + P[i, j]
            upper, lower = UL[i, j] + K[i, j], UL[j, i] + K[i, j]
            if P[i, j] != 0.0:
                lam = lam_of(i, j)
                upper += lam[0, 1] * P[i, j]
                lower += lam[1, 0] * P[i, j]
                diag[i] += lam[0, 0] * P[i, j]
                diag[j] += lam[1, 1] * P[i, j]
            xszsz[i, j], xszsz[j, i] = upper, lower
    xss[np.arange(H), np.arange(H)] = xs
    xszsz[np.arange(H), np.arange(H)] = diag
    for got, name in ((xss, "xpt_ss"), (xszsz, "xpt_szsz")):
        scale = np.abs(want[name]).max()
        assert np.abs(got - want[name]).max() <= 1e-12 * scale, name


def test_later_options_are_documented():
    """tests/test_host_logic.py writes out the names of the library's first option table; the options added since (a second
    table, so that the first one and its test stay as they are) are held to the same rule here: one row per name, described
    in include/evo_amd.h and listed in INTEGRATION.md."""
    src = open(os.path.join(ROOT, "evo_amd", "csrc", "evo_amd.hip")).read()
    body = src[src.index("static const OptionRow OPTIONS_LATER[] = {"):]
    body = body[:body.index("\n};")]
    rows = re.findall(r'^  \{"([a-z0-9_]+)", OPT_', body, re.M)
    assert rows == ["stats_kappa", "stats_kappa_min"], rows
    first = src[src.index("static const OptionRow OPTIONS[] = {"):]
    first = first[:first.index("\n};")]
    assert not set(rows) & set(re.findall(r'\{"([a-z0-9_]+)", OPT_', first))
    header = open(os.path.join(ROOT, "include", "evo_amd.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in rows:
        assert '"%s"' % n in header, "include/evo_amd.h does not document option " + n
        assert '"%s"' % n in integ, "INTEGRATION.md does not list option " + n

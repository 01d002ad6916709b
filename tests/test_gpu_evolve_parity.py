"""The device EA (evolve_randflip_kernel, evolve_general_kernel) against its NumPy mirror, bit for bit.

The kernels draw from a counter-based stream, so for a given (seed, n) the parents, flips, cuts and sparse flips are
fixed, and evo_amd.variational.eas_counter restates them from the law (test_evolve_counter_host.py ties that mirror to
the reference).  Per case (_evolve_problems.py: 256 distinct datapoints, the lpj rows uploaded) the candidate batch and
the counts must equal the mirror's on every decided datapoint, the candidate lpj must equal the float64 oracle's to
rtol 1e-9, and the batch must not depend on the "state_digest" option or on being drawn a second time.

Decided: the kernels rank parents by the float32 key -log(u) / p.  The mirror forms the key in float64 from the same
float32-rounded u and p and leaves a datapoint out, from the generation on, whose smallest relative gap among the first
P + 1 sorted keys is below TAU = 2^-18.  Derivation: from the shared float32 inputs the device key passes through at
most six float32 steps -- two conversions, v_log_f32, the multiplication by ln 2, v_rcp_f32 and a multiplication -- each
within 1 ULP = 2^-23 relative (the figures of the ISA documentation for the two transcendental instructions; the
compiler's math header here maps __logf and __fdividef to the builtin logarithm and a plain division, which are no
worse), so it lies within 6 * 2^-23 < 2^-20 of the float64 key; TAU takes a factor 4 over that.  TAU was fixed before
any device result was seen.  At most 2 % of a case's datapoints may be undecided (asserted here and, from the mirror
alone, in the host module).  Sparseflip's two float64 transcendental steps have the same rule with margins 1e-9 (distance
of log(u) / log1p(-p0) from an integer) and 1e-12 (relative, u against p1); no datapoint is expected to meet them."""
import numpy as np
import pytest

import _evolve_problems as vp

pytestmark = pytest.mark.gpu

TAU = 2.0 ** -18
UNDECIDED_CAP = 0.02
LPJ_RTOL = 1e-9


@pytest.fixture(scope="module")
def engine():
    from evo_amd.engine import Engine
    eng = Engine()
    yield eng
    eng.set_option("state_digest", 1)
    eng.set_option("background_unit", 0)
    eng.close()


def _evolve(engine, p):
    c = p["case"]
    if p["name"] in vp.FAST:
        engine.evolve_randflip(c.n_parents, c.n_children, p["seed"], bool(c.fit))
    else:
        engine.evolve_states(c.mutation, c.n_parents, c.n_children, c.n_gen, p["seed"], bool(c.fit), c.sparseness, c.p_bf)
    return engine.download_candidates()


def _device(engine, p, state_digest, calls):
    """``calls`` x (the children of problem p, downloaded) with the option "state_digest" as given."""
    engine.set_option("state_digest", state_digest)  # read by evoamd_configure
    engine.set_option("background_unit", p["bg"])
    engine.configure(p["model"], p["N"], p["D"], p["H"], p["S"], p["S_perm"], p["Cmax"])
    engine.upload_data(p["Y"])
    th = p["theta"]
    if p["model"] == "sssc":
        engine.set_params_sssc(th["W"], th["pies"], th["mus"], th["Psi"], float(th["sigma2"]))
    else:
        engine.set_params_bsc(th["W"], float(th["pi"]), float(th["sigma"]))
    engine.upload_states(p["ss"])
    if p["model"] == "sssc":
        engine.lpj_resident()  # (the pass that precedes the children in an E-step: it sizes the ES3C levels)
    engine.upload_lpj(p["lpj"])  # generation 0 depends on no device lpj
    return [_evolve(engine, p) for _ in range(calls)]


def _valid(counts, Cmax):
    return np.arange(Cmax)[None, :] < counts[:, None]


def _same_batches(a, b, label, lpj_exact):
    assert np.array_equal(a[1], b[1]), label + ": counts differ"
    v = _valid(a[1], a[0].shape[1])
    assert np.array_equal(a[0][v], b[0][v]), label + ": candidates differ"
    if lpj_exact:
        assert np.array_equal(a[2][v], b[2][v]), label + ": candidate lpj differ"
    else:
        np.testing.assert_allclose(a[2][v], b[2][v], rtol=1e-12, err_msg=label)


@pytest.mark.parametrize("mutation", ["cross", "cross_randflip", "cross_sparseflip"])
def test_crossover_is_refused_at_one_latent(engine, mutation):
    """H = 1 has no cut point (randint(1, H) is empty): evoamd_evolve_states refuses by name, changes nothing in the
    context (the validity words before and after are the same) and the next call on it is served: randflip_h1 still
    gives the mirror's batch."""
    from evo_amd.engine import EvoAmdError
    p = dict(vp.make_problem("randflip_h1"), Cmax=2)  # (room for the 2 x 1 children of two crossed parents: no other refusal)
    assert p["H"] == 1 and p["S"] == 2
    try:
        (first,) = _device(engine, p, 1, 1)
        before = engine.debug_validity()
        with pytest.raises(EvoAmdError, match="crossover needs H >= 2"):
            engine.evolve_states(mutation, 2, 1, 1, p["seed"], True, 1.0, 0.25)
        assert engine.debug_validity() == before
        again = _evolve(engine, p)
    finally:
        engine.set_option("state_digest", 1)
        engine.set_option("background_unit", 0)
    _same_batches(first, again, "randflip_h1 after the refused %s" % mutation, True)
    m_cand, m_counts, _ = vp.run_mirror(p, lambda n, slot0, new: first[2][n, slot0:slot0 + new.shape[0]])
    assert np.array_equal(first[1], m_counts) and not m_counts.any()  # S = 2^H: no child is new


@pytest.mark.parametrize("name", list(vp.CASES))
def test_children_match_the_mirror(engine, name):
    from evo_amd.variational import eas_counter as ec
    p = vp.make_problem(name)
    N, Cmax = p["N"], p["Cmax"]
    try:
        first, second = _device(engine, p, 1, 2)
        (words,) = _device(engine, p, 0, 1)
    finally:
        engine.set_option("state_digest", 1)
        engine.set_option("background_unit", 0)
    cand, counts, clpj = first
    assert counts.min() >= 0 and counts.max() <= Cmax
    # ---- the mirror, fed with the device's own candidate lpj by slot (valid while the earlier slots matched)
    m_cand, m_counts, info = vp.run_mirror(p, lambda n, slot0, new: clpj[n, slot0:slot0 + new.shape[0]])
    und = ec.undecided(info, TAU)
    share = und[:, -1].mean()
    print("%s: undecided share %.4f (%d of %d)" % (name, share, und[:, -1].sum(), N))
    assert share <= UNDECIDED_CAP, (name, share)
    G = und.shape[1]
    gen_counts = info["gen_counts"] if "gen_counts" in info else np.stack((np.zeros(N, dtype=np.int64), m_counts), axis=1)
    bad = []
    for n in range(N):
        g_und = int(np.argmax(und[n])) if und[n].any() else G   # first undecided generation
        upto = int(gen_counts[n, g_und])                        # the candidates of the decided generations
        ok = np.array_equal(cand[n, :upto], m_cand[n, :upto]) and counts[n] >= upto
        if g_und == G:
            ok = ok and counts[n] == m_counts[n]
        if not ok:
            bad.append(n)
    assert not bad, "%s: %d decided datapoints differ from the mirror, first %s (counts %s, mirror %s)" % (
        name, len(bad), bad[:8], counts[bad[:8]], m_counts[bad[:8]])
    # ---- candidate lpj against the float64 oracle
    for n in range(N):
        if counts[n]:
            np.testing.assert_allclose(clpj[n, :counts[n]], vp.oracle_lpj(p, cand[n, :counts[n]], n), rtol=LPJ_RTOL,
                                       err_msg="%s: candidate lpj of datapoint %d" % (name, n))
    # ---- the same batch drawn again, and with word de-duplication
    _same_batches(first, second, name + ", second call", True)
    _same_batches(first, words, name + ", state_digest 0", False)

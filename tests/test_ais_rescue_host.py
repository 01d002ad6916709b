"""The AIS rescue on the CPU: the NumPy mirrors alone (evo_amd.models.ais_posterior_counter with ``index``,
evo_amd.models.ais_admit_candidates_host).

1. a listed mirror equals the rows of the full one bit for bit; 2. the emission mirror against a naive restatement of the
law, on the hand-made inputs; 3. the end-to-end problem of the GPU tests reaches its edges; 4. the caps on undecided chains
hold for the lists the GPU tests use; 5. the list's refusals.
"""
import numpy as np
import pytest

import _ais_masked_problems as mp
import _ais_post_problems as pp
import _ais_rescue_problems as rp
from evo_amd.models import ais_admit_candidates_host, ais_posterior_counter, state_digest
from evo_amd.models.ais import check_index


# ---- 1. listed equals full -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_words", "partial_chunk"])
def test_listed_mirror_is_the_rows_of_the_full_one(name):
    p = pp.problem(name)
    I = np.array(rp.LISTS[name])
    assert I[0] == 0 and I[-1] == p.N - 1 and (np.diff(I) > 1).any()
    got = ais_posterior_counter(p.theta, p.Y, n_chains=p.C, n_temps=p.T, n_keep=p.K, seed=pp.STREAM_SEED, mean=True, index=I)
    assert got.keys() == p.want.keys()
    for k, v in p.want.items():
        if k == "mean":  # p W^T through BLAS, whose blocking depends on the number of rows: the product of the same rows
            assert np.allclose(got[k], np.dot(p.want["p"][I], p.theta["W"].T), rtol=1e-14, atol=1e-14), k
        else:
            assert got[k].shape == v[I].shape and np.array_equal(got[k], v[I]), k
    # first_index is added to the list's entries
    cut = int(I[1])
    shifted = ais_posterior_counter(p.theta, p.Y[cut:], n_chains=p.C, n_temps=p.T, n_keep=p.K, seed=pp.STREAM_SEED, first_index=cut,
                                    index=I[1:] - cut)
    for k in ("log_w", "rb", "chain_map_state", "p"):
        assert np.array_equal(shifted[k], p.want[k][I[1:]]), k
    # an empty list
    empty = ais_posterior_counter(p.theta, p.Y, n_chains=p.C, n_temps=p.T, n_keep=p.K, seed=pp.STREAM_SEED, index=[])
    assert empty["p"].shape == (0, p.H) and empty["log_w"].shape == (0, p.C)


def test_listed_mirror_on_incomplete_data():
    name, missing = rp.MASKED_CASE
    p = mp.problem(name, missing)
    I = np.array(rp.MASKED_LIST)
    got = ais_posterior_counter(p.theta, p.Y, n_chains=mp.C, n_temps=mp.T, n_keep=3, seed=mp.STREAM_SEED, x_infr=p.x_infr, index=I)
    for k in ("log_w", "rb", "chain_map_state", "chain_flips", "p", "p_se", "map_state", "ll", "margin"):
        assert np.array_equal(got[k], p.post[3][k][I]), k


# ---- 2. the emission law -------------------------------------------------------------------------------------------------------
def _naive(lpj, st, kn, Cmax):
    """The law restated without any ordering structure: O(C^2) comparisons per datapoint."""
    C = len(lpj)
    fin = [c for c in range(C) if np.isfinite(lpj[c])]

    def ahead(a, b):  # chain a ranks before chain b
        return lpj[a] > lpj[b] or (lpj[a] == lpj[b] and a < b)

    def same(a, b):
        return bool((st[a] == st[b]).all())

    distinct = [c for c in fin if st[c].any() and not any(ahead(o, c) and same(o, c) for o in fin)]
    new = [c for c in distinct if not any((kn[s] == st[c]).all() for s in range(len(kn)))]
    place = {c: sum(ahead(o, c) for o in new) for c in new}
    taken = sorted((c for c in new if place[c] < Cmax), key=lambda c: place[c])
    top = 0
    if lpj[0] == lpj[0]:
        for c in range(1, C):
            if lpj[c] > lpj[top]:
                top = c
    held = any((kn[s] == st[top]).all() for s in range(len(kn)))
    return taken, len(distinct), len(new), held


def test_emission_mirror_obeys_the_law_on_the_hand_made_inputs():
    lpj, st = rp.hand_inputs()
    kn = rp.hand_kn()
    Cmax = rp.HAND["Cmax"]
    want_chains = {0: [1, 2, 4], 1: [4, 3, 6], 2: [3], 4: [2, 5], 5: [1, 2, 3]}
    want_counts = {0: (7, 7, 3, False), 1: (4, 4, 3, True), 2: (1, 1, 1, False), 4: (3, 2, 2, False), 5: (6, 5, 3, True)}
    for i, n in enumerate(rp.HAND_INDEX):
        cand, cnt = ais_admit_candidates_host(lpj[i], st[i], kn[n], Cmax)
        taken, n_distinct, n_new, held = _naive(lpj[i], st[i], kn[n], Cmax)
        assert cnt["chains"] == taken == want_chains[int(n)], (n, cnt["chains"], taken)
        assert (cnt["n_distinct"], cnt["n_new"], cnt["n_proposed"], cnt["map_held"]) == (n_distinct, n_new, len(taken), held)
        assert (n_distinct, n_new, len(taken), held) == want_counts[int(n)], (n, n_distinct, n_new, len(taken), held)
        assert np.array_equal(cand, st[i][taken]) and cand.shape == (len(taken), rp.HAND["H"])
        # every clause by itself
        assert cand.any(axis=1).all(), "the all-zero state was taken"
        assert len({row.tobytes() for row in cand}) == len(cand), "a state was taken twice"
        assert not any((kn[n] == row).all(axis=1).any() for row in cand), "a state K^n holds was taken"
        assert np.isfinite(lpj[i][taken]).all() and len(taken) <= Cmax and cnt["n_proposed"] == min(cnt["n_new"], Cmax)
        assert list(lpj[i][taken]) == sorted(lpj[i][taken], reverse=True)
    # the edges the inputs are there for
    assert max(c["n_new"] for _, c in (ais_admit_candidates_host(lpj[i], st[i], kn[n], Cmax)
                                         for i, n in enumerate(rp.HAND_INDEX))) > Cmax
    assert 3 not in rp.HAND_INDEX


def test_state_digest():
    assert state_digest(np.zeros(70, dtype=bool)) == 0
    s = np.zeros(70, dtype=bool)
    s[[3, 69]] = True
    assert state_digest(s) == 2 | (3 << 8) | (69 << 22)
    s[[0, 1, 2, 4]] = True  # six active: the first four are kept
    assert state_digest(s) == 6 | (0 << 8) | (1 << 22) | (2 << 36) | (3 << 50)


# ---- 3. the end-to-end problem reaches its edges -------------------------------------------------------------------------------
def test_admit_problem_reaches_its_edges():
    q = rp.admit_problem()
    p = q.p
    assert q.Cmax < p.C
    counts = [c for _, c in q.emit]
    assert any(c["n_new"] > 0 for c in counts), "no listed datapoint has a new state"
    assert any(c["n_distinct"] < p.C for c in counts), "no listed datapoint has duplicate chain best states"
    assert any(c["map_held"] for c in counts), "K^n holds no listed datapoint's map_state"
    for (cand, c), n in zip(q.emit, q.index):
        assert c["n_proposed"] <= c["n_new"] <= c["n_distinct"] <= p.C
        assert not any((q.ss[n] == row).all(axis=1).any() for row in cand)
    # at least half of the listed datapoints have every chain decided: the GPU test can check them against host selection
    decided = (p.want["margin"][q.index] > rp.MARGIN_DECIDED).all(axis=1)
    assert decided.sum() * 2 >= len(q.index)


# ---- 4. the caps on undecided chains -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rp.LISTS))
def test_undecided_share_of_the_lists(name):
    p = pp.problem(name)
    m = p.want["margin"][np.array(rp.LISTS[name])]
    assert m.min() > pp.MARGIN_CPU
    assert (m <= rp.MARGIN_DECIDED).sum() <= rp.MAX_UNDECIDED * m.size


# ---- 5. the list's refusals ----------------------------------------------------------------------------------------------------
def test_check_index_names_the_first_offender():
    assert check_index([0, 2, 5], 6).dtype == np.int64 and check_index([], 6).size == 0
    for bad, match in (([0, 2, 2], r"index\[2\] = 2 is repeated"), ([0, 3, 1, 0], r"index\[2\] = 1 descends"),
                       ([0, 6], r"index\[1\] = 6 is outside \[0, N = 6\)"), ([-1, 0], r"index\[0\] = -1 is outside"),
                       ([[0, 1]], "1-d integer array"), ([0.0, 1.0], "1-d integer array")):
        with pytest.raises(ValueError, match=match):
            check_index(bad, 6)

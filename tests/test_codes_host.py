"""evo_amd.codes on the host: the selection rule of codes_from_dense (the NumPy mirror of posterior_codes_kernel),
PosteriorCodes.to_dense and the arithmetic behind map_q.  No GPU."""
import numpy as np
import pytest

from evo_amd.codes import F64_TINY, PosteriorCodes, _wave_sum, codes_exp, codes_from_dense


def _problem(seed=0, N=6, H=11, S=5, S_perm=0):
    rng = np.random.RandomState(seed)
    ss = rng.random_sample((N, S, H)) < 0.3
    Es = rng.random_sample((N, H)) * (rng.random_sample((N, H)) < 0.5)
    Ez = rng.normal(size=(N, H)) * (Es > 0)
    lpj = rng.normal(size=(N, S + S_perm)) * 5
    return Es, Ez, lpj, ss


def test_order_is_descending_p_then_ascending_index():
    Es = np.array([[0.1, 0.7, 0.0, 0.7, 0.3, 0.7],
                   [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])
    Ez = Es * 10 + np.arange(6)
    lpj = np.zeros((2, 3))
    ss = np.zeros((2, 3, 6), dtype=bool)
    c = codes_from_dense(Es, Ez, lpj, ss, max_active=4)
    assert c.idx.dtype == np.int32 and c.nnz.dtype == np.int32 and c.map_slot.dtype == np.int32
    np.testing.assert_array_equal(c.idx, [[1, 3, 5, 4], [0, 1, 2, 3]])  # the 0.7 tie: lower index first
    np.testing.assert_array_equal(c.p, [[0.7, 0.7, 0.7, 0.3], [0.5, 0.5, 0.5, 0.5]])
    np.testing.assert_array_equal(c.m, Ez[np.arange(2)[:, None], c.idx])
    np.testing.assert_array_equal(c.nnz, [5, 6])


def test_map_tie_takes_the_first_slot_and_permanent_slot_is_all_zero():
    Es, Ez, lpj, ss = _problem(S_perm=1)
    lpj[0, :] = [-3.0, 2.5, -1.0, 2.5, 2.5, 0.0]   # tie between K^n slots 1, 3, 4 -> 1
    lpj[1, :] = [4.0, 4.0, -1.0, 0.0, 1.0, 2.0]    # tie between the permanent slot and slot 1 -> 0
    c = codes_from_dense(Es, Ez, lpj, ss, S_perm=1)
    np.testing.assert_array_equal(c.map_slot, np.argmax(lpj, axis=1))
    assert c.map_slot[0] == 1 and c.map_slot[1] == 0
    np.testing.assert_array_equal(c.map_state[0], np.packbits(ss[0, 0]))
    assert not c.map_state[1].any()
    want = np.where((c.map_slot >= 1)[:, None], ss[np.arange(6), np.maximum(c.map_slot - 1, 0)], False)
    np.testing.assert_array_equal(c.map_states(), want)
    assert (c.map_slot[2:] >= 1).any()


def test_truncation_reports_nnz_and_short_codes_are_padded():
    Es = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3],
                   [0.0, 0.2, 0.0, 0.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    c = codes_from_dense(Es, -Es, np.zeros((3, 2)), np.zeros((3, 2, 7), dtype=bool), max_active=3)
    np.testing.assert_array_equal(c.nnz, [7, 1, 0])
    np.testing.assert_array_equal(c.truncated, [True, False, False])
    np.testing.assert_array_equal(c.idx, [[0, 1, 2], [1, -1, -1], [-1, -1, -1]])
    np.testing.assert_array_equal(c.p, [[0.9, 0.8, 0.7], [0.2, 0.0, 0.0], [0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(c.m, [[-0.9, -0.8, -0.7], [-0.2, 0.0, 0.0], [0.0, 0.0, 0.0]])
    # max_active above H: every slot beyond the row is padding
    c = codes_from_dense(Es, None, np.zeros((3, 2)), np.zeros((3, 2, 7), dtype=bool), max_active=64)
    assert c.idx.shape == (3, 64) and c.m is None
    np.testing.assert_array_equal(c.idx[0, :8], [0, 1, 2, 3, 4, 5, 6, -1])
    assert (c.idx[:, 7:] == -1).all() and (c.p[:, 7:] == 0).all()


def test_p_min_excludes_an_equal_entry_and_keeps_a_larger_one():
    v = 0.25
    Es = np.array([[v, np.nextafter(v, 1.0), np.nextafter(v, 0.0), 0.9]])
    c = codes_from_dense(Es, None, np.zeros((1, 2)), np.zeros((1, 2, 4), dtype=bool), max_active=4, p_min=v)
    np.testing.assert_array_equal(c.idx, [[3, 1, -1, -1]])
    np.testing.assert_array_equal(c.nnz, [2])
    assert c.p_min == v
    with pytest.raises(ValueError):
        codes_from_dense(Es, None, np.zeros((1, 2)), np.zeros((1, 2, 4), dtype=bool), p_min=-0.1)
    with pytest.raises(ValueError):
        codes_from_dense(Es, None, np.zeros((1, 2)), np.zeros((1, 2, 4), dtype=bool), p_min=float("nan"))
    for bad in (0, 65):
        with pytest.raises(ValueError):
            codes_from_dense(Es, None, np.zeros((1, 2)), np.zeros((1, 2, 4), dtype=bool), max_active=bad)


def test_to_dense_round_trip_of_an_untruncated_code():
    Es, Ez, lpj, ss = _problem(seed=3, N=9, H=70, S=4)
    c = codes_from_dense(Es, Ez, lpj, ss, max_active=64)
    assert (c.nnz <= 64).all()
    dEs, dEz = c.to_dense()
    np.testing.assert_array_equal(dEs, Es)
    np.testing.assert_array_equal(dEz, Ez)
    # EBSC: no Ez
    dEs, dEz = codes_from_dense(Es, None, lpj, ss, max_active=64).to_dense()
    np.testing.assert_array_equal(dEs, Es)
    assert dEz is None
    # a truncated code keeps exactly its entries
    c = codes_from_dense(Es, Ez, lpj, ss, max_active=5)
    dEs, _ = c.to_dense()
    assert ((dEs == Es) | (dEs == 0)).all() and ((dEs != 0).sum(axis=1) == np.minimum(c.nnz, 5)).all()


def test_map_state_is_packbits_of_the_bool_state_and_packed_input_is_the_same():
    Es, Ez, lpj, ss = _problem(seed=5, N=8, H=13, S=6)
    c = codes_from_dense(Es, Ez, lpj, ss)
    want = np.packbits(ss[np.arange(8), np.argmax(lpj, axis=1)], axis=-1)
    assert c.map_state.dtype == np.uint8 and c.map_state.shape == (8, 2)
    np.testing.assert_array_equal(c.map_state, want)
    np.testing.assert_array_equal(c.map_states(), ss[np.arange(8), c.map_slot])
    c2 = codes_from_dense(Es, Ez, lpj, np.packbits(ss, axis=-1))
    for name in ("idx", "p", "m", "nnz", "map_slot", "map_q", "map_state"):
        np.testing.assert_array_equal(getattr(c, name), getattr(c2, name))


def test_map_q_is_the_normalised_weight_of_the_best_state():
    """codes_exp uses additions and multiplications only (so the kernel can match it bit for bit); its error against
    np.exp is a few ulp, and map_q = q.max() / (sum q + tiny) follows to 1e-14."""
    x = -np.concatenate((np.linspace(0, 50, 20001), np.logspace(-300, 2.84, 4001), [0.0, 699.9, 700.0]))
    np.testing.assert_allclose(codes_exp(x), np.exp(x), rtol=2e-15, atol=0)
    assert codes_exp(0.0) == 1.0
    np.testing.assert_array_equal(codes_exp(np.array([-700.1, -1e300, -np.inf, np.nan])), 0.0)
    rng = np.random.RandomState(1)
    for L in (1, 12, 64, 65, 201):
        lpj = rng.normal(size=(7, L)) * 30 - 500
        q = np.exp(lpj - lpj.max(axis=1)[:, None])
        got = codes_from_dense(np.zeros((7, 3)), None, lpj, np.zeros((7, L, 3), dtype=bool)).map_q
        np.testing.assert_allclose(got, q.max(axis=1) / (q.sum(axis=1) + F64_TINY), rtol=1e-14, atol=0)
        np.testing.assert_allclose(_wave_sum(q), q.sum(axis=1), rtol=1e-14)


def test_posterior_codes_holds_what_it_is_given():
    idx = np.array([[2, 0, -1]], dtype=np.int32)
    c = PosteriorCodes(4, idx, np.array([[0.5, 0.25, 0.0]]), None, np.array([2], dtype=np.int32),
                       np.array([0], dtype=np.int32), np.array([1.0]), np.array([[0b10100000]], dtype=np.uint8))
    assert c.H == 4 and c.max_active == 3 and c.Es is None and c.Ez is None
    np.testing.assert_array_equal(c.to_dense()[0], [[0.25, 0.0, 0.5, 0.0]])
    np.testing.assert_array_equal(c.map_states(), [[True, False, True, False]])

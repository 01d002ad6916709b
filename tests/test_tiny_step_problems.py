"""CPU checks of the tiny step() cases (_tiny_step_problems.py): the oracle stays finite over the three steps, no
update meets a singular system (np.linalg.inv raises LinAlgError only for an exactly singular matrix: the condition
numbers of every step's H x H systems are printed and bounded by COND_CAP, so the oracle's pinv-plus-noise branch, which
would draw from np.random, is never entered), the K^n rows stay distinct, and H = 1 with S = 2 takes the
"No new and unique states" branch in every step."""
import numpy as np
import pytest

import _masked_problems as mp
import _tiny_step_problems as ts


@pytest.mark.parametrize("algo", ts.ALGOS)
@pytest.mark.parametrize("D,H,S", ts.SHAPES)
def test_oracle_is_well_posed(algo, D, H, S):
    Y, theta0 = ts.make_case(algo, D, H, S)
    assert Y.shape == (ts.N, D) and np.isfinite(Y).all()
    assert all(np.isfinite(np.asarray(v)).all() for v in theta0.values())
    parents, children = ts.EA[H]
    assert parents <= S <= 2 ** H
    ss0, run = ts.oracle_run(algo, D, H, S)
    assert ss0.shape == (ts.N, S, H) and len(run) == ts.STEPS
    for t, r in enumerate(run):
        print("%s D %d H %d S %d step %d: F %.6f nu %.3f nsub %.3f cond %s" % (
            algo, D, H, S, t, r["F"], r["nu"], r["nsub"], {k: "%.3g" % v for k, v in r["conds"].items()}))
        assert np.isfinite(r["F"]), t
        assert all(np.isfinite(np.asarray(v)).all() for v in r["theta"].values()), t
        assert all(v <= mp.COND_CAP for v in r["conds"].values()), (t, r["conds"])
        for n in range(ts.N):
            assert len({row.tobytes() for row in r["ss"][n]}) == S, (t, n)
        if S == 2 ** H:  # the whole state space: nothing new to find
            assert r["skipped"] and r["nu"] == 0 and r["nsub"] == 0, t
    if S < 2 ** H:  # the EA found something in some step: the K^n comparison on the GPU is not vacuous
        assert any(r["nu"] > 0 for r in run)
    assert run[-1]["F"] > run[0]["F"]


def test_cases_cover_the_lower_edge():
    assert ts.SHAPES == ((3, 1, 2), (4, 2, 3), (5, 3, 5), (6, 4, 7)) and ts.N == 23 and ts.STEPS == 3
    assert ts.EA == {1: (1, 1), 2: (2, 1), 3: (2, 2), 4: (3, 2)}
    assert all(D > 1 for D, _, _ in ts.SHAPES)  # np.cov of one column is a scalar: sssc_standard_init needs D >= 2

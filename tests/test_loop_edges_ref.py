"""The CPU oracle's pose-graph residual (numer_loop_ver2 / logSim3, oracle/tsloop_oracle.c) against tests/golden/loop_edges.npz: the same function
evaluated by mpmath at 60 digits on connections chosen per branch of the log map, either side of both branch thresholds, and where the 3x3 elimination
exchanges rows (tests/golden/make_loop_edges.py).

RES_TOL: the residual is ~200 float64 operations (unit roundoff 1.1e-16) on values of order one; the worst-conditioned connections amplify rounding by
1 / sin(theta) ~ 7 (theta = 3.0: acos and the division by 2 sqrt(1 - d^2)) times cond(W) < 10 for upsilon -- 1.1e-16 x 200 x 70 ~ 1.5e-12; 1e-12 is held.
Away from theta ~ 3 the same count without the amplification gives 2e-14 (RES_TOL_PLAIN)."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_cases as LC  # noqa: E402

RES_TOL = 1e-12
RES_TOL_PLAIN = 2e-14


def test_fixture_holds_every_branch_and_edge():
    E = LC.edges()
    names = E["name"]
    assert sorted(set(int(b) for b in E["branch"])) == [0, 1, 2, 3]
    k = {n: i for i, n in enumerate(names)}
    assert E["sigma"][k["both_sigma0"]] == 0.0 and abs(E["sigma"][k["both_sigma5e-6"]] - 5e-6) < 1e-15
    assert abs((1 - E["d"][k["near_d_below"]]) - 1.1e-5) < 1e-9 and E["branch"][k["near_d_below"]] == 0
    assert abs((1 - E["d"][k["near_d_above"]]) - 0.9e-5) < 1e-9 and E["branch"][k["near_d_above"]] == 2
    assert abs(E["sigma"][k["near_sigma_inside"]] - 5e-6) < 1e-15 and E["branch"][k["near_sigma_inside"]] == 1
    assert abs(E["sigma"][k["near_sigma_outside"]] + 2e-5) < 1e-15 and E["branch"][k["near_sigma_outside"]] == 0
    assert list(E["swap"][k["swap_col0"]]) == [1, 0] and list(E["swap"][k["swap_col1"]]) == [0, 1]
    assert abs(np.arccos(E["d"][k["general_theta3"]]) - 3.0) < 1e-9 and np.arccos(E["d"]).max() <= 3.0 + 1e-9       # the map is ill-conditioned at pi
    assert [n for n, near in zip(names, E["near"]) if near] == [n for n in names if n.startswith("near_")]
    assert set(LC.EDGE_STEPS) == {n for n in names if not n.startswith("near_")}
    np.testing.assert_allclose(E["cost"], 0.5*(E["res"]**2).sum(1), rtol=1e-15)


@pytest.mark.parametrize("name", LC.edges()["name"])
def test_oracle_residual_against_mpmath(oracle_lib, name):
    E = LC.edges(); k = LC.edge_index(name)
    r, _, _ = oracle_lib.pg_eval(E["x1"][k], E["x2"][k], E["m"][k])
    err, cost_err = LC.edge_oracle_error(k)
    print("%s: oracle - mpmath %.3e (residual), %.3e (cost %.4f)" % (name, err, cost_err, E["cost"][k]))
    assert np.array_equal(np.abs(r - E["res"][k]).max(), err)
    assert err <= (RES_TOL if np.arccos(E["d"][k]) > 2.5 else RES_TOL_PLAIN)
    if name == "both_sigma0":
        assert r[6] == 0.0                                           # every scale exactly one


def test_fixture_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    try:
        import make_loop_edges
    finally:
        sys.path.pop(0)
    F, E = make_loop_edges.compute(), LC.edges()
    assert sorted(F.keys()) == sorted(E.keys())
    for key in F:
        if key == "name":
            assert [str(s) for s in F[key]] == E[key]
        else:
            assert F[key].dtype == E[key].dtype and np.array_equal(F[key], E[key]), key

"""libtsloop.so's two optimisers (tsloop_optimize_loop, tsloop_optimize_sim3, through the C ABI) against the CPU oracle at the shapes where they change
path, with tolerances that come from the oracle's own sensitivity (tests/loop_cases.py: the case table, the admission rule and the margins; the CPU
guard tests/test_loop_cases.py keeps the table honest).

  a. one connection of the mpmath fixture (tests/golden/loop_edges.npz) between a constant and a free keyframe: cost0 against mpmath, one LM step
     against the oracle; the theta = 3 connections are rejected first steps;
  b. the solver's sizes: n6 = 12 .. 192 through the row loader of k_solve_t<false>, 198 and 288 through the blocked Cholesky, 1800;
  c. topologies synth.pose_graph never makes;  d. OptimizeSim3 around the wave and workgroup sizes, masks, far starts, every exit;
  e. a context that has been used gives the bits a fresh one gives.
Every comparison prints its figures before it asserts (docs/kernel_notes.md, "Loop closing: reference sensitivity and measured differences")."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_cases as LC  # noqa: E402
from textslam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lo(oracle_lib):
    from textslam_amd.loop import LoopOptimizer
    return LoopOptimizer(0)


def compare(case, g):
    """GPU result g against the oracle under the case's bounds; prints one record line first."""
    s = LC.oracle_sensitivity(case)
    o = s["base"]
    bx, bc = LC.bounds(case)
    dx, dc = float(np.abs(g["x"] - o["x"]).max()), abs(g["rep"]["cost1"] - o["rep"]["cost1"])
    d0 = abs(g["rep"]["cost0"] - o["rep"]["cost0"])/max(abs(o["rep"]["cost0"]), 1e-300)
    print("\nLOOPCASE %s | spread x %.3e cost1 %.3e | bound x %.3e cost1 %.3e | gpu-oracle x %.3e cost1 %.3e cost0(rel) %.3e | gpu %s oracle %s"
          % (case.name, s["spread"]["x"], s["spread"]["cost1"], bx, bc, dx, dc, d0, g["ints"], o["ints"]))
    assert s["stable"] and s["spread"]["x"] <= LC.ADMIT_SPREAD
    assert g["ints"] == o["ints"]
    if "mask" in o:
        assert np.array_equal(g["mask"], o["mask"])
    np.testing.assert_allclose(g["rep"]["cost0"], o["rep"]["cost0"], rtol=LC.COST0_RTOL, atol=0)
    assert dx <= bx, (dx, bx)
    assert dc <= bc, (dc, bc)


# ---- a. one connection
@pytest.mark.parametrize("name", LC.edges()["name"])
def test_one_connection_cost0_against_mpmath(lo, name):
    """max_it = 0: cost0 = |r|^2 / 2 of the mpmath residual within 16 x max(the oracle's own error on this connection, 1e-13 cost).  The pairs either side of
    a branch threshold are compared here only: Ceres' 1e-6 |x| differencing step would straddle the threshold."""
    E = LC.edges(); k = LC.edge_index(name)
    case = LC.Case("pg_edge_%s_it0" % name, "pg", LC.pg_edge(name), {"max_it": 0})
    g = LC.run_gpu(lo, case)
    _, oerr = LC.edge_oracle_error(k)
    bound = LC.EDGE_COST_MARGIN*max(oerr, LC.EDGE_COST_FLOOR*E["cost"][k])
    diff = abs(g["rep"]["cost0"] - E["cost"][k])
    print("\nLOOPEDGE %s | cost %.6f | oracle-mpmath %.3e | bound %.3e | gpu-mpmath %.3e" % (name, E["cost"][k], oerr, bound, diff))
    assert g["ints"] == (0, 0, 0) and g["rep"]["cost1"] == g["rep"]["cost0"]
    assert np.array_equal(g["x"], LC.inputs_of(case)["pose"])
    assert diff <= bound


@pytest.mark.parametrize("case", LC.PG_CASES, ids=lambda c: c.name)
def test_pose_graph_case(lo, case):
    d = LC.inputs_of(case)
    g = LC.run_gpu(lo, case)
    compare(case, g)
    fx = d["fixed"].astype(bool)
    assert np.array_equal(g["x"][fx], d["pose"][fx])                 # constant keyframes come back bit-equal
    if case.claims.get("accepted") == 0:                             # a rejected first step: so does everything else
        assert g["rep"]["accepted"] == 0 and g["rep"]["iters"] == 1 and np.array_equal(g["x"], d["pose"])
    elif case.opts.get("max_it") == 1:
        assert np.abs(g["x"] - d["pose"]).max() > 1e-4


# ---- d. OptimizeSim3
@pytest.mark.parametrize("case", LC.SIM3_CASES, ids=lambda c: c.name)
def test_sim3_case(lo, case):
    d = LC.inputs_of(case)
    g = LC.run_gpu(lo, case)
    compare(case, g)
    assert not g["mask"][d["inliers"] == 0].any() and g["ints"][3] == int(g["mask"].sum())
    for key in ("iters", "termination"):
        if key in case.claims:
            assert g["rep"][key] == case.claims[key]


# ---- e. a used context
def _bits(r):
    return (r["x"].tobytes(), r["ints"], np.float64(r["rep"]["cost0"]).tobytes(), np.float64(r["rep"]["cost1"]).tobytes(),
            r["mask"].tobytes() if "mask" in r else b"")


def test_used_context_gives_a_fresh_context_s_bits():
    """The context's buffers are reused and only ever grow, and every sum is described as fixed-order: a call's result must not depend on what the context
    ran before it -- a large graph, then the smallest; a large match set, then one match; then the last LDS size."""
    from textslam_amd.loop import LoopOptimizer
    m = synth.sim3_matches(seed=3, n=1500, outlier_frac=0.25)
    calls = [LC.Case("used_pg150", "pg", lambda: LC._pg(synth.pose_graph(seed=150, n_kf=150))),
             LC.Case("used_pg_free1", "pg", LC.pg_shape(1)),
             LC.Case("used_sim3_n1500", "sim3", lambda: LC._sim3(m)),
             LC.Case("used_sim3_n1", "sim3", LC.sim3_n(1)),
             LC.Case("used_pg_free27", "pg", LC.pg_shape(27))]
    used = LoopOptimizer(0)
    for c in calls:
        a = LC.run_gpu(used, c)
        b = LC.run_gpu(LoopOptimizer(0), c)
        assert a["rep"]["iters"] >= 1 and a["rep"]["status"] == 0
        assert _bits(a) == _bits(b), c.name

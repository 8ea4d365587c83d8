"""The HIP kernels against TextSLAM's OWN cost functors, through tests/golden/ref_functors.npz (recorded from the functors compiled out of the
reference tree: tests/golden/make_ref_functors.py, tests/test_ref_functors.py).  Only the fixture is read: neither the reference nor
oracle/_ref/ is needed here.  Every comparison is of ONE evaluation of the model -- residuals, Jacobians, the cost at the start point -- never
of a Levenberg-Marquardt trajectory.

Bounds: the tolerance of the matching GPU-versus-oracle assertion of the suite plus the oracle-versus-reference bound of
tests/test_ref_functors.py::TOL (ten times the measured deviation, per functor family; 0 for a family that measures 0):
  tsba_eval residuals      1e-10 absolute (tests/test_gpu_parity.py::_check_eval) + TOL[family] max(1, |r|)
  tsba_eval scene jac      1e-10 of the largest entry (same place) + TOL["jac/" family]
  Sim3 cost at the start   rtol 1e-12 (tests/test_gpu_loop.py::test_optimize_sim3_parity); inlier flags identical
  pose-graph cost          rtol 1e-9  (tests/test_gpu_loop.py::test_optimize_loop_parity)"""
import math
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ref_functors as gen  # noqa: E402
import test_ref_functors as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return gen.load()


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


@pytest.fixture(scope="module")
def lo():
    from textslam_amd.loop import LoopOptimizer
    return LoopOptimizer(0)


@pytest.mark.parametrize("name", gen.BA_CASES)
def test_tsba_eval_against_reference(gpu, oracle_lib, fix, name):
    """tsba_eval on every pyramid level of one BA case: residuals block by block in the order include/tsba.h documents (scene blocks, then text
    blocks, each in observation order) against the functor that owns the block, and the jac of the scene blocks against the fixture's Jet
    Jacobian times the plus-Jacobian (oracle/RECALLED.md row C11, still recalled).  The text functors take mu / sigma as constructor arguments:
    the fixture's are the oracle's, and the device's own must agree with them as in tests/test_gpu_parity.py."""
    P, o, levels = gen.ba_case(name)
    for l in levels:
        if P.n_tobs:
            np.testing.assert_allclose(gpu.evaluate(P, o, l)["musigma"], fix[f"ba/{name}/L{l}/musigma"], rtol=1e-11, atol=1e-10)
    t = ref.ba_deviations(oracle_lib, fix, evaluate=gpu.evaluate, cases=[name], atol=1e-10, rel=1e-10)
    dev, cnt = t.dev, t.cnt
    for k in sorted(t.raw):
        print(f"  {k:28s} device against reference {t.raw[k]:.3e}  (allowed 1e-10 + {ref.TOL[k]:.3e})")
    assert dev and sum(cnt.values()) > 0
    ref.check(dev)


@pytest.mark.parametrize("name", ["n9", "n300", "n257"])
def test_sim3_start_cost_and_inliers_against_reference(lo, fix, name):
    """tsloop_optimize_sim3 with max_it = 0 and a Huber delta far above every residual (delta = 0 would zero the cost in this kernel): cost0 is
    half the sum of squares of auto_sim's and auto_siminv's residuals over the matches flagged in, and the returned flags are those with all
    four |r_k| < 4 (no recorded |r_k| lies within 1e-6 of 4).  n = 257 leaves one match for the second round of the 256-thread sweep."""
    g = lambda k: fix[f"sim/{name}/{k}"]
    inl = g("inlier").astype(bool); res = g("res"); n = len(res)
    assert n == int(name[1:]) and 0 < inl.sum() < n
    o = lo.default_options_sim3(); o.max_it = 0; o.huber_delta = 1e12
    assert np.abs(res).max() < 1e6
    ng, sim, ig, rep = lo.OptimizeSim3(g("P1"), g("uv1"), g("P2"), g("uv2"), g("inlier"), g("x")[0], g("K"), options=o)
    assert rep["status"] == 0 and rep["iters"] == 0
    want = 0.5*math.fsum((res[inl]**2).reshape(-1))
    print(f"  {name}: cost0 {rep['cost0']:.17g} reference {want:.17g} rel {abs(rep['cost0'] - want)/want:.2e}")
    np.testing.assert_allclose(rep["cost0"], want, rtol=1e-12)
    flags = inl & np.all(np.abs(res) < 4.0, axis=1)
    assert 0 < flags.sum() < inl.sum()
    assert np.array_equal(ig, flags) and ng == int(flags.sum())


@pytest.mark.parametrize("branch", gen.LOOP_BRANCHES)
def test_pose_graph_start_cost_against_reference(lo, fix, branch):
    """tsloop_optimize_loop with max_it = 0 (it returns after the first k_pg_pre, cost0 set) on two-keyframe graphs -- one constant keyframe, one
    free, one connection: cost0 is half the squared norm of numer_loop_ver2's residual.  Fifteen connections of this branch of logSim3, each
    with the free keyframe as edge_i and as edge_j.
    NOT checked here: the ill-conditioned part of the branch |log s| >= 1e-5, d > 1 - 1e-5, and angles within 0.14 rad of pi.  The connections
    are drawn where the model is well conditioned (tests/golden/make_ref_functors.py::device_samples), because rtol 1e-9 on a cost cannot hold
    elsewhere for any evaluation in doubles (oracle and reference themselves differ by 6.8e-8 there).  Next to the |log s| threshold that
    leaves only angles of 1e-10 ... 1e-13, where d == 1.0 exactly and omega is 0 on the device; the connections with larger |log s| reach the
    angle threshold.  In that part of the branch tsloop_optimize_loop is held only to the oracle (tests/test_gpu_loop.py)."""
    e = {k: np.asarray(fix[f"loop15/{branch}/{k}"], np.float64) for k in ("meas", "x1", "x2", "res")}
    assert len(e["res"]) == 15
    o = lo.default_options_loop(); o.max_it = 0
    worst = 0.0
    for i in range(15):
        want = 0.5*math.fsum(e["res"][i]**2)
        for fixed in ([0, 1], [1, 0]):                 # the free keyframe is edge_i = 0, then edge_j = 1
            x, rep = lo.OptimizeLoop(np.stack([e["x1"][i], e["x2"][i]]), np.array(fixed, np.uint8), np.array([0], np.int32), np.array([1], np.int32), e["meas"][i][None], options=o)
            assert rep["status"] == 0 and rep["iters"] == 0
            worst = max(worst, abs(rep["cost0"] - want)/want)
            np.testing.assert_allclose(rep["cost0"], want, rtol=1e-9, err_msg=f"connection {i}, fixed {fixed}")
    print(f"  {branch}: worst relative cost0 difference {worst:.2e}")


def test_pose_graph_start_cost_of_a_graph_against_reference(lo, fix):
    """A 12-keyframe graph (two constant keyframes, 20 connections cycling through the four branches): cost0 is the sum over its connections."""
    g = {k: fix["graph12/" + k] for k in ("pose", "fixed", "edge_i", "edge_j", "meas", "res")}
    o = lo.default_options_loop(); o.max_it = 0
    x, rep = lo.OptimizeLoop(g["pose"], g["fixed"], g["edge_i"], g["edge_j"], g["meas"], options=o)
    want = 0.5*math.fsum((g["res"]**2).reshape(-1))
    print(f"  graph12: cost0 {rep['cost0']:.17g} reference {want:.17g}")
    assert rep["status"] == 0 and rep["iters"] == 0 and len(g["res"]) >= 12
    np.testing.assert_allclose(rep["cost0"], want, rtol=1e-9)

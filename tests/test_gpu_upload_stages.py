"""The seam between the two ways a problem reaches the device: a one-shot call (tsba_local_ba, tsba_pose_optim) stages lazily -- on a small window only the first
pass's level with the upload, the others when their pass begins, their buffers sized by what a level can hold at most -- while tsba_upload stages every level
eagerly and sizes the buffers by what the plans hold.  Both must compute the same bits, and a deferring call must leave nothing behind for the next one."""
import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

FIELDS = ("pose", "rho", "theta", "sgood", "tobs_good", "tfgood")


def _case(shape):
    if shape == "window":                 # three levels, a small window: levels 1 and 0 are deferred
        return synth.tiny(seed=11), abi.options_local(), "LocalBundleAdjustment"
    if shape == "window_level0_heavy":    # level 0 holds several times the features of level 2: the capacity bound, not the first level, sizes the text buffers
        return synth.tiny(seed=11, feats=(16, 8, 6)), abi.options_local(), "LocalBundleAdjustment"
    if shape == "single_frame":           # one keyframe, every landmark frozen: no plan threads, every level staged before the solve
        return synth.make_problem(1, 40, 3, 11, feats=(8, 6, 4), frozen_frac=1.0, n_out=2, max_targets=1, text_targets=1), abi.options_pose(), "PoseOptim"
    return synth.init_pair(seed=5), abi.options_init(), "InitBA"      # four levels on two keyframes


def _same(Ga, ra, Gb, rb, what):
    for k in ("iters", "accepted", "termination"):
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])
    for f in FIELDS:
        assert np.array_equal(getattr(Ga, f), getattr(Gb, f)), (what, f)


@pytest.mark.parametrize("shape", ["window", "window_level0_heavy", "single_frame", "init_ba"])
def test_one_shot_call_matches_upload_solve_download(shape):
    from textslam_amd.optimizer import Optimizer
    P, o, call = _case(shape)
    if shape == "window_level0_heavy":
        off = P.tfeat_off                                              # (the shape is what the case is about)
        assert max(off[0][j + 1] - off[0][j] for j in range(P.n_text)) >= 2*max(off[2][j + 1] - off[2][j] for j in range(P.n_text))
    lazy = Optimizer(0)
    G1 = P.copy(); r1 = getattr(lazy, call)(G1, options=o); i1 = lazy.solver_info()
    eager = Optimizer(0)
    eager.upload(P.copy(), o); r2 = eager.solve(); G2 = eager.download(P.copy()); i2 = eager.solver_info()
    assert r1["n_passes"] == r2["n_passes"] == o.n_passes
    _same(G1, r1, G2, r2, "one-shot against upload + solve + download")
    assert i1 == i2, (i1, i2)
    G3 = P.copy(); r3 = getattr(lazy, call)(G3, options=o)             # the first call's deferred state does not leak into the second
    _same(G1, r1, G3, r3, "second one-shot call on the same context")
    assert lazy.solver_info() == i1
    assert not np.array_equal(G1.pose, P.pose)                         # (something was solved)
    lazy.close(); eager.close()

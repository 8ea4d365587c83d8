"""synth.camera: the image size and intrinsics of the problems made inside the block, the 640 x 480 defaults outside it."""
import numpy as np
import pytest

from textslam_amd import synth


def _bytes(P):
    parts = [P.K, P.pose, P.rho, P.theta, P.text_box_ray, P.text_host, P.text_host_Twr, P.pt_ray, P.pt_host, P.pt_host_Trw, P.sgood, P.tobs_kf, P.tobs_text,
             P.tobs_good, P.tobs_fgood_off, P.tfgood, P.kf_initial]
    for l in range(P.n_levels):
        parts += [P.img[l], P.sobs_kf[l], P.sobs_pt[l], P.sobs_flag[l], P.sobs_uv0[l], P.tfeat_off[l], P.tfeat_raw[l], P.tfeat_uv[l], P.tfeat_ref[l]]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def test_camera_sets_and_restores_the_defaults():
    K0 = synth.K_GENERAL_MOTION.copy()
    before = _bytes(synth.tiny())
    K = np.array([768.0, 766.0, 631.5, 372.25])
    with synth.camera(1280, 720, K):
        assert (synth.W, synth.H) == (1280, 720) and np.array_equal(synth.K_GENERAL_MOTION, K)
        P = synth.tiny()
        with synth.camera(648, 480, K0):                                    # nested: the inner block restores the outer camera
            assert (synth.W, synth.H) == (648, 480)
        assert (synth.W, synth.H) == (1280, 720) and np.array_equal(synth.K_GENERAL_MOTION, K)
    assert (synth.W, synth.H) == (640, 480) and np.array_equal(synth.K_GENERAL_MOTION, K0)
    assert [P.img[l].shape[1:] for l in range(P.n_levels)] == [(720, 1280), (360, 640), (180, 320)] and np.array_equal(P.K, K)
    assert P.n_tobs > 0 and all(P.tfeat_off[l][-1] > 0 for l in range(P.n_levels))
    box = K[:2]*np.asarray(P.text_box_ray).reshape(-1, 2) + K[2:]
    assert box[:, 0].max() > 640 or box[:, 1].max() > 480                      # the planes use the larger image
    assert _bytes(synth.tiny()) == before


def test_camera_restores_after_an_error():
    K0 = synth.K_GENERAL_MOTION.copy()
    before = _bytes(synth.tiny())
    with pytest.raises(RuntimeError):
        with synth.camera(1920, 1080, K0*3.0):
            raise RuntimeError("inside the block")
    with pytest.raises(ValueError):
        with synth.camera(1, 480, K0):
            pass
    assert (synth.W, synth.H) == (640, 480) and np.array_equal(synth.K_GENERAL_MOTION, K0)
    assert _bytes(synth.tiny()) == before

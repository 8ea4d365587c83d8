"""tsba_text_label_at on the device: the labels at n pixels, without the label image.

Every comparison is exact.  The yardsticks: oracle.label_image (the CPU restatement of ShowBAReproj_TextBox -> TextBoxWithFill: the definition of correct) and
gpu.TextLabelImage (k_label) on the same state.  A test that queries "all pixels" asks for every pixel of the level in ONE call and reshapes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from textslam_amd import synth, abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP = C.POINTER(C.c_int32)


# ------------------------------------------------------------------ helpers
def _shape(P, level):
    return int(P.img[level].shape[1]), int(P.img[level].shape[2])          # h, w


def _grid(x0, x1, y0, y1):
    ys, xs = np.mgrid[y0:y1, x0:x1]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)


def _all_pixels(gpu, P, kf, level):
    h, w = _shape(P, level)
    lab = gpu.TextLabelAt(level, kf, _grid(0, w, 0, h))
    assert lab.dtype == np.int32 and lab.shape == (h*w,)
    return lab.reshape(h, w)


def _yardsticks(gpu, oracle, G, kf, level):
    ref = oracle.label_image(G, kf, level)
    img = gpu.TextLabelImage(kf, level, _shape(G, level))
    assert ref.shape == img.shape == _shape(G, level)
    return ref, img


def _check_all_pixels(gpu, oracle, G, kf, level):
    """labels at every pixel of (kf, level) == the oracle's image == k_label's image; returns (labels, oracle image)"""
    at = _all_pixels(gpu, G, kf, level)
    ref, img = _yardsticks(gpu, oracle, G, kf, level)
    print("kf %d level %d: %d labelled pixels, labels %s; differ from the oracle at %d pixels, from the label image at %d"
          % (kf, level, int((ref >= 0).sum()), sorted(set(ref[ref >= 0].astype(int).tolist())), int((at != ref).sum()), int((at != img).sum())))
    assert np.array_equal(at.astype(np.float32), ref), "kf %d level %d: %d pixels differ from the oracle" % (kf, level, int((at != ref).sum()))
    assert np.array_equal(at.astype(np.float32), img), "kf %d level %d: %d pixels differ from the label image" % (kf, level, int((at != img).sum()))
    return at, ref


def _single_plane(oracle, G, kf, level, j):
    """the oracle's label image of keyframe kf with ONE observation, of plane j: its filled quad as a mask"""
    S = G.copy()
    S.tobs_kf, S.tobs_text, S.tobs_good = np.array([kf], np.int32), np.array([j], np.int32), np.ones(1, np.uint8)
    S.tobs_fgood_off, S.tfgood = np.zeros(2, np.int32), np.zeros(0, np.uint8)
    return oracle.label_image(S, kf, level) >= 0


def _q_to_R(q):
    w, x, y, z = np.asarray(q, np.float64)/np.linalg.norm(q)
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)],
                     [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)],
                     [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]])


def _project(P, level, kf, j, rays):
    """pixels [n, 2] in keyframe kf at `level` of the host rays [n, 2] of plane j (tool::GetProjText) at P's parameters"""
    pose, theta = np.asarray(P.pose, np.float64).reshape(-1, 7), np.asarray(P.theta, np.float64).reshape(-1, 3)
    Kl = np.asarray(P.K, np.float64)*0.5**level
    Rc, tc = _q_to_R(pose[kf, :4]), pose[kf, 4:]
    host = int(P.text_host[j])
    if host >= 0:
        Rr, tr = _q_to_R(pose[host, :4]), pose[host, 4:]
        Rcr = Rc @ Rr.T
        tcr = tc - Rcr @ tr
    else:
        T = np.asarray(P.text_host_Twr, np.float64).reshape(-1, 3, 4)[j]
        Rcr, tcr = Rc @ T[:, :3], Rc @ T[:, 3] + tc
    m = np.concatenate([np.asarray(rays, np.float64).reshape(-1, 2), np.ones((len(rays), 1))], 1)
    X = m @ Rcr.T/(-(m @ theta[j]))[:, None] + tcr
    return np.stack([Kl[0]*X[:, 0]/X[:, 2] + Kl[2], Kl[1]*X[:, 1]/X[:, 2] + Kl[3]], 1)


def _corners(P, level, kf, j):
    return _project(P, level, kf, j, np.asarray(P.text_box_ray, np.float64).reshape(-1, 4, 2)[j])


def _rays_for(P, level, kf, j, target_uv):
    """host rays of plane j whose projections into kf are target_uv [n, 2] (Newton on the 2 x 2 map, numeric derivative)"""
    out = []
    start = np.asarray(P.text_box_ray, np.float64).reshape(-1, 4, 2)[j].mean(0)
    for uv in np.asarray(target_uv, np.float64):
        m = start.copy()
        for _ in range(12):
            f0 = _project(P, level, kf, j, [m])[0]
            J = np.stack([(_project(P, level, kf, j, [m + d])[0] - f0)/1e-6 for d in ([1e-6, 0], [0, 1e-6])], 1)
            m = m + np.linalg.solve(J, uv - f0)
        assert np.abs(_project(P, level, kf, j, [m])[0] - uv).max() < 1e-7
        out.append(m)
    return np.array(out)


def _ranks(P, kf):
    """tobs indices of keyframe kf's observations: rank r is observation _ranks(P, kf)[r]"""
    return np.nonzero(np.asarray(P.tobs_kf) == kf)[0]


# ------------------------------------------------------------------ contexts
@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


@pytest.fixture(scope="module")
def tiny_state(oracle_lib):
    """A context of its own that keeps the state of ONE LocalBundleAdjustment (the existing label test's problem) for the tests that share it, with the
    problem it left (G: the optimised parameters)."""
    from textslam_amd.optimizer import Optimizer
    g = Optimizer(0)
    P = synth.tiny(seed=31, n_kf=5, n_pt=80, n_text=6, text_targets=4)
    G = P.copy()
    g.LocalBundleAdjustment(G, options=abi.options_local())
    return g, G


# ------------------------------------------------------------------ 1. all pixels
def test_all_pixels_equal_oracle_and_label_image(tiny_state, oracle_lib):
    g, G = tiny_state
    for level in (0, 2):
        for kf in (0, G.n_kf - 1):
            at, ref = _check_all_pixels(g, oracle_lib, G, kf, level)
            assert (ref >= 0).any() and (at >= 0).any()


# ------------------------------------------------------------------ 2. border: clipped lines, clamped spans
def test_border_quads_outside_the_image(gpu, oracle_lib):
    kf = 3
    G = synth.border_variant(kf=kf)
    gpu.LocalBundleAdjustment(G, options=abi.options_local())
    for level in (0, 2):
        h, w = _shape(G, level)
        at, ref = _check_all_pixels(gpu, oracle_lib, G, kf, level)
        edge = np.concatenate([ref[0], ref[-1], ref[:, 0], ref[:, -1]])
        assert (edge >= 0).any(), "no labelled pixel on the image border"
        cs = np.array([np.trunc(_corners(G, level, kf, int(G.tobs_text[t]))) for t in _ranks(G, kf)]).reshape(-1, 2)
        outside = (cs[:, 0] < 0) | (cs[:, 0] >= w) | (cs[:, 1] < 0) | (cs[:, 1] >= h)
        print("level %d: %d of %d truncated corners outside the image, %d labelled border pixels" % (level, int(outside.sum()), len(cs), int((edge >= 0).sum())))
        assert outside.any(), "no truncated corner outside the image"


# ------------------------------------------------------------------ 3. painter's order
def _with_copy_of_plane(P, j):
    """P plus plane n_text = a copy of plane j (same host, same theta, same reference features) whose box rays are shifted by half the box width; its
    observations follow the original's, keyframe by keyframe (the list stays keyframe-major)"""
    Q = P.copy()
    nt = P.n_text
    box = np.asarray(P.text_box_ray, np.float64).reshape(-1, 4, 2)
    Q.theta = np.concatenate([np.asarray(P.theta).reshape(-1, 3), np.asarray(P.theta).reshape(-1, 3)[j:j + 1]])
    Q.text_host = np.concatenate([P.text_host, P.text_host[j:j + 1]])
    Q.text_host_Twr = np.concatenate([np.asarray(P.text_host_Twr).reshape(-1, 12), np.asarray(P.text_host_Twr).reshape(-1, 12)[j:j + 1]])
    Q.text_box_ray = np.concatenate([box, box[j:j + 1] + 0.5*(box[j, 1] - box[j, 0])])
    Q.truth = {}
    for l in range(P.n_levels):
        off = np.asarray(P.tfeat_off[l])
        a, b = int(off[j]), int(off[j + 1])
        Q.tfeat_off[l] = np.concatenate([off, [off[-1] + b - a]]).astype(np.int32)
        Q.tfeat_raw[l] = np.concatenate([P.tfeat_raw[l], P.tfeat_raw[l][a:b]])
        Q.tfeat_uv[l] = np.concatenate([P.tfeat_uv[l], P.tfeat_uv[l][a:b]])
        Q.tfeat_ref[l] = np.concatenate([np.asarray(P.tfeat_ref[l]).reshape(-1, 8), np.asarray(P.tfeat_ref[l]).reshape(-1, 8)[a:b]])
    tk, tt, tg, fo, fg = [], [], [], [0], []
    for t in range(P.n_tobs):
        flags = P.tfgood[P.tobs_fgood_off[t]:P.tobs_fgood_off[t + 1]]
        for plane in ([int(P.tobs_text[t])] + ([nt] if int(P.tobs_text[t]) == j else [])):
            tk.append(int(P.tobs_kf[t])); tt.append(plane); tg.append(int(P.tobs_good[t])); fg.append(flags); fo.append(fo[-1] + len(flags))
    Q.tobs_kf, Q.tobs_text, Q.tobs_good = np.array(tk, np.int32), np.array(tt, np.int32), np.array(tg, np.uint8)
    Q.tobs_fgood_off, Q.tfgood = np.array(fo, np.int32), np.concatenate(fg).astype(np.uint8)
    return Q.normalise()


def test_painters_order_later_quad_wins(gpu, oracle_lib):
    P = synth.tiny(seed=31, n_kf=5, n_pt=80, n_text=6, text_targets=4)
    kf = P.n_kf - 1
    j = int(P.tobs_text[_ranks(P, kf)[0]])                                 # a plane keyframe kf sees
    G = _with_copy_of_plane(P, j)
    assert G.n_text == P.n_text + 1 and G.n_tobs > P.n_tobs and np.all(np.diff(G.tobs_kf) >= 0)
    gpu.LocalBundleAdjustment(G, options=abi.options_local())
    obs = _ranks(G, kf)
    ra = int(np.nonzero(G.tobs_text[obs] == j)[0][0]); rb = int(np.nonzero(G.tobs_text[obs] == P.n_text)[0][0])
    assert rb == ra + 1
    for level in (0, 2):
        at, ref = _check_all_pixels(gpu, oracle_lib, G, kf, level)
        ma, mb = _single_plane(oracle_lib, G, kf, level, j), _single_plane(oracle_lib, G, kf, level, P.n_text)
        both = ma & mb
        assert both.any(), "the two quads share no pixel"
        later = np.zeros_like(both)
        for r in range(rb + 1, len(obs)):
            later |= _single_plane(oracle_lib, G, kf, level, int(G.tobs_text[obs[r]]))
        assert (both & ~later).any()
        assert np.all(at[both & ~later] == rb), "a pixel of both quads does not carry the later rank"
        assert np.all(at[ma & ~mb & ~later] == ra)


# ------------------------------------------------------------------ 4. degenerate quads
def test_degenerate_quads(gpu, oracle_lib):
    """The corners must land where they are designed, whatever the solve does: OptimizeLandmarker keeps every pose constant, and the plane is frozen (its
    host outside the problem: theta constant), so its quad in keyframe kf follows from the inputs alone."""
    P = synth.landmark_refine(n_kf=5, n_pt=60, n_text=4)
    level = 0
    h, w = _shape(P, level)
    t = int(np.nonzero(np.asarray(P.tobs_kf) != np.asarray(P.text_host)[P.tobs_text])[0][-1])      # an observation from another keyframe than the host
    kf, j = int(P.tobs_kf[t]), int(P.tobs_text[t])
    host = int(P.text_host[j])
    assert host >= 0 and host != kf
    Rh, th = _q_to_R(P.pose.reshape(-1, 7)[host, :4]), P.pose.reshape(-1, 7)[host, 4:]
    before = _corners(P, level, kf, j)
    P.text_host = P.text_host.copy(); P.text_host[j] = -1                    # frozen: T_wr of the host instead of the host
    P.text_host_Twr = np.asarray(P.text_host_Twr, np.float64).reshape(-1, 12).copy()
    P.text_host_Twr[j] = np.concatenate([Rh.T, (-Rh.T @ th)[:, None]], 1).reshape(-1)
    assert np.abs(_corners(P, level, kf, j) - before).max() < 1e-9
    c = np.floor(before.mean(0)) + 0.5
    assert 8 <= c[0] < w - 8 and 8 <= c[1] < h - 8
    cases = {
        "one pixel": c + 0.2*np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]]),
        "horizontal edge": c + np.array([[-3, -1], [3, -1], [2, 2], [-2, 1]]),
        "under one pixel high": c + np.array([[-4, -0.2], [4, -0.2], [4, 0.2], [-4, 0.2]]),
    }
    for name, target in cases.items():
        G = P.copy()
        box = np.asarray(G.text_box_ray, np.float64).reshape(-1, 4, 2).copy()
        box[j] = _rays_for(P, level, kf, j, target)
        G.text_box_ray = box
        gpu.OptimizeLandmarker(G, options=abi.options_landmarker())
        got = np.trunc(_corners(G, level, kf, j)).astype(int)
        want = np.trunc(target).astype(int)
        print("%s: corners %s (designed %s), moved by %.3g px" % (name, got.tolist(), want.tolist(), np.abs(_corners(G, level, kf, j) - target).max()))
        assert np.array_equal(got, want), "%s: a corner is not in the pixel it was designed for" % name
        mask = _single_plane(oracle_lib, G, kf, level, j)
        rows, cols = np.nonzero(mask.any(1))[0], np.nonzero(mask.any(0))[0]
        if name == "one pixel":
            assert len(set(map(tuple, got))) == 1 and mask.sum() == 1
        elif name == "horizontal edge":
            assert got[0, 1] == got[1, 1] and got[0, 0] != got[1, 0] and len(set(got[:, 1])) == 3 and len(rows) == 4
        else:
            assert len(set(got[:, 1])) == 1 and len(rows) == 1 and len(cols) == 9
        x0, x1, y0, y1 = max(got[:, 0].min() - 2, 0), min(got[:, 0].max() + 3, w), max(got[:, 1].min() - 2, 0), min(got[:, 1].max() + 3, h)
        px = _grid(x0, x1, y0, y1)
        at = gpu.TextLabelAt(level, kf, px)
        ref, img = _yardsticks(gpu, oracle_lib, G, kf, level)
        rank = int(np.nonzero(G.tobs_text[_ranks(G, kf)] == j)[0][0])
        assert (ref[px[:, 1], px[:, 0]] == rank).any(), "%s: the quad is not visible in the oracle's image" % name
        assert np.array_equal(at.astype(np.float32), ref[px[:, 1], px[:, 0]]), name
        assert np.array_equal(at.astype(np.float32), img[px[:, 1], px[:, 0]]), name


# ------------------------------------------------------------------ 5. more than one chunk of 64 observations
def test_more_than_one_chunk(gpu, oracle_lib):
    P = synth.make_problem(4, 60, 100, 5, feats=(12, 8, 6), text_targets=3)
    kf, level = 1, 2
    obs = _ranks(P, kf)
    assert P.n_tobs > 128
    assert (obs < 64).any() and ((obs >= 64) & (obs < 128)).any() and (obs >= 128).any(), "keyframe %d's observations do not span three chunks" % kf
    G = P.copy()
    gpu.LocalBundleAdjustment(G, options=abi.options_local())
    at, ref = _check_all_pixels(gpu, oracle_lib, G, kf, level)
    seen = obs[np.unique(at[at >= 0])]                                      # tobs index of every rank that occurs as a label
    print("keyframe %d: %d observations (tobs %d..%d), labels from %d of them: %d below 64, %d in [64, 128), %d from 128 on"
          % (kf, len(obs), obs.min(), obs.max(), len(seen), int((seen < 64).sum()), int(((seen >= 64) & (seen < 128)).sum()), int((seen >= 128).sum())))
    assert (seen < 64).any() and ((seen >= 64) & (seen < 128)).any() and (seen >= 128).any()


# ------------------------------------------------------------------ 6. every entry point
def _sample_px(rng, h, w, n=200):
    px = np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], 1)
    return np.concatenate([px, [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]]]).astype(np.int32)


@pytest.mark.parametrize("entry", ["PoseOptim", "InitBA", "OptimizeLandmarker"])
def test_every_entry_point(gpu, entry):
    rng = np.random.default_rng(17)
    if entry == "PoseOptim":
        G = synth.make_problem(1, 200, 6, 13, feats=(8, 6, 4), frozen_frac=1.0, n_out=4, max_targets=1, text_targets=1)
        gpu.PoseOptim(G, options=abi.options_pose())
        assert gpu.solver_info()["pose_kernel"] == 1                        # the fused pose-only kernel
        kfs = [0]
    elif entry == "InitBA":
        G = synth.init_pair(n_pt=120, n_text=3)
        gpu.InitBA(G, options=abi.options_init())
        kfs = [1]
    else:
        G = synth.landmark_refine(n_kf=5, n_pt=150, n_text=4)
        gpu.OptimizeLandmarker(G, options=abi.options_landmarker())
        kfs = [G.n_kf - 2, G.n_kf - 1]                                       # the two newest keyframes, in ONE call
    level = 0
    h, w = _shape(G, level)
    px = _sample_px(rng, h, w)
    # half of the random pixels on the labelled part of the image, so that labels >= 0 are sampled
    imgs = {k: gpu.TextLabelImage(k, level, (h, w)) for k in kfs}
    for k in kfs:
        ys, xs = np.nonzero(imgs[k] >= 0)
        assert len(ys) > 0, "keyframe %d has no labelled pixel" % k
    kf = np.repeat(np.array(kfs, np.int32), len(px))
    q = np.concatenate([px]*len(kfs))
    ys, xs = np.nonzero(imgs[kfs[-1]] >= 0)
    pick = rng.integers(0, len(ys), 100)
    q[-104:-4] = np.stack([xs[pick], ys[pick]], 1)
    at = gpu.TextLabelAt(level, kf, q)
    want = np.concatenate([imgs[k][q[i*len(px):(i + 1)*len(px), 1], q[i*len(px):(i + 1)*len(px), 0]] for i, k in enumerate(kfs)])
    print("%s: %d queries, %d labelled" % (entry, len(q), int((at >= 0).sum())))
    assert (at >= 0).any() and (at < 0).any()
    assert np.array_equal(at.astype(np.float32), want)


# ------------------------------------------------------------------ 7. call semantics
def _raw(g, level, n, kf, px, label):
    p = lambda a: None if a is None else a.ctypes.data_as(IP)
    return g.lib.tsba_text_label_at(g.ctx, int(level), int(n), p(kf), p(px), p(label))


def test_call_semantics(tiny_state, gpu):
    from textslam_amd.optimizer import Optimizer
    g, G = tiny_state
    level = 0
    h, w = _shape(G, level)
    rng = np.random.default_rng(3)
    # mixed keyframes in one call == one query per call, and == the reversed list reversed
    ys, xs = np.nonzero(g.TextLabelImage(G.n_kf - 1, level, (h, w)) >= 0)
    pick = rng.integers(0, len(ys), 20)
    px = np.concatenate([_sample_px(rng, h, w, 40), np.stack([xs[pick], ys[pick]], 1)]).astype(np.int32)
    kf = rng.integers(0, G.n_kf, len(px)).astype(np.int32); kf[-20:] = G.n_kf - 1
    mixed = g.TextLabelAt(level, kf, px)
    assert (mixed >= 0).any() and (mixed < 0).any()
    single = np.array([g.TextLabelAt(level, kf[i:i + 1], px[i:i + 1])[0] for i in range(len(px))], np.int32)
    assert np.array_equal(mixed, single)
    assert np.array_equal(g.TextLabelAt(level, kf[::-1].copy(), px[::-1].copy())[::-1], mixed)
    for k in range(G.n_kf):                                                 # and == that keyframe's label image
        img = g.TextLabelImage(k, level, (h, w))
        assert np.array_equal(mixed[kf == k].astype(np.float32), img[px[kf == k, 1], px[kf == k, 0]])
    # pixels outside the level image
    out = np.array([[-1, 0], [0, -1], [w, 0], [0, h], [2**30, 2**30]], np.int32)
    inside = px[-1:]
    lab = g.TextLabelAt(level, G.n_kf - 1, np.concatenate([out, inside]))
    assert np.all(lab[:5] == -1) and lab[5] == mixed[-1] >= 0
    h2, w2 = _shape(G, 2)
    assert np.all(g.TextLabelAt(2, G.n_kf - 1, np.array([[w2, 0], [0, h2], [w - 1, h - 1]], np.int32)) == -1)      # the LEVEL's size decides
    # n == 0
    assert _raw(g, level, 0, None, None, None) == 0
    assert g.TextLabelAt(level, 0, np.zeros((0, 2), np.int32)).shape == (0,)
    # argument errors: TSBA_ERR_ARG, nothing written
    one_kf, one_px = np.array([0, 0], np.int32), np.array([[5, 5], [6, 6]], np.int32)
    for name, args in (("kf == n_kf", (level, 2, np.array([0, G.n_kf], np.int32), one_px)), ("kf < 0", (level, 2, np.array([-1, 0], np.int32), one_px)),
                       ("level == n_levels", (G.n_levels, 2, one_kf, one_px)), ("level < 0", (-1, 2, one_kf, one_px)), ("n < 0", (level, -1, one_kf, one_px)),
                       ("kf NULL", (level, 2, None, one_px)), ("px NULL", (level, 2, one_kf, None))):
        sentinel = np.full(2, 77, np.int32)
        assert _raw(g, *args, sentinel) == -1, name
        assert np.all(sentinel == 77), name
    assert _raw(g, level, 2, one_kf, one_px, None) == -1                    # NULL label
    assert b"tsba_text_label_at" in g.lib.tsba_last_error(g.ctx)
    assert np.array_equal(g.TextLabelAt(level, kf, px), mixed)              # the context still answers
    # a level of the problem that the options never use is not on the device
    o1 = abi.options_local(); o1.n_passes = 1; o1.levels[0] = 0
    gpu.upload(G.copy(), o1); gpu.solve()
    sentinel = np.full(2, 77, np.int32)
    assert _raw(gpu, 0, 2, one_kf, one_px, sentinel) == 0 and np.all(sentinel != 77)
    sentinel[:] = 77
    assert _raw(gpu, 2, 2, one_kf, one_px, sentinel) == -1 and np.all(sentinel == 77)
    # a keyframe without text observations
    I = synth.init_pair(n_pt=120, n_text=3)
    assert not (np.asarray(I.tobs_kf) == 0).any() and (np.asarray(I.tobs_kf) == 1).any()
    gpu.InitBA(I, options=abi.options_init())
    hi, wi = _shape(I, 0)
    assert np.all(gpu.TextLabelAt(0, 0, _grid(0, wi, 0, hi)) == -1)
    assert (gpu.TextLabelAt(0, 1, _grid(0, wi, 0, hi)) >= 0).any()
    # a fresh context: nothing uploaded
    fresh = Optimizer(0)
    sentinel[:] = 77
    assert _raw(fresh, 0, 2, one_kf, one_px, sentinel) == -4 and np.all(sentinel == 77)
    assert _raw(fresh, 0, 0, None, None, None) == -4
    fresh.close()


# ------------------------------------------------------------------ 8. state untouched
def _params(P):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (P.pose, P.rho, P.theta, P.sgood, P.tobs_good, P.tfgood))


def test_state_untouched(gpu):
    P = synth.tiny(seed=31, n_kf=5, n_pt=80, n_text=6, text_targets=4)
    h, w = _shape(P, 0)
    gpu.upload(P.copy(), abi.options_local())
    gpu.solve()
    A = _params(gpu.download(P.copy()))
    lab = gpu.TextLabelAt(0, P.n_kf - 1, _grid(0, w, 0, h))
    assert (lab >= 0).any()
    gpu.TextLabelAt(2, np.arange(40, dtype=np.int32) % P.n_kf, _grid(0, 8, 0, 5))
    B = _params(gpu.download(P.copy()))
    gpu.solve()
    Cc = _params(gpu.download(P.copy()))
    assert A == B, "tsba_text_label_at changed the state of the last solve"
    assert A == Cc, "a solve after tsba_text_label_at gives another result"
    assert np.array_equal(gpu.TextLabelAt(0, P.n_kf - 1, _grid(0, w, 0, h)), lab)


# ------------------------------------------------------------------ 9. from C++ through the adapter
def test_labels_at_centres_from_cxx(tmp_path, gpu):
    exe = str(tmp_path / "label_at_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "label_at_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsba", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    P = synth.make_problem(1, 200, 6, 13, feats=(8, 6, 4), frozen_frac=1.0, n_out=4, max_targets=1, text_targets=1)
    h, w = _shape(P, 0)
    G = P.copy()
    gpu.PoseOptim(G, options=abi.options_pose())
    img = gpu.TextLabelImage(0, 0, (h, w))
    ys, xs = np.nonzero(img >= 0)
    assert len(ys) > 0
    rng = np.random.default_rng(9)
    pick = rng.integers(0, len(ys), 12)
    inside = np.stack([xs[pick], ys[pick]], 1).astype(np.float64)
    inside[:4] += [[0.5, 0.5], [-0.5, 0.5], [0.5, -0.5], [-0.5, -0.5]]       # x.5: C round goes away from zero
    inside[4:8] += rng.uniform(-0.49, 0.49, (4, 2))
    centres = np.concatenate([inside, [[0.49, 0.49], [-0.5, 10.0], [w - 0.5, 10.0], [w - 0.51, h - 0.51], [1e12, -3.0]], rng.uniform(0, [w - 1, h - 1], (8, 2))])
    dump, cfile, out = str(tmp_path / "pose.bin"), str(tmp_path / "centres.bin"), str(tmp_path / "out.bin")
    abi.write_dump(dump, P.copy(), abi.STATE_NOTREACHWIN)
    with open(cfile, "wb") as f:
        f.write(np.ascontiguousarray(centres, np.float64).tobytes())
    res = subprocess.run([exe, dump, cfile, out], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "label at from C++: ok" in res.stdout, res.stdout
    raw = open(out, "rb").read()
    assert len(raw) == 7*8 + 4*len(centres)
    pose = np.frombuffer(raw, np.float64, 7)
    got = np.frombuffer(raw, np.float32, len(centres), 7*8)
    print("from C++: pose differs from the Python call's by %.3g" % np.abs(pose - np.asarray(G.pose, np.float64).reshape(-1)).max())
    assert np.abs(pose - np.asarray(G.pose, np.float64).reshape(-1)).max() < 1e-9      # the same solve
    r = np.where(centres >= 0, np.floor(centres + 0.5), np.ceil(centres - 0.5))        # C round
    r = np.where(np.abs(r) < 2.0**31, r, -1).astype(np.int32)
    want = gpu.TextLabelAt(0, 0, r)
    print("from C++: labels %s" % got.tolist())
    assert np.array_equal(got, want.astype(np.float32))
    ok = (r[:, 0] >= 0) & (r[:, 0] < w) & (r[:, 1] >= 0) & (r[:, 1] < h)
    assert (~ok).sum() >= 3 and np.all(got[~ok] == -1) and (got[:4] >= 0).sum() + (got[4:8] >= 0).sum() > 0
    assert np.array_equal(got[ok], img[r[ok, 1], r[ok, 0]])

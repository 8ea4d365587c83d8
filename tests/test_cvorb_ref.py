"""The CPU restatement of docs/cvorb_recalled.md (tests/cvorb_ref.py) against what can be known without OpenCV, so that a misunderstanding it shares
with the kernels cannot pass as agreement: cv::ORB's level sizes and quotas, angle and descriptor against the ORB-SLAM oracle where the two
extractors share their arithmetic (level 0), the sign of the Harris response on corner / edge / flat, the cuts' tie rule, the mask against the
oracle's cv::fillPoly, and that the shared fixture reaches every branch."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvorb_ref as R                                                 # noqa: E402
import oracle                                                         # noqa: E402


def test_level_sizes_and_quotas():
    sizes = R.level_sizes(640, 480)
    assert [s[0] for s in sizes] == [640, 533, 444, 370, 309, 257, 214, 179]
    assert [s[1] for s in sizes] == [480, 400, 333, 278, 231, 193, 161, 134]
    assert R.quotas(500) == [109, 90, 75, 63, 52, 44, 36, 31] and sum(R.quotas(500)) == 500
    assert R.level_sizes(200, 150)[4:] == [(96, 72), (80, 60), (67, 50), (56, 42)]
    assert sum(R.quotas(60)) == 60 and min(R.quotas(60)) >= 1
    assert R.quotas(1) == [0, 0, 0, 0, 0, 0, 0, 1]                     # (a quota of 0 keeps nothing; the last level takes the remainder)
    # the ORB-SLAM pyramid rounds cols * (1 / scale) with a cumulative fp32 scale: not the same planes
    pyr = R.pyramid(R.fixture_image())
    assert [p.shape[::-1] for p in pyr] == R.level_sizes(320, 240)


def test_level0_angle_and_descriptor_equal_the_orbslam_oracle():
    """Whole-frame quad: a level-0 keypoint at a position the ORB-SLAM oracle also keeps at octave 0 has the same angle and descriptor, bit for bit
    (IC_Angle, the blur and the taps are shared at level 0; the responses are not: Harris here, FAST score there)."""
    img = R.fixture_image()
    kp, desc = R.Frame(img).extract([R.FULL_320], nfeatures=2000)[0]         # (2000: most FAST corners of level 0 stay)
    kpo, desco = oracle.orb_extract(img)
    at = {(float(k[0]), float(k[1])): i for i, k in enumerate(kpo) if k[5] == 0}
    common = [(i, at[(float(k[0]), float(k[1]))]) for i, k in enumerate(kp) if k[5] == 0 and (float(k[0]), float(k[1])) in at]
    print("level-0 keypoints: restatement %d, oracle %d, common positions %d" % (int((kp[:, 5] == 0).sum()), len(at), len(common)))
    assert len(common) >= 50
    for i, j in common:
        assert kp[i, 3].view(np.uint32) == kpo[j, 3].view(np.uint32)
        assert np.array_equal(desc[i], desco[j])
    # and the whole-frame mask changes nothing: the quad covers every pixel
    assert R.mask_quad(320, 240, R.FULL_320).all()


def test_harris_sign_on_corner_edge_flat():
    corner = np.full((64, 64), 40, np.uint8); corner[32:, 32:] = 200   # an L-corner at (32, 32)
    edge = np.full((64, 64), 40, np.uint8); edge[:, 32:] = 200         # a straight vertical edge
    flat = np.full((64, 64), 90, np.uint8)
    r = [R.harris(p, [32], [32])[0] for p in (corner, edge, flat)]
    print("Harris response: corner %.6g  edge %.6g  flat %.6g" % tuple(r))
    assert r[0] > 0 and r[1] < 0 and r[2] == 0
    assert R.harris(flat, [], []).shape == (0,)
    # the sums by hand on the edge: Ix = 640 on the two columns beside the step, Iy = 0 -> a = 14 * 640^2, b = c = 0 -> -0.04 a^2 scale^4
    a = np.float32(14 * 640 * 640)
    assert r[1] == (np.float32(0) - (np.float32(0.04) * a) * a) * R._HARRIS_S4


def test_cut_keeps_all_ties_and_never_fewer_than_asked():
    rng = np.random.default_rng(5)
    for trial in range(200):
        n_pts = int(rng.integers(0, 60)); n = int(rng.integers(0, 40))
        v = rng.integers(20, 30, n_pts).astype(np.float32) if trial % 2 else rng.normal(0, 1, n_pts).astype(np.float32)
        keep = R.retain_best(v, n)
        assert keep.sum() >= min(n, n_pts)
        if n == 0:
            assert (not keep.any()) if n_pts > 0 else True
        if keep.any() and not keep.all():
            assert v[keep].min() > v[~keep].max()                      # a threshold: no tie is split
            assert (v >= v[keep].min()).sum() == keep.sum()
            assert (v > v[keep].min()).sum() < n                       # and the threshold is the n-th largest value
    assert R.retain_best(np.array([0.0, -0.0, 1.0], np.float32), 2).all()        # -0.f equals +0.f


def test_mask_equals_the_oracles_fillpoly():
    quads = [R.QUADS_320[0], R.QUADS_320[1], R.QUADS_320[2], [[5.9, 5.9], [5.2, 5.1], [5.0, 5.5], [5.7, 5.3]], [[-40, -40], [-10, -40], [-10, -5], [-40, -5]]]
    for q in quads:
        m = R.mask_quad(320, 240, q)
        ref = oracle.fillpoly4(320, 240, np.trunc(np.asarray(q, np.float64)).astype(np.int32))
        assert np.array_equal(m != 0, ref != 0)
    assert R.mask_quad(320, 240, quads[2]).sum() > 0 and R.mask_quad(320, 240, quads[3]).sum() == 1 and R.mask_quad(320, 240, quads[4]).sum() == 0
    assert int(R.mask_quad(320, 240, [[-0.9, -0.9], [3.9, -0.2], [3.2, 2.9], [-0.5, 2.1]]).sum()) == 12     # truncation toward zero: (0, 0) .. (3, 2)


def test_fixture_reaches_every_branch():
    seen = dict(emptied=0, ties=0, no_ties=0, uncut=0, quota_cut=0)
    for name, nf in (("320", 500), ("320", 60), ("320", 30), ("200", 500), ("200", 60)):
        img, res, stats = R.reference(name, nf)
        for d, st in enumerate(stats):
            assert sum(s["after2"] for s in st) == len(res[d][0])
            for s in st:
                if s["w"] <= 62 or s["h"] <= 62:
                    assert s["fast"] == 0; seen["emptied"] += 1
                if s["fast"] > 2 * s["quota"]:
                    seen["ties" if s["after1"] > 2 * s["quota"] else "no_ties"] += 1
                else:
                    seen["uncut"] += 1
                if s["after1"] > s["quota"]:
                    seen["quota_cut"] += 1; assert s["after2"] >= s["quota"]
        if name == "320":
            assert len(res[3][0]) == 0 and len(res[0][0]) > 0          # the quad inside the 31-px border: no keypoint
            kp = res[1][0]
            key = kp[:, 5].astype(np.int64) * 10 ** 8 + np.rint(kp[:, 1] / R.level_scales()[kp[:, 5].astype(int)]).astype(np.int64) * 10 ** 4 + np.rint(kp[:, 0] / R.level_scales()[kp[:, 5].astype(int)]).astype(np.int64)
            assert (np.diff(key) > 0).all()                            # level-major, raster order inside a level
        if name == "200":
            lv = np.concatenate([r[0][:, 5] for r in res])
            assert lv.max() == 4 and (lv == 4).any()                   # levels 5 - 7 (80 x 60, 67 x 50, 56 x 42) are emptied, level 4 (96 x 72) is not
            l4 = np.concatenate([r[0][r[0][:, 5] == 4] for r in res])
            y4 = np.rint(l4[:, 1] / R.level_scales()[4])
            assert y4.min() >= 31 and y4.max() <= 40                   # its 10-row band
        if (name, nf) == ("320", 30):
            assert all(s["fast"] > 2 * s["quota"] and s["after1"] > s["quota"] for s in stats[0])      # the large quad: every level is cut twice
    print(seen)
    assert all(v > 0 for v in seen.values()), seen

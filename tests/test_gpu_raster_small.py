"""The quad fill (csrc/tsraster.h) on images far below the 640 x 480 mask: 33 x 17 and 97 x 61 with 2 levels (17 x 9, 49 x 31), row lengths that are no
multiple of 32, so spans straddle mask words and a wrong window offset, word mask or slot base shows.  The quads are the QUADS table of
tests/cxx/raster_rows_host.cpp as fractions of the level size, at both levels.
  tsframe_box_pixels        (raster_quad with 1024 threads, wg_ordered_slot) equals oracle.frame_box_pixels bit for bit;
  tsframe_text_object_info  (raster_quad_rows, quad_box at two scales) gives the statistics, ok and pixels of its single calls on the same context;
  tsframe_pyramid_pts_batch (wg_ordered_slot in k_pts_batch) with one grid below PTS_LDS_CELLS cells and one above gives the single calls' results."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INV2 = [1.0, 0.5]
SIZES = [(33, 17), (97, 61)]
# (name, corner fractions of (w, h), integer offsets): corner = f * (w, h) + d
QUADS = [
    ("inside",                 (0.20, 0.30, 0.60, 0.25, 0.70, 0.60, 0.25, 0.70), (0,)*8),
    ("inside, full height",    (0.20, 0.00, 0.45, 0.00, 0.47, 1.00, 0.18, 1.00), (0, 2, 0, 3, 0, -3, 0, -4)),
    ("inside, one row high",   (0.30, 0.50, 0.60, 0.50, 0.61, 0.50, 0.29, 0.50), (0, 0, 0, 0, 0, 1, 0, 1)),
    ("whole image",            (0.00, 0.00, 1.00, 0.00, 1.00, 1.00, 0.00, 1.00), (0, 0, -1, 0, -1, -1, 0, -1)),
    ("left corner outside",    (-0.20, 0.40, 0.40, 0.30, 0.45, 0.70, 0.10, 0.75), (0,)*8),
    ("right corner outside",   (0.60, 0.30, 1.25, 0.45, 0.90, 0.80, 0.55, 0.70), (0,)*8),
    ("top corner outside",     (0.30, 0.20, 0.50, -0.35, 0.70, 0.25, 0.50, 0.60), (0,)*8),
    ("bottom corner outside",  (0.30, 0.70, 0.55, 0.40, 0.75, 0.75, 0.50, 1.40), (0,)*8),
    ("all corners outside",    (-0.30, -0.30, 1.30, -0.25, 1.35, 1.30, -0.25, 1.20), (0,)*8),
    ("far outside, over it",   (-3.00, -2.00, 4.00, -2.50, 3.50, 3.00, -2.50, 3.50), (0,)*8),
    ("diamond through sides",  (0.50, -0.40, 1.40, 0.50, 0.50, 1.40, -0.40, 0.50), (0,)*8),
    ("outside, not over it",   (1.10, 0.20, 1.50, 0.25, 1.45, 0.60, 1.15, 0.55), (0,)*8),
    ("above, not over it",     (0.20, -0.50, 0.60, -0.45, 0.55, -0.10, 0.25, -0.15), (0,)*8),
    ("two equal corners",      (0.20, 0.20, 0.20, 0.20, 0.70, 0.45, 0.30, 0.90), (0,)*8),
    ("zero height",            (0.10, 0.50, 0.40, 0.50, 0.90, 0.50, 0.60, 0.50), (0,)*8),
    ("zero height, outside x", (-0.30, 0.75, 0.40, 0.75, 1.30, 0.75, 0.60, 0.75), (0,)*8),
    ("zero width",             (0.50, 0.05, 0.50, 0.40, 0.50, 0.95, 0.50, 0.60), (0,)*8),
    ("one point",              (0.50, 0.50, 0.50, 0.50, 0.50, 0.50, 0.50, 0.50), (0,)*8),
    ("bow tie",                (0.20, 0.10, 0.80, 0.90, 0.80, 0.10, 0.20, 0.90), (0,)*8),
    ("bow tie, outside",       (-0.20, -0.10, 1.20, 1.10, 1.20, -0.10, -0.20, 1.10), (0,)*8),
    ("last row and column",    (0.60, 0.70, 1.00, 0.70, 1.00, 1.00, 0.60, 1.00), (0, 0, -1, 0, -1, -1, 0, -1)),
    ("sliver",                 (0.05, 0.05, 0.95, 0.93, 0.95, 0.94, 0.05, 0.06), (0,)*8),
]
PIX = ("u", "v", "featureInten", "featureNInten")


def _quads(w, h):
    size = np.array([w, h]*4, np.float64)
    return np.array([np.array(f)*size + np.array(d, np.float64) for _, f, d in QUADS]).reshape(-1, 4, 2)


def _img(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


@pytest.fixture(scope="module")
def fr():
    from textslam_amd.frame import Frame
    return Frame(0)


@pytest.mark.parametrize("w,h", SIZES)
def test_box_pixels_equal_the_oracle(fr, oracle_lib, w, h):
    img = _img(w, h, w)
    pyr = oracle_lib.frame_pyramid(img, 2)
    fr.GetPyrMat(img, 2)
    filled = 0
    for l in range(2):
        lh, lw = pyr[l][0].shape
        assert (lw, lh) == ((w, h), ((w + 1)//2, (h + 1)//2))[l]
        for (name, _, _), q in zip(QUADS, _quads(lw, lh)):
            got = fr.GetBoxAllPixs(l, q, 100.5, 31.25)
            ref = oracle_lib.frame_box_pixels(pyr[l][0], q, 100.5, 31.25)
            assert got["u"].dtype == np.int32 and got["v"].dtype == np.int32
            assert [got[k].tobytes() for k in PIX] == [np.ascontiguousarray(r).tobytes() for r in ref], (l, name)
            filled += len(ref[0]) > 0
        assert len(fr.GetBoxAllPixs(l, _quads(lw, lh)[3], 0.0, 1.0)["u"]) == lw*lh          # "whole image": every pixel
    assert filled >= 2*17                                                                 # (the quads beside the image fill nothing)


@pytest.mark.parametrize("w,h", SIZES)
def test_object_info_equals_its_single_calls(fr, w, h):
    img = _img(w + 1, h, w)
    fr.GetPyrMat(img, 2)
    quads = _quads(w, h)                                                                  # level-0 corners; level 1 takes them times 0.5
    none = {"level_off": np.zeros(3, np.int32), "u": np.zeros(0), "v": np.zeros(0), "inten": np.zeros(0)}
    got = fr.GetObjectInfoBatch(quads, INV2, [none]*len(quads))
    n_ok = 0
    for (name, _, _), q, g in zip(QUADS, quads, got):
        one = fr.GetObjectInfoBatch(q[None], INV2, [none])[0]
        assert g["statistics"].tobytes() == one["statistics"].tobytes() and g["ok"].tobytes() == one["ok"].tobytes(), name
        p = g["vRefPixs"]
        assert [p[k].tobytes() for k in PIX] == [one["vRefPixs"][k].tobytes() for k in PIX], name
        mu, sg = g["statistics"][0]
        box = fr.GetBoxAllPixs(0, q, mu, sg if g["ok"][0] else 1.0)
        assert [p[k].tobytes() for k in PIX[:3]] == [box[k].tobytes() for k in PIX[:3]], name
        if g["ok"][0]:
            assert p["featureNInten"].tobytes() == box["featureNInten"].tobytes(), name
            assert mu == p["featureInten"].sum()/len(p["u"]), name                       # the moments' mask is the pixels' mask
        else:
            assert not p["featureNInten"].any(), name
        n_ok += int(g["ok"][0]) + int(g["ok"][1])
    assert n_ok >= 2*14


def test_pyramid_pts_batch_equals_the_single_calls(fr):
    from textslam_amd.frame import PTS_LDS_CELLS
    w, h = 97, 61
    img = _img(5, h, w)
    fr.GetPyrMat(img, 2)
    rng = np.random.default_rng(6)
    box = (10.25, 8.5, 80.75, 50.0)
    text = np.stack([rng.uniform(box[0], box[2], 60), rng.uniform(box[1], box[3], 60)], 1).astype(np.float32)
    n = 36000
    scene = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)
    # the level-1 grids (tool.cc:599-616 / :898-907): n s^2 + 100 cells for a text set, + 500 for the scene, split by the aspect ratio
    wh = 49/31
    assert int(np.sqrt((n*0.25 + 500)/wh))*int(np.sqrt((n*0.25 + 500)*wh)) > PTS_LDS_CELLS > 60*0.25 + 100
    got = fr.GetPyramidPtsBatch([(0, text, box), (1, scene, None)], INV2)
    ref = [fr.GetPyramidPts(text, box[:2], box[2:], INV2), fr.GetPyramidPtsScene(scene, INV2)]
    for g, r in zip(got, ref):
        assert sorted(g) == sorted(r)
        for k in r:
            assert g[k].dtype == r[k].dtype and g[k].tobytes() == r[k].tobytes(), k
        assert g["level_off"][2] > g["level_off"][1] > 0                                   # features on both levels
    assert got[1]["level_off"][2] - got[1]["level_off"][1] > 1024                          # more than one tile of the compaction

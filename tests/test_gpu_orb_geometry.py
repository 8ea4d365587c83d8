"""The ORB front-end (libtsorb.so) at image sizes and strides off the 16-pixel grid, against the CPU oracle: every pyramid level with its border, the blurred
first and last level, and the features (x, y, size, angle, response, octave, 32 descriptor bytes) -- bit-exact, no tolerance anywhere.  The oracle itself is
pinned at these shapes by tests/test_orb_oracle.py.

Stale bytes cannot pass: before every forced plan or shape the same context runs once on the bitwise complement of the image(s), same geometry, so a tile
that a plan left unwritten holds wrong bytes.

What the sizes are about (textslam_amd/csrc/tsorb.hip): the 4- and 8-byte unaligned loads and the byte paths of level0_item / k_resize, k_pyramid_one's tile
sizing, FAST's dword staging and its two instances, the quadtree's start from round(width / height) nodes, the partial 64 x 64 blur tiles.

The limits (include/tsorb.h, next to tsorb_upload): a level under 62 px has no 30-px cell ((side - 32) / 30 = 0, the reference's ComputeKeyPointsOctTree divides
by it), and a level whose search area is more than twice as high as wide starts the reference's quadtree from round(width / height) = 0 nodes.  So the smallest
square at 8 levels is 221 x 221 (level 7: 62 px), not 199 x 199 (level 7: 56 px, a 24-px search area): 199 x 199 and (2.0, 3 levels) on 241 x 323 (level 2:
60 px) are refusals here, and their places in the extraction cases are taken by 221 x 221 and 247 x 323."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from orb_geometry import GEOMETRIES, OTHER_PYRAMIDS, accepted, geometry_images, level_sizes, most_levels, noise_frame      # noqa: E402
from textslam_amd.orbextractor import ORBextractor, synthetic_frame                                                         # noqa: E402

pytestmark = pytest.mark.gpu
QL_CAND = 4096                                      # candidates of a level the LDS quadtree holds (tsorb.hip): more take the serial pass
_REF = {}


def _same(a, b, what=None):
    kp_a, d_a = a; kp_b, d_b = b
    assert kp_a.shape == kp_b.shape, (what, kp_a.shape, kp_b.shape)
    assert np.array_equal(kp_a[:, [0, 1, 2, 4, 5]], kp_b[:, [0, 1, 2, 4, 5]]), what       # x, y, size, response, octave: bit-exact
    assert np.array_equal(kp_a[:, 3], kp_b[:, 3]), what                                  # angle
    assert np.array_equal(d_a, d_b), what                                                # 256-bit descriptors


def _ref(oracle, img, nfeatures=1000, scale=1.2, nlevels=8):
    """The oracle's answer for one image, computed once and left unchanged: every level, the blurred first and last level, the features."""
    key = (img.shape, img.tobytes(), nfeatures, scale, nlevels)
    if key not in _REF:
        lev = [oracle.orb_level(img, l, scale=scale, nlevels=nlevels) for l in range(nlevels)]
        blur = {l: oracle.orb_level(img, l, scale=scale, nlevels=nlevels, blurred=True) for l in sorted({0, nlevels - 1})}
        feat = oracle.orb_extract(img, nfeatures=nfeatures, scale=scale, nlevels=nlevels, cap=16384)
        sizes = level_sizes(img.shape[0], img.shape[1], scale, nlevels)
        assert [(a.shape[0] - 38, a.shape[1] - 38) for a in lev] == sizes, sizes       # the sizes the cases are chosen by, from the oracle
        for a in lev + list(blur.values()) + list(feat):
            a.setflags(write=False)
        _REF[key] = dict(lev=lev, blur=blur, feat=feat)
    return _REF[key]


def _check(ex, f, got, ref, what):
    """Frame f of the resident batch against a reference dictionary: levels, blurred levels, features."""
    for l, a in enumerate(ref["lev"]):
        b = ex.debug_level(f, l)
        assert b.shape == a.shape and np.array_equal(b, a), (what, "level", l, int((b != a).sum()) if b.shape == a.shape else b.shape)
    for l, a in ref["blur"].items():
        b = ex.debug_level(f, l, True)
        assert b.shape == a.shape and np.array_equal(b, a), (what, "blurred level", l)
    _same(got, ref["feat"], what)


def _padded(imgs, pad, fill):
    """[n, h, w + pad] buffer with the images in its first w columns and `fill` (a value, or a generator for random bytes) in the pad; returns (buffer, view)."""
    imgs = imgs if imgs.ndim == 3 else imgs[None]
    n, h, w = imgs.shape
    buf = np.full((n, h, w + pad), fill, np.uint8) if isinstance(fill, int) else fill.integers(0, 256, (n, h, w + pad)).astype(np.uint8)
    buf[:, :, :w] = imgs
    return buf, buf[:, :, :w]


def _run(ex, imgs, pad=0, fill=255):
    """Complement first (same geometry and stride), then the images."""
    if pad == 0:
        ex.extract_batch(255 - imgs)
        return ex.extract_batch(imgs)
    _, v = _padded(255 - imgs, pad, 0)
    ex.extract_batch(v, stride=v.shape[-1] + pad)
    _, v = _padded(imgs, pad, fill)
    return ex.extract_batch(v, stride=v.shape[-1] + pad)


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_single_frame_every_plan(oracle_lib, name):
    """One frame under every pyramid plan (tsorb_debug_pyramid -1, 0 = the chain, 1, 2, 3, and every split level 100 + s of the two launches) and, under the
    default pyramid, every FAST shape (tsorb_debug_fast_shape 0 .. 3).  Where the host finds no tiling that fits k_pyramid_one's buffers for a forced plan
    (q_inst < 0, tsorb_upload's tiling lambda), tsorb_run goes down its list: the two launches need both halves to fit, else the one launch for all levels
    if that fits, else (plan 3) the pairs if every pair fits, else the launch per level -- another plan, the same bytes, which is what is asserted here."""
    (h, w), nlevels = GEOMETRIES[name]
    assert accepted(h, w, 1.2, nlevels)
    for kind, img in geometry_images(name):
        ref = _ref(oracle_lib, img, nlevels=nlevels)
        if name[0] in "fg":
            assert len(ref["feat"][0]) >= 5, (name, kind, len(ref["feat"][0]))          # the case cannot pass empty
        ex = ORBextractor(1000, 1.2, nlevels, 20, 7, device=0)
        try:
            for mode in [-1, 0, 1, 2, 3] + [100 + s for s in range(nlevels)]:
                ex.debug_pyramid(mode)
                if mode >= 100:
                    ex.debug_pyramid(1)              # (100 + s moves the split; the shape is the two launches)
                got = _run(ex, img)[0]
                _check(ex, 0, got, ref, (name, kind, "pyramid plan", mode))
            ex.debug_pyramid(100 + 3); ex.debug_pyramid(-1)
            for shape in (0, 1, 2, 3):
                ex.debug_fast_shape(shape)
                got = _run(ex, img)[0]
                _check(ex, 0, got, ref, (name, kind, "fast shape", shape))
        finally:
            ex.close()


def _oracle_candidates(oracle, lev, ini_th=20, min_th=7):
    """Candidates of one level before the quadtree, ORBextractor.cc:780-830 cell by cell with the oracle's FAST (oracle.orb_fast = its cell routine on a ROI)."""
    roi = lev[19:-19, 19:-19]; h, w = roi.shape
    min_b, max_x, max_y = 16, w - 16, h - 16
    n_cols, n_rows = int(np.float32(max_x - min_b) / np.float32(30)), int(np.float32(max_y - min_b) / np.float32(30))
    w_cell, h_cell = int(np.ceil(np.float32(max_x - min_b) / n_cols)), int(np.ceil(np.float32(max_y - min_b) / n_rows))
    total = 0
    for i in range(n_rows):
        y0 = min_b + i * h_cell; y1 = min(y0 + h_cell + 6, max_y)
        if y0 >= max_y - 3:
            continue
        for j in range(n_cols):
            x0 = min_b + j * w_cell; x1 = min(x0 + w_cell + 6, max_x)
            if x0 >= max_x - 6:
                continue
            cell = np.ascontiguousarray(lev[19 + y0:19 + y1, 19 + x0:19 + x1])
            n = len(oracle.orb_fast(cell, ini_th, cap=4096))
            total += n if n else len(oracle.orb_fast(cell, min_th, cap=4096))
    return total


@pytest.mark.parametrize("name", ["a_479x637", "c_243x323"])
def test_batches(oracle_lib, name):
    """Batches of 3 (the few-frames plan), 6 (above P1_MAX_N: a launch per level) and, on the small geometry, 26 (from 24 frames the detector splits in two
    launches).  Frames 0 and n - 1 against the oracle, levels and features; every other frame against its own single-frame result.  The last frame of the batch
    of 6 is the noise image: its level-1 loads run to the end of the image allocation, and whether it takes the quadtree's serial pass follows from the oracle's
    candidate counts (more than QL_CAND on a level), which is what tsorb_debug_fallbacks must then say."""
    (h, w), nlevels = GEOMETRIES[name]
    ex = ORBextractor(1000, 1.2, nlevels, 20, 7, device=0); one = ORBextractor(1000, 1.2, nlevels, 20, 7, device=0)
    try:
        for n in (3, 6) + ((26,) if name.startswith("c_") else ()):
            imgs = np.stack([synthetic_frame(600 + 40 * n + s, w, h) for s in range(n)])
            if n == 6:
                imgs[n - 1] = noise_frame(77, w, h)
            ex.extract_batch(255 - imgs)
            before = ex.debug_fallbacks()
            res = ex.extract_batch(imgs)
            fired = ex.debug_fallbacks() - before
            for f in range(n):
                if f in (0, n - 1):
                    _check(ex, f, res[f], _ref(oracle_lib, imgs[f], nlevels=nlevels), (name, n, f))
                else:
                    alone = one.extract_batch(imgs[f])[0]
                    _same(res[f], alone, (name, n, f))
                    for l in range(nlevels):
                        assert np.array_equal(ex.debug_level(f, l), one.debug_level(0, l)), (name, n, f, l)
            if n == 6:
                counts = [_oracle_candidates(oracle_lib, a) for a in _ref(oracle_lib, imgs[n - 1], nlevels=nlevels)["lev"]]
                print(name, "noise frame: candidates per level", counts, "serial passes", fired)
                assert fired == (1 if max(counts) > QL_CAND else 0), (counts, fired)
            else:
                assert fired == 0
    finally:
        ex.close(); one.close()


@pytest.mark.parametrize("pad", [1, 3, 7, 24, 64])
def test_padded_rows(oracle_lib, pad):
    """stride = w + pad, the pad bytes 255 and then random, as batches of 1, 3 and 6: levels and features equal the oracle's (which is the stride == w result:
    that equality is test_single_frame_every_plan and test_batches), also after a second upload of the same geometry and stride, which only moves the pixels
    (tsorb_upload's same-geometry path).  The pad bytes are never part of any output."""
    rng = np.random.default_rng(900 + pad)
    for name in ["a_479x637", "c_243x323"] + (["b_376x1241"] if pad == 3 else []):
        (h, w), nlevels = GEOMETRIES[name]
        frames = np.stack([synthetic_frame(700 + s, w, h) for s in range(6)])
        ex = ORBextractor(1000, 1.2, nlevels, 20, 7, device=0); plain = ORBextractor(1000, 1.2, nlevels, 20, 7, device=0)
        try:
            for n in (1, 3, 6):
                imgs = frames[:n]
                base = plain.extract_batch(imgs)                                        # stride == w
                for fill in (255, rng, rng):                                            # (the third: the same geometry and stride again, other pad bytes)
                    res = _run(ex, imgs, pad, fill)
                    for f in range(n):
                        _same(res[f], base[f], (name, pad, n, f))
                        for l in range(nlevels):
                            assert np.array_equal(ex.debug_level(f, l), plain.debug_level(f, l)), (name, pad, n, f, l)
                        if f in (0, n - 1):
                            _check(ex, f, res[f], _ref(oracle_lib, imgs[f], nlevels=nlevels), (name, pad, n, f))
        finally:
            ex.close(); plain.close()


@pytest.mark.parametrize("nfeatures,scale,nlevels,shape", OTHER_PYRAMIDS[:2] + [(300, 2.0, 3, (247, 323))])
def test_other_pyramids_off_grid(oracle_lib, nfeatures, scale, nlevels, shape):
    """tests/test_gpu_orb.py's other pyramids at odd sizes, under the default plan and the chain.  (2.0, 3 levels) runs on 247 x 323: on 241 x 323 its last level
    is 60 x 81, under the 62 px of a cell -- that size is one of test_refusals_at_the_size_limits' cases."""
    h, w = shape
    assert accepted(h, w, scale, nlevels)
    img = synthetic_frame(90 + nlevels, w, h)
    ref = _ref(oracle_lib, img, nfeatures, scale, nlevels)
    ex = ORBextractor(nfeatures, scale, nlevels, 20, 7, device=0)
    try:
        for mode in (-1, 0):
            ex.debug_pyramid(mode)
            _check(ex, 0, _run(ex, img)[0], ref, (nfeatures, scale, nlevels, shape, mode))
    finally:
        ex.close()


@pytest.mark.parametrize("seed", range(8))
def test_seeded_sweep(oracle_lib, seed):
    """Five drawn geometries per seed: h, w in [64, 400], pad in {0, 1, 2, 3, 5}, scale in {1.2, 1.35, 1.5}, nfeatures in {100, 500}; nlevels = the largest value
    <= 8 that the limits of include/tsorb.h accept (every level >= 62 px on both sides with a search area at most twice as high as wide; a draw too tall for
    even one level is taken lying down, w and h swapped).  By construction the upload accepts every draw: a refusal fails the test."""
    rng = np.random.default_rng(4000 + seed)
    for k in range(5):
        h, w = int(rng.integers(64, 401)), int(rng.integers(64, 401))
        pad = int(rng.choice([0, 1, 2, 3, 5])); scale = float(rng.choice([1.2, 1.35, 1.5])); nfeatures = int(rng.choice([100, 500]))
        if most_levels(h, w, scale) == 0:
            h, w = w, h
        nlevels = most_levels(h, w, scale)
        draw = dict(seed=seed, k=k, h=h, w=w, pad=pad, scale=scale, nfeatures=nfeatures, nlevels=nlevels)
        assert nlevels >= 1, draw
        img = synthetic_frame(5000 + 10 * seed + k, w, h)
        ref = _ref(oracle_lib, img, nfeatures, scale, nlevels)
        ex = ORBextractor(nfeatures, scale, nlevels, 20, 7, device=0)
        try:
            _check(ex, 0, _run(ex, img[None], pad, rng)[0], ref, draw)
        finally:
            ex.close()


def _raw_extract(ex, img, w=None, h=None, stride=None, cap=None):
    """tsorb_extract_batch on sentinel-filled outputs (the pattern of _raw in tests/test_gpu_text_orb.py): rc, and whether the outputs are untouched."""
    img = np.ascontiguousarray(img, np.uint8)
    h = img.shape[0] if h is None else h; w = img.shape[1] if w is None else w; stride = img.shape[1] if stride is None else stride
    cap = ex.cap if cap is None else cap
    kp = np.full((cap, 6), 7.0, np.float32); de = np.full((cap, 32), 0x5a, np.uint8); cn = np.full(1, -77, np.int32)
    rc = ex.lib.tsorb_extract_batch(ex.ctx, img.ctypes.data_as(C.POINTER(C.c_uint8)), 1, w, h, stride, kp.ctypes.data_as(C.POINTER(C.c_float)),
                                    de.ctypes.data_as(C.POINTER(C.c_uint8)), cn.ctypes.data_as(C.POINTER(C.c_int32)), cap)
    return rc, bool(np.all(kp == 7.0) and np.all(de == 0x5a) and np.all(cn == -77))


def test_refusals_at_the_size_limits(oracle_lib):
    """Fault-free refusals: TSORB_ERR_ARG with the reason in tsorb_last_error, nothing launched, the caller's buffers untouched, the resident batch as it was --
    and the context then extracts the smallest accepted square.  198 x 400 and 400 x 198 at 8 levels (level 7: 55 px; the second is also too tall from level 0 on, which is the reason it is given), 199 x 199 (56 px: a 24-px search area),
    220 x 220 (61 px), (2.0, 3 levels) on 241 x 323 (60 px), a side of 63, stride = w - 1, and a frame whose search area is more than twice as high as wide
    (400 x 150: round(118 / 368) = 0 initial nodes -- before this limit was checked, such a frame reached the quadtree's serial pass, which indexed node -1)."""
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=0); ex3 = ORBextractor(300, 2.0, 3, 20, 7, device=0); ex1 = ORBextractor(1000, 1.2, 1, 20, 7, device=0)
    try:
        img0 = synthetic_frame(800, 323, 243)
        held = ex.extract_batch(img0)[0]                                               # a resident batch the refusals must leave alone
        lev0 = ex.debug_level(0, 3)
        err = lambda e: e.lib.tsorb_last_error(e.ctx).decode()
        for (h, w), word in (((198, 400), "62 px"), ((400, 198), "twice as high"), ((199, 199), "62 px"), ((220, 220), "62 px"), ((400, 150), "twice as high")):
            assert not accepted(h, w, 1.2, 8)
            last = oracle_lib.orb_level(np.zeros((h, w), np.uint8), 7).shape
            assert (last[0] - 38, last[1] - 38) == level_sizes(h, w)[7]                  # the size that decides, from the oracle
            rc, clean = _raw_extract(ex, synthetic_frame(801, w, h))
            assert rc == -1 and clean and "tsorb_upload" in err(ex) and word in err(ex), (h, w, rc, clean, err(ex))
        rc, clean = _raw_extract(ex3, synthetic_frame(802, 323, 241))
        assert rc == -1 and clean and "62 px" in err(ex3), err(ex3)
        rc, clean = _raw_extract(ex1, synthetic_frame(803, 150, 400))                   # one level: the search area's shape alone
        assert rc == -1 and clean and "twice as high" in err(ex1), err(ex1)
        big = synthetic_frame(804, 200, 200)
        for kw, word in ((dict(w=63), "64 x 64"), (dict(h=63), "64 x 64"), (dict(w=200, stride=199), "stride")):
            rc, clean = _raw_extract(ex1, big, **kw)
            assert rc == -1 and clean and word in err(ex1), (kw, err(ex1))
        assert np.array_equal(ex.debug_level(0, 3), lev0)                              # the resident batch is still there
        again = ex.download()[0]
        _same(again, held)
        (h, w), _ = GEOMETRIES["e_221x221"]
        img = synthetic_frame(805, w, h)
        _check(ex, 0, _run(ex, img)[0], _ref(oracle_lib, img), "221 x 221 after the refusals")
        img = noise_frame(806, 64, 64)
        _check(ex1, 0, _run(ex1, img)[0], _ref(oracle_lib, img, nlevels=1), "64 x 64 after the refusals")
    finally:
        ex.close(); ex3.close(); ex1.close()


def test_window_search_on_an_off_grid_frame(oracle_lib):
    """tsorb_match_set_frame + tsorb_match_search on two resident 479 x 637 frames against oracle.orb_match: the queries and the three max_cand values of
    tests/test_gpu_orb.py's parity test, with the frame's own bounds and a query at its last pixel."""
    h, w = 479, 637
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    try:
        imgs = np.stack([synthetic_frame(40, w, h), synthetic_frame(41, w, h)])
        (kpA, dA), (kpB, dB) = _run(ex, imgs)
        _same((kpB, dB), _ref(oracle_lib, imgs[1])["feat"])
        bounds = (0.0, float(w), 0.0, float(h))
        rng = np.random.default_rng(9)
        nq = kpA.shape[0]
        qxy = (kpA[:, :2] + rng.normal(0, 3.0, (nq, 2))).astype(np.float32)
        qr = np.where(rng.random(nq) < 0.5, 15.0, 40.0).astype(np.float32)
        oct_ = kpA[:, 5].astype(np.int32)
        qlev = np.stack([oct_ - 1, oct_ + 1], 1).astype(np.int32)
        keys = ("cand_cnt", "best_idx", "best_dist", "best_dist2", "cand_idx", "cand_dist")
        ex.match_set_frame(1, bounds)
        ref = oracle_lib.orb_match(kpB, dB, bounds, qxy, qr, qlev, dA, max_cand=8)
        got = ex.match_search(qxy, qr, qlev, dA, max_cand=8)
        for k in keys:
            assert np.array_equal(got[k], ref[k]), k
        assert (ref["cand_cnt"] > 0).mean() > 0.5 and ref["cand_cnt"].max() > 8
        qxy2 = qxy[:96].copy()
        qxy2[:9] = [[-500.0, -500.0], [5.0, 5.0], [636.0, 478.0], [320.0, 240.0], [2000.0, 100.0], [0.0, 478.0], [636.0, 0.0], [320.0, -30.0], [636.5, 478.5]]
        qr2 = np.where(np.arange(96) % 3 == 0, 300.0, 120.0).astype(np.float32)
        for mc in (4, 0, 256):
            ref3 = oracle_lib.orb_match(kpB, dB, bounds, qxy2, qr2, qlev[:96], dA[:96], max_cand=mc)
            got3 = ex.match_search(qxy2, qr2, qlev[:96], dA[:96], max_cand=mc)
            for k in keys:
                assert np.array_equal(got3[k], ref3[k]), (mc, k)
        assert ref3["cand_cnt"].max() > 128 and ref3["cand_cnt"][2] > 0                  # the query at (636, 478) finds candidates
    finally:
        ex.close()


def test_roi_of_a_larger_image(oracle_lib):
    """A cv::Mat ROI: the image is a window of a larger canvas, its stride the canvas' row, its last row ending with the canvas -- tsorb_upload reads
    (n h - 1) stride + w bytes, not n h stride.  The canvas around the window is random and is never part of any output."""
    rng = np.random.default_rng(31)
    for name in ("a_479x637", "c_243x323"):
        (h, w), nlevels = GEOMETRIES[name]
        img = synthetic_frame(820, w, h)
        ref = _ref(oracle_lib, img, nlevels=nlevels)
        ex = ORBextractor(1000, 1.2, nlevels, 20, 7, device=0)
        try:
            for x0, y0, right in ((37, 10, 0), (5, 3, 13)):
                canvas = rng.integers(0, 256, (1, y0 + h, x0 + w + right)).astype(np.uint8)
                canvas[0, y0:, x0:x0 + w] = 255 - img
                ex.extract_batch(canvas[:, y0:, x0:x0 + w], stride=canvas.shape[2])
                canvas[0, y0:, x0:x0 + w] = img
                got = ex.extract_batch(canvas[:, y0:, x0:x0 + w], stride=canvas.shape[2])[0]
                _check(ex, 0, got, ref, (name, x0, y0, right))
        finally:
            ex.close()


def test_more_cells_than_the_lds_quadtree_holds(oracle_lib):
    """1079 x 1919: level 0 has 62 x 34 = 2108 cells, more than the 2048 offsets k_octree keeps in LDS, so the level takes the serial pass (no frame the suite
    had was larger than 1280 x 720: 902 cells; this frame's levels 0 and 1 also carry more than QL_CAND candidates, 6727 and 4982 by the oracle's count).
    Default plan and the chain."""
    h, w = 1079, 1919
    img = np.ascontiguousarray(np.tile(synthetic_frame(830), (3, 3))[:h, :w])
    ref = _ref(oracle_lib, img)
    ex = ORBextractor(1000, 1.2, 8, 20, 7, device=0)
    try:
        for mode in (-1, 0):
            ex.debug_pyramid(mode)
            ex.extract_batch(255 - img)
            before = ex.debug_fallbacks()
            got = ex.extract_batch(img)[0]
            assert ex.debug_fallbacks() == before + 1, mode
            _check(ex, 0, got, ref, (h, w, mode))
    finally:
        ex.close()

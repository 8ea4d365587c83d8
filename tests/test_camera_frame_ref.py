"""The camera-frame entry without a GPU: the numpy restatement of docs/undistort_recalled.md (tests/camera_frame_ref.py) against what the arithmetic
must give where that is known in closed form -- the identity at zero distortion, the direct evaluation of the distortion model within half a
fixed-point step, hand-computed grey values -- and the five new symbols in the headers, the Python mirrors and the built libraries."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_frame_ref as R  # noqa: E402

SIZES = [(640, 480), (1241, 376), (4100, 6), (96, 70), (64, 20), (323, 243)]


def camera_K(w, h):
    """The reference's K at 640 x 480 and above, halved for the small sizes."""
    return R.K_REF if w >= 640 or h >= 480 else tuple(0.5*k for k in R.K_REF)


@pytest.mark.parametrize("w,h", SIZES)
def test_zero_distortion_is_the_identity(w, h):
    K = camera_K(w, h)
    xy, frac = R.undist_map(w, h, K, (0, 0, 0, 0, 0))
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    assert np.array_equal(xy[..., 0], j) and np.array_equal(xy[..., 1], i) and not frac.any()
    rng = np.random.default_rng(w*10007 + h)
    for shape in ((h, w, 3), (h, w)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        assert np.array_equal(R.undistort(img, K, (0, 0, 0, 0, 0), maps=(xy, frac)), img)


def test_strip_rows():
    assert [R.strip_rows(w, h) for w, h in SIZES] == [6, 3, 1, 42, 20, 12]
    assert 70 - 42 == 28 and 243 % 12 == 3 and 376 % 3 == 1 and 480 % 6 == 0      # the last strips the GPU test's sizes were chosen for


def test_invert3_closed_form():
    ir = R.invert3([[2.0, 0.0, 3.0], [0.0, 4.0, 5.0], [0.0, 0.0, 1.0]])
    assert ir == [0.5, 0.0, -1.5, 0.0, 0.25, -1.25, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("name", sorted(R.CAMERAS))
def test_fixed_point_map_against_direct_evaluation(name):
    dist, K_new = R.CAMERAS[name]
    u, v = R.map_uv(640, 480, R.K_REF, dist, K_new)
    xy, frac, iu, iv = R.fixed_point(u, v)
    ud, vd = R.map_uv_direct(640, 480, R.K_REF, dist, K_new)
    eu = np.abs(iu/32.0 - ud).max(); ev = np.abs(iv/32.0 - vd).max()
    print(name, "max |iu/32 - u_direct| = %.7f, |iv/32 - v_direct| = %.7f" % (eu, ev))
    assert eu <= 1/64 + 1e-6 and ev <= 1/64 + 1e-6                # half a step of the rounding + a margin far above fp64 noise
    # the split into integer and fraction gives the fixed-point value back
    assert np.array_equal(xy[..., 0].astype(np.int64)*32 + (frac & 31), iu) and np.array_equal(xy[..., 1].astype(np.int64)*32 + (frac >> 5), iv)


def test_border_branches_are_exercised():
    """The cameras of the GPU test reach what they were chosen for at 640 x 480: pincushion and newK leave the image (fully and by single taps) and reach
    negative fixed-point coordinates, barrel stays inside."""
    w, h = 640, 480
    for name, outside in (("barrel", False), ("pincushion", True), ("newK", True)):
        dist, K_new = R.CAMERAS[name]
        xy, frac = R.undist_map(w, h, R.K_REF, dist, K_new)
        sx = xy[..., 0].astype(int); sy = xy[..., 1].astype(int)
        full_out = (sx >= w) | (sx + 1 < 0) | (sy >= h) | (sy + 1 < 0)
        all_in = (sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)
        partial = ~full_out & ~all_in
        neg = (sx < 0) | (sy < 0)
        assert bool(full_out.any()) == outside and bool(neg.any()) == outside
        if outside:
            assert partial.sum() > 1000


def test_saturate_and_short_cast():
    t = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e12, -1e12, np.nan, 2147483647.4])
    assert list(R.saturate_int(t)) == [0, 2, 2, 0, -2, 2147483647, -2147483648, -2147483648, 2147483647]
    xy, frac, iu, iv = R.fixed_point(np.array([[40000.0, -0.03125]]), np.array([[-1.0, 3.96875]]))
    assert list(iu[0]) == [1280000, -1] and list(iv[0]) == [-32, 127]
    assert xy[0, 0, 0] == np.int16(40000 - 65536) and xy[0, 1, 0] == -1 and xy[0, 0, 1] == -1 and xy[0, 1, 1] == 3      # (short): wraps; >> is arithmetic
    assert list(frac[0]) == [0, 31*32 + 31]


def test_remap_weights_and_border():
    img = np.array([[10, 20], [30, 40]], np.uint8)
    xy = np.array([[[0, 0], [1, 1], [-1, 0], [0, 0]]], np.int16)
    frac = np.array([[16*32 + 16, 0, 31, 8*32 + 24]], np.uint16)
    out = R.remap(img, xy, frac)
    # centre of the four: 25; the corner itself; a tap pair left of the image: (1 * 0 + 31 * 10) / 32 = 9.69 -> 10; a = 24, b = 8: 21.25 -> 21
    assert list(out[0]) == [25, 40, 10, (8*24*32*10 + 24*24*32*20 + 8*8*32*30 + 24*8*32*40 + 16384) >> 15]
    a, b = np.meshgrid(np.arange(32), np.arange(32))
    assert ((32 - a)*(32 - b)*32 + a*(32 - b)*32 + (32 - a)*b*32 + a*b*32 == 32768).all()


def test_grey_of_hand_computed_triples():
    bgr = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 37], [1, 1, 1]]], np.uint8)
    # (1868 B + 9617 G + 4899 R + 8192) >> 14, by hand
    want = [255, 0, 29, 150, 76, 130, 1]
    assert list(R.grey(bgr, R.RAW_BGR)[0]) == want
    assert list(R.grey(bgr[..., ::-1], R.RAW_RGB)[0]) == want
    assert (1868*255 + 8192) >> 14 == 29 and (9617*255 + 8192) >> 14 == 150 and (4899*255 + 8192) >> 14 == 76
    assert (1868*10 + 9617*200 + 4899*37 + 8192) >> 14 == 130 and 1868 + 9617 + 4899 == 16384
    g = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(R.grey(g, R.RAW_GREY), g)


NEW = {"tsframe.h": ["tsframe_set_camera", "tsframe_set_raw_image", "tsframe_get_undist_map"], "tsorb.h": ["tsorb_upload_device", "tsorb_extract_device"]}
ARGS = {
    "tsframe_set_camera": ["void *ctx", "int w", "int h", "const double K[4]", "const double dist[5]", "const double K_new[4]"],
    "tsframe_set_raw_image": ["void *ctx", "const uint8_t *raw", "int stride", "int format", "int n_levels", "uint8_t *undist_out"],
    "tsframe_get_undist_map": ["void *ctx", "int16_t *xy", "uint16_t *frac"],
    "tsorb_upload_device": ["void *ctx", "const uint8_t *dev_imgs", "int n", "int w", "int h", "int stride", "int cap"],
    "tsorb_extract_device": ["void *ctx", "const uint8_t *dev_imgs", "int n", "int w", "int h", "int stride", "float *kp", "uint8_t *desc", "int32_t *count",
                             "int cap"],
}


def test_header_mirror_and_library_agree_on_the_new_symbols():
    import __graft_entry__ as ge
    from textslam_amd import frame, orbextractor
    libs = {"tsframe.h": "libtsframe.so", "tsorb.h": "libtsorb.so"}
    if not all(os.path.exists(os.path.join(ROOT, "textslam_amd", so)) for so in libs.values()):
        ge.build()
    mirrors = {"tsframe.h": (frame.EXPORTED_SYMBOLS, frame._load()), "tsorb.h": (orbextractor.EXPORTED_SYMBOLS, orbextractor.load_library())}
    for header, names in NEW.items():
        text = open(os.path.join(ROOT, "include", header)).read()
        lib = C.CDLL(os.path.join(ROOT, "textslam_amd", libs[header]))             # symbol lookup only: no context, no device
        exported, L = mirrors[header]
        for name in names:
            m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, text)
            assert m, "include/%s does not declare %s" % (header, name)
            args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
            assert args == ARGS[name]
            assert hasattr(lib, name), name
            assert name in exported
            assert len(getattr(L, name).argtypes) == len(ARGS[name]) and getattr(L, name).restype is C.c_int
    text = open(os.path.join(ROOT, "include", "tsframe.h")).read()
    for d, v in (("TSFRAME_RAW_BGR", frame.RAW_BGR), ("TSFRAME_RAW_RGB", frame.RAW_RGB), ("TSFRAME_RAW_GREY", frame.RAW_GREY)):
        assert int(re.search(r"^#define\s+%s\s+(\d+)" % d, text, re.M).group(1)) == v == getattr(R, d[len("TSFRAME_"):])
    for meth in ("SetCamera", "SetRawImage", "undist_map"):
        assert callable(getattr(frame.Frame, meth))
    for meth in ("upload_device", "extract_device"):
        assert callable(getattr(orbextractor.ORBextractor, meth))
    assert "undistort_recalled.md" in text and os.path.exists(os.path.join(ROOT, "docs", "undistort_recalled.md"))

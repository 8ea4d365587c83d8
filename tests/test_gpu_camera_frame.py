"""The camera-frame entry on the GPU, bit for bit (everything after the fp64 map is integer): tsframe_set_camera's map and tsframe_set_raw_image's
undistorted image against the numpy restatement of docs/undistort_recalled.md (tests/camera_frame_ref.py), the resident pyramid against a second
context given tsframe_set_image(the restatement's grey), tsorb_extract_device on the resident level 0 against tsorb_extract_batch on the same bytes
from the host, every refusal, and adapter/tsframe_camera_frame.hpp from C++."""
import ctypes as C
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_frame_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

# (w, h, n_levels): two strips of 42 + 28 rows; one strip; strips of one row; a last strip of 3 rows; the reference's size; a last strip of one row
SIZES = [(96, 70, 4), (64, 20, 3), (4100, 6, 1), (323, 243, 4), (640, 480, 4), (1241, 376, 4)]
FORMATS = [(R.RAW_BGR, 3), (R.RAW_RGB, 3), (R.RAW_GREY, 1)]


def camera_K(w, h):
    """The reference's K at 640 x 480 and above, halved for the small sizes."""
    return R.K_REF if w >= 640 or h >= 480 else tuple(0.5*k for k in R.K_REF)


@functools.lru_cache(maxsize=None)
def ref_map(w, h, name):
    dist, K_new = R.CAMERAS[name]
    xy, frac = R.undist_map(w, h, camera_K(w, h), dist, K_new)
    xy.setflags(write=False); frac.setflags(write=False)
    return xy, frac


def blocks_image(w, h, seed):
    """The 8 x 8 block image of test_gpu_text_orb.py: blocks of {40, 180} plus uniform noise in [-12, 12]."""
    rng = np.random.default_rng(seed)
    blocks = rng.choice(np.array([40.0, 180.0]), size=((h + 7)//8, (w + 7)//8))
    img = np.kron(blocks, np.ones((8, 8)))[:h, :w] + rng.uniform(-12, 12, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def raw_image(kind, w, h, ch, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    else:
        img = np.stack([blocks_image(w, h, seed + 31*k) for k in range(ch)], -1)
    return img if ch == 3 else img[..., 0]


def padded(img, pad):
    """The image as the first columns of a row-padded buffer whose pad bytes are 0xA5; pad == 0: the image itself."""
    if pad == 0:
        return np.ascontiguousarray(img)
    h, w = img.shape[:2]; ch = 1 if img.ndim == 2 else 3
    buf = np.full((h, w*ch + pad), 0xA5, np.uint8)
    view = np.ndarray(img.shape, np.uint8, buffer=buf, strides=(buf.strides[0], 3, 1) if ch == 3 else (buf.strides[0], 1))
    view[...] = img
    return view


def planes(fr, n_levels):
    return [fr.level(l, k) for l in range(n_levels) for k in range(4)]


def pts_outcome(fr, w, h, n_levels):
    """tsframe_pyramid_pts (scene grid) on the resident pyramid: its bytes, or its refusal."""
    from textslam_amd.frame import FrameError
    rng = np.random.default_rng(7)
    xy = (rng.uniform(0, 1, (200, 2))*[w - 1, h - 1]).astype(np.float32)
    try:
        o = fr.GetPyramidPtsScene(xy, [0.5**l for l in range(n_levels)])
    except FrameError as e:
        return str(e)
    return b"".join(o[k].tobytes() for k in ("level_off", "u", "v", "idx", "inten", "in"))


@pytest.fixture(scope="module")
def frames():
    from textslam_amd.frame import Frame
    return Frame(0), Frame(0)


@pytest.mark.parametrize("name", ["zero", "barrel", "pincushion", "newK"])
@pytest.mark.parametrize("w,h,n_levels", SIZES)
def test_bit_equal_to_the_restatement(frames, w, h, n_levels, name):
    fr, fr_ref = frames
    dist, K_new = R.CAMERAS[name]
    fr.SetCamera(w, h, camera_K(w, h), dist, K_new)
    xy, frac = ref_map(w, h, name)
    gxy, gfrac = fr.undist_map()
    assert np.array_equal(gxy, xy) and np.array_equal(gfrac, frac)
    if name == "zero":
        assert not frac.any()
    case = 0
    for fmt, ch in FORMATS:
        for kind in ("noise", "blocks"):
            for pad in (0, 5):
                case += 1
                img = raw_image(kind, w, h, ch, 1000*case + w)
                want_und, want_grey = R.camera_frame(img, fmt, None, None, maps=(xy, frac))
                und = fr.SetRawImage(padded(img, pad), fmt, n_levels, want_undistorted=True)
                assert und.shape == img.shape and np.array_equal(und, want_und), (fmt, kind, pad)
                if name == "zero":
                    assert np.array_equal(und, img)
                fr_ref.GetPyrMat(want_grey, n_levels)
                for a, b in zip(planes(fr, n_levels), planes(fr_ref, n_levels)):
                    assert np.array_equal(a, b), (fmt, kind, pad)
                # without the colour plane: the same level 0 (the other instance of the kernel)
                assert fr.SetRawImage(padded(img, pad), fmt, n_levels) is None and np.array_equal(fr.level(0), want_grey)
    assert pts_outcome(fr, w, h, n_levels) == pts_outcome(fr_ref, w, h, n_levels)
    gxy2, gfrac2 = fr.undist_map()                                    # every frame above used the one map
    assert np.array_equal(gxy2, xy) and np.array_equal(gfrac2, frac)


def test_judge_after_either_setup_gives_equal_bytes(frames):
    fr, fr_ref = frames
    w, h = 640, 480
    dist, K_new = R.CAMERAS["pincushion"]
    fr.SetCamera(w, h, R.K_REF, dist, K_new)
    img = raw_image("blocks", w, h, 3, 5)
    _, grey = R.camera_frame(img, R.RAW_BGR, None, None, maps=ref_map(w, h, "pincushion"))
    fr.SetRawImage(img, R.RAW_BGR, 4); fr_ref.GetPyrMat(grey, 4)
    K = np.array(R.K_REF)
    n = 6
    theta = np.tile([0.0, 0.0, -0.5], (n, 1)); Tcr = np.tile(np.eye(4)[:3], (n, 1, 1)); Tcr[:, 0, 3] = np.linspace(-0.02, 0.02, n)
    px = np.array([[[200 + 30*i, 150], [300 + 30*i, 150], [300 + 30*i, 220], [200 + 30*i, 220]] for i in range(n)], np.float64)
    ray = np.stack([(px[..., 0] - K[2])/K[0], (px[..., 1] - K[3])/K[1]], -1)
    uu, vv = np.meshgrid(np.arange(210, 290, 4), np.arange(155, 215, 4))
    uv = np.stack([uu.ravel(), vv.ravel()], -1).astype(np.int16)
    off = np.arange(n + 1, dtype=np.int32)*len(uv)
    uvs = np.concatenate([uv + [30*i, 0] for i in range(n)]).astype(np.int16)
    inten = grey[uvs[:, 1], uvs[:, 0]]
    dete = np.array([[250.0, 180.0], [400.0, 190.0]])
    outs = [f.TextJudgeBatch(0, theta, Tcr, ray, off, uvs, inten, K, K, dete_xy=dete) for f in (fr, fr_ref)]
    for k in ("pass", "reason", "cos", "zncc", "box_uv", "dete_bits"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    assert outs[0]["pass"].any()


def test_second_camera_replaces_the_map(frames):
    fr, _ = frames
    dist, K_new = R.CAMERAS["newK"]
    fr.SetCamera(96, 70, camera_K(96, 70), dist, K_new)
    fr.SetRawImage(raw_image("noise", 96, 70, 3, 1), R.RAW_BGR, 2)
    dist, K_new = R.CAMERAS["barrel"]
    fr.SetCamera(64, 20, camera_K(64, 20), dist, K_new)
    xy, frac = fr.undist_map()
    assert xy.shape == (20, 64, 2) and np.array_equal(xy, ref_map(64, 20, "barrel")[0]) and np.array_equal(frac, ref_map(64, 20, "barrel")[1])
    img = raw_image("noise", 64, 20, 1, 2)
    und = fr.SetRawImage(img, R.RAW_GREY, 2, want_undistorted=True)
    assert np.array_equal(und, R.undistort(img, None, None, maps=ref_map(64, 20, "barrel"))) and fr.level_shape(0) == (20, 64)
    # a frame's size is the camera's: a stride below the new width is refused
    assert fr.lib.tsframe_set_raw_image(fr.ctx, img.ctypes.data_as(C.POINTER(C.c_uint8)), 63, R.RAW_GREY, 2, None) == -1


def test_refusals_leave_everything_untouched():
    from textslam_amd.frame import Frame
    fr = Frame(0); L = fr.lib
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))            # noqa: E731
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))             # noqa: E731
    err = lambda: L.tsframe_last_error(fr.ctx).decode()               # noqa: E731
    w, h = 96, 70
    K = np.array(camera_K(w, h)); dist = np.array(R.CAMERAS["barrel"][0]); raw = raw_image("noise", w, h, 3, 3)
    xy_p = np.full((h, w, 2), 0x5A5A, np.int16); frac_p = np.full((h, w), 0x5A5A, np.uint16); und_p = np.full((h, w, 3), 0x5A, np.uint8)
    i16 = C.POINTER(C.c_int16); u16 = C.POINTER(C.c_uint16)
    # before a camera: TSFRAME_ERR_STATE for a frame and for the map
    assert L.tsframe_set_raw_image(fr.ctx, up(raw), 3*w, R.RAW_BGR, 2, up(und_p)) == -3 and "tsframe_set_raw_image" in err()
    assert L.tsframe_get_undist_map(fr.ctx, xy_p.ctypes.data_as(i16), frac_p.ctypes.data_as(u16)) == -3 and "tsframe_get_undist_map" in err()
    assert (xy_p == 0x5A5A).all() and (frac_p == 0x5A5A).all() and (und_p == 0x5A).all()
    assert L.tsframe_level_size(fr.ctx, 0, None, None) == -1                                     # no planes yet
    fr.SetCamera(w, h, K, dist); fr.SetRawImage(raw, R.RAW_BGR, 2)
    map0 = fr.undist_map(); planes0 = planes(fr, 2)

    def untouched():
        m = fr.undist_map()
        return (np.array_equal(m[0], map0[0]) and np.array_equal(m[1], map0[1]) and fr.level_shape(0) == (h, w) and fr.level_shape(1) == (35, 48) and
                all(np.array_equal(a, b) for a, b in zip(planes(fr, 2), planes0)) and (und_p == 0x5A).all() and (xy_p == 0x5A5A).all() and (frac_p == 0x5A5A).all())

    bad_K = [K*[0, 1, 1, 1], K*[1, 0, 1, 1], K*[np.nan, 1, 1, 1], K*[1, 1, np.inf, 1]]
    cams = [(w, h, None, dist, None), (w, h, K, None, None), (1, h, K, dist, None), (w, 1, K, dist, None), (8193, h, K, dist, None), (w, 8193, K, dist, None),
            (w, h, K, dist*[1, 1, np.nan, 1, 1], None), (w, h, K, np.array([0, 0, 0, 0, -np.inf]), None)]
    cams += [(w, h, k, dist, None) for k in bad_K] + [(w, h, K, dist, k) for k in bad_K]
    for cw, ch_, k, d, kn in cams:
        rc = L.tsframe_set_camera(fr.ctx, cw, ch_, dp(k) if k is not None else None, dp(d) if d is not None else None, dp(kn) if kn is not None else None)
        assert rc == -1 and "tsframe_set_camera" in err(), (cw, ch_, k, d, kn)
        assert untouched()
    frames_bad = [(None, 3*w, R.RAW_BGR, 2), (raw, 3*w - 1, R.RAW_BGR, 2), (raw, 3*w - 1, R.RAW_RGB, 2), (raw, w - 1, R.RAW_GREY, 2), (raw, 3*w, 3, 2),
                  (raw, 3*w, -1, 2), (raw, 3*w, R.RAW_BGR, 0), (raw, 3*w, R.RAW_BGR, 9), (raw, -3*w, R.RAW_BGR, 2)]
    for r, stride, fmt, nl in frames_bad:
        rc = L.tsframe_set_raw_image(fr.ctx, up(r) if r is not None else None, stride, fmt, nl, up(und_p))
        assert rc == -1 and "tsframe_set_raw_image" in err(), (stride, fmt, nl)
        assert untouched()
    for a, b in ((None, frac_p.ctypes.data_as(u16)), (xy_p.ctypes.data_as(i16), None)):
        assert L.tsframe_get_undist_map(fr.ctx, a, b) == -1 and "tsframe_get_undist_map" in err()
        assert untouched()
    assert L.tsframe_set_camera(None, w, h, dp(K), dp(dist), None) == -1 and L.tsframe_set_raw_image(None, up(raw), 3*w, 0, 2, None) == -1
    assert L.tsframe_get_undist_map(None, xy_p.ctypes.data_as(i16), frac_p.ctypes.data_as(u16)) == -1 and untouched()
    # and the context still works
    und = fr.SetRawImage(raw, R.RAW_BGR, 2, want_undistorted=True)
    assert np.array_equal(und, R.undistort(raw, None, None, maps=ref_map(w, h, "barrel")))


# ---- ORB from the resident level 0
QUADS = np.array([[[60, 50], [200, 55], [205, 120], [58, 118]], [[150, 100], [300, 100], [300, 200], [150, 200]]], np.float64)


def _text_outcome(ex):
    from textslam_amd.orbextractor import TsorbError
    try:
        return [(k.tobytes(), d.tobytes()) for k, d in ex.extract_text(0, QUADS, 500)]
    except TsorbError as e:                                           # (level 0 above 640 x 480: refused, after either upload alike)
        return str(e)


@pytest.mark.parametrize("w,h", [(323, 243), (640, 480), (1241, 376)])
def test_orb_from_the_resident_level(frames, w, h):
    from textslam_amd.orbextractor import ORBextractor
    fr, _ = frames
    dist, K_new = R.CAMERAS["barrel"]
    fr.SetCamera(w, h, camera_K(w, h), dist, K_new)
    ex_dev, ex_host = ORBextractor(device=0), ORBextractor(device=0)
    for seed in (11, 12):                                             # the second frame takes the same-geometry fast path
        fr.SetRawImage(raw_image("blocks", w, h, 3, seed), R.RAW_BGR, 4)
        grey = fr.level(0)
        kp_h, de_h = ex_host.extract_batch(grey)[0]
        kp_d, de_d = ex_dev.extract_device(fr.level_device_ptr(0), 1, h, w)[0]
        assert len(kp_h) > 100 and kp_d.tobytes() == kp_h.tobytes() and de_d.tobytes() == de_h.tobytes(), seed
        assert _text_outcome(ex_dev) == _text_outcome(ex_host)
    # the staged form, and the source may change once upload_device has returned
    ex_dev.upload_device(fr.level_device_ptr(0), 1, h, w)
    fr.SetRawImage(raw_image("noise", w, h, 3, 13), R.RAW_BGR, 4)
    ex_dev.run()
    kp_d, de_d = ex_dev.download()[0]
    assert kp_d.tobytes() == kp_h.tobytes() and de_d.tobytes() == de_h.tobytes()
    ex_dev.close(); ex_host.close()


def test_orb_refuses_a_host_pointer(frames):
    from textslam_amd.orbextractor import ORBextractor
    fr, _ = frames
    w, h = 323, 243
    dist, K_new = R.CAMERAS["barrel"]
    fr.SetCamera(w, h, camera_K(w, h), dist, K_new)
    fr.SetRawImage(raw_image("blocks", w, h, 1, 21), R.RAW_GREY, 2)
    ex = ORBextractor(device=0); L = ex.lib
    want = ex.extract_device(fr.level_device_ptr(0), 1, h, w)[0]
    host = fr.level(0)
    kp = np.full((ex.cap, 6), 7.0, np.float32); de = np.full((ex.cap, 32), 0x5A, np.uint8); cnt = np.full(1, -7, np.int32)
    fp, up, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    args = (1, w, h, w, kp.ctypes.data_as(fp), de.ctypes.data_as(up), cnt.ctypes.data_as(ip), ex.cap)
    for ptr in (host.ctypes.data, None):
        assert L.tsorb_extract_device(ex.ctx, C.c_void_p(ptr), *args) == -1 and "tsorb_upload_device" in L.tsorb_last_error(ex.ctx).decode()
        assert L.tsorb_upload_device(ex.ctx, C.c_void_p(ptr), 1, w, h, w, ex.cap) == -1
        assert (kp == 7.0).all() and (de == 0x5A).all() and cnt[0] == -7
    # the shared checks of tsorb_upload
    assert L.tsorb_upload_device(ex.ctx, C.c_void_p(fr.level_device_ptr(0)), 1, w, h, w - 1, ex.cap) == -1 and "stride < w" in L.tsorb_last_error(ex.ctx).decode()
    # the resident batch stayed as it was
    ex.run(); got = ex.download()[0]
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    ex.close()


# ---- adapter/tsframe_camera_frame.hpp from C++
def test_adapter_from_cxx(tmp_path, frames):
    from textslam_amd.orbextractor import ORBextractor
    exe = str(tmp_path / "camera_frame_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "camera_frame_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsframe", "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    txt = open(os.path.join(ROOT, "adapter", "tsframe_camera_frame.hpp")).read()
    assert "#include <opencv" not in txt and '#include "opencv' not in txt
    fr, _ = frames
    w, h, nl = 323, 243, 4
    dist, K_new = R.CAMERAS["newK"]
    K = camera_K(w, h)
    ex = ORBextractor(device=0)
    for fmt, ch, pad in ((R.RAW_RGB, 3, 7), (R.RAW_GREY, 1, 0)):
        img = raw_image("blocks", w, h, ch, 40 + ch)
        view = padded(img, pad); stride = view.strides[0]
        buf = np.full((h, stride), 0xA5, np.uint8); np.ndarray(img.shape, np.uint8, buffer=buf, strides=view.strides)[...] = img
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<7i", w, h, stride, ch, int(fmt == R.RAW_RGB), nl, 1))
            f.write(np.array(K, np.float64).tobytes() + np.array(dist, np.float64).tobytes() + np.array(K_new, np.float64).tobytes())
            f.write(buf.tobytes())
        res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and "camera frame from C++: ok" in res.stdout, res.stdout + res.stderr
        # the Python mirror
        fr.SetCamera(w, h, K, dist, K_new)
        und = fr.SetRawImage(view, fmt, nl, want_undistorted=True)
        kp, de = ex.extract_device(fr.level_device_ptr(0), 1, h, w)[0]
        raw = open(outp, "rb").read()
        (n,) = struct.unpack_from("<i", raw, 0); off = 4
        assert n == len(kp) and n > 100
        assert raw[off:off + 24*n] == kp.tobytes(); off += 24*n
        assert raw[off:off + 32*n] == de.tobytes(); off += 32*n
        assert raw[off:off + und.size] == und.tobytes(); off += und.size
        for l in range(nl):
            lw, lh = struct.unpack_from("<ii", raw, off); off += 8
            assert (lh, lw) == fr.level_shape(l)
            for k in range(4):
                assert raw[off:off + lw*lh] == fr.level(l, k).tobytes(), (l, k); off += lw*lh
        assert off == len(raw)
    ex.close()

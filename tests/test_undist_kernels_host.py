"""The camera-frame kernels (csrc/tsundist.h) on the host: tests/cxx/undist_kernels_host.cpp compiles k_undist_map and k_undist_grey as plain C++, one
"thread" at a time, with -fsanitize=address,undefined on heap blocks of exactly the library's sizes.  Its map, level 0 and colour plane equal the numpy
restatement (tests/camera_frame_ref.py) bit for bit at every size and camera of tests/test_gpu_camera_frame.py, and a remap through a map of random
entries touches nothing outside the raw frame.  No GPU, and no code loaded into Python: a stand-alone program."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_frame_ref as R  # noqa: E402

SIZES = [(96, 70), (64, 20), (4100, 6), (323, 243), (640, 480), (1241, 376), (7, 5), (2, 2)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("undist_host") / "undist_kernels_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-g", "-O1", "-I" + os.path.join(ROOT, "textslam_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cxx", "undist_kernels_host.cpp")])
    return out


@pytest.mark.parametrize("w,h", SIZES)
def test_kernels_as_host_code_equal_the_restatement(exe, tmp_path, w, h):
    K = R.K_REF if w >= 640 or h >= 480 else tuple(0.5*k for k in R.K_REF)
    rng = np.random.default_rng(w*31 + h)
    case = 0
    for name in ("zero", "barrel", "pincushion", "newK"):
        dist, K_new = R.CAMERAS[name]
        xy, frac = R.undist_map(w, h, K, dist, K_new)
        fmt, ch, pad = [(R.RAW_BGR, 3, 0), (R.RAW_RGB, 3, 5), (R.RAW_GREY, 1, 3), (R.RAW_BGR, 3, 1)][case % 4]; case += 1
        img = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
        stride = w*ch + pad
        buf = np.full((h, stride), 0xA5, np.uint8); buf[:, :w*ch] = img.reshape(h, w*ch)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<6i", w, h, stride, ch, int(fmt == R.RAW_RGB), 17 + case))
            f.write(np.array(K, np.float64).tobytes() + np.array(dist, np.float64).tobytes() + np.array(K_new if K_new else K, np.float64).tobytes())
            f.write(buf.tobytes()[:(h - 1)*stride + w*ch])
        res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and "undist kernels host: ok" in res.stdout, res.stdout + res.stderr
        raw = open(outp, "rb").read()
        n = w*h
        assert len(raw) == 4*n + 2*n + n + n*ch
        assert np.array_equal(np.frombuffer(raw, np.int16, 2*n).reshape(h, w, 2), xy), name
        assert np.array_equal(np.frombuffer(raw, np.uint16, n, 4*n).reshape(h, w), frac), name
        und, grey = R.camera_frame(img if ch == 3 else img[..., 0], fmt, None, None, maps=(xy, frac))
        assert np.array_equal(np.frombuffer(raw, np.uint8, n, 6*n).reshape(h, w), grey), name
        assert np.array_equal(np.frombuffer(raw, np.uint8, n*ch, 7*n).reshape(und.shape), und), name

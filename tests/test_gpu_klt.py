"""tsframe_klt_track on the device: bit-equal to the CPU restatement (tests/klt_ref.py, docs/klt_recalled.md) on the whole fixture, every point
independent of the others in the call, the resident planes untouched, every argument error, and the adapter's split from C++."""
import ctypes as C
import os
import struct
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as R                                                   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def calls():
    return R.fixture()


@pytest.fixture(scope="module")
def frames(calls):
    """One context pair per distinct image pair, four resident levels each (what GetPyrMat keeps for the BA)."""
    from textslam_amd.frame import Frame
    out = {}
    for c in calls:
        key = (id(c["A"]), id(c["B"]))
        if key not in out:
            fa, fb = Frame(0), Frame(0)
            fa.GetPyrMat(c["A"], 4); fb.GetPyrMat(c["B"], 4)
            out[key] = (fa, fb)
    return lambda c: out[(id(c["A"]), id(c["B"]))]


def _gpu(frames, c, pts=None):
    fa, fb = frames(c)
    return fb.TrackKLT(fa, c["pts"] if pts is None else pts, c["win"], c["max_level"], c["max_iter"], c["eps"], c["min_eig"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_klt_matches_restatement(calls, frames):
    total = 0
    for c in calls:
        pI, pJ = R.build_pyramid(c["A"], c["win"], c["max_level"]), R.build_pyramid(c["B"], c["win"], c["max_level"])
        ref_xy, ref_st, _ = R.track(pI, pJ, c["pts"], c["win"], c["max_iter"], c["eps"], c["min_eig"])
        xy, st = _gpu(frames, c)
        assert xy.dtype == np.float32 and xy.shape == ref_xy.shape and st.dtype == np.uint8
        fin = np.isfinite(ref_xy).all(1) & np.isfinite(xy).all(1)
        dev = np.abs(xy[fin].astype(np.float64) - ref_xy[fin].astype(np.float64)).max() if fin.any() else 0.0
        print("%-20s n %3d  levels %d  win %2d  status 1: %3d  status differs: %d  positions differing in bits: %d  largest |difference| %.3g px"
              % (c["name"], len(st), len(pI), c["win"], int(ref_st.sum()), int((st != ref_st).sum()),
                 int((_bits(xy) != _bits(ref_xy)).any(1).sum()), dev))
        assert np.array_equal(st, ref_st), c["name"]
        assert np.array_equal(_bits(xy), _bits(ref_xy)), c["name"]
        total += len(st)
    assert total >= 400


def test_points_independent_and_deterministic(calls, frames):
    for c in calls:
        if c["name"] not in ("main", "win31_level1", "small_dropped_level"):
            continue
        n = len(c["pts"])
        xy, st = _gpu(frames, c)
        xy2, st2 = _gpu(frames, c)
        assert xy.tobytes() == xy2.tobytes() and st.tobytes() == st2.tobytes()
        perm = np.random.default_rng(2).permutation(n)
        xp, sp = _gpu(frames, c, c["pts"][perm])
        assert np.array_equal(_bits(xp), _bits(xy[perm])) and np.array_equal(sp, st[perm])
        sub = np.arange(n)[3::5]                                       # a subset whose size is not a multiple of the workgroup's four points
        xs, ss = _gpu(frames, c, c["pts"][sub])
        assert np.array_equal(_bits(xs), _bits(xy[sub])) and np.array_equal(ss, st[sub])
        for i in list(range(0, n, 7)) + [n - 1]:
            x1, s1 = _gpu(frames, c, c["pts"][i:i + 1])
            assert np.array_equal(_bits(x1), _bits(xy[i:i + 1])) and s1[0] == st[i], (c["name"], i)


def test_resident_planes_unchanged_and_argument_errors(calls, frames):
    from textslam_amd.frame import Frame, FrameError
    c = calls[0]
    fa, fb = frames(c)
    L = fb.lib
    fp = C.POINTER(C.c_float); up = C.POINTER(C.c_uint8)
    pts = np.ascontiguousarray(c["pts"][:8], np.float32)

    def raw(prev=fa, cur=fb, n=8, xy=pts, win=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4, nxt=True, st=True):
        o_xy = np.full((8, 2), 7.0, np.float32); o_st = np.full(8, 0x5a, np.uint8)
        rc = L.tsframe_klt_track(None if prev is None else prev.ctx, None if cur is None else cur.ctx, n, None if xy is None else xy.ctypes.data_as(fp),
                                 win, max_level, max_iter, eps, min_eig, o_xy.ctypes.data_as(fp) if nxt else None, o_st.ctypes.data_as(up) if st else None)
        return rc, bool(np.all(o_xy == 7.0) and np.all(o_st == 0x5a))

    before = [f.level(l, k).copy() for f in (fa, fb) for l in range(4) for k in range(4)]
    rc, same = raw(); assert rc == 0 and not same
    rc, same = raw(n=0, xy=None, nxt=False, st=False); assert rc == 0                       # n == 0: nothing to do
    rc, same = raw(n=0); assert rc == 0 and same
    empty = Frame(0)                                                                        # a context without an image
    small = Frame(0); small.GetPyrMat(np.ascontiguousarray(c["A"][:240, :320]), 4)          # another level-0 size
    two = Frame(0); two.GetPyrMat(c["A"], 2)                                                # too few resident levels for max_level 3
    cases = [("prev_ctx NULL", dict(prev=None)), ("cur_ctx NULL", dict(cur=None)), ("n < 0", dict(n=-1)), ("prev_xy NULL", dict(xy=None)),
             ("next_xy NULL", dict(nxt=False)), ("status NULL", dict(st=False)), ("win even", dict(win=20)), ("win 1", dict(win=1)), ("win 33", dict(win=33)),
             ("max_level -1", dict(max_level=-1)), ("max_level 8", dict(max_level=8)), ("max_iter 0", dict(max_iter=0)), ("max_iter 101", dict(max_iter=101)),
             ("eps < 0", dict(eps=-0.5)), ("eps NaN", dict(eps=float("nan"))), ("level-0 sizes differ", dict(prev=small)),
             ("level-0 sizes differ (cur)", dict(cur=small)), ("prev holds 2 levels", dict(prev=two)), ("cur holds 2 levels", dict(cur=two)),
             ("max_level 7 on 4 resident levels", dict(max_level=7, win=3))]
    for name, kw in cases:
        rc, same = raw(**kw)
        assert rc == -1 and same, name
        if kw.get("cur", fb) is not None:
            assert "tsframe_klt_track" in L.tsframe_last_error(kw.get("cur", fb).ctx).decode(), name
    for name, kw in (("prev without image", dict(prev=empty)), ("cur without image", dict(cur=empty))):
        rc, same = raw(**kw)
        assert rc == -3 and same, name
    import torch
    if torch.cuda.device_count() > 1:                                                       # contexts on different devices
        other = Frame(1); other.GetPyrMat(c["A"], 4)
        rc, same = raw(prev=other); assert rc == -1 and same
    with pytest.raises(FrameError):
        fb.TrackKLT(empty, pts)
    rc, same = raw(prev=two, cur=two, max_level=1); assert rc == 0 and not same             # two levels are enough for max_level 1
    x1, s1 = two.TrackKLT(two, pts, max_level=1)                                            # a context against itself: nothing moves
    assert np.all(s1 == 1) and np.abs(x1 - pts).max() < 0.01
    e_xy, e_st = fb.TrackKLT(fa, np.zeros((0, 2), np.float32))
    assert e_xy.shape == (0, 2) and e_st.shape == (0,)
    for cc in calls[:4]:
        _gpu(frames, cc)
    after = [f.level(l, k) for f in (fa, fb) for l in range(4) for k in range(4)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_adapter_split_from_cxx(tmp_path, calls, frames):
    exe = str(tmp_path / "klt_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "klt_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsframe", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    c = calls[0]
    pts = c["pts"]
    sizes = [0, 17, 1, 0, 40, len(pts) - 58 - 5, 5, 0]                                      # detections, some without a feature
    assert sum(sizes) == len(pts) and min(sizes) == 0
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<iiii", c["A"].shape[1], c["A"].shape[0], 4, len(sizes)))
        f.write(c["A"].tobytes()); f.write(c["B"].tobytes())
        at = 0
        for m in sizes:
            f.write(struct.pack("<i", m)); f.write(np.ascontiguousarray(pts[at:at + m], np.float32).tobytes()); at += m
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "klt from C++: ok" in res.stdout, res.stdout
    xy, st = _gpu(frames, c)
    raw = open(outp, "rb").read()
    off = 0; at = 0
    for m in sizes:
        (got_m,) = struct.unpack_from("<i", raw, off); off += 4
        assert got_m == m                                                                   # empty inner vectors are preserved
        g_xy = np.frombuffer(raw, np.float32, 2*m, off).reshape(m, 2); off += 8*m
        g_st = np.frombuffer(raw, np.uint8, m, off); off += m
        assert np.array_equal(_bits(g_xy), _bits(xy[at:at + m])) and np.array_equal(g_st, st[at:at + m])
        at += m
    assert off == len(raw)

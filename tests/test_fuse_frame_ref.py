"""tsorb_fuse_frame without a GPU: the restatement of cv::pointPolygonTest (tests/fuse_frame_ref.py, docs/pointpolygon_recalled.md) on hand cases and against an exact
even-odd count, the same test as csrc/tsfuse.h states it (compiled by plain g++) on 20 000 seeded pairs, the C++ driver's host transcription of
tool::BoundFeatDele_T + frame::FeatFusion list for list, and the C ABI: header, library and Python mirror agree, and a NULL context is refused."""
import ctypes as C
import os
import re
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvorb_ref as R                                                 # noqa: E402
import fuse_frame_ref as FR                                           # noqa: E402

HDR = os.path.join(ROOT, "include", "tsorb.h")
CSRC = os.path.join(ROOT, "textslam_amd", "csrc")
SQUARE = [[10, 10], [30, 10], [30, 20], [10, 20]]
SLANT = [[10, 10], [30, 14], [28, 30], [8, 24]]


def test_hand_cases():
    pp = FR.point_polygon_positive
    assert pp(SQUARE, 20.0, 15.0) and pp(SQUARE, 10.5, 10.25) and pp(SLANT, 20.0, 20.0)             # strictly inside
    for x, y in ((20.0, 10.0), (30.0, 15.5), (10.0, 19.75), (20.0, 20.0)):                          # on an edge: the distance is zero
        assert not pp(SQUARE, x, y), (x, y)
    assert not pp(SLANT, 20.0, 12.0) and not pp(SLANT, 29.0, 22.0)                                  # on a slanted edge (exactly representable points of it)
    for x, y in SQUARE + SLANT:                                                                     # on a vertex
        assert not pp(SQUARE if [x, y] in SQUARE else SLANT, float(x), float(y)), (x, y)
    for x, y in ((40.0, 10.0), (5.0, 20.0), (30.0, 25.0), (10.0, 5.0)):                             # on the extension of an edge
        assert not pp(SQUARE, x, y), (x, y)
    assert not pp(SLANT, 40.0, 16.0) and not pp(SLANT, 0.0, 8.0)                                    # (the extension of SLANT's first edge)
    for x, y in ((0.0, 0.0), (20.0, 9.75), (30.25, 15.0), (20.0, 25.0), (-5.0, 15.0), (1e6, 15.0)):  # outside
        assert not pp(SQUARE, x, y), (x, y)
    # a point whose y equals a vertex's y: one crossing is counted, not two and not none
    assert pp(SLANT, 20.0, 14.0) and pp(SLANT, 12.0, 24.0) and not pp(SLANT, 31.0, 14.0) and not pp(SLANT, 7.0, 24.0) and not pp(SLANT, 40.0, 10.0)
    assert pp([[0, 0], [10, 10], [20, 0], [10, 30]], 10.0, 12.0) and not pp([[0, 0], [10, 10], [20, 0], [10, 30]], 10.0, 5.0)     # y of the reflex vertex, above and below it
    # the orientation does not matter, nor where the contour starts
    assert pp(SQUARE[::-1], 20.0, 15.0) and pp(SLANT[2:] + SLANT[:2], 20.0, 20.0) and not pp([], 1.0, 1.0)
    # the polygons of a detection: GetNewDeteBox's corner order and cv::Point's truncation (towards zero, also below zero)
    assert FR.shrunk_quad([[60.0, 50.0], [259.9, 50.0], [259.9, 189.0], [60.0, 189.0]], -3.0) == [[63, 53], [256, 53], [256, 186], [63, 186]]
    assert FR.shrunk_quad([[-0.5, -4.2], [9.9, -4.2], [9.9, 7.7], [-0.5, 7.7]], -3.0) == [[2, -1], [6, -1], [6, 4], [2, 4]]
    assert FR.bbox_quad([-1.5, 2.9, 7.2, 8.0]) == [[-1, 2], [7, 2], [7, 8], [-1, 8]]


def _even_odd_exact(poly, x4, y4):
    """Exact even-odd rule in integers for the point (x4 / 4, y4 / 4): False on the boundary.  An edge counts when exactly one end lies at or below the point's y and
    the edge passes strictly to the right of the point."""
    P = [(4 * px, 4 * py) for px, py in poly]
    count = 0
    for (ax, ay), (bx, by) in zip(P[-1:] + P[:-1], P):
        cross = (bx - ax) * (y4 - ay) - (by - ay) * (x4 - ax)
        if cross == 0 and min(ax, bx) <= x4 <= max(ax, bx) and min(ay, by) <= y4 <= max(ay, by):
            return False
        if (ay <= y4) != (by <= y4):
            # x of the edge at y4, compared with x4: (ax + (y4 - ay) (bx - ax) / (by - ay)) > x4
            num, den = (y4 - ay) * (bx - ax) - (x4 - ax) * (by - ay), by - ay
            if (num > 0) == (den > 0) and num != 0:
                count += 1
    return count % 2 == 1


NARROW = [[100.0, 60.0], [105.0, 60.0], [105.0, 180.0], [100.0, 180.0]]          # 5 px wide: the shrunk polygon's left and right sides change places
BOWTIE = [[100.0, 60.0], [104.0, 60.0], [130.0, 100.0], [90.0, 100.0]]          # narrower than 2 |win| at the top only: the shrunk polygon crosses itself
FLAT = [[40.0, 20.0], [80.0, 21.0], [80.0, 25.0], [40.0, 24.0]]                 # 4 px high, slanted: top and bottom change places


@pytest.mark.parametrize("quad", [NARROW, BOWTIE, FLAT], ids=["inverted", "bow-tie", "flat"])
def test_narrow_quads_decide_by_parity(quad):
    poly = FR.shrunk_quad(quad, -3.0)
    xs, ys = [p[0] for p in poly], [p[1] for p in poly]
    if quad is NARROW:
        assert poly[0][0] > poly[1][0]                                  # inverted
    n_in = n = 0
    for y4 in range(4 * min(ys) - 6, 4 * max(ys) + 7, 1 if max(ys) - min(ys) < 20 else 3):
        for x4 in range(4 * min(xs) - 6, 4 * max(xs) + 7):
            got = FR.point_polygon_positive(poly, x4 / 4.0, y4 / 4.0)
            assert got == _even_odd_exact(poly, x4, y4), (poly, x4 / 4.0, y4 / 4.0, got)
            n += 1; n_in += got
    print(poly, n, "points,", n_in, "inside")
    assert 0 < n_in < n


def _build(tmp_path, name, src, extra=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-I" + CSRC, *extra, "-o", exe, os.path.join(ROOT, "tests", "cxx", src)])
    return exe


def _seeded_pairs(n=20000, seed=17):
    """n (quad, point) pairs; half of the points lie on an edge or a vertex of their quad (where float32 can hold such a point)."""
    rng = np.random.default_rng(seed)
    polys = np.zeros((n, 4, 2), np.int32); pts = np.zeros((n, 2), np.float32)
    for i in range(n):
        c = rng.integers(-40, 700, 2); s = rng.integers(1, 200, 2)
        base = np.array([[0, 0], [s[0], 0], [s[0], s[1]], [0, s[1]]])
        p = c + base + rng.integers(-12, 13, (4, 2)) * (rng.random() < 0.8)
        if rng.random() < 0.3:
            p = p[rng.permutation(4)]                                  # any order: crossed and degenerate contours too
        if rng.random() < 0.05:
            p[rng.integers(4)] = p[rng.integers(4)]                    # a repeated vertex
        polys[i] = p
        kind = rng.integers(3) if i % 2 else rng.integers(3, 6)       # every second point exactly on a vertex or an edge
        k = rng.integers(4); a, b = p[k - 1].astype(np.float64), p[k].astype(np.float64)
        if kind == 0:
            pt = b                                                     # a vertex
        elif kind in (1, 2):
            pt = a + (b - a) * rng.integers(0, 9) / 8.0                # on the edge, at an eighth
        elif kind == 3:
            pt = a + (b - a) * rng.uniform(-0.5, 1.5)                  # near the edge's line, extension included
        elif kind == 4:
            pt = np.array([rng.uniform(p[:, 0].min() - 5, p[:, 0].max() + 5), float(p[rng.integers(4), 1])])     # a vertex's y
        else:
            pt = np.array([rng.uniform(p[:, 0].min() - 5, p[:, 0].max() + 5), rng.uniform(p[:, 1].min() - 5, p[:, 1].max() + 5)])
            if rng.random() < 0.5:
                pt = np.rint(pt * 4) / 4                               # FAST corners scaled back: often on the quarter grid
        pts[i] = pt
    return polys, pts


def test_header_statement_equals_the_restatement(tmp_path):
    exe = _build(tmp_path, "point_polygon_host", "point_polygon_host.cpp")
    polys, pts = _seeded_pairs()
    inp, outp = tmp_path / "pp_in.bin", tmp_path / "pp_out.bin"
    rec = np.zeros(len(polys), np.dtype([("p", np.int32, (4, 2)), ("pt", np.float32, 2)])); rec["p"] = polys; rec["pt"] = pts
    inp.write_bytes(np.int32(len(polys)).tobytes() + rec.tobytes())
    subprocess.check_call([exe, str(inp), str(outp)])
    got = np.frombuffer(outp.read_bytes(), np.uint8)
    ref = np.array([FR.point_polygon_positive(polys[i].tolist(), pts[i, 0], pts[i, 1]) for i in range(len(polys))], np.uint8)
    print(len(ref), "pairs,", int(ref.sum()), "inside; differing:", int((got != ref).sum()))
    assert got.shape == ref.shape and 2000 < ref.sum() < 12000
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:10]
    # the two polygons of a detection, truncation included
    rng = np.random.default_rng(23)
    v = np.concatenate([rng.uniform(-50, 700, (300, 12)), rng.choice([-3.0, -7.5, 2.25, 0.0], (300, 1))], 1)
    v[:50, :12] = np.rint(v[:50, :12] * 2) / 2
    inp.write_bytes(np.int32(len(v)).tobytes() + np.ascontiguousarray(v, np.float64).tobytes())
    subprocess.check_call([exe, "--polys", str(inp), str(outp)])
    got = np.frombuffer(outp.read_bytes(), np.int32).reshape(-1, 2, 4, 2)
    for i in range(len(v)):
        assert got[i, 0].tolist() == FR.shrunk_quad(v[i, :8], v[i, 12]) and got[i, 1].tolist() == FR.bbox_quad(v[i, 8:12]), i


def test_host_mode_of_the_driver_equals_the_restatement(tmp_path):
    exe = _build(tmp_path, "fuse_frame_from_cxx", "fuse_frame_from_cxx.cpp", ("-DFUSE_HOST_ONLY",))
    img, raw, _ = R.reference("320", 500)
    rng = np.random.default_rng(31)
    skp = rng.uniform(0, 300, (37, 6)).astype(np.float32); sde = rng.integers(0, 256, (37, 32)).astype(np.uint8)
    skp[:, 5] = rng.integers(0, 8, 37)                                 # (the octave is an int in cv::KeyPoint)
    bb = FR.bbox_of(R.QUADS_320); bb[1] = [95.0, 60.0, 250.0, 180.0]              # (a bounding box that cuts as well)
    for scene, win in (((skp, sde), -3.0), ((skp[:0], sde[:0]), -6.5)):          # with and without scene rows (FeatFusion's two branches)
        ref = FR.fuse_frame(scene[0], scene[1], raw, R.QUADS_320, bb, win)
        kept = np.diff(ref["text_off"]).tolist()
        assert all(0 < k < r for k, r in zip(kept[:3], ref["raw_count"][:3])) and kept[3] == 0
        inp, outp = tmp_path / "host_in.bin", tmp_path / "host_out.bin"
        inp.write_bytes(FR.host_input(scene[0], scene[1], raw, R.QUADS_320, bb, win))
        res = subprocess.run([exe, "--host", str(inp), str(outp)], capture_output=True, text=True)
        assert res.returncode == 0 and "fuse frame from C++: ok" in res.stdout, res.stdout + res.stderr
        FR.assert_lists_equal(FR.read_lists(outp.read_bytes()), FR.lists_of(ref, 4))


# ---- the C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    so = os.path.join(ROOT, "textslam_amd", "libtsorb.so")
    if not os.path.exists(so):
        ge.build()
    from textslam_amd import orbextractor
    return orbextractor.load_library()


_CTYPE = {C.c_void_p: "void *", C.c_int: "int", C.c_double: "double", C.POINTER(C.c_int32): "int32_t *", C.POINTER(C.c_float): "float *", C.POINTER(C.c_double): "double *",
          C.POINTER(C.c_uint8): "uint8_t *"}


def test_header_library_and_mirror_agree(lib, tmp_path):
    from textslam_amd import orbextractor
    name = "tsorb_fuse_frame"
    text = open(HDR).read()
    assert name in set(re.findall(r"\b(tsorb_[a-z_0-9]+)\s*\(", text)), name + " not declared in include/tsorb.h"
    assert hasattr(lib, name), name + " not exported by libtsorb.so"
    assert name in orbextractor.EXPORTED_SYMBOLS and hasattr(orbextractor.ORBextractor, "fuse_frame")
    fn = getattr(lib, name)
    assert fn.restype == C.c_int and len(fn.argtypes) == 20
    args = [("const " + _CTYPE[t]) if k in (3, 4) else _CTYPE[t] for k, t in enumerate(fn.argtypes)]          # quad and bbox are the const pointers of the prototype
    src = tmp_path / "sig.c"
    src.write_text('#include "tsorb.h"\nint (*p_%s)(%s) = %s;\n' % (name, ", ".join(args), name))
    cmd = ["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sig.o"), str(src)]
    subprocess.check_call(cmd)
    bad = tmp_path / "bad.c"                                           # the check has teeth: float corners where the header has doubles do not compile
    bad.write_text(src.read_text().replace("const double *, const double *", "const float *, const double *", 1))
    assert bad.read_text() != src.read_text()
    assert subprocess.run(cmd[:-3] + ["-o", str(tmp_path / "bad.o"), str(bad)], capture_output=True).returncode != 0


def test_refused_without_a_context(lib):
    """A NULL context is an argument error before anything else is looked at (no device needed), and no output is touched."""
    kp = np.full((4, 6), 7.0, np.float32); de = np.full((4, 32), 0x5a, np.uint8); ints = np.full(4 + 4 + 2 + 1 + 2, -77, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    quad = np.array([[1.0, 1.0], [9.0, 1.0], [9.0, 9.0], [1.0, 9.0]]); bb = np.array([1.0, 1.0, 9.0, 9.0])
    rc = lib.tsorb_fuse_frame(None, 0, 1, quad.ctypes.data_as(C.POINTER(C.c_double)), bb.ctypes.data_as(C.POINTER(C.c_double)), -3.0, 500, 4, 4, 0.0, 320.0, 0.0, 240.0,
                              kp.ctypes.data_as(C.POINTER(C.c_float)), de.ctypes.data_as(C.POINTER(C.c_uint8)), ip(ints[0:4]), ip(ints[4:8]), ip(ints[8:10]), ip(ints[10:11]), ip(ints[11:13]))
    assert rc == -1 and np.all(kp == 7.0) and np.all(de == 0x5a) and np.all(ints == -77)

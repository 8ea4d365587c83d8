"""tsframe_pyramid_pts_batch (include/tsframe.h): tool::GetPyramidPts for all feature sets of a frame in one launch.  Every set's slice is
compared with np.array_equal / tobytes against the CPU oracle (oracle/tsframe_oracle.c) and against the single call tsframe_pyramid_pts: no
tolerance anywhere.  The single call is the batch of one set, so the same sets go through it too.  The shapes are the smallest that reach every path of the kernel: empty and one-feature sets, grids on both sides of the LDS
capacity (and two grids in the device scratch at once), one level, eight levels, levels of a few pixels."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("level_off", "idx", "u", "v", "inten", "in")
INV4 = [1.0, 0.5, 0.25, 0.125]
ERR_ARG, ERR_STATE = -1, -3


def _img(seed, h, w):
    rng = np.random.default_rng(seed)
    base = ndimage.gaussian_filter(rng.normal(0, 1, (h, w)), 3.0)
    return np.clip(128 + 600*base + rng.normal(0, 5, (h, w)), 0, 255).astype(np.uint8)


def _text(rng, n, box, w, h, extras=True):
    """n text keypoints: most inside the box; with extras also on the box's max edges (the m == cw rule), outside the box (level 0 only) and
    within a pixel of the image border (in = 0).  The box's corners are exact in float32, so 'on the edge' is exact."""
    special = []
    if extras:
        special = [(box[2], 0.5*(box[1] + box[3])), (0.5*(box[0] + box[2]), box[3]), (box[2], box[3]), (box[0], box[1]),            # on the edges
                   (box[0] - 9.5, box[1] - 7.25), (box[2] + 6.0, box[3] + 3.0), (-3.0, 10.0), (w + 4.0, h + 2.0),                # outside the box / the image
                   (w - 0.5, 0.5*h), (0.5*w, h - 0.75), (0.0, 0.0), (w - 1.0, h - 1.0), (0.25, h - 0.25)]                        # at the image border
        special = special[:n]
    m = n - len(special)
    xy = np.stack([rng.uniform(box[0], box[2], m), rng.uniform(box[1], box[3], m)], 1)
    xy = np.concatenate([xy, np.asarray(special, np.float64).reshape(-1, 2)]).astype(np.float32)
    return xy[rng.permutation(n)]


def _scene(rng, n, w, h):
    xy = np.stack([rng.uniform(-0.5, w - 0.5, n), rng.uniform(-0.5, h - 0.5, n)], 1).astype(np.float32)
    xy[::17] = np.rint(xy[::17])
    return xy


def _same(got, ref, what=""):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k)


def _bytes(d):
    return b"".join(np.ascontiguousarray(d[k]).tobytes() for k in KEYS)


def _single(fr, s, inv):
    """One set through the single call tsframe_pyramid_pts."""
    m, xy, box = s
    return fr.GetPyramidPts(xy, box[:2], box[2:], inv) if m == 0 else fr.GetPyramidPtsScene(xy, inv)


def _oracle(oracle_lib, sets, pyr, inv):
    return [oracle_lib.frame_pyramid_pts(m, xy, box, pyr, inv) for m, xy, box in sets]


@pytest.fixture(scope="module")
def fr():
    from textslam_amd.frame import Frame
    return Frame(0)


@pytest.fixture(scope="module")
def mixed(oracle_lib):
    """Test 1's frame (131 x 97, 4 levels) and sets, with the oracle's result per set; shared, read-only."""
    w, h = 131, 97
    img = _img(21, h, w)
    pyr = oracle_lib.frame_pyramid(img, 4)
    rng = np.random.default_rng(22)
    box_a, box_b, box_c = (20.25, 12.5, 101.75, 80.0), (40.0, 30.0, 90.5, 55.25), (5.0, 60.0, 125.0, 90.0)
    odd = _text(rng, 32, box_c, w, h, extras=False)
    odd.reshape(-1)[::3] = np.rint(odd.reshape(-1)[::3])                    # every third coordinate integral
    odd = np.concatenate([odd, odd[[3, 9, 9, 20, 31]]])                      # five exact duplicates of earlier points: n = 37
    sets = [(0, _text(rng, 300, box_a, w, h), box_a),
            (1, _scene(rng, 700, w, h), None),
            (0, np.zeros((0, 2), np.float32), box_b),
            (0, _text(rng, 1, box_b, w, h, extras=False), box_b),
            (0, odd, box_c),
            (0, _text(rng, 150, box_a, w, h), box_a)]
    assert [len(s[1]) for s in sets] == [300, 700, 0, 1, 37, 150]
    return {"img": img, "pyr": pyr, "sets": sets, "ref": _oracle(oracle_lib, sets, pyr, INV4)}


def test_bit_equal_to_the_oracle_mixed_sets(fr, mixed):
    fr.GetPyrMat(mixed["img"], 4)
    got = fr.GetPyramidPtsBatch(mixed["sets"], INV4)
    assert len(got) == len(mixed["sets"])
    for i, (g, r) in enumerate(zip(got, mixed["ref"])):
        _same(g, r, i)
        assert g["level_off"][0] == 0 and g["level_off"][1] == len(mixed["sets"][i][1])          # level 0 holds every raw feature
    # not trivial: coarse levels keep proper, non-empty subsets; features outside the image and dropped features exist
    for i in (0, 1, 5):
        n = len(mixed["sets"][i][1]); cnt = np.diff(mixed["ref"][i]["level_off"])
        assert all(0 < c < n for c in cnt[1:]), (i, cnt)
    assert 0 < mixed["ref"][0]["in"].sum() < len(mixed["ref"][0]["in"])


def test_equal_to_the_single_call_byte_for_byte(fr, mixed):
    fr.GetPyrMat(mixed["img"], 4)
    got = fr.GetPyramidPtsBatch(mixed["sets"], INV4)
    for i, (m, xy, box) in enumerate(mixed["sets"]):
        assert _bytes(got[i]) == _bytes(_single(fr, (m, xy, box), INV4)), i


def test_sets_are_independent_and_scratch_is_reused(fr, mixed, oracle_lib):
    fr.GetPyrMat(mixed["img"], 4)
    sets = mixed["sets"]
    fwd = fr.GetPyramidPtsBatch(sets, INV4)
    rev = fr.GetPyramidPtsBatch(sets[::-1], INV4)
    for i in range(len(sets)):
        assert _bytes(rev[len(sets) - 1 - i]) == _bytes(fwd[i]), i
        assert _bytes(fr.GetPyramidPtsBatch([sets[i]], INV4)[0]) == _bytes(fwd[i]), i
    rng = np.random.default_rng(23)
    many = []
    for k in range(40):
        if k % 7 == 3:
            many.append((1, _scene(rng, 90 + 11*k, 131, 97), None))
        else:
            x0, y0 = rng.uniform(0, 60), rng.uniform(0, 50)
            box = (float(np.float32(x0)), float(np.float32(y0)), float(np.float32(x0 + rng.uniform(20, 70))), float(np.float32(y0 + rng.uniform(10, 45))))
            many.append((0, _text(rng, 20 + 3*k, box, 131, 97), box))
    first = fr.GetPyramidPtsBatch(many, INV4)
    two = fr.GetPyramidPtsBatch(sets[:2], INV4)
    again = fr.GetPyramidPtsBatch(many, INV4)
    assert [_bytes(a) for a in again] == [_bytes(a) for a in first]
    assert [_bytes(a) for a in two] == [_bytes(a) for a in fwd[:2]]
    for k in (0, 3, 39):                                                    # and the 40-set call is right, not only repeatable
        _same(first[k], oracle_lib.frame_pyramid_pts(many[k][0], many[k][1], many[k][2], mixed["pyr"], INV4), k)


def _scene_grid(n, s, w, h):
    """The scene grid of a level (the expressions of tsframe_pyramid_pts): ncell, cw, ch."""
    ncell = int(n*s*s + 500)
    wh = w/h
    return ncell, int(math.sqrt(ncell*wh)), int(math.sqrt(ncell/wh))


@pytest.fixture(scope="module")
def big(oracle_lib):
    """A 640 x 480 frame, 4 levels, with six sets whose level-1 grids lie on both sides of the LDS capacity, and the oracle's result per set; shared,
    read-only."""
    from textslam_amd.frame import PTS_LDS_CELLS
    w, h = 640, 480
    img = _img(24, h, w)
    pyr = oracle_lib.frame_pyramid(img, 4)
    # the largest n whose level-1 ncell is <= the capacity and the smallest above it; the kernel decides on cw * ch <= ncell, so also the two n
    # on either side of that, and a larger set whose level-1 grid is a second one in the device scratch
    n_lo = max(n for n in range(4*(PTS_LDS_CELLS - 500) - 8, 4*(PTS_LDS_CELLS - 500) + 8) if _scene_grid(n, 0.5, 320, 240)[0] <= PTS_LDS_CELLS)
    assert _scene_grid(n_lo, 0.5, 320, 240)[0] == PTS_LDS_CELLS and _scene_grid(n_lo + 1, 0.5, 320, 240)[0] == PTS_LDS_CELLS + 1
    n = n_lo
    while _scene_grid(n, 0.5, 320, 240)[1]*_scene_grid(n, 0.5, 320, 240)[2] <= PTS_LDS_CELLS:
        n += 1
    g_in, g_out = _scene_grid(n - 1, 0.5, 320, 240), _scene_grid(n, 0.5, 320, 240)
    assert g_in[1]*g_in[2] <= PTS_LDS_CELLS < g_out[1]*g_out[2]
    rng = np.random.default_rng(25)
    box = (200.0, 150.0, 460.0, 260.0)
    sets = [(1, _scene(rng, n_lo, w, h), None), (1, _scene(rng, n_lo + 1, w, h), None), (0, _text(rng, 60, box, w, h), box),
            (1, _scene(rng, n - 1, w, h), None), (1, _scene(rng, n, w, h), None), (1, _scene(rng, 40000, w, h), None)]
    return {"img": img, "sets": sets, "ref": _oracle(oracle_lib, sets, pyr, INV4)}


def test_both_sides_of_the_lds_capacity(fr, big):
    fr.GetPyrMat(big["img"], 4)
    sets = big["sets"]
    got = fr.GetPyramidPtsBatch(sets, INV4)
    for i, (g, r) in enumerate(zip(got, big["ref"])):
        _same(g, r, i)
        cnt = np.diff(r["level_off"])
        assert all(0 < c < len(sets[i][1]) for c in cnt[1:]), (i, cnt)
    # the single call is the batch of one set: the same choice between LDS and scratch per level, on every one of the six
    for i, s in enumerate(sets):
        _same(_single(fr, s, INV4), big["ref"][i], ("single", i))


def test_nothing_left_over_in_the_scratch(fr, big):
    """A grid in the device scratch is initialised by its own workgroup, not by a memset: a large scene set, a small text set whose block lies where that
    grid lay, a batch of the two and the large set again, on one context."""
    fr.GetPyrMat(big["img"], 4)
    scene, text = big["sets"][5], big["sets"][2]
    assert len(scene[1]) == 40000 and len(text[1]) == 60
    first = _single(fr, scene, INV4)
    small = _single(fr, text, INV4)
    both = fr.GetPyramidPtsBatch([scene, text], INV4)
    last = _single(fr, scene, INV4)
    _same(first, big["ref"][5], "first"); _same(small, big["ref"][2], "text"); _same(last, big["ref"][5], "last")
    _same(both[0], big["ref"][5], "batch scene"); _same(both[1], big["ref"][2], "batch text")
    assert _bytes(first) == _bytes(last)


@pytest.mark.parametrize("shape,levels", [((18, 33), 4), ((18, 33), 1), ((480, 640), 8)])
def test_level_counts_and_small_levels(fr, oracle_lib, shape, levels):
    h, w = shape
    img = _img(26 + levels, h, w)
    fr.GetPyrMat(img, levels)
    pyr = oracle_lib.frame_pyramid(img, levels)
    inv = [2.0**-l for l in range(levels)]
    rng = np.random.default_rng(27)
    box = (float(np.float32(0.25*w)), float(np.float32(0.2*h)), float(np.float32(0.8*w)), float(np.float32(0.75*h)))
    sets = [(0, _text(rng, 120, box, w, h), box), (1, _scene(rng, 400, w, h), None), (0, _text(rng, 9, box, w, h, extras=False), box)]
    one = _text(rng, 1, box, w, h, extras=False)
    extra = [(0, np.zeros((0, 2), np.float32), box), (1, np.zeros((0, 2), np.float32), None), (0, one, box), (1, one, None)]
    ref = _oracle(oracle_lib, sets + extra, pyr, inv)
    got = fr.GetPyramidPtsBatch(sets, inv)
    for i, (g, r) in enumerate(zip(got, ref)):
        _same(g, r, i)
        assert len(g["level_off"]) == levels + 1
        if levels == 1:
            assert list(g["level_off"]) == [0, len(sets[i][1])]
    if levels > 1:
        assert 0 < np.diff(got[1]["level_off"])[-1] < 400
    # the same sets, and sets of no and of one feature in both modes, through the single call
    for i, (s, r) in enumerate(zip(sets + extra, ref)):
        g = _single(fr, s, inv)
        _same(g, r, ("single", i))
        n = len(s[1])
        assert len(g["level_off"]) == levels + 1 and g["level_off"][0] == 0 and g["level_off"][1] == n
        if levels == 1:
            assert list(g["level_off"]) == [0, n]
        if n == 0:
            assert not g["level_off"].any()


class _Raw:
    """One raw ctypes call with sentinel-filled outputs."""

    def __init__(self, fr, sets, inv, n_levels):
        self.fr = fr
        self.ns = len(sets)
        self.mode = np.array([s[0] for s in sets], np.int32)
        xys = [np.ascontiguousarray(s[1], np.float32).reshape(-1, 2) for s in sets]
        self.off = np.zeros(self.ns + 1, np.int32); self.off[1:] = np.cumsum([len(a) for a in xys])
        self.xy = np.concatenate(xys + [np.zeros((1, 2), np.float32)])
        self.box = np.array([s[2] if s[2] is not None else (np.nan,)*4 for s in sets], np.float64).reshape(-1, 4)      # a scene set's box is never read
        self.inv = np.array(inv, np.float64)
        cap = max(1, int(self.off[-1])*n_levels)
        self.lo = np.full((self.ns, n_levels + 1), -77, np.int32)
        self.u = np.full(cap, -7.5); self.v = np.full(cap, -7.5); self.I = np.full(cap, -7.5)
        self.idx = np.full(cap, -77, np.int32); self.inn = np.full(cap, 99, np.uint8)

    def call(self, ctx=None, n_set=None, null=()):
        ip, dp, fp, up = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        a = {"mode": self.mode.ctypes.data_as(ip), "xy_off": self.off.ctypes.data_as(ip), "xy": self.xy.ctypes.data_as(fp), "box": self.box.ctypes.data_as(dp),
             "inv": self.inv.ctypes.data_as(dp), "level_off": self.lo.ctypes.data_as(ip), "u": self.u.ctypes.data_as(dp), "v": self.v.ctypes.data_as(dp),
             "idx": self.idx.ctypes.data_as(ip), "inten": self.I.ctypes.data_as(dp), "in": self.inn.ctypes.data_as(up)}
        for k in null:
            a[k] = None
        ctx = self.fr.ctx if ctx is None else ctx
        rc = self.fr.lib.tsframe_pyramid_pts_batch(ctx, self.ns if n_set is None else n_set, a["mode"], a["xy_off"], a["xy"], a["box"], a["inv"], a["level_off"],
                                                   a["u"], a["v"], a["idx"], a["inten"], a["in"])
        return rc, self.fr.lib.tsframe_last_error(ctx).decode()

    def untouched(self):
        return (np.all(self.lo == -77) and np.all(self.u == -7.5) and np.all(self.v == -7.5) and np.all(self.I == -7.5) and np.all(self.idx == -77)
                and np.all(self.inn == 99))


def test_arguments(fr, mixed):
    from textslam_amd.frame import Frame
    fr.GetPyrMat(mixed["img"], 4)
    sets = mixed["sets"]

    def refused(raw, code=ERR_ARG, names=None, **kw):
        rc, msg = raw.call(**kw)
        assert rc == code, (rc, msg, kw)
        assert "tsframe_pyramid_pts_batch" in msg, msg
        if names is not None:
            assert names in msg, msg
        assert raw.untouched(), kw

    # NULL pointers where data is needed
    for name in ("mode", "xy_off", "inv", "level_off", "xy", "box", "u", "v", "idx", "inten", "in"):
        refused(_Raw(fr, sets, INV4, 4), null=(name,))
    refused(_Raw(fr, sets, INV4, 4), n_set=-1)
    # a mode other than 0 or 1
    raw = _Raw(fr, sets, INV4, 4); raw.mode[4] = 2
    refused(raw, names="set 4")
    raw = _Raw(fr, sets, INV4, 4); raw.mode[0] = -1
    refused(raw, names="set 0")
    # xy_off
    raw = _Raw(fr, sets, INV4, 4); raw.off[0] = 1
    refused(raw)
    raw = _Raw(fr, sets, INV4, 4); raw.off[2] = raw.off[1] - 1
    refused(raw)
    # a total above INT32_MAX / n_levels (refused before any feature is read)
    raw = _Raw(fr, sets[:1], INV4, 4); raw.off[1] = (2**31 - 1)//4 + 1
    refused(raw)
    # a degenerate grid: an empty box in set 2 of 4
    four = [sets[0], sets[3], (0, sets[4][1], (50.0, 40.0, 50.0, 70.0)), sets[5]]
    refused(_Raw(fr, four, INV4, 4), names="set 2")
    four[2] = (0, sets[4][1], (50.0, 40.0, 90.0, 40.0))
    refused(_Raw(fr, four, INV4, 4), names="set 2")
    # coordinates that are not finite, or above 2^20 in magnitude: xy, a mode-0 box, inv_scale
    for bad in (np.nan, np.inf, -np.inf, 2.0**20 + 1, -(2.0**21)):
        raw = _Raw(fr, sets, INV4, 4); raw.xy[1000, 1] = bad                 # (the feature of set 3)
        refused(raw, names="set 3")
        raw = _Raw(fr, sets, INV4, 4); raw.box[4, 2] = bad
        refused(raw, names="set 4")
        raw = _Raw(fr, sets, INV4, 4); raw.inv[2] = bad
        refused(raw)
    # no image: TSFRAME_ERR_STATE
    fresh = Frame(0)
    refused(_Raw(fr, sets, INV4, 4), code=ERR_STATE, ctx=fresh.ctx)
    # n_set == 0 with every pointer NULL
    assert fr.lib.tsframe_pyramid_pts_batch(fr.ctx, 0, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert fr.lib.tsframe_pyramid_pts_batch(fresh.ctx, 0, None, None, None, None, None, None, None, None, None, None, None) == 0
    # sets without a feature: nothing to launch, the level_off rows are zeros; the data pointers are not needed
    raw = _Raw(fr, [sets[2], (1, np.zeros((0, 2), np.float32), None)], INV4, 4)
    rc, msg = raw.call(null=("xy", "u", "v", "idx", "inten", "in"))
    assert rc == 0 and np.all(raw.lo == 0), (rc, msg)
    # a 2^20 coordinate itself is inside the bound, and a scene set's box is not read (NaN here)
    raw = _Raw(fr, sets, INV4, 4); raw.xy[5, 0] = 2.0**20; raw.xy[400, 1] = -(2.0**20)
    rc, msg = raw.call()
    assert rc == 0, msg
    # after all that the context still answers test 1's call
    got = fr.GetPyramidPtsBatch(sets, INV4)
    for i, (g, r) in enumerate(zip(got, mixed["ref"])):
        _same(g, r, i)


def test_adapter_from_cxx(tmp_path, fr, mixed):
    exe = str(tmp_path / "pyramid_pts_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "pyramid_pts_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsframe", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    img = mixed["img"]
    text = [s for s in mixed["sets"] if s[0] == 0]
    scene = mixed["sets"][1][1]
    K = (212.125, 209.75, 64.5, 47.25)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<iiii", img.shape[1], img.shape[0], 4, len(text)))
        f.write(struct.pack("<4d", *K)); f.write(np.asarray(INV4, np.float64).tobytes()); f.write(img.tobytes())
        for _, xy, box in text:
            f.write(struct.pack("<i4d", len(xy), *box)); f.write(np.ascontiguousarray(xy, np.float32).tobytes())
        f.write(struct.pack("<i", len(scene))); f.write(scene.astype(np.float64).tobytes())
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "pyramid pts from C++: ok" in res.stdout, res.stdout
    fr.GetPyrMat(img, 4)
    got = fr.GetPyramidPtsBatch(text + [(1, scene, None)], INV4)             # the Python mirror
    raw = open(outp, "rb").read()
    at = 0
    tf = np.dtype([("d", "<f8", 8), ("q", "<i4", 2), ("b", "u1", 2)])
    sf = np.dtype([("d", "<f8", 4), ("q", "<i4", 2)])
    for i, (_, xy, box) in enumerate(text):
        g = got[i]
        ray = np.stack([(xy[:, 0].astype(np.float64) - K[2])/K[0], (xy[:, 1].astype(np.float64) - K[3])/K[1], np.ones(len(xy))], 1)     # tool.cc:656, in double
        for l in range(4):
            (m,) = struct.unpack_from("<i", raw, at); at += 4
            a, b = int(g["level_off"][l]), int(g["level_off"][l + 1])
            assert m == b - a, (i, l)
            rec = np.frombuffer(raw, tf, m, at); at += tf.itemsize*m
            assert np.array_equal(rec["d"][:, 0], g["u"][a:b]) and np.array_equal(rec["d"][:, 1], g["v"][a:b]), (i, l)
            assert np.array_equal(rec["d"][:, 2], g["u"][a:b]) and np.array_equal(rec["d"][:, 3], g["v"][a:b]), (i, l)          # feature = (u, v)
            assert np.array_equal(rec["d"][:, 4], g["inten"][a:b]), (i, l)
            assert rec["d"][:, 5:8].tobytes() == np.ascontiguousarray(ray[g["idx"][a:b]]).tobytes(), (i, l)                       # the raw feature's ray, to the bit
            assert np.all(rec["q"][:, 0] == l) and np.array_equal(rec["q"][:, 1], g["idx"][a:b]), (i, l)
            assert np.all(rec["b"][:, 0] == 0) and np.array_equal(rec["b"][:, 1], g["in"][a:b]), (i, l)                           # INITIAL = false, IN
    g = got[len(text)]
    for l in range(4):
        (m,) = struct.unpack_from("<i", raw, at); at += 4
        a, b = int(g["level_off"][l]), int(g["level_off"][l + 1])
        assert m == b - a, l
        rec = np.frombuffer(raw, sf, m, at); at += sf.itemsize*m
        assert np.array_equal(rec["d"][:, 0], g["u"][a:b]) and np.array_equal(rec["d"][:, 1], g["v"][a:b])
        assert np.array_equal(rec["d"][:, 2], g["u"][a:b]) and np.array_equal(rec["d"][:, 3], g["v"][a:b])
        assert np.all(rec["q"][:, 0] == l) and np.array_equal(rec["q"][:, 1], g["idx"][a:b])
    assert at == len(raw)

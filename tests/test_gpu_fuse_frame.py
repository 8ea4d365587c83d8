"""tsorb_fuse_frame on the device: every output array bit-equal to the CPU restatement (tests/fuse_frame_ref.py over ex.download() and cvorb_ref.Frame.extract) on the
shared fixtures, the searched set it leaves byte for byte the one tsorb_match_set_features builds from the returned arrays, n_dete == 0, the resident batch and the
text extraction untouched, edge quads, the two capacities, every argument error, and the adapter from C++."""
import ctypes as C
import os
import struct
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvorb_ref as R                                                 # noqa: E402
import fuse_frame_ref as FR                                           # noqa: E402

pytestmark = pytest.mark.gpu
B320 = (0.0, 320.0, 0.0, 240.0)
KEYS = ("kp", "desc", "obj", "src", "text_off", "raw_count")


@pytest.fixture(scope="module")
def ex320():
    """The 320 x 240 fixture image resident as frame 0 (the scene extraction's upload)."""
    from textslam_amd.orbextractor import ORBextractor
    ex = ORBextractor()
    ex.extract_batch(R.fixture_image())
    return ex


def _bytes(a):
    return np.ascontiguousarray(a).tobytes()


def _same(got, ref, what):
    assert got["n_scene"] == ref["n_scene"], what
    for k in KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        print("%s %s: shape %s (restatement %s)" % (what, k, g.shape, r.shape))
        assert g.dtype == r.dtype and g.shape == r.shape, (what, k, g.dtype, r.dtype, g.shape, r.shape)
        assert _bytes(g) == _bytes(r), (what, k)                       # floats as bit patterns


def _ref(ex, raw, quads, bbox=None, win=-3.0):
    skp, sde = ex.download()[0]
    return FR.fuse_frame(skp, sde, raw, quads, FR.bbox_of(quads) if bbox is None else bbox, win)


TABLE = {("320", 500): ([477, 477, 407, 0], [335, 353, 355, 0]), ("320", 60): ([60, 60, 57, 0], [27, 24, 24, 0])}


@pytest.mark.parametrize("nfeatures", [500, 60])
def test_bit_equal_to_the_restatement_320(ex320, nfeatures):
    img, raw, _ = R.reference("320", nfeatures)
    ref = _ref(ex320, raw, R.QUADS_320)
    kept = np.diff(ref["text_off"]).tolist()
    print("raw", ref["raw_count"].tolist(), "kept", kept, "scene", ref["n_scene"])
    assert (ref["raw_count"].tolist(), kept) == TABLE[("320", nfeatures)]          # not vacuous: three detections cut, at 500 across the 256-row chunk, one empty
    got = ex320.fuse_frame(0, R.QUADS_320, FR.bbox_of(R.QUADS_320), B320, nfeatures=nfeatures)
    _same(got, ref, "320 x 240, nfeatures %d," % nfeatures)
    assert ref["n_scene"] > 0 and (got["obj"][:got["n_scene"]] == -1).all()


def test_bit_equal_to_the_restatement_200():
    from textslam_amd.orbextractor import ORBextractor
    img, raw, _ = R.reference("200", 500)
    ex = ORBextractor(nlevels=4)
    try:
        ex.extract_batch(img)
        ref = _ref(ex, raw, R.QUADS_200)
        assert int(ref["raw_count"][1]) == 230 and int(np.diff(ref["text_off"])[1]) == 164
        got = ex.fuse_frame(0, R.QUADS_200, FR.bbox_of(R.QUADS_200), (0.0, 200.0, 0.0, 150.0))
        _same(got, ref, "200 x 150,")
    finally:
        ex.close()


def _queries(fused, seed=5, nq=40):
    """nq seeded queries near features of the fused set, half of them near text rows."""
    rng = np.random.default_rng(seed)
    n, ns = len(fused["kp"]), fused["n_scene"]
    q = np.concatenate([rng.choice(ns, nq // 2, replace=False), ns + rng.choice(n - ns, nq - nq // 2, replace=False)])
    qxy = fused["kp"][q, :2] + rng.uniform(-3, 3, (nq, 2)).astype(np.float32)
    return qxy, np.full(nq, 12.0, np.float32), None, fused["desc"][q]


def test_the_searched_set(ex320):
    ex320.match_set_frame(0, B320)                                     # (another set first)
    got = ex320.fuse_frame(0, R.QUADS_320, FR.bbox_of(R.QUADS_320), B320)
    args = _queries(got)
    m_a = ex320.match_search(*args, max_cand=64); c_a = ex320.match_search_claim(*args)
    ex320.match_set_features(got["kp"], got["desc"], B320)
    m_b = ex320.match_search(*args, max_cand=64); c_b = ex320.match_search_claim(*args)
    for k in m_a:
        assert _bytes(m_a[k]) == _bytes(m_b[k]), k
    assert _bytes(c_a["match12"]) == _bytes(c_b["match12"]) and _bytes(c_a["match_dist"]) == _bytes(c_b["match_dist"]) and c_a["n_match"] == c_b["n_match"]
    assert (m_a["best_idx"] >= got["n_scene"]).any() and (c_a["match12"] >= got["n_scene"]).any()      # a best match is a text row
    assert m_a["cand_cnt"].max() > 1


def test_no_detection_is_the_scene_set(ex320):
    skp, sde = ex320.download()[0]
    got = ex320.fuse_frame(0, np.zeros((0, 4, 2)), np.zeros((0, 4)), B320)
    assert got["n_scene"] == len(skp) and _bytes(got["kp"]) == _bytes(skp) and _bytes(got["desc"]) == _bytes(sde)
    assert (got["obj"] == -1).all() and np.array_equal(got["src"], np.arange(len(skp))) and got["text_off"].tolist() == [len(skp)] and got["raw_count"].shape == (0,)
    rng = np.random.default_rng(2)
    q = rng.choice(len(skp), 40, replace=False)
    args = (skp[q, :2] + rng.uniform(-3, 3, (40, 2)).astype(np.float32), np.full(40, 12.0, np.float32), None, sde[q])
    m_a = ex320.match_search(*args)
    ex320.match_set_frame(0, B320)
    m_b = ex320.match_search(*args)
    assert all(_bytes(m_a[k]) == _bytes(m_b[k]) for k in m_a)
    # no pointer of the detection arrays is read: NULL quads, bbox and raw_count
    kp = np.zeros((ex320.cap, 6), np.float32); de = np.zeros((ex320.cap, 32), np.uint8); obj = np.zeros(ex320.cap, np.int32); off = np.zeros(1, np.int32); n2 = np.zeros(2, np.int32)
    rc = ex320.lib.tsorb_fuse_frame(ex320.ctx, 0, 0, None, None, -3.0, 500, 564, ex320.cap, *B320, kp.ctypes.data_as(C.POINTER(C.c_float)), de.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    obj.ctypes.data_as(C.POINTER(C.c_int32)), None, off.ctypes.data_as(C.POINTER(C.c_int32)), None, n2.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0 and n2.tolist() == [len(skp)] * 2 and _bytes(kp[:len(skp)]) == _bytes(skp)


def test_state(ex320):
    before = ex320.download()[0]
    text0 = ex320.extract_text(0, R.QUADS_320, 500)
    lev0 = [ex320.debug_level(0, l).copy() for l in range(8)]
    bb = FR.bbox_of(R.QUADS_320)
    fwd = ex320.fuse_frame(0, R.QUADS_320, bb, B320)
    after = ex320.download()[0]
    assert _bytes(before[0]) == _bytes(after[0]) and _bytes(before[1]) == _bytes(after[1])
    assert all(np.array_equal(a, ex320.debug_level(0, l)) for l, a in enumerate(lev0))
    text1 = ex320.extract_text(0, R.QUADS_320, 500)
    assert all(_bytes(a[0]) == _bytes(b[0]) and _bytes(a[1]) == _bytes(b[1]) for a, b in zip(text0, text1))
    # the order of the detections: the quads reversed reverse the slices
    rev = ex320.fuse_frame(0, R.QUADS_320[::-1], bb[::-1], B320)
    assert rev["n_scene"] == fwd["n_scene"] and rev["raw_count"].tolist() == fwd["raw_count"].tolist()[::-1]
    for d in range(4):
        a = slice(fwd["text_off"][d], fwd["text_off"][d + 1]); b = slice(rev["text_off"][3 - d], rev["text_off"][4 - d])
        assert a.stop - a.start == b.stop - b.start
        assert _bytes(fwd["kp"][a]) == _bytes(rev["kp"][b]) and _bytes(fwd["desc"][a]) == _bytes(rev["desc"][b]) and _bytes(fwd["src"][a]) == _bytes(rev["src"][b]), d
        assert (fwd["obj"][a] == d).all() and (rev["obj"][b] == 3 - d).all()
    # 20 detections, then 4 again: the scratch grows and is reused
    few = ex320.fuse_frame(0, R.QUADS_320, bb, B320, nfeatures=60)
    many = ex320.fuse_frame(0, np.concatenate([R.QUADS_320] * 5), np.concatenate([bb] * 5), B320, nfeatures=60)
    again = ex320.fuse_frame(0, R.QUADS_320, bb, B320, nfeatures=60)
    assert all(_bytes(few[k]) == _bytes(again[k]) for k in KEYS)
    assert many["raw_count"].tolist() == few["raw_count"].tolist() * 5 and np.array_equal(np.diff(many["text_off"]), np.tile(np.diff(few["text_off"]), 5))
    for d in range(20):
        a = slice(many["text_off"][d], many["text_off"][d + 1]); b = slice(few["text_off"][d % 4], few["text_off"][d % 4 + 1])
        assert _bytes(many["kp"][a]) == _bytes(few["kp"][b]) and _bytes(many["desc"][a]) == _bytes(few["desc"][b]) and (many["obj"][a] == d).all(), d


def test_edge_quads(ex320):
    narrow = [[100.0, 60.0], [105.0, 60.0], [105.0, 180.0], [100.0, 180.0]]       # 5 px wide: narrower than 2 |win|, the shrunk polygon is inverted
    off = [[-90, -50], [-20, -50], [-20, -8], [-90, -8]]
    quads = np.array([narrow, off, R.FULL_320], np.float64)
    raw = R.Frame(R.fixture_image()).extract(quads, 500)
    ref = _ref(ex320, raw, quads)
    got = ex320.fuse_frame(0, quads, FR.bbox_of(quads), B320)
    print("edge quads: raw", ref["raw_count"].tolist(), "kept", np.diff(ref["text_off"]).tolist())
    _same(got, ref, "edge quads,")
    assert ref["raw_count"][1] == 0 and ref["raw_count"][2] >= 400 and np.diff(ref["text_off"])[2] > 0
    # a bounding box smaller than the quad cuts too (the second test of tool.cc:484), and another win
    bb = FR.bbox_of(R.QUADS_320); bb[0] = [100.0, 80.0, 200.0, 150.0]
    img, raw4, _ = R.reference("320", 500)
    ref = _ref(ex320, raw4, R.QUADS_320, bb, -7.5)
    got = ex320.fuse_frame(0, R.QUADS_320, bb, B320, win=-7.5)
    _same(got, ref, "own bounding box, win -7.5,")
    assert 0 < np.diff(ref["text_off"])[0] < TABLE[("320", 500)][1][0]


def _raw(ex, frame=0, n=None, quads=R.QUADS_320, bbox="auto", win=-3.0, nfeatures=500, cap_text=564, cap=3000, bounds=B320, ctx=True, null=()):
    quads = None if quads is None else np.ascontiguousarray(quads, np.float64)
    if isinstance(bbox, str):
        bbox = None if quads is None else FR.bbox_of(quads)
    bbox = None if bbox is None else np.ascontiguousarray(bbox, np.float64)
    n = (0 if quads is None else len(quads.reshape(-1, 4, 2))) if n is None else n
    rows, nd = max(cap, 1), max(n, 1)
    o = dict(kp=np.full((rows, 6), 7.0, np.float32), desc=np.full((rows, 32), 0x5a, np.uint8), obj=np.full(rows, -77, np.int32), src=np.full(rows, -77, np.int32),
             text_off=np.full(nd + 1, -77, np.int32), raw_count=np.full(nd, -77, np.int32), n_out=np.full(2, -77, np.int32))
    p = lambda k, t: None if k in null else o[k].ctypes.data_as(C.POINTER(t))
    rc = ex.lib.tsorb_fuse_frame(ex.ctx if ctx else None, frame, n, None if quads is None else quads.ctypes.data_as(C.POINTER(C.c_double)),
                                 None if bbox is None else bbox.ctypes.data_as(C.POINTER(C.c_double)), win, nfeatures, cap_text, cap, *bounds,
                                 p("kp", C.c_float), p("desc", C.c_uint8), p("obj", C.c_int32), p("src", C.c_int32), p("text_off", C.c_int32), p("raw_count", C.c_int32), p("n_out", C.c_int32))
    return rc, o


def _untouched(o, but=()):
    fill = dict(kp=7.0, desc=0x5a)
    return all(bool(np.all(a == fill.get(k, -77))) for k, a in o.items() if k not in but)


def test_capacities(ex320):
    img, raw, _ = R.reference("320", 500)
    ref = _ref(ex320, raw, R.QUADS_320)
    counts, n, ns = ref["raw_count"].tolist(), len(ref["kp"]), ref["n_scene"]
    prev = ex320.fuse_frame(0, R.QUADS_320[:1], FR.bbox_of(R.QUADS_320[:1]), B320, nfeatures=60)       # the previous set
    args = _queries(prev, seed=9)
    m0 = ex320.match_search(*args)
    # cap_text one too small: detections 0 and 1 do not fit
    rc, o = _raw(ex320, cap_text=max(counts) - 1)
    assert rc == -1 and "cap_text" in ex320.lib.tsorb_last_error(ex320.ctx).decode()
    assert o["raw_count"].tolist() == counts and int(o["n_out"][0]) == ns             # the counts are complete
    fit = [k for d, k in enumerate(np.diff(ref["text_off"]).tolist()) if counts[d] <= max(counts) - 1]
    assert int(o["n_out"][1]) == ns + sum(fit)                                          # (a detection that does not fit has no rows to test: n counts the others)
    assert _untouched(o, ("raw_count", "n_out"))
    m1 = ex320.match_search(*args)
    assert all(_bytes(m0[k]) == _bytes(m1[k]) for k in m0)                              # still the previous set
    # cap one too small
    rc, o = _raw(ex320, cap=n - 1)
    assert rc == -1 and "cap" in ex320.lib.tsorb_last_error(ex320.ctx).decode()
    assert o["raw_count"].tolist() == counts and o["n_out"].tolist() == [ns, n] and _untouched(o, ("raw_count", "n_out"))
    m1 = ex320.match_search(*args)
    assert all(_bytes(m0[k]) == _bytes(m1[k]) for k in m0)
    # each exactly large enough
    rc, o = _raw(ex320, cap_text=max(counts), cap=n)
    assert rc == 0 and o["n_out"].tolist() == [ns, n] and o["raw_count"].tolist() == counts
    assert _bytes(o["kp"]) == _bytes(ref["kp"]) and _bytes(o["desc"]) == _bytes(ref["desc"]) and _bytes(o["obj"]) == _bytes(ref["obj"]) and _bytes(o["src"]) == _bytes(ref["src"])
    assert _bytes(o["text_off"]) == _bytes(ref["text_off"])
    m2 = ex320.match_search(*args)
    assert any(_bytes(m0[k]) != _bytes(m2[k]) for k in m0)                              # and now the new one


def test_arguments(ex320):
    from textslam_amd.orbextractor import ORBextractor, TsorbError
    prev = ex320.fuse_frame(0, R.QUADS_320[:1], FR.bbox_of(R.QUADS_320[:1]), B320, nfeatures=60)
    args = _queries(prev, seed=4)
    m0 = ex320.match_search(*args)
    rc, o = _raw(ex320); assert rc == 0 and not _untouched(o)
    rc, o = _raw(ex320, null=("src", "raw_count")); assert rc == 0 and int(o["n_out"][1]) > int(o["n_out"][0]) > 0      # the two optional outputs
    ex320.fuse_frame(0, R.QUADS_320[:1], FR.bbox_of(R.QUADS_320[:1]), B320, nfeatures=60)
    qn = R.QUADS_320.copy(); qn[1, 2, 0] = np.nan
    qi = R.QUADS_320.copy(); qi[0, 0, 1] = -np.inf
    qb = R.QUADS_320.copy(); qb[2, 3, 0] = 2.0 ** 30 + 1024
    bn = FR.bbox_of(R.QUADS_320); bn[3, 1] = np.nan
    bb = FR.bbox_of(R.QUADS_320); bb[0, 2] = -2.0 ** 31
    cases = [("ctx NULL", dict(ctx=False)), ("quad NULL", dict(quads=None, n=2)), ("bbox NULL", dict(bbox=None)), ("kp NULL", dict(null=("kp",))), ("desc NULL", dict(null=("desc",))),
             ("obj NULL", dict(null=("obj",))), ("text_off NULL", dict(null=("text_off",))), ("n_out NULL", dict(null=("n_out",))),
             ("frame -1", dict(frame=-1)), ("frame 1 of a batch of 1", dict(frame=1)), ("n_dete < 0", dict(n=-1)), ("nfeatures 0", dict(nfeatures=0)), ("cap_text 0", dict(cap_text=0)),
             ("cap 0", dict(cap=0)), ("NaN corner", dict(quads=qn, bbox=FR.bbox_of(R.QUADS_320))), ("infinite corner", dict(quads=qi, bbox=FR.bbox_of(R.QUADS_320))),
             ("corner beyond 2^30", dict(quads=qb, bbox=FR.bbox_of(R.QUADS_320))), ("NaN bbox", dict(bbox=bn)), ("bbox beyond 2^30", dict(bbox=bb)),
             ("win NaN", dict(win=float("nan"))), ("win infinite", dict(win=float("inf"))), ("win beyond 2^30", dict(win=-2.0 ** 31)),
             ("max_x == min_x", dict(bounds=(5.0, 5.0, 0.0, 240.0))), ("max_y < min_y", dict(bounds=(0.0, 320.0, 240.0, 0.0))), ("bounds NaN", dict(bounds=(0.0, float("nan"), 0.0, 240.0)))]
    for name, kw in cases:
        rc, o = _raw(ex320, **kw)
        assert rc == -1 and _untouched(o), name
        if kw.get("ctx", True):
            assert "tsorb_fuse_frame" in ex320.lib.tsorb_last_error(ex320.ctx).decode(), name
    m1 = ex320.match_search(*args)
    assert all(_bytes(m0[k]) == _bytes(m1[k]) for k in m0)             # nothing was launched: the searched set is what it was
    fresh = ORBextractor()                                             # no batch resident
    rc, o = _raw(fresh); assert rc == -1 and _untouched(o)
    fresh.upload(R.fixture_image())                                    # uploaded but not run
    rc, o = _raw(fresh); assert rc == -1 and _untouched(o)
    with pytest.raises(TsorbError):
        fresh.fuse_frame(0, R.QUADS_320, FR.bbox_of(R.QUADS_320), B320)
    fresh.close()
    big = ORBextractor(); big.extract_batch(np.pad(R.fixture_image(), ((0, 240), (0, 328)), mode="reflect"))     # 648 x 480: level 0 larger than 640 x 480
    rc, o = _raw(big); assert rc == -1 and _untouched(o) and "640" in big.lib.tsorb_last_error(big.ctx).decode()
    big.close()


def test_adapter_from_cxx(tmp_path, ex320):
    exe = str(tmp_path / "fuse_frame_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-I" + os.path.join(ROOT, "textslam_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "fuse_frame_from_cxx.cpp"), "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    img = R.fixture_image()
    bb = FR.bbox_of(R.QUADS_320)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<iiii", img.shape[1], img.shape[0], 8, len(R.QUADS_320)))
        f.write(img.tobytes()); f.write(np.ascontiguousarray(R.QUADS_320, np.float64).tobytes()); f.write(np.ascontiguousarray(bb, np.float64).tobytes())
        f.write(np.array(B320, np.float64).tobytes())
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "fuse frame from C++: ok" in res.stdout, res.stdout
    got = ex320.fuse_frame(0, R.QUADS_320, bb, B320)                   # the Python mirror
    lists = FR.read_lists(open(outp, "rb").read())
    FR.assert_lists_equal(lists, FR.lists_of(got, len(R.QUADS_320)))

"""libtsframe's feature calls share one device block and one pinned block on their context (the image uploads use the pinned block too), libtsorb's
window search and text extraction keep blocks of their own, and all of them only grow (textslam_amd/csrc/tsstage.h).  Different calls in turn on ONE
context, so that a later call lays its sub-arrays into blocks an earlier one sized and that still hold the earlier call's bytes:

  libtsframe, a 96 x 80 image with 3 levels:
    1. tsframe_neighbours, n = 1: the blocks are at their smallest;
    2. tsframe_text_object_info, 3 objects (one whose quad lies wholly outside the image: no pixel; one without features), pix_cap == 0 (count only:
       the short download), then with pixels;
    3. tsframe_box_pixels with cap == 0, cap == the count, cap == the count - 1 (refused: n_out holds the count, the arrays are untouched);
    4. tsframe_klt_track against a second context, n = 5, win = 5;
    5. tsframe_pyramid_pts_batch, 2 sets, one of them empty, the grids small enough for LDS;
    6. tsframe_text_judge, n = 2, with dete_bits and without;
    7. tsframe_set_image of a 200 x 160 image, then step 1: blocks far larger than the call needs, holding earlier bytes;
    8. tsframe_set_camera + tsframe_set_raw_image with undist_out (the pinned block carries the raw frame in and the colour plane out), then step 4.
  libtsorb:
    1. tsorb_match_set_features, n = 40;
    2. tsorb_match_search, nq = 3, qlev NULL, cand_idx and best_dist2 omitted;
    3. tsorb_match_search, nq = 33, max_cand = 4, everything given;
    4. step 2 again;
    5. tsorb_text_extract on a resident 160 x 120 frame with 1, 3, 1 detections and an odd cap, so that nd * cap is odd (kp's 24 * nd * cap bytes are then
       no multiple of 16, the one place where a 16-byte layout and a packed one put desc at different offsets).

Every output of every step equals, bit for bit, the same call on a fresh context of its own; an output the caller omitted keeps its fill value, and so does
every byte of an output array beyond what the call reports written.  The calls go through the C ABI with raw arrays, every output pre-filled."""
import ctypes as C
import faulthandler
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64, I32, U8, I16, U32 = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int32, C.c_uint8, C.c_int16, C.c_uint32))
_CT = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32, np.dtype(np.uint8): U8, np.dtype(np.int16): I16, np.dtype(np.uint32): U32}
FILL = 77
W, H, LEVELS = 96, 80, 3
INV_SCALE = np.array([1.0, 0.5, 0.25])
K0 = np.array([90.0, 90.0, 48.0, 40.0])


@pytest.fixture(autouse=True)
def time_limit():
    """A call that does not return ends the process with a traceback instead of holding the device."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _p(a):
    return None if a is None else a.ctypes.data_as(_CT[a.dtype])


def _outs(shapes):
    """Output arrays with every BYTE set to FILL."""
    return {k: np.full(np.prod(s, dtype=int)*np.dtype(t).itemsize, FILL, np.uint8).view(t).reshape(s) for k, (s, t) in shapes.items()}


def _filled(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def _same(got, ref, step):
    assert got.keys() == ref.keys(), step
    for k in ref:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (step, k)


def image(w, h, seed, channels=None):
    """Random 8 x 8 blocks with a little noise: corners for KLT and ORB, a spread of intensities for the statistics."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels is None else (h, w, channels)
    blocks = rng.integers(30, 226, ((h + 7)//8, (w + 7)//8) + shape[2:])
    img = np.kron(blocks, np.ones((8, 8) + (1,)*(len(shape) - 2), np.int64))[:h, :w]
    return np.ascontiguousarray(np.clip(img + rng.integers(-12, 13, shape), 0, 255), np.uint8)


# ---------------------------------------------------------------------------------------------------------------- libtsframe
def _ok(fr, rc):
    assert rc == 0, fr.lib.tsframe_last_error(fr.ctx).decode()


def set_small(fr):
    _ok(fr, fr.lib.tsframe_set_image(fr.ctx, _p(image(W, H, 1)), W, H, LEVELS))
    return _levels(fr)


def set_big(fr):
    _ok(fr, fr.lib.tsframe_set_image(fr.ctx, _p(image(200, 160, 2)), 200, 160, LEVELS))
    return _levels(fr)


def set_raw(fr):
    raw = image(W, H, 3, channels=3)
    _ok(fr, fr.lib.tsframe_set_camera(fr.ctx, W, H, _p(K0), _p(np.array([-0.2, 0.05, 0.001, -0.001, 0.0])), None))
    o = _outs(dict(undist=((H, W, 3), np.uint8)))
    _ok(fr, fr.lib.tsframe_set_raw_image(fr.ctx, _p(raw), 3*W, 0, LEVELS, _p(o["undist"])))
    o.update(_levels(fr))
    return o


def _levels(fr):
    """The resident level images: what the upload through the pinned block left on the device."""
    o = {}
    for l in range(LEVELS):
        w, h = C.c_int(0), C.c_int(0)
        _ok(fr, fr.lib.tsframe_level_size(fr.ctx, l, C.byref(w), C.byref(h)))
        o["level%d" % l] = np.full((h.value, w.value), FILL, np.uint8)
        _ok(fr, fr.lib.tsframe_get_level(fr.ctx, l, 0, _p(o["level%d" % l])))
    return o


def neighbours(fr):
    uv = np.array([[20.25, 30.5]])
    o = _outs(dict(inten8=(8, np.float64), ninten8=(8, np.float64), inn=(1, np.uint8)))
    _ok(fr, fr.lib.tsframe_neighbours(fr.ctx, 0, _p(uv), 1, 100.0, 20.0, _p(o["inten8"]), _p(o["ninten8"]), _p(o["inn"])))
    return o


OBJ_QUADS = np.array([[(10.5, 12.2), (60.3, 14.8), (58.1, 40.4), (12.7, 38.9)],            # 0: inside, 5 features over the 3 levels
                      [(300.5, 200.0), (360.0, 200.0), (360.0, 240.5), (300.5, 240.5)],    # 1: wholly outside the image: no pixel; 1 feature
                      [(40.0, 45.0), (80.0, 45.0), (80.0, 70.0), (40.0, 70.0)]])           # 2: inside, no feature
OBJ_FEAT_OFF = np.array([0, 2, 3, 3], np.int32)
OBJ_LEVEL_OFF = np.array([[0, 2, 4, 5], [0, 1, 1, 1], [0, 0, 0, 0]], np.int32)
OBJ_PIX_SLOTS = 3000                                                    # above the sum of the three clamped level-0 boxes


def object_info(fr, pix_cap):
    nslot = int(OBJ_FEAT_OFF[-1])*LEVELS
    u = np.zeros(nslot); v = np.zeros(nslot); inten = np.zeros(nslot)
    u[:5] = [20.5, 40.25, 10.75, 25.0, 8.5]; v[:5] = [20.0, 30.5, 12.25, 15.5, 7.25]; inten[:5] = [100.0, 120.5, 90.25, 80.0, 130.0]
    u[6] = 94.75; v[6] = 78.5; inten[6] = 50.0                          # object 1's feature at the image corner: its last taps fall outside
    o = _outs(dict(musigma=((3, LEVELS, 2), np.float64), ok=((3, LEVELS), np.uint8), ninten=(nslot, np.float64), inten8=((nslot, 8), np.float64),
                   ninten8=((nslot, 8), np.float64), inn=(nslot, np.uint8), pix_off=(4, np.int32), pix_u=(OBJ_PIX_SLOTS, np.int32),
                   pix_v=(OBJ_PIX_SLOTS, np.int32), pix_inten=(OBJ_PIX_SLOTS, np.float64), pix_ninten=(OBJ_PIX_SLOTS, np.float64)))
    pix = [None]*4 if pix_cap == 0 else [_p(o[k]) for k in ("pix_u", "pix_v", "pix_inten", "pix_ninten")]
    _ok(fr, fr.lib.tsframe_text_object_info(fr.ctx, 3, _p(OBJ_QUADS), _p(INV_SCALE), _p(OBJ_FEAT_OFF), _p(OBJ_LEVEL_OFF), _p(u), _p(v), _p(inten), pix_cap,
                                            _p(o["musigma"]), _p(o["ok"]), _p(o["ninten"]), _p(o["inten8"]), _p(o["ninten8"]), _p(o["inn"]), _p(o["pix_off"]), *pix))
    return o


def check_object_info(o, with_pixels):
    off = o["pix_off"]
    assert off[0] == 0 and off[1] > 0 and off[2] == off[1] and off[3] > off[2] and off[3] < OBJ_PIX_SLOTS      # object 1 has no pixel
    for k in ("pix_u", "pix_v", "pix_inten", "pix_ninten"):
        assert _filled(o[k][off[3] if with_pixels else 0:]), k
        assert not with_pixels or not _filled(o[k][:off[3]]), k
    for k in ("ninten", "inn"):                                         # slots past level_off[i][L] of a slice are not written
        assert _filled(o[k][5:6]) and _filled(o[k][7:]) and not _filled(o[k][:5]), k
    assert _filled(o["inten8"][5]) and _filled(o["inten8"][7:]) and not _filled(o["inten8"][6])


BOX_QUAD = np.array([(12.5, 10.2), (70.3, 15.8), (66.1, 50.4), (15.7, 44.9)])
BOX_SLOTS = 4000                                                        # above the clamped box's 59 x 41 pixels


def box_pixels(fr, cap, expect_rc=0):
    o = _outs(dict(n_out=(1, np.int32), u=(BOX_SLOTS, np.int32), v=(BOX_SLOTS, np.int32), inten=(BOX_SLOTS, np.float64), ninten=(BOX_SLOTS, np.float64)))
    arr = [None]*4 if cap == 0 else [_p(o[k]) for k in ("u", "v", "inten", "ninten")]
    rc = fr.lib.tsframe_box_pixels(fr.ctx, 0, _p(BOX_QUAD), 110.0, 35.0, cap, _p(o["n_out"]), *arr)
    assert rc == expect_rc, (rc, fr.lib.tsframe_last_error(fr.ctx).decode())
    return o


def klt(fr, prev):
    xy = np.array([[24.0, 24.0], [40.5, 32.25], [56.0, 48.0], [72.0, 16.0], [90.0, 70.0]], np.float32)
    o = _outs(dict(next_xy=((5, 2), np.float32), status=(5, np.uint8)))
    _ok(fr, fr.lib.tsframe_klt_track(prev.ctx, fr.ctx, 5, _p(xy), 5, 2, 30, 0.01, 1e-4, _p(o["next_xy"]), _p(o["status"])))
    return o


def pts_batch(fr):
    mode = np.array([0, 1], np.int32); xy_off = np.array([0, 7, 7], np.int32)             # a text set of 7 features, an empty scene set
    xy = np.array([[22.5, 21.0], [30.25, 25.5], [41.0, 33.75], [50.5, 28.0], [35.0, 40.0], [26.0, 44.5], [55.5, 47.25]], np.float32)
    box = np.array([[15.0, 15.0, 65.0, 55.0], [0.0, 0.0, 0.0, 0.0]])
    cap = 7*LEVELS
    o = _outs(dict(level_off=((2, LEVELS + 1), np.int32), u=(cap, np.float64), v=(cap, np.float64), idx=(cap, np.int32), inten=(cap, np.float64), inn=(cap, np.uint8)))
    _ok(fr, fr.lib.tsframe_pyramid_pts_batch(fr.ctx, 2, _p(mode), _p(xy_off), _p(xy), _p(box), _p(INV_SCALE), *[_p(o[k]) for k in o]))
    return o


def text_judge(fr, with_bits):
    # plane 0: fronto-parallel at depth 1 under the identity motion, so every reference pixel projects onto itself; plane 1: shifted sideways
    theta = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, -1.0]])
    Tcr = np.zeros((2, 3, 4)); Tcr[:, 0, 0] = Tcr[:, 1, 1] = Tcr[:, 2, 2] = 1.0; Tcr[1, 0, 3] = 0.05
    corners = np.array([(20.0, 20.0), (60.0, 20.0), (60.0, 50.0), (20.0, 50.0)])
    ray = np.tile(((corners - K0[2:])/K0[:2])[None], (2, 1, 1))
    vv, uu = np.mgrid[22:48:2, 22:58:2]
    uv1 = np.stack([uu.ravel(), vv.ravel()], 1).astype(np.int16)
    pix_uv = np.ascontiguousarray(np.concatenate([uv1, uv1[:101]]))
    img = image(W, H, 1)
    pix_inten = np.ascontiguousarray(img[pix_uv[:, 1], pix_uv[:, 0]])
    pix_off = np.array([0, len(uv1), len(pix_uv)], np.int32)
    dete = np.array([[40.0, 35.0], [5.0, 5.0], [57.6, 47.4]])
    o = _outs(dict(ok=(2, np.uint8), reason=(2, np.int32), cos=(2, np.float64), zncc=(2, np.float64), box_uv=((2, 8), np.float64), dete_bits=((2, 1), np.uint32)))
    _ok(fr, fr.lib.tsframe_text_judge(fr.ctx, 0, 2, _p(theta), _p(Tcr), _p(ray), _p(pix_off), _p(pix_uv), _p(pix_inten), _p(K0), _p(K0), 0.0, 6, 0.1,
                                      3, _p(dete), _p(o["ok"]), _p(o["reason"]), _p(o["cos"]), _p(o["zncc"]), _p(o["box_uv"]), _p(o["dete_bits"]) if with_bits else None))
    return o


def test_frame_calls_in_turn_on_one_context_equal_fresh_contexts():
    from textslam_amd.frame import Frame
    prev = Frame(); set_small(prev)                                     # the KLT calls' previous frame: read in place, its own blocks are not used
    states = {"small": set_small, "big": set_big, "raw": set_raw}
    steps = [("set_image 96 x 80", None, set_small),
             ("neighbours", "small", neighbours),
             ("object_info, count only", "small", lambda fr: object_info(fr, 0)),
             ("object_info", "small", lambda fr: object_info(fr, OBJ_PIX_SLOTS)),
             ("box_pixels, count only", "small", lambda fr: box_pixels(fr, 0)),
             ("box_pixels", "small", None),                             # (cap = the count: filled in below)
             ("box_pixels, cap one short", "small", None),
             ("klt", "small", lambda fr: klt(fr, prev)),
             ("pts_batch", "small", pts_batch),
             ("text_judge with dete_bits", "small", lambda fr: text_judge(fr, True)),
             ("text_judge without", "small", lambda fr: text_judge(fr, False)),
             ("set_image 200 x 160", None, set_big),
             ("neighbours in large blocks", "big", neighbours),
             ("set_camera + set_raw_image", None, set_raw),
             ("klt after the raw frame", "raw", lambda fr: klt(fr, prev))]
    first = Frame(); set_small(first)
    count = int(box_pixels(first, 0)["n_out"][0])
    assert 1000 < count < BOX_SLOTS
    steps[5] = (steps[5][0], "small", lambda fr: box_pixels(fr, count))
    steps[6] = (steps[6][0], "small", lambda fr: box_pixels(fr, count - 1, expect_rc=-1))

    def fresh(state, f):
        fr = Frame()
        if state:
            states[state](fr)
        return f(fr)
    ref = {name: fresh(state, f) for name, state, f in steps}
    # the fresh answers are answers: what a call reports written is written, everything else keeps the fill
    assert not _filled(ref["neighbours"]["inten8"]) and ref["neighbours"]["inn"][0] == 1
    check_object_info(ref["object_info, count only"], False); check_object_info(ref["object_info"], True)
    o = ref["box_pixels, count only"]; assert o["n_out"][0] == count and all(_filled(o[k]) for k in ("u", "v", "inten", "ninten"))
    o = ref["box_pixels"]; assert o["n_out"][0] == count and all(_filled(o[k][count:]) and not _filled(o[k][:count]) for k in ("u", "v", "inten", "ninten"))
    o = ref["box_pixels, cap one short"]; assert o["n_out"][0] == count and all(_filled(o[k]) for k in ("u", "v", "inten", "ninten"))
    for name in ("klt", "klt after the raw frame"):
        assert not _filled(ref[name]["next_xy"]) and ref[name]["status"].max() <= 1
    assert ref["klt"]["status"].sum() >= 3                              # (the same image in both contexts: the points stay where they are)
    o = ref["pts_batch"]; m = int(o["level_off"][0, LEVELS])
    assert 0 < m <= 7*LEVELS and (o["level_off"][1] == 0).all() and all(_filled(o[k][m:]) and not _filled(o[k][:m]) for k in ("u", "v", "idx", "inten", "inn"))
    o = ref["text_judge with dete_bits"]; assert o["ok"][0] == 1 and o["zncc"][0] > 0.99 and o["dete_bits"][0, 0] == 0b101 and not _filled(o["box_uv"])
    o = ref["text_judge without"]; assert _filled(o["dete_bits"]) and o["ok"][0] == 1
    assert not _filled(ref["set_camera + set_raw_image"]["undist"])
    shared = Frame()
    for name, _, f in steps:
        _same(f(shared), ref[name], name)


# ---------------------------------------------------------------------------------------------------------------- libtsorb
ORB_W, ORB_H = 160, 120
TEXT_CAP = 95                                                           # odd, and so is nd * cap for 1 and 3 detections
TEXT_QUADS = np.array([[(36.0, 36.0), (120.0, 38.0), (118.0, 84.0), (38.0, 82.0)],
                       [(50.5, 40.0), (100.0, 40.0), (100.0, 70.5), (50.5, 70.5)],
                       [(60.0, 50.0), (125.0, 45.0), (124.0, 86.0), (62.0, 88.0)]])


def _okx(ex, rc):
    assert rc == 0, ex.lib.tsorb_last_error(ex.ctx).decode()


def set_features(ex):
    rng = np.random.default_rng(5)
    kp6 = np.zeros((40, 6), np.float32); kp6[:, 0] = rng.uniform(5, ORB_W - 5, 40); kp6[:, 1] = rng.uniform(5, ORB_H - 5, 40); kp6[:, 2] = 31.0
    kp6[:, 5] = rng.integers(0, 4, 40)
    desc = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    _okx(ex, ex.lib.tsorb_match_set_features(ex.ctx, _p(kp6), _p(desc), 40, 0.0, float(ORB_W), 0.0, float(ORB_H)))
    return {}


def search(ex, nq, max_cand, full):
    rng = np.random.default_rng(100 + nq)
    qxy = np.stack([rng.uniform(10, ORB_W - 10, nq), rng.uniform(10, ORB_H - 10, nq)], 1).astype(np.float32)
    qr = np.full(nq, 45.0, np.float32); qlev = np.tile(np.array([0, 3], np.int32), (nq, 1)); qdesc = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    o = _outs(dict(cand_idx=((nq, max_cand), np.int32), cand_dist=((nq, max_cand), np.int32), cand_cnt=(nq, np.int32), best_idx=(nq, np.int32),
                   best_dist=(nq, np.int32), best_dist2=(nq, np.int32)))
    omit = () if full else ("cand_idx", "best_dist2")
    _okx(ex, ex.lib.tsorb_match_search(ex.ctx, nq, _p(qxy), _p(qr), _p(qlev) if full else None, _p(qdesc), max_cand, *[None if k in omit else _p(o[k]) for k in o]))
    return o


def text_extract(ex, nd):
    o = _outs(dict(kp=((nd, TEXT_CAP, 6), np.float32), desc=((nd, TEXT_CAP, 32), np.uint8), count=(nd, np.int32)))
    _okx(ex, ex.lib.tsorb_text_extract(ex.ctx, 0, nd, _p(np.ascontiguousarray(TEXT_QUADS[:nd])), 40, TEXT_CAP, _p(o["kp"]), _p(o["desc"]), _p(o["count"])))
    return o


def test_orb_calls_in_turn_on_one_context_equal_fresh_contexts():
    from textslam_amd.orbextractor import ORBextractor

    def new():
        ex = ORBextractor(nlevels=4)                                    # (160 x 120: the scene pyramid has room for four levels; cv::ORB's eight do not depend on it)
        ex.extract_batch(image(ORB_W, ORB_H, 9))
        return ex
    steps = [("set_features", False, set_features),
             ("search 3, outputs omitted", True, lambda ex: search(ex, 3, 4, False)),
             ("search 33", True, lambda ex: search(ex, 33, 4, True)),
             ("search 3 again", True, lambda ex: search(ex, 3, 4, False)),
             ("text_extract 1", False, lambda ex: text_extract(ex, 1)),
             ("text_extract 3", False, lambda ex: text_extract(ex, 3)),
             ("text_extract 1 again", False, lambda ex: text_extract(ex, 1))]

    def fresh(needs_features, f):
        ex = new()
        if needs_features:
            set_features(ex)
        return f(ex)
    ref = {name: fresh(needs, f) for name, needs, f in steps}
    for name in ("search 3, outputs omitted", "search 3 again"):
        o = ref[name]
        assert _filled(o["cand_idx"]) and _filled(o["best_dist2"]) and not _filled(o["cand_cnt"]) and not _filled(o["best_idx"]) and not _filled(o["cand_dist"])
    o = ref["search 33"]
    assert not any(_filled(o[k]) for k in o) and o["cand_cnt"].max() > 0 and (o["best_idx"] >= 0).any()
    for name, nd in (("text_extract 1", 1), ("text_extract 3", 3), ("text_extract 1 again", 1)):
        o = ref[name]
        assert (o["count"] > 0).all() and (o["count"] <= TEXT_CAP).all(), (name, o["count"])
        for d in range(nd):                                             # rows past count[d] keep the fill
            n = int(o["count"][d])
            assert _filled(o["kp"][d, n:]) and _filled(o["desc"][d, n:]) and not _filled(o["kp"][d, :n]) and o["desc"][d, :n].any(), (name, d)
    shared = new()
    for name, _, f in steps:
        _same(f(shared), ref[name], name)

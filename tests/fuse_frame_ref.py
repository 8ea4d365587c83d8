"""TEST INFRASTRUCTURE: the numpy restatement of tool::BoundFeatDele_T (src/tool.cc:456-508) and frame::FeatFusion (src/frame.cc:257-325) over the raw text
features of cvorb_ref.Frame(...).extract(...) and given scene rows.  docs/pointpolygon_recalled.md is cv::pointPolygonTest; point_polygon_positive below restates it
with float32 differences widened to double, independently of csrc/tsfuse.h (tests/test_fuse_frame_ref.py compares the two on 20 000 seeded pairs)."""
import numpy as np

F = np.float32
D = np.float64
FLT_MAX = float(np.finfo(np.float32).max)


def trunc_int(v):
    """cv::Point(double, double): truncation towards zero (a value no int holds: INT32_MIN, as csrc/tsfuse.h states it)."""
    v = float(v)
    return int(v) if -2147483649.0 < v < 2147483648.0 else -2147483648


def shrunk_quad(quad, win):
    """tool::GetNewDeteBox + vV2vP: [4, 2] ints."""
    q = np.asarray(quad, D).reshape(4, 2); w = float(win)
    return [[trunc_int(q[0, 0] - w), trunc_int(q[0, 1] - w)], [trunc_int(q[1, 0] + w), trunc_int(q[1, 1] - w)],
            [trunc_int(q[2, 0] + w), trunc_int(q[2, 1] + w)], [trunc_int(q[3, 0] - w), trunc_int(q[3, 1] + w)]]


def bbox_quad(bbox):
    """tool::GetbbDeteBox + vV2vP from vTextDeteMin x, y, vTextDeteMax x, y."""
    x0, y0, x1, y1 = [trunc_int(v) for v in np.asarray(bbox, D).reshape(4)]
    return [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]


def bbox_of(quads):
    """vTextDeteMin / vTextDeteMax: the corners' min and max, [n, 4]."""
    q = np.asarray(quads, D).reshape(-1, 4, 2)
    return np.concatenate([q.min(1), q.max(1)], 1)


def point_polygon_positive(poly_int, x, y):
    """cv::pointPolygonTest(contour of int points, Point2f(x, y), measureDist = true) > 0."""
    poly = [(F(int(px)), F(int(py))) for px, py in poly_int]           # Point -> Point2f
    if not poly:
        return False
    x, y = F(x), F(y)
    min_num, min_den, counter = FLT_MAX, 1.0, 0
    vx, vy = poly[-1]
    for nx, ny in poly:
        v0x, v0y, vx, vy = vx, vy, nx, ny
        dx, dy = float(F(vx - v0x)), float(F(vy - v0y))
        dx1, dy1 = float(F(x - v0x)), float(F(y - v0y))
        dx2, dy2 = float(F(x - vx)), float(F(y - vy))
        den = 1.0
        if dx1 * dx + dy1 * dy <= 0:
            num = dx1 * dx1 + dy1 * dy1
        elif dx2 * dx + dy2 * dy >= 0:
            num = dx2 * dx2 + dy2 * dy2
        else:
            num = dy1 * dx - dx1 * dy
            num *= num
            den = dx * dx + dy * dy
        if num * min_den < min_num * den:
            min_num, min_den = num, den
            if min_num == 0:
                break
        if (v0y <= y and vy <= y) or (v0y > y and vy > y):
            continue
        t = dy1 * dx - dx1 * dy
        if dy < 0:
            t = -t
        counter += t > 0
    return bool(min_num != 0 and counter % 2 == 1)


def bound_feat_dele_t(raw, quads, bbox, win=-3.0):
    """raw: list of (kp [k, 6], desc [k, 32]) per detection.  Returns per detection (kp, desc, idx): the kept rows in raw order and their raw indices (IdxNewText)."""
    out = []
    for (kp, desc), quad, bb in zip(raw, np.asarray(quads, D).reshape(-1, 4, 2), np.asarray(bbox, D).reshape(-1, 4)):
        ps, pb = shrunk_quad(quad, win), bbox_quad(bb)
        idx = np.array([i for i in range(len(kp)) if point_polygon_positive(ps, kp[i, 0], kp[i, 1]) and point_polygon_positive(pb, kp[i, 0], kp[i, 1])], np.int32)
        out.append((np.ascontiguousarray(kp[idx], F).reshape(-1, 6), np.ascontiguousarray(desc[idx], np.uint8).reshape(-1, 32), idx))
    return out


def feat_fusion(scene_kp, scene_desc, kept):
    """frame::FeatFusion over the scene rows and bound_feat_dele_t's result: a dict with tsorb_fuse_frame's arrays."""
    scene_kp = np.ascontiguousarray(scene_kp, F).reshape(-1, 6); scene_desc = np.ascontiguousarray(scene_desc, np.uint8).reshape(-1, 32)
    ns = len(scene_kp)
    off = np.zeros(len(kept) + 1, np.int32)
    off[0] = ns
    off[1:] = ns + np.cumsum([len(k[0]) for k in kept], dtype=np.int64)
    return dict(kp=np.concatenate([scene_kp] + [k[0] for k in kept]), desc=np.concatenate([scene_desc] + [k[1] for k in kept]),
                obj=np.concatenate([np.full(ns, -1, np.int32)] + [np.full(len(k[0]), d, np.int32) for d, k in enumerate(kept)]),
                src=np.concatenate([np.arange(ns, dtype=np.int32)] + [k[2].astype(np.int32) for k in kept]),
                text_off=off, raw_count=None, n_scene=ns)


def fuse_frame(scene_kp, scene_desc, raw, quads, bbox, win=-3.0):
    """What ORBextractor.fuse_frame returns, from the scene rows (ex.download()) and the raw text features (cvorb_ref.Frame.extract)."""
    out = feat_fusion(scene_kp, scene_desc, bound_feat_dele_t(raw, quads, bbox, win))
    out["raw_count"] = np.array([len(r[0]) for r in raw], np.int32)
    return out


# ------------------------------------------------------------------ the lists of tests/cxx/fuse_frame_from_cxx.cpp (its dump format is stated at its top)
def lists_of(fused, n_dete):
    """The reference's members (vKeysScene .. iN) from a fuse_frame dictionary (the restatement's or the mirror's)."""
    ns, n, off = int(fused["n_scene"]), len(fused["kp"]), np.asarray(fused["text_off"], np.int64)
    sl = [slice(int(off[d]), int(off[d + 1])) for d in range(n_dete)]
    return dict(iNScene=ns, iNTextObj=n_dete, iNTextFea=n - ns, iN=n, vKeysScene=fused["kp"][:ns], mDescrScene=fused["desc"][:ns],
                vKeysText=[fused["kp"][s] for s in sl], mDescrText=[fused["desc"][s] for s in sl],
                vKeysTextIdx=[np.arange(s.start, s.stop, dtype=np.int32) for s in sl], IdxNewText=[np.asarray(fused["src"][s], np.int32) for s in sl],
                vKeys=fused["kp"], mDescr=fused["desc"], vTextObjInfo=np.asarray(fused["obj"], np.int32), vKeysSceneIdx=np.arange(ns, dtype=np.int32))


def read_lists(raw):
    """Parse the driver's dump."""
    pos = [0]

    def take(dtype, count, shape):
        a = np.frombuffer(raw, dtype, count, pos[0]).reshape(shape); pos[0] += a.nbytes
        return a
    ns, nd, nt, n = (int(v) for v in take(np.int32, 4, (4,)))
    out = dict(iNScene=ns, iNTextObj=nd, iNTextFea=nt, iN=n, vKeysScene=take(F, 6 * ns, (ns, 6)), mDescrScene=take(np.uint8, 32 * ns, (ns, 32)),
               vKeysText=[], mDescrText=[], vKeysTextIdx=[], IdxNewText=[])
    for _ in range(nd):
        k = int(take(np.int32, 1, (1,))[0])
        out["vKeysText"].append(take(F, 6 * k, (k, 6))); out["mDescrText"].append(take(np.uint8, 32 * k, (k, 32)))
        out["vKeysTextIdx"].append(take(np.int32, k, (k,))); out["IdxNewText"].append(take(np.int32, k, (k,)))
    out.update(vKeys=take(F, 6 * n, (n, 6)), mDescr=take(np.uint8, 32 * n, (n, 32)), vTextObjInfo=take(np.int32, n, (n,)), vKeysSceneIdx=take(np.int32, ns, (ns,)))
    assert pos[0] == len(raw), (pos[0], len(raw))
    return out


def assert_lists_equal(got, ref):
    """List for list, byte for byte (floats as bit patterns)."""
    assert sorted(got) == sorted(ref)
    for k, r in ref.items():
        g = got[k]
        if isinstance(r, int):
            assert g == r, (k, g, r)
            continue
        gs, rs = (g, r) if isinstance(r, list) else ([g], [r])
        assert len(gs) == len(rs), k
        for d, (a, b) in enumerate(zip(gs, rs)):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (k, d, a.shape, b.shape)


def host_input(scene_kp, scene_desc, raw, quads, bbox, win):
    """The --host mode's input file."""
    import struct
    parts = [struct.pack("<ii", len(scene_kp), len(raw)), np.ascontiguousarray(scene_kp, F).tobytes(), np.ascontiguousarray(scene_desc, np.uint8).tobytes(),
             np.ascontiguousarray(quads, D).tobytes(), np.ascontiguousarray(bbox, D).tobytes(), struct.pack("<d", float(win))]
    for kp, desc in raw:
        parts += [struct.pack("<i", len(kp)), np.ascontiguousarray(kp, F).tobytes(), np.ascontiguousarray(desc, np.uint8).tobytes()]
    return b"".join(parts)

"""numpy restatement of a keyframe's new scene points as docs/newpoints_recalled.md states them: frame::AssignFeaturesToGrid / GetFeaturesInArea (the grid and the
candidates' order), tracking::DescriptorDistance, the claim chain of tracking::SearchForTriangular / SearchForInitializ transcribed from the reference's two loops,
GetForTriangular's triangulation between two general cameras (PixToCam's float points, cvTriangulatePoints' 4 x 4 in double, its null vector by np.linalg.svd rounded to
float as a 4-vector, the float division by its last entry) and CheckTriangular operation by operation.  What tsorb_match_search_claim and tsorb_match_new_points
(include/tsorb.h, textslam_amd/csrc/tsclaim.h) are compared with, the worlds the tests commit to and the sensitivity of the triangulation.

The triangulation's pieces that tracking::GetTextTheta shares (pix_to_cam, null_vectors, points_of) are tests/text_theta_ref.py's."""
import functools
import numpy as np
import text_theta_ref as T

F32, F64, I32 = np.float32, np.float64, np.int32
INT_MAX = 2147483647
COLS, ROWS = 64, 48                                                      # FRAME_GRID_COLS, FRAME_GRID_ROWS
_ERR = dict(invalid="ignore", divide="ignore", over="ignore")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
same32 = T.same32


# ---- the grid and the candidates (frame.cc:372-468, in the doubles tsorb_match_search uses)
def _cround(v):
    """C's round(): halves away from zero."""
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def build_grid(kp6, bounds):
    """AssignFeaturesToGrid: every cell lists its features in index order.  Returns (off [COLS*ROWS + 1], lst): cell (ix, iy) is lst[off[ix*ROWS + iy]:off[ix*ROWS + iy + 1]]."""
    kp6 = np.asarray(kp6, F32).reshape(-1, 6); min_x, max_x, min_y, max_y = [float(b) for b in bounds]
    iw, ih = COLS/(max_x - min_x), ROWS/(max_y - min_y)
    px = _cround((kp6[:, 0].astype(F64) - min_x)*iw); py = _cround((kp6[:, 1].astype(F64) - min_y)*ih)
    inside = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    cell = np.where(inside, px*ROWS + py, -1).astype(np.int64)
    idx = np.flatnonzero(inside); order = idx[np.argsort(cell[idx], kind="stable")]
    off = np.zeros(COLS*ROWS + 1, np.int64); np.add.at(off, cell[idx] + 1, 1)
    return np.cumsum(off), order, (min_x, min_y, iw, ih)


def candidates(grid, kp6, x, y, r, min_level, max_level):
    """GetFeaturesInArea: the indices in the reference's order (window cells column by column, index order inside a cell)."""
    off, lst, (min_x, min_y, iw, ih) = grid
    x, y, r = F32(x), F32(y), F32(r)
    c0x = max(0, int(np.floor((float(x) - min_x - float(r))*iw)))
    c1x = min(COLS - 1, int(np.ceil((float(x) - min_x + float(r))*iw)))
    c0y = max(0, int(np.floor((float(y) - min_y - float(r))*ih)))
    c1y = min(ROWS - 1, int(np.ceil((float(y) - min_y + float(r))*ih)))
    if c0x >= COLS or c1x < 0 or c0y >= ROWS or c1y < 0 or c1x < c0x or c1y < c0y:
        return np.zeros(0, np.int64)
    c = np.concatenate([lst[off[ix*ROWS + c0y]:off[ix*ROWS + c1y + 1]] for ix in range(c0x, c1x + 1)])
    keep = np.ones(len(c), bool)
    if min_level > 0 or max_level >= 0:
        octave = kp6[c, 5].astype(np.int64)
        keep &= ~(octave < min_level)
        if max_level >= 0:
            keep &= ~(octave > max_level)
    dx = kp6[c, 0] - x; dy = kp6[c, 1] - y                                # float arithmetic
    keep &= (np.abs(dx) < r) & (np.abs(dy) < r)
    return c[keep]


def hamming(d, rows):
    """tracking::DescriptorDistance of descriptor d [32] against rows [k, 32]."""
    return _POP[np.bitwise_xor(np.asarray(rows, np.uint8).reshape(-1, 32), np.asarray(d, np.uint8).reshape(1, 32))].sum(axis=1).astype(np.int64)


def lists(w):
    """Every query's candidates and distances, before any eligibility or vMatchDist test."""
    kp6 = np.asarray(w["kp6"], F32).reshape(-1, 6); grid = build_grid(kp6, w["bounds"]); out = []
    for q in range(len(w["qxy"])):
        l0, l1 = (-1, -1) if w.get("qlev") is None else [int(v) for v in w["qlev"][q]]
        c = candidates(grid, kp6, w["qxy"][q][0], w["qxy"][q][1], w["qr"][q], l0, l1)
        out.append((c, hamming(w["qdesc"][q], np.asarray(w["desc2"], np.uint8).reshape(-1, 32)[c])))
    return out


# ---- the chain (tracking.cc:1347-1411 and :1045-1109: the two loops are one but for the ratio test)
def chain_lists(cands, n2, elig2, th_low, use_ratio, ratio, trace=None):
    """trace (a dict): counts the steals and the candidates vMatchDist hid."""
    nq = len(cands); steals = hidden = 0
    vMatchIdx12 = [-1]*nq; vMatchDist = [INT_MAX]*n2; vMatchIdx21 = [-1]*n2; dist12 = [-1]*nq
    nMatches = 0
    for i1 in range(nq):
        c, dd = cands[i1]
        if len(c) == 0:
            continue
        bestDist, bestDist2, bestIdx2 = INT_MAX, INT_MAX, -1
        for i2, dist in zip(c.tolist(), dd.tolist()):
            if elig2 is not None and not elig2[i2]:                      # F2.vMatches2D3D[i2] >= 0
                continue
            if vMatchDist[i2] <= dist:
                hidden += 1
                continue
            if dist < bestDist:
                bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2
            elif dist < bestDist2:
                bestDist2 = dist
        if bestDist <= th_low:
            if use_ratio and not (float(bestDist) < float(bestDist2)*float(ratio)):
                continue
            if vMatchIdx21[bestIdx2] >= 0:
                vMatchIdx12[vMatchIdx21[bestIdx2]] = -1; dist12[vMatchIdx21[bestIdx2]] = -1
                nMatches -= 1; steals += 1
            vMatchIdx12[i1] = bestIdx2; vMatchIdx21[bestIdx2] = i1; vMatchDist[bestIdx2] = bestDist; dist12[i1] = bestDist
            nMatches += 1
    assert nMatches == sum(1 for m in vMatchIdx12 if m >= 0)
    if trace is not None:
        trace.update(steals=steals, hidden=hidden)
    return np.array(vMatchIdx12, I32).reshape(nq), np.array(dist12, I32).reshape(nq), nMatches


def chain(w, cands=None, trace=None):
    cands = lists(w) if cands is None else cands
    elig = None if w.get("elig2") is None else np.asarray(w["elig2"]).reshape(-1) != 0
    return chain_lists(cands, len(w["kp6"]), elig, int(w["th_low"]), bool(w["use_ratio"]), float(w["ratio"]), trace)


# ---- the triangulation between two general cameras (tracking.cc:1413-1443) and CheckTriangular (:1461-1497)
def pixels(w, m12):
    """pt1, pt2 [M, 2] float32 of the matches in query order (MatchRaw's order) and their query numbers."""
    rows = np.flatnonzero(np.asarray(m12) >= 0)
    return np.asarray(w["q_px"], F32).reshape(-1, 2)[rows], np.asarray(w["kp6"], F32).reshape(-1, 6)[np.asarray(m12)[rows], :2], rows


def system(w, pt1, pt2):
    """cvTriangulatePoints' 4 x 4 per match [M, 4, 4] in double: x*P[2][k] - P[0][k], y*P[2][k] - P[1][k] for P1 = Trw and P2 = Tcw."""
    fx, fy, cx, cy = [float(v) for v in w["K"]]
    P1 = np.asarray(w["Trw"], F64).reshape(-1, 4)[:3]; P2 = np.asarray(w["Tcw"], F64).reshape(-1, 4)[:3]
    x1 = T.pix_to_cam(pt1[:, 0], cx, fx).astype(F64)[:, None]; y1 = T.pix_to_cam(pt1[:, 1], cy, fy).astype(F64)[:, None]
    x2 = T.pix_to_cam(pt2[:, 0], cx, fx).astype(F64)[:, None]; y2 = T.pix_to_cam(pt2[:, 1], cy, fy).astype(F64)[:, None]
    A = np.empty((len(pt1), 4, 4))
    with np.errstate(**_ERR):
        A[:, 0] = x1*P1[2] - P1[0]; A[:, 1] = y1*P1[2] - P1[1]; A[:, 2] = x2*P2[2] - P2[0]; A[:, 3] = y2*P2[2] - P2[1]
    return A


def triangulate(w, pt1, pt2, rng=None):
    """p4d /= p4d(3) of every match: [M, 3] float32."""
    return T.points_of(T.null_vectors(system(w, pt1, pt2), rng))[0] if len(pt1) else np.zeros((0, 3), F32)


def check(w, X, pt1, pt2):
    """CheckTriangular on the float points X [M, 3], operation by operation in doubles: b3dRaw [M].  No depth test; a NaN error passes both `>` tests."""
    fx, fy, cx, cy = [F64(v) for v in w["K"]]; th = F32(int(w["th_reproj"]))
    Trw = np.asarray(w["Trw"], F64).reshape(-1, 4)[:3]; Tcw = np.asarray(w["Tcw"], F64).reshape(-1, 4)[:3]
    p = np.asarray(X, F32).astype(F64).reshape(-1, 3); pt1 = np.asarray(pt1, F32).astype(F64); pt2 = np.asarray(pt2, F32).astype(F64)
    with np.errstate(**_ERR):
        ok = np.isfinite(p[:, 0]) & np.isfinite(p[:, 1]) & np.isfinite(p[:, 2])
        ref = [((Trw[r, 0]*p[:, 0] + Trw[r, 1]*p[:, 1]) + Trw[r, 2]*p[:, 2]) + Trw[r, 3] for r in range(3)]
        cur = [((Tcw[r, 0]*p[:, 0] + Tcw[r, 1]*p[:, 1]) + Tcw[r, 2]*p[:, 2]) + Tcw[r, 3] for r in range(3)]
        u1 = (fx*ref[0])/ref[2] + cx; v1 = (fy*ref[1])/ref[2] + cy
        ok &= ~((u1 < 0) | (v1 < 0))
        e1 = ((u1 - pt1[:, 0])*(u1 - pt1[:, 0]) + (v1 - pt1[:, 1])*(v1 - pt1[:, 1])).astype(F32)
        ok &= ~(e1 > th)
        u2 = (fx*cur[0])/cur[2] + cx; v2 = (fy*cur[1])/cur[2] + cy
        e2 = ((u2 - pt2[:, 0])*(u2 - pt2[:, 0]) + (v2 - pt2[:, 1])*(v2 - pt2[:, 1])).astype(F32)
        ok &= ~(e2 > th)
    return ok


def run(w, p3d=None, rng=None, cands=None):
    """The two calls' outputs.  p3d [nq, 3]: check THESE points (the rows with a match) instead of the restatement's own."""
    m12, md, nm = chain(w, cands); nq = len(m12)
    pt1, pt2, rows = pixels(w, m12)
    X = triangulate(w, pt1, pt2, rng) if p3d is None else np.asarray(p3d, F32).reshape(-1, 3)[rows]
    P = np.zeros((nq, 3), F32); good = np.zeros(nq, bool)
    P[rows] = X; good[rows] = check(w, X, pt1, pt2)
    return dict(match12=m12, match_dist=md, n_match=nm, p3d=P, good=good, n_good=int(good.sum()))


def sensitivity(w, m12=None, draws=3):
    """How far the 4 x 4's entries moved at the 1e-13 relative level move the point: per query (zero without a match) the largest |X' - X| / max|X| in fp64, and the
    largest movement of the float point in float steps."""
    m12 = chain(w)[0] if m12 is None else m12
    pt1, pt2, rows = pixels(w, m12); nq = len(m12)
    rel = np.zeros(nq); ulp = np.zeros(nq, np.int64)
    if len(rows):
        A = system(w, pt1, pt2); v = T.null_vectors(A); X = T.points_of(v)[0]
        with np.errstate(**_ERR):
            X64 = v[:, :3]/v[:, 3:4]
            for k in range(draws):
                v2 = T.null_vectors(A, np.random.default_rng(1000 + k)); Y = T.points_of(v2)[0]
                rel[rows] = np.maximum(rel[rows], np.abs(v2[:, :3]/v2[:, 3:4] - X64).max(axis=1)/np.abs(X64).max(axis=1))
                ulp[rows] = np.maximum(ulp[rows], np.abs(T._ordered(X) - T._ordered(Y)).max(axis=1))
    return dict(rel=rel, ulp=ulp)


# ---- the worlds
K0 = (458.5, 457.25, 367.25, 248.375)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
RADIUS = float(F32(80)*F32(1.2))                                         # SearchForTriangular: Win*ScaleORB in float


def _rot(a):
    th = np.linalg.norm(a); k = a/th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th)*Kx + (1 - np.cos(th))*(Kx @ Kx)


def cameras(rng):
    """Two cameras, neither the identity: a few degrees each, 0.5 apart mostly sideways -- a baseline of a tenth of the scene's depth (3 .. 5) and more."""
    Trw = np.column_stack([_rot(rng.normal(0, 0.02, 3)), rng.normal(0, 0.05, 3)])
    Tcw = np.column_stack([_rot(rng.normal(0, 0.02, 3)), Trw[:, 3] + np.array([-0.5, 0.0, 0.0]) + rng.normal(0, 0.03, 3)])
    return Trw, Tcw


def _flip(rng, d, k):
    out = np.unpackbits(np.asarray(d, np.uint8)); out[rng.permutation(256)[:k]] ^= 1
    return np.packbits(out)


def _views(rng, Trw, Tcw, K, uv2, noise):
    """The frame's pixels uv2 [n, 2] at depths 3 .. 5 seen from the keyframe: [n, 2] with `noise` px."""
    fx, fy, cx, cy = K; n = len(uv2); z = rng.uniform(3.0, 5.0, n)
    Xc = np.column_stack([(uv2[:, 0] - cx)/fx*z, (uv2[:, 1] - cy)/fy*z, z])
    Xw = (Xc - Tcw[:, 3]) @ Tcw[:, :3]                                    # R^T (Xc - t)
    Xr = Xw @ Trw[:, :3].T + Trw[:, 3]
    return np.column_stack([Xr[:, 0]/Xr[:, 2]*fx + cx, Xr[:, 1]/Xr[:, 2]*fy + cy]) + rng.normal(0, noise, (n, 2))


def scene_world(seed, n2, nq, level=True, elig="all", use_ratio=False, spread=None, area=None, qr=RADIUS, max_flip=40, init=False, bad_every=0):
    """A keyframe and a frame over one scene.  The frame's n2 features lie in `area` (x0, x1, y0, y1; the image by default); query j is the keyframe's view of feature
    perm[j % n2] with 0.3 px of noise, its descriptor that feature's with up to max_flip bits turned (nq > n2: several queries contend for a feature).  spread: every
    feature's descriptor is a common one with that many bits turned (neighbours within th_low of each other) instead of an independent one.  elig 'half': every
    second feature of the frame has a map point already.  init: SearchForInitializ's shape -- octave 0 only, the ratio test.  bad_every: every such query's pixel is 8 px of noise off (CheckTriangular has something to refuse)."""
    rng = np.random.default_rng(seed); K = K0; Trw, Tcw = cameras(rng)
    x0, x1, y0, y1 = area if area is not None else (20.0, 620.0, 20.0, 460.0)
    uv2 = np.column_stack([rng.uniform(x0, x1, n2), rng.uniform(y0, y1, n2)]).astype(F32)
    octv = np.zeros(n2) if init else rng.choice([0, 0, 0, 1, 1, 2, 3], n2)
    kp6 = np.zeros((n2, 6), F32); kp6[:, :2] = uv2; kp6[:, 2] = 31.0; kp6[:, 5] = octv
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    desc2 = np.stack([_flip(rng, base, spread) if spread is not None else rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(n2)]) if n2 else np.zeros((0, 32), np.uint8)
    src = np.concatenate([rng.permutation(n2) for _ in range(-(-nq//max(n2, 1)))])[:nq] if nq else np.zeros(0, np.int64)
    q_px = _views(rng, Trw, Tcw, K, uv2[src].astype(F64), 0.3).astype(F32) if nq else np.zeros((0, 2), F32)
    if bad_every and nq:
        q_px[::bad_every] += rng.normal(0, 8.0, (len(q_px[::bad_every]), 2)).astype(F32)
    qdesc = np.stack([_flip(rng, desc2[s], int(rng.integers(0, max_flip + 1))) for s in src]) if nq else np.zeros((0, 32), np.uint8)
    qlev = np.column_stack([octv[src], octv[src]]).astype(I32) if level else None
    e = None if elig == "all" else (np.arange(n2) % 2 == 0).astype(np.uint8)
    return dict(kp6=kp6, desc2=desc2, bounds=BOUNDS, qxy=q_px.copy(), qr=np.full(nq, qr, F32), qlev=qlev, qdesc=qdesc, elig2=e, th_low=50, use_ratio=bool(use_ratio or init),
                ratio=0.9, q_px=q_px, Trw=Trw, Tcw=Tcw, K=np.array(K, F64), th_reproj=9, source=src)


WINDOW_COUNTS = (0, 1, 64, 65, 129, 600)


def windows_world(seed=40):
    """Windows that hold exactly 0, 1, 64, 65, 129 and 600 candidates (600: above any fixed row of a query's list), a window that leaves the grid and a query outside it.
    Cluster k's features lie within 8 px of its centre in the frame; three queries each, the keyframe's views of its first three features (of its only one), with a
    70-px radius that holds the whole cluster and nothing else.  No level filter; the descriptors of a cluster within th_low of each other."""
    rng = np.random.default_rng(seed); K = K0; Trw, Tcw = cameras(rng)
    centres = [(110.0, 110.0), (290.0, 110.0), (470.0, 110.0), (110.0, 330.0), (290.0, 330.0), (470.0, 330.0)]
    uv2, desc2, qsrc, qxy_extra = [], [], [], []
    for (cxk, cyk), n in zip(centres, WINDOW_COUNTS):
        a0 = sum(len(u) for u in uv2)
        ang = rng.uniform(0, 2*np.pi, n); rad = 8.0*np.sqrt(rng.uniform(0, 1, n))
        uv2.append(np.column_stack([cxk + rad*np.cos(ang), cyk + rad*np.sin(ang)]))
        base = rng.integers(0, 256, 32, dtype=np.uint8); desc2 += [_flip(rng, base, 18) for _ in range(n)]
        qsrc += [a0 + j for j in range(min(n, 3))]
        if n == 0:
            qxy_extra.append((cxk, cyk))
    uv2 = np.concatenate(uv2).astype(F32); n2 = len(uv2)
    border = np.array([[6.0, 200.0], [9.0, 236.0], [630.0, 470.0]], F32)           # features near the image's edge: their queries' windows leave the grid
    qsrc += list(range(n2, n2 + len(border))); uv2 = np.concatenate([uv2, border]); desc2 += [rng.integers(0, 256, 32, dtype=np.uint8) for _ in border]; n2 = len(uv2)
    kp6 = np.zeros((n2, 6), F32); kp6[:, :2] = uv2; kp6[:, 2] = 31.0; kp6[:, 5] = rng.choice([0, 1, 2], n2)
    desc2 = np.stack(desc2); src = np.array(qsrc)
    q_px = _views(rng, Trw, Tcw, K, uv2[src].astype(F64), 0.3).astype(F32)
    qdesc = np.stack([_flip(rng, desc2[s], int(rng.integers(0, 12))) for s in src])
    # the empty window and two queries outside the grid (left of it and below it), with descriptors of their own
    extra = np.array(qxy_extra + [(-200.0, 100.0), (300.0, 900.0)], F32)
    q_px = np.concatenate([q_px, extra]); qdesc = np.concatenate([qdesc, rng.integers(0, 256, (len(extra), 32), dtype=np.uint8)]); nq = len(q_px)
    return dict(kp6=kp6, desc2=desc2, bounds=BOUNDS, qxy=q_px.copy(), qr=np.full(nq, 70.0, F32), qlev=None, qdesc=qdesc, elig2=None, th_low=50, use_ratio=False, ratio=0.9,
                q_px=q_px, Trw=Trw, Tcw=Tcw, K=np.array(K, F64), th_reproj=9, source=np.concatenate([src, np.full(len(extra), -1)]))


def pairs_world(seed, n):
    """n features, n queries, every query its own feature's view with 5 bits turned and independent descriptors: exactly n accepted matches."""
    return scene_world(seed, n, n, max_flip=5)


WORLDS = {
    "pairs_1": lambda: pairs_world(51, 1), "pairs_64": lambda: pairs_world(52, 64), "pairs_65": lambda: pairs_world(53, 65), "pairs_257": lambda: pairs_world(54, 257),
    "s63_q4": lambda: scene_world(55, 63, 4), "s64_q5_none": lambda: dict(scene_world(56, 64, 5), qdesc=np.random.default_rng(56).integers(0, 256, (5, 32), dtype=np.uint8)),
    "contend_255": lambda: scene_world(57, 65, 255, level=False, spread=16, area=(280.0, 360.0, 200.0, 260.0), bad_every=7),
    "s1000_q0": lambda: scene_world(58, 1000, 0), "s1000_q256": lambda: scene_world(59, 1000, 256, elig="half", bad_every=7), "init_s1000_q257": lambda: scene_world(60, 1000, 257, init=True, qr=100.0, spread=24, max_flip=55),
    "s5000_q3000": lambda: scene_world(61, 5000, 3000, bad_every=7), "windows": windows_world,
}
ALL = list(WORLDS)


@functools.lru_cache(maxsize=None)
def make(name):
    """A committed world (shared, read-only)."""
    return WORLDS[name]()


@functools.lru_cache(maxsize=None)
def cand_lists(name):
    return lists(make(name))


@functools.lru_cache(maxsize=None)
def answer(name):
    return run(make(name), cands=cand_lists(name))


@functools.lru_cache(maxsize=None)
def sens(name):
    return sensitivity(make(name), answer(name)["match12"])

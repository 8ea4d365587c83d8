"""numpy restatement of the new text planes' RANSAC as docs/texttheta_recalled.md states it: tracking::GetTextTheta's triangulation (PixToCam's float points,
cvTriangulatePoints' 4 x 4 in double, its null vector by np.linalg.svd rounded to float as a 4-vector, the float division by its last entry, rho = 1/z), the host rays,
SolveTheta's closed form and its score operation by operation in IEEE doubles, and the keep loop.  What tsorb_match_text_theta_ransac (include/tsorb.h,
textslam_amd/csrc/tstexttheta.h) is compared with, the worlds the tests commit to, the sensitivity of the triangulation and the condition the worlds have to meet.

`hypothesis_scalar` is the definition: one hypothesis, scalar by scalar in Python floats.  `hypotheses` runs the same operations on numpy float64 arrays over a plane's
hypotheses (elementwise IEEE operations, the features still one after the other), and tests/test_text_theta_ref.py holds the two equal in every bit."""
import functools
import numpy as np

F32, F64 = np.float32, np.float64
TH = float(F32(5.991))                                                   # const float th = 5.991, used as a double
MAX_FEAT = 1024
_ERR = dict(invalid="ignore", divide="ignore", over="ignore")


# ---- the triangulation (tracking.cc:1667-1698)
def pix_to_cam(p, c, f):
    """tool::PixToCam: (p.x - cx)/fx in double, stored in a cv::Point2f."""
    with np.errstate(**_ERR):
        return ((np.asarray(p, F32).astype(F64) - F64(c))/F64(f)).astype(F32)


def system(w):
    """cvTriangulatePoints' 4 x 4 per feature [N, 4, 4] in double: x*P[2][k] - P[0][k], y*P[2][k] - P[1][k] for P1 = [I | 0] and P2 = Tcr."""
    fx, fy, cx, cy = [float(v) for v in w["K"]]
    P1 = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]); P2 = np.asarray(w["Tcr"], F64).reshape(3, 4)
    h = np.asarray(w["host_xy"], F32).reshape(-1, 2); t = np.asarray(w["targ_xy"], F32).reshape(-1, 2)
    x1 = pix_to_cam(h[:, 0], cx, fx).astype(F64)[:, None]; y1 = pix_to_cam(h[:, 1], cy, fy).astype(F64)[:, None]
    x2 = pix_to_cam(t[:, 0], cx, fx).astype(F64)[:, None]; y2 = pix_to_cam(t[:, 1], cy, fy).astype(F64)[:, None]
    A = np.empty((len(h), 4, 4))
    with np.errstate(**_ERR):
        A[:, 0] = x1*P1[2] - P1[0]; A[:, 1] = y1*P1[2] - P1[1]; A[:, 2] = x2*P2[2] - P2[0]; A[:, 3] = y2*P2[2] - P2[1]
    return A


def null_vectors(A, rng=None):
    """The right singular vector of the smallest singular value of every 4 x 4 (fp64; a non-finite system gives NaN); rng: the entries moved at the 1e-13 relative level."""
    A = np.asarray(A, F64)
    if rng is not None:
        A = A*(1.0 + 1e-13*rng.uniform(-1.0, 1.0, A.shape))
    v = np.full((len(A), 4), np.nan); ok = np.isfinite(A).all(axis=(1, 2))
    if ok.any():
        v[ok] = np.linalg.svd(A[ok])[2][:, 3, :]
    return v


def points_of(v):
    """p4d (the float 4-vector) /= p4d(3): the reciprocal in double rounded to float, one float product per entry; rho = 1.0/(double)z."""
    v4 = np.asarray(v, F64).astype(F32)
    with np.errstate(**_ERR):
        r = (1.0/v4[:, 3].astype(F64)).astype(F32)
        X = (v4[:, :3]*r[:, None]).astype(F32)
        rho = 1.0/X[:, 2].astype(F64)
    assert X.dtype == F32
    return X, rho


def triangulate(w, rng=None):
    return points_of(null_vectors(system(w), rng))


# ---- rays, solve, score (tracking.cc:1870-1917)
def features(w, rho):
    """The five doubles SolveTheta reads of every feature: ray x, ray y, rho, target x, target y."""
    fx, fy, cx, cy = [float(v) for v in w["K"]]
    h = np.asarray(w["host_xy"], F32).reshape(-1, 2).astype(F64); t = np.asarray(w["targ_xy"], F32).reshape(-1, 2).astype(F64)
    with np.errstate(**_ERR):
        return np.column_stack([(h[:, 0] - cx)/fx, (h[:, 1] - cy)/fy, np.asarray(rho, F64), t[:, 0], t[:, 1]]).reshape(-1, 5)


def solve(m1, m2, m3):
    """:1883-1892 as written; works on Python floats and on numpy arrays alike."""
    A = m3[1]/m3[0]
    B = 1.0/m3[0]
    C = (1.0 - m2[0]*B)/(m2[1] - m2[0]*A)
    D = (((A*C - B)*m1[0]) - C*m1[1]) + 1.0
    rho3pie = m3[2]/m3[0]
    rho2pie = (m2[2] - rho3pie*m2[0])/(m2[1] - m2[0]*A)
    rho1pie = (m1[2] - rho3pie*m1[0]) - rho2pie*(m1[1] - A*m1[0])
    th2 = rho1pie/D
    th1 = rho2pie - C*th2
    th0 = (rho3pie - A*th1) - B*th2
    return th0, th1, th2


def chi_of(T, K, th, f):
    """One feature's chiSquare2 under theta (:1897-1904); Eigen's fixed-size products left to right."""
    fx, fy, cx, cy = K; m0, m1 = f[0], f[1]
    rhoPred = (m0*th[0] + m1*th[1]) + 1.0*th[2]
    inv = 1.0/rhoPred
    P0 = ((T[0]*m0 + T[1]*m1) + T[2]*1.0)*inv + T[3]
    P1 = ((T[4]*m0 + T[5]*m1) + T[6]*1.0)*inv + T[7]
    P2 = ((T[8]*m0 + T[9]*m1) + T[10]*1.0)*inv + T[11]
    u = P0/P2*fx + cx; v = P1/P2*fy + cy
    eu = f[3] - u; ev = f[4] - v
    return eu*eu + ev*ev


def _div(a, b):
    """IEEE division on Python floats (Python raises where the processor gives inf or NaN)."""
    with np.errstate(**_ERR):
        return float(F64(a)/F64(b))


class _Ieee(float):
    """A Python float whose division follows IEEE 754: everything else is Python's own double arithmetic."""
    def __truediv__(self, o): return _Ieee(_div(self, o))
    def __rtruediv__(self, o): return _Ieee(_div(o, self))
    def __mul__(self, o): return _Ieee(float.__mul__(self, o))
    __rmul__ = __mul__
    def __add__(self, o): return _Ieee(float.__add__(self, o))
    __radd__ = __add__
    def __sub__(self, o): return _Ieee(float.__sub__(self, o))
    def __rsub__(self, o): return _Ieee(float.__rsub__(self, o))
    def __neg__(self): return _Ieee(float.__neg__(self))


def hypothesis_scalar(T, K, F, tri):
    """One hypothesis over a plane's features F [n, 5], scalar by scalar: (score, the NEGATED theta)."""
    T = [_Ieee(x) for x in T]; K = [_Ieee(x) for x in K]; F = [[_Ieee(x) for x in row] for row in F]
    th = solve(F[tri[0]], F[tri[1]], F[tri[2]])
    score = 0.0
    for f in F:
        chi = chi_of(T, K, th, f)
        if chi > TH:
            continue
        score = float(score) + float(TH - chi)
    return float(score), [float(-th[0]), float(-th[1]), float(-th[2])]


def hypotheses(T, K, F, tri):
    """Every hypothesis of a plane: hyp_score [H], hyp_theta [H, 3] (negated).  Vectorised over the hypotheses, the features in index order."""
    T = [F64(x) for x in T]; K = [F64(x) for x in K]; F = np.asarray(F, F64).reshape(-1, 5); tri = np.asarray(tri, np.int64).reshape(-1, 3)
    with np.errstate(**_ERR):
        m = [[F[tri[:, j], k] for k in range(3)] for j in range(3)]
        th = solve(m[0], m[1], m[2])
        score = np.zeros(len(tri))
        for f in F:
            chi = chi_of(T, K, th, f)
            score = np.where(chi > TH, score, score + (TH - chi))
        return score, np.column_stack([-th[0], -th[1], -th[2]]).reshape(-1, 3)


def select(score):
    """:1712-1725: `BestScore < score` from -1.0 in hypothesis order."""
    best, idx = -1.0, -1
    for i, s in enumerate(np.asarray(score, F64).tolist()):
        if best < s:
            best, idx = s, i
    return idx


def run(w, rho=None, rng=None):
    """The call's outputs.  rho None: w['rho'] when the world gives it (the initializer's path), the triangulation otherwise."""
    off = np.asarray(w["off"], np.int64); hoff = np.asarray(w["hyp_off"], np.int64); P = len(off) - 1; N, H = int(off[-1]), int(hoff[-1])
    given = rho if rho is not None else w.get("rho")
    if given is None:
        p3d, rho_used = triangulate(w, rng) if N else (np.zeros((0, 3), F32), np.zeros(0))
    else:
        p3d, rho_used = np.zeros((N, 3), F32), np.asarray(given, F64).copy()
    F = features(w, rho_used); T = np.asarray(w["Tcr"], F64).reshape(12); tri = np.asarray(w["triple"], np.int64).reshape(-1, 3)
    hs, ht = np.zeros(H), np.zeros((H, 3)); sel = np.full(P, -1, np.int32); theta = np.zeros((P, 3)); score = np.zeros(P)
    for p in range(P):
        a, b, h0, h1 = off[p], off[p + 1], hoff[p], hoff[p + 1]
        assert b - a <= MAX_FEAT
        if b - a < 3 or h1 == h0:
            continue
        assert ((tri[h0:h1] >= 0) & (tri[h0:h1] < b - a)).all()
        hs[h0:h1], ht[h0:h1] = hypotheses(T, w["K"], F[a:b], tri[h0:h1])
        k = select(hs[h0:h1]); sel[p] = k
        if k >= 0:
            theta[p] = ht[h0 + k]; score[p] = hs[h0 + k]
    return dict(sel=sel, theta=theta, score=score, p3d=p3d, rho=rho_used, hyp_score=hs, hyp_theta=ht)


# ---- comparisons
def same64(a, b):
    """Equal as bit patterns (-0.0 is not 0.0), NaNs in the same places (a NaN's sign and payload are the processor's)."""
    a = np.ascontiguousarray(a, F64); b = np.ascontiguousarray(b, F64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def same32(a, b):
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def same_answer(got, ref, keys=("sel", "theta", "score", "hyp_score", "hyp_theta", "rho")):
    return all(np.array_equal(got[k], ref[k]) if k == "sel" else same64(got[k], ref[k]) for k in keys)


def sensitivity(w, draws=3):
    """How far the 4 x 4's entries moved at the 1e-13 relative level move the point: per feature the largest |X' - X| / max|X| in fp64 (before any rounding), and the
    largest movement of the float point in float steps."""
    A = system(w); v = null_vectors(A); X, _ = points_of(v)
    with np.errstate(**_ERR):
        X64 = v[:, :3]/v[:, 3:4]
        rel = np.zeros(len(A)); ulp = np.zeros(len(A), np.int64)
        for k in range(draws):
            v2 = null_vectors(A, np.random.default_rng(1000 + k)); Y, _ = points_of(v2)
            rel = np.maximum(rel, np.abs(v2[:, :3]/v2[:, 3:4] - X64).max(axis=1)/np.abs(X64).max(axis=1))
            ulp = np.maximum(ulp, np.abs(_ordered(X) - _ordered(Y)).max(axis=1))
    return dict(rel=rel, ulp=ulp)


def _ordered(a):
    i = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.int64)
    return np.where(i & 0x80000000, 0x80000000 - i, i)


def conditions_hold(w):
    """The condition of the full comparison: every triangulated float point is finite and does not move under the sensitivity probe."""
    if w.get("rho") is not None or int(np.asarray(w["off"])[-1]) == 0:
        return True
    X, _ = triangulate(w)
    return bool(np.isfinite(X).all() and (sensitivity(w)["ulp"] == 0).all())


# ---- the worlds
K0 = (458.5, 457.25, 367.25, 248.375)                                    # cx is a float: a feature can sit at x == cx exactly


def draw_triples(n, H, rng):
    """tool::GetRANSACIdx (src/tool.cc:1366-1390): the available list refilled for every hypothesis; randi uniform in [0, size - 1], swap with the back, pop."""
    out = np.zeros((H, 3), np.int32)
    for h in range(H):
        avail = list(range(n))
        for j in range(3):
            r = int(rng.integers(0, len(avail))); out[h, j] = avail[r]; avail[r] = avail[-1]; avail.pop()
    return out


def motion(rng, baseline=0.25):
    """A keyframe-to-frame motion: about 3 degrees, a baseline of about 0.25 mostly sideways."""
    a = rng.normal(0, 0.03, 3); th = np.linalg.norm(a); k = a/th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th)*Kx + (1 - np.cos(th))*(Kx @ Kx)
    t = np.array([baseline, 0.0, 0.0]) + rng.normal(0, 0.03, 3)
    return np.column_stack([R, t])


def plane_features(rng, n, T, K, noise=0.3, outliers=0.25):
    """n features of one text plane at depth about 3: host pixels in a 160 x 60 box, rho = a m0 + b m1 + c, the targets with `noise` px and `outliers` displaced by
    5 - 30 px.  Returns host [n, 2], targ [n, 2] float32, the un-negated true theta, the inlier mask and the disparity |target - target at infinity| in pixels."""
    fx, fy, cx, cy = K
    x0 = rng.uniform(60, 500); y0 = rng.uniform(60, 380)
    host = np.column_stack([rng.uniform(x0, x0 + 160, n), rng.uniform(y0, y0 + 60, n)]).astype(F32)
    th = np.array([rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08), 1/3.0 + rng.uniform(-0.03, 0.03)])
    m = np.column_stack([(host[:, 0].astype(F64) - cx)/fx, (host[:, 1].astype(F64) - cy)/fy, np.ones(n)])
    rho = m @ th
    proj = lambda X: np.column_stack([X[:, 0]/X[:, 2]*fx + cx, X[:, 1]/X[:, 2]*fy + cy])
    clean = proj((m/rho[:, None]) @ T[:, :3].T + T[:, 3]); far = proj(m @ T[:, :3].T)
    inl = np.ones(n, bool); inl[rng.permutation(n)[:int(round(outliers*n))]] = False
    targ = clean + rng.normal(0, noise, (n, 2))
    ang = rng.uniform(0, 2*np.pi, n); rad = rng.uniform(5, 30, n)
    targ[~inl] += np.column_stack([np.cos(ang), np.sin(ang)])[~inl]*rad[~inl, None]
    return host, targ.astype(F32), th, inl, np.linalg.norm(clean - far, axis=1)


def batch_world(seed, sizes, hyps, K=K0, noise=0.3, outliers=0.25):
    """A keyframe's planes: sizes[p] features and hyps[p] hypotheses each.  A plane of fewer than 3 features draws (0, n - 1, 0) triples."""
    rng = np.random.default_rng(seed); T = motion(rng)
    host, targ, truth, inl, disp, tri = [], [], [], [], [], []
    for n, H in zip(sizes, hyps):
        h, t, th, i, d = plane_features(rng, n, T, K, noise, outliers)
        host.append(h); targ.append(t); truth.append(th); inl.append(i); disp.append(d)
        tri.append(draw_triples(n, H, rng) if n >= 3 else np.tile(np.array([[0, n - 1, 0]], np.int32), (H, 1)))
    cat = lambda xs, dt, tail: np.concatenate(xs).astype(dt) if xs else np.zeros((0,) + tail, dt)
    return dict(off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), hyp_off=np.concatenate([[0], np.cumsum(hyps)]).astype(np.int32),
                host_xy=cat(host, F32, (2,)), targ_xy=cat(targ, F32, (2,)), triple=cat(tri, np.int32, (3,)).reshape(-1, 3), Tcr=T, K=np.array(K, F64),
                truth=np.array(truth), inlier=cat(inl, bool, ()), disparity=cat(disp, F64, ()), rho=None)


_MIXED = ([8, 63, 2, 64, 65, 20, 257, 3, 12], [64, 65, 5, 200, 257, 0, 1, 64, 200])      # one plane of 2 features, one without hypotheses
_B33 = ([8 + (7*i) % 63 for i in range(33)], [200 if i % 5 else 1 + (64*i) % 257 for i in range(33)])
WORLDS = {
    "n3_h1": (11, [3], [1]), "n3_h64": (12, [3], [64]), "n8_h64": (13, [8], [64]), "n63_h65": (14, [63], [65]), "n64_h200": (15, [64], [200]),
    "n65_h257": (16, [65], [257]), "n257_h200": (17, [257], [200]), "n1024_h64": (18, [1024], [64]), "n20_h200": (19, [20], [200]), "n60_h200": (20, [60], [200]),
    "mixed_9": (21,) + _MIXED, "batch_33": (22,) + _B33,
}
ALL = list(WORLDS)
GIVEN = ["init_9"]                                                       # the initializer's path: rho given (the triangulated rho of mixed_9 rounded through float)


@functools.lru_cache(maxsize=None)
def _make(name):
    if name == "init_9":
        w = dict(_make("mixed_9")); w["rho"] = answer("mixed_9")["rho"].astype(F32).astype(F64)
        return w
    seed, sizes, hyps = WORLDS[name]
    return batch_world(seed, sizes, hyps)


def make(name):
    """A committed world (shared, read-only)."""
    return _make(name)


@functools.lru_cache(maxsize=None)
def answer(name):
    return run(make(name))


def plane_world(w, p):
    """Plane p of a batch as a world of its own."""
    a, b, h0, h1 = int(w["off"][p]), int(w["off"][p + 1]), int(w["hyp_off"][p]), int(w["hyp_off"][p + 1])
    out = dict(w, off=np.array([0, b - a], np.int32), hyp_off=np.array([0, h1 - h0], np.int32), host_xy=w["host_xy"][a:b], targ_xy=w["targ_xy"][a:b],
               triple=w["triple"][h0:h1], truth=w["truth"][p:p + 1], inlier=w["inlier"][a:b], disparity=w["disparity"][a:b])
    out["rho"] = None if w.get("rho") is None else w["rho"][a:b]
    return out

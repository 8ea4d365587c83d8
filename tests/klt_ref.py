"""CPU restatement of tsframe_klt_track (pyramidal Lucas-Kanade as docs/klt_recalled.md states it: exact integer window sums rounded once to
fp32, every later operation one fp32 operation in the written order), and the numpy-only synthetic image pairs its tests use.

The restatement is written from docs/klt_recalled.md alone.  It is slow (one Python loop per point) and meant for tests and diagnostics only.
`track` also records why every level loop of every point ended, so that a fixture can show which branches it reaches."""
import numpy as np

F = np.float32
FLT_EPSILON = np.finfo(np.float32).eps
# why a level ended: the window of I out of range; flat patch / singular matrix; the window of J out of range; |delta|^2 <= eps^2;
# the oscillation rule; the iteration cap
RANGE_I, MINEIG, RANGE_J, EPS, OSC, CAP = "range_I", "min_eig", "range_J", "eps", "osc", "cap"


# ------------------------------------------------------------------------------------------------ planes
def r101(p, n):
    """BORDER_REFLECT_101 of integer indices."""
    p = np.asarray(p).copy()
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2*n - 2 - p, p)


def pyrdown(img):
    """cv::pyrDown (8U): [1 4 6 4 1] x [1 4 6 4 1], REFLECT_101, (sum + 128) >> 8."""
    h, w = img.shape
    dh, dw = (h + 1)//2, (w + 1)//2
    k = np.array([1, 4, 6, 4, 1], np.int32)
    xs = r101(2*np.arange(dw)[:, None] - 2 + np.arange(5)[None], w)
    ys = r101(2*np.arange(dh)[:, None] - 2 + np.arange(5)[None], h)
    t = (img.astype(np.int32)[:, xs]*k).sum(-1)
    s = (t[ys, :]*k[None, :, None]).sum(1)
    return ((s + 128) >> 8).astype(np.uint8)


def build_pyramid(img, win=21, max_level=3):
    """Levels 0 .. L, L <= max_level: level l is dropped with all coarser ones if its width or height is <= win."""
    img = np.ascontiguousarray(img, np.uint8)
    assert img.shape[0] > win and img.shape[1] > win
    pyr = [img]
    for _ in range(max_level):
        nxt = pyrdown(pyr[-1])
        if nxt.shape[1] <= win or nxt.shape[0] <= win:
            break
        pyr.append(nxt)
    return pyr


def scharr(img):
    """dx = S(x+1, y) - S(x-1, y), S = 3 I(y-1) + 10 I(y) + 3 I(y+1); dy the transpose rule; REFLECT_101; exact in int16."""
    h, w = img.shape
    I = img.astype(np.int32)
    ym, yp = r101(np.arange(h) - 1, h), r101(np.arange(h) + 1, h)
    xm, xp = r101(np.arange(w) - 1, w), r101(np.arange(w) + 1, w)
    S = 3*I[ym] + 10*I + 3*I[yp]
    T = 3*I[:, xm] + 10*I + 3*I[:, xp]
    return (S[:, xp] - S[:, xm]).astype(np.int16), (T[yp] - T[ym]).astype(np.int16)


# ------------------------------------------------------------------------------------------------ one point
def _in_range(x, y, win, w, h):
    """The range test in fp32, before any integer conversion; None when it fails."""
    if not (np.isfinite(x) and np.isfinite(y)) or not (abs(x) < F(1 << 20) and abs(y) < F(1 << 20)):
        return None
    fx, fy = np.floor(F(x)), np.floor(F(y))
    if fx < F(-win) or fx >= F(w) or fy < F(-win) or fy >= F(h):
        return None
    return int(fx), int(fy)


def _weights(a, b):
    s = F(1 << 14)
    one = F(1)
    iw00 = int(np.rint(F(F(F(one - a)*F(one - b))*s)))                 # cvRound: half to even
    iw01 = int(np.rint(F(F(a*F(one - b))*s)))
    iw10 = int(np.rint(F(F(F(one - a)*b)*s)))
    return iw00, iw01, iw10, (1 << 14) - iw00 - iw01 - iw10


def _blend(P, w4, shift):
    v = P[:-1, :-1]*w4[0] + P[:-1, 1:]*w4[1] + P[1:, :-1]*w4[2] + P[1:, 1:]*w4[3]
    return (v + (1 << (shift - 1))) >> shift                           # arithmetic shift (int64)


def _window_img(img, ix, iy, win, w4):
    h, w = img.shape
    xs = r101(ix + np.arange(win + 1), w); ys = r101(iy + np.arange(win + 1), h)
    return _blend(img[np.ix_(ys, xs)].astype(np.int64), w4, 9)


def _window_der(d, ix, iy, win, w4):
    h, w = d.shape
    xs = ix + np.arange(win + 1); ys = iy + np.arange(win + 1)
    okx = (xs >= 0) & (xs < w); oky = (ys >= 0) & (ys < h)
    P = np.zeros((win + 1, win + 1), np.int64)
    P[np.ix_(oky, okx)] = d[np.ix_(ys[oky], xs[okx])]
    return _blend(P, w4, 14)


def _fl(s):
    """An exact integer sum (below 2^45: exact in fp64) rounded once to fp32."""
    return F(np.float64(int(s)))


def track(pyrI, pyrJ, pts, win=21, max_iter=30, eps=0.01, min_eig=1e-4, der=None):
    """Returns (next_xy float32 [n, 2], status uint8 [n], info): info[i] = [(level, reason, iterations)] from the coarsest level down."""
    assert win % 2 == 1 and 3 <= win <= 31 and 1 <= max_iter <= 100 and eps >= 0
    assert len(pyrI) == len(pyrJ) and all(a.shape == b.shape for a, b in zip(pyrI, pyrJ))
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    der = [scharr(x) for x in pyrI] if der is None else der
    nl = len(pyrI)
    half = F((win - 1)//2)
    eps2 = F(F(eps)*F(eps)); min_eig = F(min_eig)
    SC = F(1.0/(1 << 20))
    out = pts.copy(); status = np.ones(len(pts), np.uint8); info = [[] for _ in pts]
    for k, p in enumerate(pts):
        if not (np.isfinite(p[0]) and np.isfinite(p[1])):
            status[k] = 0                                             # out[k] stays the input, bit for bit
            continue
        nx = ny = F(0)
        for lv in range(nl - 1, -1, -1):
            I, J = pyrI[lv], pyrJ[lv]; dX, dY = der[lv]; h, w = I.shape
            sc = F(1.0/(1 << lv))
            px, py = F(p[0]*sc), F(p[1]*sc)
            if lv == nl - 1:
                nx, ny = px, py
            else:
                nx, ny = F(nx*F(2)), F(ny*F(2))
            ox, oy = nx, ny
            px, py = F(px - half), F(py - half)
            ip = _in_range(px, py, win, w, h)
            if ip is None:
                if lv == 0:
                    status[k] = 0
                info[k].append((lv, RANGE_I, 0))
                continue
            ix, iy = ip
            w4 = _weights(F(px - F(ix)), F(py - F(iy)))
            Iw = _window_img(I, ix, iy, win, w4); Ix = _window_der(dX, ix, iy, win, w4); Iy = _window_der(dY, ix, iy, win, w4)
            A11 = F(_fl((Ix*Ix).sum())*SC); A12 = F(_fl((Ix*Iy).sum())*SC); A22 = F(_fl((Iy*Iy).sum())*SC)
            D = F(F(A11*A22) - F(A12*A12))
            dd = F(A11 - A22)
            me = F(F(F(A22 + A11) - np.sqrt(F(F(dd*dd) + F(F(F(4)*A12)*A12))))/F(2*win*win))
            if me < min_eig or D < FLT_EPSILON:
                if lv == 0:
                    status[k] = 0
                info[k].append((lv, MINEIG, 0))
                continue
            D = F(F(1)/D)
            nx, ny = F(nx - half), F(ny - half)
            pdx = pdy = F(0)
            reason, j = CAP, 0
            for j in range(max_iter):
                jp = _in_range(nx, ny, win, w, h)
                if jp is None:
                    if lv == 0:
                        status[k] = 0
                    reason = RANGE_J
                    break
                jx, jy = jp
                w4 = _weights(F(nx - F(jx)), F(ny - F(jy)))
                diff = _window_img(J, jx, jy, win, w4) - Iw
                b1 = F(_fl((diff*Ix).sum())*SC); b2 = F(_fl((diff*Iy).sum())*SC)
                dx = F(F(F(A12*b2) - F(A22*b1))*D); dy = F(F(F(A12*b1) - F(A11*b2))*D)
                nx, ny = F(nx + dx), F(ny + dy)
                ox, oy = F(nx + half), F(ny + half)
                if F(F(dx*dx) + F(dy*dy)) <= eps2:
                    reason = EPS
                    break
                if j > 0 and abs(F(dx + pdx)) < F(0.01) and abs(F(dy + pdy)) < F(0.01):
                    ox, oy = F(ox - F(dx*F(0.5))), F(oy - F(dy*F(0.5)))
                    reason = OSC
                    break
                pdx, pdy = dx, dy
            info[k].append((lv, reason, j + (0 if reason == RANGE_J else 1)))
            nx, ny = ox, oy
        out[k] = (ox, oy)
        if status[k] and _in_range(F(ox - half), F(oy - half), win, pyrJ[0].shape[1], pyrJ[0].shape[0]) is None:
            status[k] = 0
            info[k].append((0, RANGE_J, 0))
    return out, status, info


def track_images(A, B, pts, win=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4):
    """cv::calcOpticalFlowPyrLK(A, B, pts) as restated: builds both pyramids by the level rule, then `track`."""
    return track(build_pyramid(A, win, max_level), build_pyramid(B, win, max_level), pts, win, max_iter, eps, min_eig)


# ------------------------------------------------------------------------------------------------ synthetic pairs (numpy only)
def gaussian_blur(img, sigma):
    """Separable Gaussian, truncated at 4 sigma, symmetric border."""
    r = int(4.0*sigma + 0.5)
    k = np.exp(-0.5*(np.arange(-r, r + 1)/sigma)**2); k /= k.sum()
    a = np.pad(np.asarray(img, np.float64), r, mode="symmetric")
    t = np.zeros((img.shape[0], a.shape[1]))
    for i in range(2*r + 1):
        t += k[i]*a[i:i + img.shape[0], :]
    o = np.zeros(img.shape)
    for i in range(2*r + 1):
        o += k[i]*t[:, i:i + img.shape[1]]
    return o


def bilinear(img, xs, ys):
    """Bilinear samples of a float image at (xs, ys); coordinates are clamped to the image."""
    h, w = img.shape
    xs = np.clip(xs, 0.0, w - 1.0); ys = np.clip(ys, 0.0, h - 1.0)
    x0 = np.minimum(np.floor(xs).astype(np.int64), w - 2); y0 = np.minimum(np.floor(ys).astype(np.int64), h - 2)
    a = xs - x0; b = ys - y0
    return (1 - a)*(1 - b)*img[y0, x0] + a*(1 - b)*img[y0, x0 + 1] + (1 - a)*b*img[y0 + 1, x0] + a*b*img[y0 + 1, x0 + 1]


_BASE = {}


def _base(seed):
    if seed not in _BASE:
        from textslam_amd.orbextractor import synthetic_frame
        _BASE[seed] = gaussian_blur(synthetic_frame(seed, 800, 640).astype(np.float64), 1.0)
    return _BASE[seed]


def _u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def pair(M, t, seed=7, w=640, h=480, scale=1.0):
    """Two w x h views of one blurred synthetic scene: a point p of A appears in B at M p + t (ground truth).  scale > 1 looks at the scene from
    further away (a small image of the same content)."""
    base = _base(seed)
    M = np.asarray(M, np.float64); t = np.asarray(t, np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    A = _u8(bilinear(base, 80.0 + scale*xx, 80.0 + scale*yy))
    Mi = np.linalg.inv(M)
    xa = Mi[0, 0]*(xx - t[0]) + Mi[0, 1]*(yy - t[1]); ya = Mi[1, 0]*(xx - t[0]) + Mi[1, 1]*(yy - t[1])
    B = _u8(bilinear(base, 80.0 + scale*xa, 80.0 + scale*ya))
    return A, B


PAIRS = [("shift_3.3_-2.6", np.eye(2), (3.3, -2.6)), ("shift_14.25_9.5", np.eye(2), (14.25, 9.5)),
         ("affine", np.array([[1.02, 0.015], [-0.015, 1.02]]), (-9.0, 4.0))]


def interior_points(A, win=21, cell=40, seed=1):
    """The strongest Scharr response of every cell x cell block whose window (and its bilinear tap) is fully inside, at a random sub-pixel offset."""
    h, w = A.shape
    dx, dy = scharr(A)
    resp = np.abs(dx.astype(np.int32)) + np.abs(dy.astype(np.int32))
    rng = np.random.default_rng(seed)
    m = (win - 1)//2 + 2
    pts = []
    for gy in range(cell, h - cell - m + 1, cell):
        for gx in range(cell, w - cell - m + 1, cell):
            blk = resp[gy:gy + cell, gx:gx + cell]
            j = np.unravel_index(blk.argmax(), blk.shape)
            pts.append((gx + j[1] + rng.uniform(-.5, .5), gy + j[0] + rng.uniform(-.5, .5)))
    return np.array(pts, np.float32)


def fixture():
    """The calls the GPU test replays: a list of dicts (name, A, B, pts, win, max_level, max_iter, eps, min_eig, kinds).  kinds[i] says what
    point i is there for; test_klt_ref.test_fixture_covers_the_cases counts what the restatement does with them."""
    M, t = PAIRS[1][1], PAIRS[1][2]
    A, B = pair(M, t)
    A = A.copy(); B = B.copy()
    A[200:280, 300:380] = 100; B[200:280, 300:380] = 100               # a flat patch in both views
    rng = np.random.default_rng(5)
    pts, kinds = [], []

    def add(kind, p):
        pts.append(p); kinds.append(kind)
    for p in interior_points(A)[::2]:
        add("interior", p)
    for _ in range(48):                                               # within 10 px of the border: the window crosses it
        side = rng.integers(4)
        add("border", [(rng.uniform(0, 9), rng.uniform(0, 479)), (rng.uniform(630, 639), rng.uniform(0, 479)),
                       (rng.uniform(0, 639), rng.uniform(0, 9)), (rng.uniform(0, 639), rng.uniform(470, 479))][side])
    for i, y in enumerate((35.5, 77.0, 120.25, 166.5, 233.0, 301.75, 350.0, 388.5, 441.0)):   # the shift carries these past the right / lower edge
        add("leaves", (637.0 + 0.3*i, y))
    for i, x in enumerate((50.5, 131.0, 220.0, 290.5, 415.25, 500.0, 577.75)):
        add("leaves", (x, 476.5 + 0.4*i))
    add("flat", (340.0, 240.0)); add("flat", (337.3, 243.6)); add("flat", (345.5, 236.25))
    add("out_level0_only", (-15.0, 100.0)); add("out_level0_only", (200.0, -14.5))
    add("out_coarse_too", (-40.0, 100.0)); add("out_coarse_too", (700.0, 500.0)); add("out_coarse_too", (1.0e7, 3.0)); add("out_coarse_too", (5.0, -3.0e6))
    add("non_finite", (np.nan, 5.0)); add("non_finite", (np.inf, -np.inf)); add("non_finite", (17.0, np.nan))
    pts = np.array(pts, np.float32)
    dflt = dict(win=21, max_level=3, max_iter=30, eps=0.01, min_eig=1e-4)
    calls = [dict(dflt, name="main", A=A, B=B, pts=pts, kinds=kinds)]
    sub = [i for i, k in enumerate(kinds) if k != "interior" or i % 3 == 0]
    calls.append(dict(dflt, name="win15", A=A, B=B, pts=pts[sub], kinds=[kinds[i] for i in sub], win=15))
    calls.append(dict(dflt, name="win31_level1", A=A, B=B, pts=pts[sub], kinds=[kinds[i] for i in sub], win=31, max_level=1, eps=0.03))
    calls.append(dict(dflt, name="max_iter2", A=A, B=B, pts=pts[sub], kinds=[kinds[i] for i in sub], max_iter=2))
    Ma, ta = PAIRS[2][1], PAIRS[2][2]
    A2, B2 = pair(Ma, ta)
    p2 = interior_points(A2)[1::3]
    calls.append(dict(dflt, name="affine", A=A2, B=B2, pts=p2, kinds=["interior"]*len(p2)))
    As, Bs = pair(np.eye(2), (2.4, -1.7), w=160, h=120, scale=4.0)    # 160 x 120: level 3 (20 x 15) is dropped by the size rule
    ps = np.concatenate([interior_points(As, cell=20), np.array([[3.0, 60.0], [80.0, 117.5], [-30.0, 20.0]], np.float32)])
    calls.append(dict(dflt, name="small_dropped_level", A=As, B=Bs, pts=ps, kinds=["interior"]*(len(ps) - 3) + ["border", "border", "out_coarse_too"]))
    return calls

"""CPU restatement of docs/cvorb_recalled.md: frame::FeatExtracText = cv::ORB::create()->detect on the frame masked to a detection quad and
->compute on the frame itself (OpenCV 3.3 defaults), with the document's two stand-ins (a cut keeps every tie; level-major raster order).

Written from the document, independently of the kernels (textslam_amd/csrc/tscvorb.h).  From the oracle it takes what the document allows: whole-image
FAST (oracle.orb_fast, tested against a brute-force arc test), the blur of a plane (oracle.orb_level(plane, 0, blurred=True)), fastAtan2 and the
BRIEF pattern of include/orb_pattern.h.  The cv::ORB level sizes and their resize, the mask, the Harris response, the cuts and the order are its own."""
import ctypes as C
import math
import os
import re
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import oracle                                                          # noqa: E402

F = np.float32
NLEVELS, EDGE_THRESHOLD, PATCH, HALF, FAST_TH, HARRIS_BLOCK = 8, 31, 31, 15, 20, 7
SCALE_FACTOR = float(F(1.2))                                           # cv::ORB::create(scaleFactor = 1.2f), kept in a double member


# ------------------------------------------------------------------ parameters
def level_scales():
    return np.array([F(math.pow(SCALE_FACTOR, l)) for l in range(NLEVELS)], F)


def level_sizes(w, h):
    """(width, height) per level: cvRound(cols / scale), cvRound(rows / scale), the division in fp32."""
    return [(int(np.rint(F(w) / s)), int(np.rint(F(h) / s))) for s in level_scales()]


def quotas(nfeatures):
    factor = F(1.0 / SCALE_FACTOR)
    n = F(nfeatures) * (F(1) - factor) / (F(1) - F(math.pow(float(factor), float(NLEVELS))))
    out, total = [], 0
    for _ in range(NLEVELS - 1):
        out.append(int(np.rint(F(n)))); total += out[-1]
        n = F(n) * factor
    out.append(max(nfeatures - total, 0))
    return out


_UMAX = None
_PATTERN = None


def umax():
    global _UMAX
    if _UMAX is None:
        _UMAX = [int(v) for v in oracle.orb_params()[2]]
    return _UMAX


def pattern():
    """The 256 x 4 steered-BRIEF taps of include/orb_pattern.h as fp32 (x0, y0, x1, y1)."""
    global _PATTERN
    if _PATTERN is None:
        txt = open(os.path.join(ROOT, "include", "orb_pattern.h")).read()
        body = txt[txt.index("{", txt.index("ORB_BIT_PATTERN_31")) + 1:]
        body = body[:body.index("}")]
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        body = re.sub(r"//[^\n]*", " ", body)
        v = np.array([int(t) for t in re.findall(r"-?\d+", body)], np.int32)
        assert v.size == 1024, v.size
        _PATTERN = v.reshape(256, 4).astype(F)
    return _PATTERN


# ------------------------------------------------------------------ cv::resize INTER_LINEAR, 8-bit (RECALLED V4), to an arbitrary size
def resize_linear(src, dw, dh):
    sh, sw = src.shape
    scale_x, scale_y = 1.0 / (dw / sw), 1.0 / (dh / sh)
    fx = ((np.arange(dw) + 0.5) * scale_x - 0.5).astype(F)
    sx = np.floor(fx).astype(np.int64); fx = (fx - sx.astype(F)).astype(F)
    lo, hi = sx < 0, sx >= sw - 1
    fx[lo | hi] = 0; sx[lo] = 0; sx[hi] = sw - 1
    a0 = np.rint((F(1) - fx) * F(2048)).astype(np.int64); a1 = np.rint(fx * F(2048)).astype(np.int64)
    sx1 = np.minimum(sx + 1, sw - 1)
    fy = ((np.arange(dh) + 0.5) * scale_y - 0.5).astype(F)
    sy = np.floor(fy).astype(np.int64); fy = (fy - sy.astype(F)).astype(F)
    b0 = np.rint((F(1) - fy) * F(2048)).astype(np.int64)[:, None]; b1 = np.rint(fy * F(2048)).astype(np.int64)[:, None]
    r0 = src[np.clip(sy, 0, sh - 1)].astype(np.int64); r1 = src[np.clip(sy + 1, 0, sh - 1)].astype(np.int64)
    s0 = r0[:, sx] * a0 + r0[:, sx1] * a1; s1 = r1[:, sx] * a0 + r1[:, sx1] * a1
    return ((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)


def pyramid(img):
    img = np.ascontiguousarray(img, np.uint8)
    out = [img]
    for (w, h) in level_sizes(img.shape[1], img.shape[0])[1:]:
        out.append(resize_linear(out[-1], w, h))
    return out


# ------------------------------------------------------------------ tool::GetMask: cv::fillPoly of the quad, corners truncated like cv::Point
def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _clip_line(w, h, x1, y1, x2, y2):
    right, bottom = w - 1, h - 1

    def code(x, y):
        return (x < 0) + (x > right) * 2 + (y < 0) * 4 + (y > bottom) * 8
    c1, c2 = code(x1, y1), code(x2, y2)
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int((a - y1) * (x2 - x1) / (y2 - y1)); y1 = a; c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int((a - y2) * (x2 - x1) / (y2 - y1)); y2 = a; c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int((a - x1) * (y2 - y1) / (x2 - x1)); x1 = a; c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int((a - x2) * (y2 - y1) / (x2 - x1)); x2 = a; c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def _line8(m, x1, y1, x2, y2):
    h, w = m.shape
    if not (0 <= x1 < w and 0 <= x2 < w and 0 <= y1 < h and 0 <= y2 < h):
        ok, x1, y1, x2, y2 = _clip_line(w, h, x1, y1, x2, y2)
        if not ok:
            return
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err, x, y = major - 2 * minor, x1, y1
    for _ in range(major + 1):
        if 0 <= x < w and 0 <= y < h:
            m[y, x] = 1
        neg = err < 0
        err += -2 * minor + (2 * major if neg else 0)
        if steep:
            y += sy; x += 1 if neg else 0
        else:
            x += 1; y += sy if neg else 0


def mask_quad(w, h, quad):
    """uint8 [h, w], 1 inside: the boundary by cv::LineIterator (8-connected), the interior by 16.16 fixed-point scanline spans."""
    pts = [(int(quad[k][0]), int(quad[k][1])) for k in range(4)]       # int(): truncation toward zero, as cv::Point(double, double)
    m = np.zeros((h, w), np.uint8)
    edges = []
    for k in range(4):
        (x0, y0), (x1, y1) = pts[k - 1], pts[k]
        _line8(m, x0, y0, x1, y1)
        if y0 != y1:
            top, bot = ((x0, y0), (x1, y1)) if y0 < y1 else ((x1, y1), (x0, y0))
            edges.append((top[1], bot[1], top[0] << 16, _tdiv((x1 - x0) << 16, y1 - y0)))
    if len(edges) < 2:
        return m
    y_min, y_max = min(e[0] for e in edges), max(e[1] for e in edges)
    if y_max < 0 or y_min >= h:
        return m
    for y in range(max(y_min, 0), min(y_max, h)):
        xs = sorted(e[2] + (y - e[0]) * e[3] for e in edges if e[0] <= y < e[1])
        for i in range(0, len(xs) - 1, 2):
            xa, xb = (xs[i] + 65535) >> 16, xs[i + 1] >> 16
            if xa < w and xb >= 0:
                m[y, max(xa, 0):min(xb, w - 1) + 1] = 1
    return m


# ------------------------------------------------------------------ detection
def fast_level(plane):
    """cv::FAST(20, nms) on a whole level: [n, 3] x, y, score in raster order."""
    if plane.shape[0] < 7 or plane.shape[1] < 7:
        return np.zeros((0, 3), F)
    return oracle.orb_fast(plane, FAST_TH, cap=plane.shape[0] * plane.shape[1] // 4 + 64)


def border_keep(x, y, w, h, border=EDGE_THRESHOLD):
    """KeyPointsFilter::runByImageBorder."""
    if w <= 2 * border or h <= 2 * border:
        return np.zeros(len(x), bool)
    return (x >= border) & (x < w - border) & (y >= border) & (y < h - border)


def retain_best(values, n):
    """The stand-in for KeyPointsFilter::retainBest(n): every point whose value is >= the n-th largest value (all ties); -0.f equals +0.f."""
    values = np.asarray(values) + 0                                    # (+ 0: -0.f -> +0.f)
    if n < 0 or len(values) <= n:
        return np.ones(len(values), bool)
    if n == 0:
        return np.zeros(len(values), bool)
    return values >= np.sort(values)[len(values) - n]


_HARRIS_SCALE = F(1) / (F(4 * HARRIS_BLOCK) * F(255))
_HARRIS_S4 = F(F(F(_HARRIS_SCALE * _HARRIS_SCALE) * _HARRIS_SCALE) * _HARRIS_SCALE)


def harris(plane, xs, ys):
    """HarrisResponses, blockSize 7, k = 0.04: exact integer sums, then one fp32 expression in the written order."""
    xs = np.asarray(xs, np.int64); ys = np.asarray(ys, np.int64)
    if len(xs) == 0:
        return np.zeros(0, F)
    o = np.arange(-3, 4)
    Y = ys[:, None, None] + o[None, :, None]; X = xs[:, None, None] + o[None, None, :]
    P = plane.astype(np.int64)

    def at(dy, dx):
        return P[Y + dy, X + dx]
    ix = (at(0, 1) - at(0, -1)) * 2 + (at(-1, 1) - at(-1, -1)) + (at(1, 1) - at(1, -1))
    iy = (at(1, 0) - at(-1, 0)) * 2 + (at(1, -1) - at(-1, -1)) + (at(1, 1) - at(-1, 1))
    a = (ix * ix).sum((1, 2)); b = (iy * iy).sum((1, 2)); c = (ix * iy).sum((1, 2))
    assert max(a.max(), b.max(), np.abs(c).max()) < 2 ** 31
    fa, fb, fc = a.astype(F), b.astype(F), c.astype(F)
    s = fa + fb
    return (((fa * fb - fc * fc) - (F(0.04) * s) * s) * _HARRIS_S4).astype(F)


def ic_angle(plane, x, y):
    P = plane.astype(np.int64)
    um = umax()
    m10 = sum(u * int(P[y, x + u]) for u in range(-HALF, HALF + 1))
    m01 = 0
    for v in range(1, HALF + 1):
        d = um[v]
        rp, rm = P[y + v, x - d:x + d + 1], P[y - v, x - d:x + d + 1]
        u = np.arange(-d, d + 1)
        m10 += int((u * (rp + rm)).sum()); m01 += v * int((rp - rm).sum())
    L = oracle.orb_lib()
    return F(L.tsorb_oracle_atan2(C.c_float(float(m01)), C.c_float(float(m10))))


def describe(blur, cx, cy, angle):
    rad = F(angle) * F(math.pi / float(F(180.0)))
    a, b = F(math.cos(float(rad))), F(math.sin(float(rad)))
    pt = pattern()
    x0, y0, x1, y1 = pt[:, 0], pt[:, 1], pt[:, 2], pt[:, 3]
    t0 = blur[cy + np.rint(x0 * b + y0 * a).astype(np.int64), cx + np.rint(x0 * a - y0 * b).astype(np.int64)]
    t1 = blur[cy + np.rint(x1 * b + y1 * a).astype(np.int64), cx + np.rint(x1 * a - y1 * b).astype(np.int64)]
    return np.packbits((t0 < t1).reshape(32, 8), axis=1, bitorder="little").reshape(32)


def detect(masked, nfeatures, stats=None):
    """cv::ORB detect on one (masked) image -> [k, 6] x, y, size, angle, response, octave; level-major, raster order inside a level."""
    q = quotas(nfeatures)
    sc = level_scales()
    out = []
    for l, plane in enumerate(pyramid(masked)):
        h, w = plane.shape
        k = fast_level(plane)
        k = k[border_keep(k[:, 0], k[:, 1], w, h)]
        keep1 = retain_best(k[:, 2], 2 * q[l])
        k1 = k[keep1]
        resp = harris(plane, k1[:, 0], k1[:, 1])
        keep2 = retain_best(resp, q[l])
        if stats is not None:
            stats.append(dict(level=l, w=w, h=h, fast=len(k), quota=q[l], after1=int(keep1.sum()), after2=int(keep2.sum())))
        for (x, y, _), r in zip(k1[keep2], resp[keep2]):                # (fast_level is in raster order; the cuts keep it)
            xi, yi = int(x), int(y)
            out.append([F(xi) * sc[l], F(yi) * sc[l], F(PATCH) * sc[l], ic_angle(plane, xi, yi), r, F(l)])
    return np.array(out, F).reshape(-1, 6)


class Frame:
    """The compute side of a frame: the unmasked pyramid and its blurred copy, once."""
    def __init__(self, img):
        self.img = np.ascontiguousarray(img, np.uint8)
        self.pyr = pyramid(self.img)
        self.blur = [oracle.orb_level(p, 0, nlevels=1, blurred=True) for p in self.pyr]

    def compute(self, kp):
        h, w = self.img.shape
        keep = border_keep(kp[:, 0], kp[:, 1], w, h)                   # runByImageBorder(31) in level-0 coordinates
        assert keep.all()                                              # (the document shows that it removes nothing)
        sc = level_scales()
        desc = np.zeros((len(kp), 32), np.uint8)
        for i, k in enumerate(kp):
            l = int(k[5]); inv = F(1) / sc[l]
            desc[i] = describe(self.blur[l], int(np.rint(F(k[0]) * inv)), int(np.rint(F(k[1]) * inv)), k[3])
        return desc

    def extract(self, quads, nfeatures=500, stats=None):
        """frame::FeatExtracText: a list of (kp [k, 6], desc [k, 32]) per detection quad."""
        h, w = self.img.shape
        out = []
        for quad in np.asarray(quads, np.float64).reshape(-1, 4, 2):
            st = [] if stats is not None else None
            kp = detect(self.img * mask_quad(w, h, quad), nfeatures, st)
            if stats is not None:
                stats.append(st)
            out.append((kp, self.compute(kp)))
        return out


# ------------------------------------------------------------------ the fixture shared by tests/test_cvorb_ref.py and tests/test_gpu_text_orb.py
def fixture_image():
    """320 x 240: a 30 x 40 array of {40, 180} blocks of 8 x 8 pixels plus uniform noise in [-12, 12]."""
    rng = np.random.default_rng(3)
    blocks = rng.choice(np.array([40.0, 180.0]), size=(30, 40))
    img = np.kron(blocks, np.ones((8, 8))) + rng.uniform(-12, 12, (240, 320))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)



FULL_320 = [[0, 0], [319, 0], [319, 239], [0, 239]]
QUADS_320 = np.array([
    [[60.0, 50.0], [259.9, 50.0], [259.9, 189.0], [60.0, 189.0]],      # large, axis-aligned: 200 x 140
    [[90.3, 40.7], [270.2, 85.5], [245.8, 200.1], [70.6, 150.9]],      # rotated
    [[200.5, -30.2], [350.7, 20.0], [330.1, 160.6], [190.9, 120.3]],   # a corner (two) outside the frame
    [[2.0, 3.0], [29.5, 2.2], [28.0, 28.9], [3.3, 27.0]],              # inside the 31-px border: no keypoint
], np.float64)
QUADS_200 = np.array([
    [[10.0, 8.0], [190.0, 12.0], [185.0, 140.0], [14.0, 136.0]],
    [[70.0, 40.0], [150.5, 48.2], [140.0, 110.7], [60.2, 100.0]],
], np.float64)

_CACHE = {}


def reference(name, nfeatures):
    """The restatement's result for a fixture call, computed once per session: name = "320" (fixture_image, QUADS_320) or "200" (its top-left 200 x 150, QUADS_200)."""
    key = (name, nfeatures)
    if key not in _CACHE:
        img = fixture_image() if name == "320" else np.ascontiguousarray(fixture_image()[:150, :200])
        fkey = ("frame", name)
        if fkey not in _CACHE:
            _CACHE[fkey] = Frame(img)
        stats = []
        res = _CACHE[fkey].extract(QUADS_320 if name == "320" else QUADS_200, nfeatures, stats)
        for kp, desc in res:
            kp.setflags(write=False); desc.setflags(write=False)
        _CACHE[key] = (img, res, stats)
    return _CACHE[key]

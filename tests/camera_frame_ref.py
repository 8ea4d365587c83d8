"""CPU restatement of docs/undistort_recalled.md in numpy: cv::undistort (strips, initUndistortRectifyMap CV_16SC2, remap INTER_LINEAR /
BORDER_CONSTANT 0) and the 8-bit BGR / RGB -> grey conversion, OpenCV 3.3's non-IPP path as recalled.  Every written floating-point operation is
one IEEE fp64 operation (numpy never contracts to FMA), the accumulation along a row is np.add.accumulate (strictly left to right), and
everything after the map is integer.  Not a test module: tests/test_camera_frame_ref.py and tests/test_gpu_camera_frame.py import it."""
import numpy as np

RAW_BGR, RAW_RGB, RAW_GREY = 0, 1, 2
CHANNELS = {RAW_BGR: 3, RAW_RGB: 3, RAW_GREY: 1}
K_REF = (384.396254546, 382.825746531, 315.635886103, 249.182929809)      # the reference's indoor yaml files (640 x 480), fx fy cx cy

# the cameras of tests/test_gpu_camera_frame.py: dist = k1 k2 p1 p2 k3, K_new (None: K)
CAMERAS = {
    "zero": ((0.0, 0.0, 0.0, 0.0, 0.0), None),
    "barrel": ((-0.28, 0.07, 2e-4, -3e-4, 0.0), None),
    "pincushion": ((0.30, 0.05, -1e-3, 8e-4, 0.01), None),
    "newK": ((-0.28, 0.07, 2e-4, -3e-4, 0.0), (300.0, 300.0, 330.0, 230.0)),
}


def strip_rows(w, h):
    """U1: rows per strip of cv::undistort."""
    return min(max(1, 4096//max(w, 1)), h)


def invert3(A):
    """U2: cv::invert's closed 3 x 3 form (d = 1 / det3, every cofactor times d), row-major 9 values."""
    a = [[float(A[r][c]) for c in range(3)] for r in range(3)]
    det = a[0][0]*(a[1][1]*a[2][2] - a[1][2]*a[2][1]) - a[0][1]*(a[1][0]*a[2][2] - a[1][2]*a[2][0]) + a[0][2]*(a[1][0]*a[2][1] - a[1][1]*a[2][0])
    d = 1.0/det
    return [(a[1][1]*a[2][2] - a[1][2]*a[2][1])*d, (a[0][2]*a[2][1] - a[0][1]*a[2][2])*d, (a[0][1]*a[1][2] - a[0][2]*a[1][1])*d,
            (a[1][2]*a[2][0] - a[1][0]*a[2][2])*d, (a[0][0]*a[2][2] - a[0][2]*a[2][0])*d, (a[0][2]*a[1][0] - a[0][0]*a[1][2])*d,
            (a[1][0]*a[2][1] - a[1][1]*a[2][0])*d, (a[0][1]*a[2][0] - a[0][0]*a[2][1])*d, (a[0][0]*a[1][1] - a[0][1]*a[1][0])*d]


def _distort(x, y, K, dist):
    """U4 from the normalised x, y on: the distorted pixel u, v."""
    fx, fy, cx, cy = [float(t) for t in K]
    k1, k2, p1, p2, k3 = [float(t) for t in dist]
    x2 = x*x; y2 = y*y
    r2 = x2 + y2; _2xy = 2*x*y
    kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2)/(1 + ((0.0*r2 + 0.0)*r2 + 0.0)*r2)
    xd = x*kr + p1*_2xy + p2*(r2 + 2*x2)
    yd = y*kr + p1*(r2 + 2*y2) + p2*_2xy
    return fx*xd + cx, fy*yd + cy


def map_uv(w, h, K, dist, K_new=None):
    """U1 - U4: the fp64 source coordinates u, v [h, w] in the literal order (strips, closed inverse, serial accumulation along the row)."""
    Kn = K if K_new is None else K_new
    fxn, fyn, cxn, cyn = [float(t) for t in Kn]
    s0 = strip_rows(w, h)
    u = np.zeros((h, w)); v = np.zeros((h, w))
    for y0 in range(0, h, s0):
        rows = min(s0, h - y0)
        ir = invert3([[fxn, 0.0, cxn], [0.0, fyn, cyn - y0], [0.0, 0.0, 1.0]])
        i = np.arange(rows, dtype=np.float64)

        def chain(a, b, step):
            t = np.full((rows, w), step); t[:, 0] = i*a + b
            return np.add.accumulate(t, axis=1)
        _x = chain(ir[1], ir[2], ir[0]); _y = chain(ir[4], ir[5], ir[3]); _w = chain(ir[7], ir[8], ir[6])
        w_ = 1.0/_w
        u[y0:y0 + rows], v[y0:y0 + rows] = _distort(_x*w_, _y*w_, K, dist)
    return u, v


def map_uv_direct(w, h, K, dist, K_new=None):
    """The same coordinates without strips or accumulation: x = (j - cx') / fx', y = (i - cy') / fy' per pixel."""
    Kn = K if K_new is None else K_new
    fxn, fyn, cxn, cyn = [float(t) for t in Kn]
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return _distort((j - cxn)/fxn, (i - cyn)/fyn, K, dist)


def saturate_int(t):
    """U5: saturate_cast<int>(double): round half to even, clamped to int32; NaN gives INT_MIN."""
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(t), -2147483648.0, 2147483647.0)
    return np.where(np.isnan(r), -2147483648.0, r).astype(np.int64)


def fixed_point(u, v):
    """U5: xy int16 [h, w, 2], frac uint16 [h, w], and the 27.5 fixed-point iu, iv themselves."""
    iu = saturate_int(u*32); iv = saturate_int(v*32)
    xy = np.stack([(iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16)], -1)      # (short): wraps modulo 2^16
    frac = ((iv & 31)*32 + (iu & 31)).astype(np.uint16)
    return xy, frac, iu, iv


def undist_map(w, h, K, dist, K_new=None):
    u, v = map_uv(w, h, K, dist, K_new)
    xy, frac, _, _ = fixed_point(u, v)
    return xy, frac


def remap(img, xy, frac):
    """U6: cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) of img [h, w] or [h, w, c] uint8 through the fixed-point map."""
    src = img.reshape(img.shape[0], img.shape[1], -1).astype(np.int64)
    h, w, _ = src.shape
    sx = xy[..., 0].astype(np.int64); sy = xy[..., 1].astype(np.int64)
    a = (frac & 31).astype(np.int64); b = (frac >> 5).astype(np.int64)
    acc = np.zeros(sx.shape + (src.shape[2],), np.int64)
    for dy, dx, W in ((0, 0, (32 - a)*(32 - b)*32), (0, 1, a*(32 - b)*32), (1, 0, (32 - a)*b*32), (1, 1, a*b*32)):
        x = sx + dx; y = sy + dy
        ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        tap = np.where(ok[..., None], src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)
        acc += W[..., None]*tap
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out.reshape(xy.shape[:2] + img.shape[2:])


def grey(img, fmt):
    """U7: cvtColor BGR2GRAY / RGB2GRAY (8-bit, 14-bit coefficients); a grey image passes through."""
    if fmt == RAW_GREY:
        return img.reshape(img.shape[0], img.shape[1]).copy()
    p = img.astype(np.int64)
    B, G, R = (p[..., 0], p[..., 1], p[..., 2]) if fmt == RAW_BGR else (p[..., 2], p[..., 1], p[..., 0])
    return ((1868*B + 9617*G + 4899*R + 8192) >> 14).astype(np.uint8)


def undistort(img, K, dist, K_new=None, maps=None):
    """cv::undistort(img, K, dist, K_new); maps = (xy, frac) reuses a map built before."""
    xy, frac = maps if maps is not None else undist_map(img.shape[1], img.shape[0], K, dist, K_new)
    return remap(img, xy, frac)


def camera_frame(img, fmt, K, dist, K_new=None, maps=None):
    """What tsframe_set_raw_image computes: (undistorted image in the input's channel order, its grey)."""
    und = undistort(img, K, dist, K_new, maps)
    return und, grey(und, fmt)

"""tsframe_text_object_info (include/tsframe.h): mapText::GetObjectInfo for a keyframe's new text objects in one launch.  The reference result is
composed from the oracle's functions (frame_pyramid, musigma on the level image with the scaled corners, frame_neighbours, frame_box_pixels).
ok and mu are compared exactly, sigma at rtol 1e-11 (the tolerance musigma is held to in tests/test_gpu_parity.py: the two sides sum the squares in
different orders).  Everything that depends on mu, sigma is compared twice: bit for bit against the oracle's functions and the single calls
tsframe_neighbours / tsframe_box_pixels fed the call's own mu, sigma, and end to end against the oracle's mu, sigma at rtol 1e-10 (one division by a
sigma known to 1e-11).  The shapes are the smallest that reach every path: a 131 x 97 image whose coarsest level is 17 x 13, and a 648 x 480 one
whose level-0 mask needs two row bands."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV4 = [1.0, 0.5, 0.25, 0.125]
ERR_ARG, ERR_STATE = -1, -3
NAME = "tsframe_text_object_info"

QUADS = np.array([[(30.3, 20.7), (90.2, 35.1), (84.6, 60.9), (24.9, 45.2)],              # rotated
                  [(40.25, 30.5), (100.75, 30.5), (100.75, 52.25), (40.25, 52.25)],       # axis-aligned, fractional corners
                  [(100.5, 70.2), (150.3, 75.8), (145.1, 110.4), (95.7, 104.9)],          # partly outside the image
                  [(10.0, 8.0), (22.0, 8.0), (22.0, 88.0), (10.0, 88.0)],                 # thin: columns 1 .. 2 at level 3
                  [(50.0, 60.0), (110.0, 90.0), (110.0, 62.0), (52.0, 92.0)]])            # bow-tie corner order
NO_FEATURE = 1                                                                           # the object of the main case without any feature
OUTSIDE = np.array([(200.5, 150.0), (260.0, 150.0), (260.0, 190.5), (200.5, 190.5)])      # wholly outside a 131 x 97 image


def _img(seed, h, w):
    rng = np.random.default_rng(seed)
    base = ndimage.gaussian_filter(rng.normal(0, 1, (h, w)), 3.0)
    return np.clip(128 + 600*base + rng.normal(0, 5, (h, w)), 0, 255).astype(np.uint8)


def _bbox(quad):
    return (float(quad[:, 0].min()), float(quad[:, 1].min()), float(quad[:, 0].max()), float(quad[:, 1].max()))


def _manual_feats(oracle_lib, rng, quad, inv, pyr, per_level):
    """Features that do not come from GetPyramidPts: per level random positions around the scaled quad (some past the image border), featureInten = the
    bilinear sample (tap 0 of the INTERVAL8 neighbourhood)."""
    off, us, vs, Is = [0], [], [], []
    for l, n in enumerate(per_level):
        h, w = pyr[l][0].shape
        x0, y0, x1, y1 = [c*inv[l] for c in _bbox(quad)]
        u = rng.uniform(x0 - 3, x1 + 3, n); v = rng.uniform(y0 - 3, y1 + 3, n)
        u[::5] = np.rint(u[::5]); v[::7] = np.rint(v[::7])
        I = oracle_lib.frame_neighbours(pyr[l][0], np.stack([u, v], 1), 0.0, 1.0)[0][:, 0] if n else np.zeros(0)
        us.append(u); vs.append(v); Is.append(I); off.append(off[-1] + n)
    return {"level_off": np.array(off, np.int32), "u": np.concatenate(us), "v": np.concatenate(vs), "inten": np.concatenate(Is)}


def _zeros(a):
    return np.ascontiguousarray(a).tobytes() == bytes(a.size*a.itemsize)                 # +0.0 exactly, not -0.0


def _check(fr, oracle_lib, g, quad, f, pyr, inv, singles=True):
    """One object's result g against the oracle (and, with singles, against tsframe_neighbours / tsframe_box_pixels on fr's resident pyramid)."""
    L = len(inv)
    for l in range(L):
        img = pyr[l][0]
        ok_o, mu_o, sg_o = oracle_lib.musigma(img, quad*inv[l])
        mu, sg = float(g["statistics"][l, 0]), float(g["statistics"][l, 1])
        assert bool(g["ok"][l]) == bool(ok_o), l
        assert mu == mu_o, (l, mu, mu_o)                                                  # exact: integer sums
        np.testing.assert_allclose(sg, sg_o, rtol=1e-11, atol=0)
        a, b = int(f["level_off"][l]), int(f["level_off"][l + 1])
        uv = np.stack([f["u"][a:b], f["v"][a:b]], 1).reshape(-1, 2)
        I8, N8, inn, N = g["neighbourInten"][a:b], g["neighbourNInten"][a:b], g["IN"][a:b], g["featureNInten"][a:b]
        raw = oracle_lib.frame_neighbours(img, uv, 0.0, 1.0)
        assert I8.tobytes() == raw[0].tobytes() and inn.tobytes() == raw[2].tobytes(), l  # independent of sigma: the oracle directly
        if ok_o:
            own = oracle_lib.frame_neighbours(img, uv, mu, sg)
            assert N8.tobytes() == own[1].tobytes(), l
            assert N.tobytes() == ((f["inten"][a:b] - mu)/sg).tobytes(), l
            if singles and b > a:
                one = fr.CalNormvec(l, uv, mu, sg)
                assert I8.tobytes() == one[0].tobytes() and N8.tobytes() == one[1].tobytes() and inn.tobytes() == one[2].tobytes(), l
            np.testing.assert_allclose(N8, oracle_lib.frame_neighbours(img, uv, mu_o, sg_o)[1], rtol=1e-10, atol=0)
            np.testing.assert_allclose(N, (f["inten"][a:b] - mu_o)/sg_o, rtol=1e-10, atol=0)
        else:
            assert _zeros(N8) and _zeros(N), l
            assert sg == 0.0
    # level 0: the box pixels
    img = pyr[0][0]
    ok_o, mu_o, sg_o = oracle_lib.musigma(img, quad*inv[0])
    mu, sg = float(g["statistics"][0, 0]), float(g["statistics"][0, 1])
    p = g["vRefPixs"]
    u, v, I, N = oracle_lib.frame_box_pixels(img, quad*inv[0], mu, sg if ok_o else 1.0)
    assert p["u"].dtype == np.int32 and p["u"].tobytes() == u.tobytes() and p["v"].tobytes() == v.tobytes(), "pixel order / count"
    assert p["featureInten"].tobytes() == I.tobytes()
    if ok_o:
        assert p["featureNInten"].tobytes() == N.tobytes()
        if singles:
            one = fr.GetBoxAllPixs(0, quad*inv[0], mu, sg)
            assert all(p[k].tobytes() == one[k].tobytes() for k in ("u", "v", "featureInten", "featureNInten"))
        np.testing.assert_allclose(p["featureNInten"], oracle_lib.frame_box_pixels(img, quad*inv[0], mu_o, sg_o)[3], rtol=1e-10, atol=0)
    else:
        assert _zeros(p["featureNInten"])
    return len(u)


def _bytes(g):
    p = g["vRefPixs"]
    parts = [g["statistics"], g["ok"], g["level_off"], g["featureNInten"], g["neighbourInten"], g["neighbourNInten"], g["IN"],
             p["u"], p["v"], p["featureInten"], p["featureNInten"]]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


@pytest.fixture(scope="module")
def fr():
    from textslam_amd.frame import Frame
    return Frame(0)


@pytest.fixture(scope="module")
def main(fr, oracle_lib):
    """The main case: 131 x 97, 4 levels (the coarsest 17 x 13), five objects with features from GetPyramidPtsBatch; shared, read-only."""
    w, h = 131, 97
    img = _img(41, h, w)
    pyr = oracle_lib.frame_pyramid(img, 4)
    assert pyr[3][0].shape == (13, 17)
    rng = np.random.default_rng(42)
    sets = []
    for i, q in enumerate(QUADS):
        x0, y0, x1, y1 = _bbox(q)
        n = 0 if i == NO_FEATURE else 40 + 9*i
        xy = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], 1).astype(np.float32)
        sets.append((0, xy, (x0, y0, x1, y1)))
    fr.GetPyrMat(img, 4)
    feats = fr.GetPyramidPtsBatch(sets, INV4)
    assert len(feats[NO_FEATURE]["u"]) == 0 and all(np.diff(feats[i]["level_off"])[-1] > 0 for i in (0, 2, 3, 4))     # features on every level
    return {"img": img, "pyr": pyr, "feats": feats, "got": [dict(g) for g in fr.GetObjectInfoBatch(QUADS, INV4, feats)]}


def test_main_case_against_the_oracle_and_the_single_calls(fr, main, oracle_lib):
    fr.GetPyrMat(main["img"], 4)
    got = fr.GetObjectInfoBatch(QUADS, INV4, main["feats"])
    assert len(got) == len(QUADS)
    npix = [_check(fr, oracle_lib, g, q, f, main["pyr"], np.array(INV4)) for g, q, f in zip(got, QUADS, main["feats"])]
    assert all(n > 100 for n in npix)
    assert all(g["ok"].all() for g in got)
    # not trivial: the partly outside quad has features whose last tap is outside, the thin quad is two columns wide at level 3
    assert 0 < got[2]["IN"].sum() < len(got[2]["IN"])
    x = QUADS[3][:, 0]*INV4[3]
    assert int(x.min()) == 1 and int(x.max()) == 2


def test_objects_are_independent(fr, main):
    fr.GetPyrMat(main["img"], 4)
    fwd = main["got"]
    rev = fr.GetObjectInfoBatch(QUADS[::-1], INV4, main["feats"][::-1])
    n = len(QUADS)
    for i in range(n):
        assert _bytes(rev[n - 1 - i]) == _bytes(fwd[i]), i
        assert _bytes(fr.GetObjectInfoBatch(QUADS[i:i + 1], INV4, main["feats"][i:i + 1])[0]) == _bytes(fwd[i]), i


def test_ok_zero_constant_region_and_no_pixel(fr, main, oracle_lib):
    inv = np.array(INV4)
    rng = np.random.default_rng(43)
    # a constant image: sigma = 0 with mu kept; a quad wholly outside: no pixel, mu = sigma = 0
    img = np.full((97, 131), 90, np.uint8)
    pyr = oracle_lib.frame_pyramid(img, 4)
    quads = np.stack([QUADS[0], OUTSIDE])
    feats = [_manual_feats(oracle_lib, rng, q, inv, pyr, (30, 11, 5, 3)) for q in quads]
    fr.GetPyrMat(img, 4)
    got = fr.GetObjectInfoBatch(quads, INV4, feats)
    for g, q, f in zip(got, quads, feats):
        _check(fr, oracle_lib, g, q, f, pyr, inv)
        assert not g["ok"].any()
    assert np.all(got[0]["statistics"] == [90.0, 0.0]) and np.all(got[1]["statistics"] == 0.0)
    assert len(got[0]["vRefPixs"]["u"]) > 1000 and np.all(got[0]["vRefPixs"]["featureInten"] == 90.0) and len(got[1]["vRefPixs"]["u"]) == 0
    assert got[0]["neighbourInten"].max() > 89.0                                         # the raw values are written (bilinear weights round)
    # the same two kinds of object among the main case's, on the main image with a flat patch: the others are unaffected
    img = main["img"].copy(); img[:60, :80] = 90
    pyr = oracle_lib.frame_pyramid(img, 4)
    flat = np.array([(8.0, 8.0), (40.0, 9.0), (39.5, 30.0), (8.5, 29.0)])
    quads = np.concatenate([QUADS[:2], flat[None], QUADS[2:], OUTSIDE[None]])
    extra = [_manual_feats(oracle_lib, rng, q, inv, pyr, (25, 9, 4, 2)) for q in (flat, OUTSIDE)]
    fr.GetPyrMat(img, 4)
    sets = [(0, np.stack([rng.uniform(_bbox(q)[0], _bbox(q)[2], 30), rng.uniform(_bbox(q)[1], _bbox(q)[3], 30)], 1).astype(np.float32), _bbox(q)) for q in QUADS]
    pts = fr.GetPyramidPtsBatch(sets, INV4)
    feats = pts[:2] + extra[:1] + pts[2:] + extra[1:]
    got = fr.GetObjectInfoBatch(quads, INV4, feats)
    for g, q, f in zip(got, quads, feats):
        _check(fr, oracle_lib, g, q, f, pyr, inv, singles=False)
    assert not got[2]["ok"].any() and np.all(got[2]["statistics"] == [90.0, 0.0]) and not got[6]["ok"].any()
    assert all(got[i]["ok"].any() for i in (0, 1, 3, 4, 5))
    alone = fr.GetObjectInfoBatch(QUADS, INV4, pts)
    assert [_bytes(got[i]) for i in (0, 1, 3, 4, 5)] == [_bytes(a) for a in alone]


def test_row_bands(fr, oracle_lib):
    """648 x 480: 311 040 pixels, so level 0 goes in bands of 307200 // 648 = 474 rows from the box's first row."""
    w, h = 648, 480
    img = _img(44, h, w)
    pyr = oracle_lib.frame_pyramid(img, 2)
    inv = np.array([1.0, 0.5])
    quads = np.array([[(100.5, 2.0), (300.0, 2.5), (310.0, 478.0), (90.0, 477.5)],      # rows 2 .. 478: two bands (2 .. 475, 476 .. 478)
                      [(400.0, 100.0), (600.0, 120.0), (590.0, 200.0), (395.0, 180.0)]])   # inside one band
    assert 307200//w == 474
    rng = np.random.default_rng(45)
    feats = [_manual_feats(oracle_lib, rng, q, inv, pyr, (50, 20)) for q in quads]
    fr.GetPyrMat(img, 2)
    got = fr.GetObjectInfoBatch(quads, inv, feats)
    npix = [_check(fr, oracle_lib, g, q, f, pyr, inv) for g, q, f in zip(got, quads, feats)]
    v = got[0]["vRefPixs"]["v"]
    assert v.min() == 2 and v.max() == 478 and np.all(np.diff(v) >= 0) and (v == 475).any() and (v == 476).any()       # in order across the band edge
    assert npix[0] > 80000 and npix[1] > 10000


def test_full_image_quad_fills_the_mask(fr, oracle_lib):
    """640 x 480: a full-image quad gives 307 200 pixels, the LDS mask's exact capacity."""
    w, h = 640, 480
    img = _img(46, h, w)
    pyr = oracle_lib.frame_pyramid(img, 2)
    inv = np.array([1.0, 0.5])
    quads = np.array([[(0.0, 0.0), (639.0, 0.0), (639.0, 479.0), (0.0, 479.0)]])
    feats = [_manual_feats(oracle_lib, np.random.default_rng(47), quads[0], inv, pyr, (40, 15))]
    fr.GetPyrMat(img, 2)
    got = fr.GetObjectInfoBatch(quads, inv, feats)
    assert _check(fr, oracle_lib, got[0], quads[0], feats[0], pyr, inv) == 307200
    assert got[0]["statistics"][0, 0] == img.astype(np.int64).sum()/307200


class _Raw:
    """One raw ctypes call with sentinel-filled outputs."""

    def __init__(self, fr, quads, inv, feats, pix_cap):
        self.fr = fr
        self.L = L = len(inv)
        self.n = n = len(quads)
        self.quad = np.ascontiguousarray(quads, np.float64).copy()
        self.inv = np.array(inv, np.float64)
        self.lo = np.ascontiguousarray([f["level_off"] for f in feats], np.int32).reshape(n, L + 1)
        self.cnt = [int(r[L]) for r in self.lo]
        self.foff = np.zeros(n + 1, np.int32); self.foff[1:] = np.cumsum([max(int(r[1]), (c + L - 1)//L) for r, c in zip(self.lo, self.cnt)])       # the slices of tsframe_pyramid_pts_batch
        cap = max(1, int(self.foff[n])*L)
        self.u = np.zeros(cap); self.v = np.zeros(cap); self.I = np.zeros(cap)
        for i, f in enumerate(feats):
            b = int(self.foff[i])*L
            self.u[b:b + self.cnt[i]] = f["u"]; self.v[b:b + self.cnt[i]] = f["v"]; self.I[b:b + self.cnt[i]] = f["inten"]
        self.pix_cap = pix_cap
        self.ms = np.full((n, L, 2), -7.5); self.ok = np.full((n, L), 99, np.uint8)
        self.N = np.full(cap, -7.5); self.I8 = np.full((cap, 8), -7.5); self.N8 = np.full((cap, 8), -7.5); self.inn = np.full(cap, 99, np.uint8)
        pc = max(1, pix_cap)
        self.poff = np.full(n + 1, -77, np.int32); self.pu = np.full(pc, -77, np.int32); self.pv = np.full(pc, -77, np.int32)
        self.pI = np.full(pc, -7.5); self.pN = np.full(pc, -7.5)

    def call(self, ctx=None, n_obj=None, null=(), pix_cap=None):
        ip, dp, up = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        a = {"quad": self.quad.ctypes.data_as(dp), "inv": self.inv.ctypes.data_as(dp), "feat_off": self.foff.ctypes.data_as(ip), "level_off": self.lo.ctypes.data_as(ip),
             "u": self.u.ctypes.data_as(dp), "v": self.v.ctypes.data_as(dp), "inten": self.I.ctypes.data_as(dp),
             "musigma": self.ms.ctypes.data_as(dp), "ok": self.ok.ctypes.data_as(up), "ninten": self.N.ctypes.data_as(dp), "inten8": self.I8.ctypes.data_as(dp),
             "ninten8": self.N8.ctypes.data_as(dp), "in": self.inn.ctypes.data_as(up), "pix_off": self.poff.ctypes.data_as(ip), "pix_u": self.pu.ctypes.data_as(ip),
             "pix_v": self.pv.ctypes.data_as(ip), "pix_inten": self.pI.ctypes.data_as(dp), "pix_ninten": self.pN.ctypes.data_as(dp)}
        for k in null:
            a[k] = None
        ctx = self.fr.ctx if ctx is None else ctx
        rc = self.fr.lib.tsframe_text_object_info(ctx, self.n if n_obj is None else n_obj, a["quad"], a["inv"], a["feat_off"], a["level_off"], a["u"], a["v"], a["inten"],
                                                  self.pix_cap if pix_cap is None else pix_cap, a["musigma"], a["ok"], a["ninten"], a["inten8"], a["ninten8"], a["in"],
                                                  a["pix_off"], a["pix_u"], a["pix_v"], a["pix_inten"], a["pix_ninten"])
        return rc, self.fr.lib.tsframe_last_error(ctx).decode()

    def pix_untouched(self):
        return np.all(self.pu == -77) and np.all(self.pv == -77) and np.all(self.pI == -7.5) and np.all(self.pN == -7.5)

    def untouched(self):
        return (self.pix_untouched() and np.all(self.ms == -7.5) and np.all(self.ok == 99) and np.all(self.N == -7.5) and np.all(self.I8 == -7.5)
                and np.all(self.N8 == -7.5) and np.all(self.inn == 99) and np.all(self.poff == -77))

    def features_match(self, got):
        """The feature outputs and statistics equal the mirror's result; the slices' padding is untouched."""
        for i, g in enumerate(got):
            b = int(self.foff[i])*self.L; e = b + self.cnt[i]; z = int(self.foff[i + 1])*self.L
            if not (self.ms[i].tobytes() == g["statistics"].tobytes() and np.array_equal(self.ok[i] != 0, g["ok"]) and self.N[b:e].tobytes() == g["featureNInten"].tobytes()
                    and self.I8[b:e].tobytes() == g["neighbourInten"].tobytes() and self.N8[b:e].tobytes() == g["neighbourNInten"].tobytes()
                    and self.inn[b:e].tobytes() == g["IN"].tobytes()):
                return False
            if not (np.all(self.N[e:z] == -7.5) and np.all(self.I8[e:z] == -7.5) and np.all(self.N8[e:z] == -7.5) and np.all(self.inn[e:z] == 99)):
                return False
        return True


def test_capacity(fr, main):
    fr.GetPyrMat(main["img"], 4)
    got = main["got"]
    counts = [len(g["vRefPixs"]["u"]) for g in got]
    total = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    # one below the total: refused, pix_off complete, the pixel arrays untouched, the other outputs written
    raw = _Raw(fr, QUADS, INV4, main["feats"], total - 1)
    rc, msg = raw.call()
    assert rc == ERR_ARG and NAME in msg, (rc, msg)
    assert np.array_equal(raw.poff, off) and raw.pix_untouched() and raw.features_match(got)
    # pix_cap == 0 counts only, the pixel arrays may be NULL
    raw = _Raw(fr, QUADS, INV4, main["feats"], 0)
    rc, msg = raw.call(null=("pix_u", "pix_v", "pix_inten", "pix_ninten"))
    assert rc == 0, msg
    assert np.array_equal(raw.poff, off) and raw.pix_untouched() and raw.features_match(got)
    # the exact capacity succeeds
    raw = _Raw(fr, QUADS, INV4, main["feats"], total)
    rc, msg = raw.call()
    assert rc == 0, msg
    assert np.array_equal(raw.poff, off) and raw.features_match(got)
    for i, g in enumerate(got):
        a, b = off[i], off[i + 1]; p = g["vRefPixs"]
        assert (raw.pu[a:b].tobytes() == p["u"].tobytes() and raw.pv[a:b].tobytes() == p["v"].tobytes() and raw.pI[a:b].tobytes() == p["featureInten"].tobytes()
                and raw.pN[a:b].tobytes() == p["featureNInten"].tobytes()), i


def test_arguments(fr, main):
    from textslam_amd.frame import Frame
    fr.GetPyrMat(main["img"], 4)
    feats = main["feats"]
    CAP = 20000

    def refused(raw, code=ERR_ARG, names=None, **kw):
        rc, msg = raw.call(**kw)
        assert rc == code, (rc, msg, kw)
        assert NAME in msg, msg
        if names is not None:
            assert names in msg, msg
        assert raw.untouched(), kw

    def fresh():
        return _Raw(fr, QUADS, INV4, feats, CAP)

    # NULL pointers where data is needed
    for name in ("quad", "inv", "feat_off", "level_off", "u", "v", "inten", "musigma", "ok", "ninten", "inten8", "ninten8", "in", "pix_off",
                 "pix_u", "pix_v", "pix_inten", "pix_ninten"):
        refused(fresh(), null=(name,))
    refused(fresh(), n_obj=-1)
    refused(fresh(), pix_cap=-1)
    # feat_off
    raw = fresh(); raw.foff[0] = 1
    refused(raw)
    raw = fresh(); raw.foff[3] = raw.foff[2] - 1
    refused(raw, names="object 2")
    # level_off rows: not starting at 0, decreasing, ending above the slice
    raw = fresh(); raw.lo[2, 0] = 1
    refused(raw, names="object 2")
    raw = fresh(); raw.lo[3, 2] = raw.lo[3, 1] - 1
    refused(raw, names="object 3")
    raw = fresh(); raw.lo[4, 4] = (raw.foff[5] - raw.foff[4])*4 + 1
    refused(raw, names="object 4")
    raw = fresh(); raw.lo[NO_FEATURE, 4] = 1; raw.lo[NO_FEATURE, 3] = 1                    # an object without a slice cannot hold a feature
    refused(raw, names="object %d" % NO_FEATURE)
    # corners and inv_scale that are not finite or >= 1e9 in magnitude; u / v that are not finite
    for bad in (np.nan, np.inf, -np.inf, 1e9, -2e9):
        raw = fresh(); raw.quad[3, 2, 1] = bad
        refused(raw, names="object 3")
        raw = fresh(); raw.inv[2] = bad
        refused(raw)
    for bad in (np.nan, np.inf, -np.inf):
        raw = fresh(); raw.u[int(raw.foff[2])*4 + 5] = bad
        refused(raw, names="object 2")
        raw = fresh(); raw.v[int(raw.foff[4])*4] = bad
        refused(raw, names="object 4")
    # what lies past level_off[i][L] in a slice is not read: NaN there is no error
    raw = fresh()
    assert raw.cnt[0] < (raw.foff[1] - raw.foff[0])*4
    raw.u[raw.cnt[0]] = np.nan; raw.v[raw.cnt[0]] = np.inf
    rc, msg = raw.call()
    assert rc == 0 and raw.features_match(main["got"]), msg
    # no image: TSFRAME_ERR_STATE
    blank = Frame(0)
    refused(fresh(), code=ERR_STATE, ctx=blank.ctx)
    # n_obj == 0 with every pointer NULL
    for ctx in (fr.ctx, blank.ctx):
        assert fr.lib.tsframe_text_object_info(ctx, 0, None, None, None, None, None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None) == 0
    # objects without any feature need no feature array
    raw = _Raw(fr, QUADS[:2], INV4, [feats[NO_FEATURE], feats[NO_FEATURE]], CAP)
    rc, msg = raw.call(null=("u", "v", "inten", "ninten", "inten8", "ninten8", "in"))
    assert rc == 0 and raw.ms[1].tobytes() == main["got"][1]["statistics"].tobytes(), msg
    # after all that the context still answers the main call
    got = fr.GetObjectInfoBatch(QUADS, INV4, feats)
    assert [_bytes(g) for g in got] == [_bytes(g) for g in main["got"]]


def test_resident_planes_stay_as_they_are(fr, main):
    fr.GetPyrMat(main["img"], 4)
    before = [fr.level(l, k).tobytes() for l in range(4) for k in range(4)]
    fr.GetObjectInfoBatch(QUADS, INV4, main["feats"])
    assert [fr.level(l, k).tobytes() for l in range(4) for k in range(4)] == before
    assert before[0] == main["img"].tobytes()


def test_adapter_from_cxx(tmp_path, fr, main):
    exe = str(tmp_path / "object_info_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "object_info_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsframe", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    img = main["img"]; feats = main["feats"]
    K = np.array([[212.125/s, 209.75/s, 64.5/s, 47.25/s] for s in (1.0, 2.0, 4.0, 8.0)])
    good = [1, 1, 0, 1, 1]                                                               # detection 2 is not good: no object
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<iiii", img.shape[1], img.shape[0], 4, len(QUADS)))
        f.write(np.asarray(INV4, np.float64).tobytes()); f.write(K.tobytes()); f.write(img.tobytes())
        for i, q in enumerate(QUADS):
            f.write(struct.pack("<i", good[i])); f.write(np.ascontiguousarray(q, np.float64).tobytes())
            for l in range(4):
                a, b = int(feats[i]["level_off"][l]), int(feats[i]["level_off"][l + 1])
                f.write(struct.pack("<i", b - a))
                f.write(np.stack([feats[i]["u"][a:b], feats[i]["v"][a:b], feats[i]["inten"][a:b]], 1).reshape(-1, 3).astype(np.float64).tobytes())
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "object info from C++: ok" in res.stdout, res.stdout
    keep = [i for i in range(len(QUADS)) if good[i]]
    fr.GetPyrMat(img, 4)
    got = fr.GetObjectInfoBatch(QUADS[keep], INV4, [feats[i] for i in keep], K=K[0])      # the Python mirror
    raw = open(outp, "rb").read()
    at = 0
    tf = np.dtype([("d", "<f8", 57), ("nn", "<i4"), ("b", "u1", 2)])
    pf = np.dtype([("d", "<f8", 9), ("q", "<i4", 2), ("b", "u1", 2)])
    DX = np.array([0, 2, 1, 0, -1, -2, -1, 0], np.float64); DY = np.array([0, 0, -1, -2, -1, 0, 1, 2], np.float64)
    for g, i in zip(got, keep):
        head = np.frombuffer(raw, "<f8", 8 + 32 + 8, at); at += 8*48
        assert head[:8].tobytes() == g["statistics"].tobytes(), i
        dete = np.stack([QUADS[i]*s for s in INV4])
        assert head[8:40].tobytes() == dete.tobytes(), i                                  # vTextDete[l]
        assert head[40:].tobytes() == ((dete[0] - K[0, 2:])/K[0, :2]).tobytes(), i         # vTextDeteRay, to the bit
        for l in range(4):
            (m,) = struct.unpack_from("<i", raw, at); at += 4
            a, b = int(g["level_off"][l]), int(g["level_off"][l + 1])
            assert m == b - a, (i, l)
            rec = np.frombuffer(raw, tf, m, at); at += tf.itemsize*m
            assert g["ok"][l]
            assert np.all(rec["nn"] == 8) and np.all(rec["b"][:, 0] == 1) and np.array_equal(rec["b"][:, 1], g["IN"][a:b]), (i, l)       # INITIAL = true, IN
            assert rec["d"][:, 0].tobytes() == g["featureNInten"][a:b].tobytes(), (i, l)
            assert rec["d"][:, 1:9].tobytes() == g["neighbourInten"][a:b].tobytes() and rec["d"][:, 9:17].tobytes() == g["neighbourNInten"][a:b].tobytes(), (i, l)
            u, v = feats[i]["u"][a:b], feats[i]["v"][a:b]
            nb = np.stack([u[:, None] + DX, v[:, None] + DY], 2)                          # [m, 8, 2]
            assert rec["d"][:, 17:33].tobytes() == nb.tobytes(), (i, l)
            ray = np.concatenate([(nb - K[l, 2:])/K[l, :2], np.ones((m, 8, 1))], 2)
            assert rec["d"][:, 33:57].tobytes() == ray.tobytes(), (i, l)
        (m,) = struct.unpack_from("<i", raw, at); at += 4
        p = g["vRefPixs"]
        assert m == len(p["u"]) and m > 0, i
        rec = np.frombuffer(raw, pf, m, at); at += pf.itemsize*m
        assert np.array_equal(rec["d"][:, 0], p["u"]) and np.array_equal(rec["d"][:, 1], p["v"]) and np.array_equal(rec["d"][:, 2:4], rec["d"][:, 0:2]), i
        assert rec["d"][:, 4].tobytes() == p["featureInten"].tobytes() and rec["d"][:, 5].tobytes() == p["featureNInten"].tobytes(), i
        assert rec["d"][:, 6:9].tobytes() == p["ray"].tobytes(), i
        assert np.all(rec["q"][:, 0] == 0) and np.array_equal(rec["q"][:, 1], np.arange(m)) and np.all(rec["b"][:, 0] == 0) and np.all(rec["b"][:, 1] == 1), i
        st = struct.unpack_from("<ii", raw, at); at += 8
        n0 = int(g["level_off"][1])
        assert st == (n0, n0), i
    assert at == len(raw)

"""tsframe_text_judge: tracking::TextJudgeSingle (/root/reference/src/tracking.cc:1991-2131) for a frame's text planes in one launch -- against a
numpy restatement of the reference's four steps (sequential sums, as std::accumulate and the reference's loops have them), every branch, the
independence of a plane from its neighbours, level 1, the resident planes, argument errors, and the adapter's pack_text_judge from C++."""
import ctypes as C
import math
import os
import re
import struct
import subprocess
import numpy as np
import pytest

from textslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASS, ORIENT, DEPTH, BOX, ZNCC = 0, 1, 2, 3, 4


# ------------------------------------------------------------------------------------------------ the reference, restated
def _sample(img, pu, pv):
    """tool::GetIntenBilinterPtr: 0 outside (and at a NaN position, which the reference's int conversion sends below 0)."""
    h, w = img.shape
    with np.errstate(invalid="ignore"):
        fin = ~(np.isnan(pu) | np.isnan(pv))
        x0 = np.floor(np.where(fin, pu, -1.0)); y0 = np.floor(np.where(fin, pv, -1.0))
        x1 = np.ceil(np.where(fin, pu, -1.0)); y1 = np.ceil(np.where(fin, pv, -1.0))
        ok = fin & (x0 >= 0) & (y0 >= 0) & (x1 < w) & (y1 < h)
    xi, yi = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
    a, b = np.where(ok, pu - x0, 0.0), np.where(ok, pv - y0, 0.0)
    xr, yb = np.minimum(xi + 1, w - 1), np.minimum(yi + 1, h - 1)
    p00, p01, p10, p11 = (img[yi, xi].astype(np.float64), img[yi, xr].astype(np.float64), img[yb, xi].astype(np.float64), img[yb, xr].astype(np.float64))
    I = (1.0 - a)*(1.0 - b)*p00 + a*(1.0 - b)*p01 + (1.0 - a)*b*p10 + a*b*p11
    return np.where(ok, I, 0.0)


def _proj(th, T, r0, r1, K):
    """tool::GetProjText: (u, v, z) of the rays (r0, r1, 1)."""
    fx, fy, cx, cy = K
    invz = -(r0*th[0] + r1*th[1] + 1.0*th[2])
    X = (T[0, 0]*r0 + T[0, 1]*r1 + T[0, 2]*1.0)/invz + T[0, 3]
    Y = (T[1, 0]*r0 + T[1, 1]*r1 + T[1, 2]*1.0)/invz + T[1, 3]
    Z = (T[2, 0]*r0 + T[2, 1]*r1 + T[2, 2]*1.0)/invz + T[2, 3]
    return fx*X/Z + cx, fy*Y/Z + cy, Z


def _seq(x):
    return float(np.cumsum(x)[-1])


def _round_half_away(x):
    r = math.trunc(x)
    return r + (1 if x > 0 else -1) if abs(x - r) >= 0.5 else r


def judge_ref(cur, w0h0, th, T, ray, pu, pv, pin, K_ref, K, cos_min, margin, zncc_min, dete):
    """One plane, steps 1-4 of the reference (with the decisions of DESIGN.md: plain mean ZNCC; n <= 1 rejected with NaN; a detection centre
    outside the label image is not associated).  Returns (reason, cos, zncc, box [4, 2], dete flags or None)."""
    th = [float(x) for x in th]; T = np.asarray(T, np.float64).reshape(-1, 4)
    h, w = cur.shape
    c0, c1, c2 = float(T[2, 0]), float(T[2, 1]), float(T[2, 2])
    nv = math.sqrt(th[0]*th[0] + th[1]*th[1] + th[2]*th[2])*math.sqrt(c0*c0 + c1*c1 + c2*c2)
    with np.errstate(all="ignore"):
        cs = float(np.float64(th[0]*c0 + th[1]*c1 + th[2]*c2)/np.float64(nv))
    reason = ORIENT if abs(cs) < cos_min else PASS
    with np.errstate(all="ignore"):
        u, v, z = _proj(th, T, ray[:, 0].astype(np.float64), ray[:, 1].astype(np.float64), K)
    if reason == PASS:
        for b in range(4):
            if z[b] < 0:
                reason = DEPTH; break
            if u[b] <= margin or u[b] >= w - margin or v[b] <= margin or v[b] >= h - margin:
                reason = BOX; break
    zn = float("nan")
    if reason == PASS and zncc_min > -2.0:
        n = len(pin)
        if n >= 2:
            fx, fy, cx, cy = K_ref
            r0 = (pu.astype(np.float64) - cx)/fx; r1 = (pv.astype(np.float64) - cy)/fy
            with np.errstate(all="ignore"):
                qu, qv, _ = _proj(th, T, r0, r1, K)
            cur_s = _sample(cur, qu, qv); ref_s = pin.astype(np.float64)
            mr, mc = _seq(ref_s)/n, _seq(cur_s)/n
            sr = math.sqrt(_seq((ref_s - mr)*(ref_s - mr))/(n - 1)); sc = math.sqrt(_seq((cur_s - mc)*(cur_s - mc))/(n - 1))
            zn = _seq(((ref_s - mr)/sr)*((cur_s - mc)/sc))/n if (sr != 0 and sc != 0) else -100.0
        if not (zn >= zncc_min):
            reason = ZNCC
    flags = None
    if dete is not None:
        flags = np.zeros(len(dete), bool)
        if reason == PASS:
            import oracle
            W0, H0 = w0h0
            mask = oracle.fillpoly4(W0, H0, [int(u[0]), int(v[0]), int(u[1]), int(v[1]), int(u[2]), int(v[2]), int(u[3]), int(v[3])])
            for j, (x, y) in enumerate(dete):
                if not (np.isfinite(x) and np.isfinite(y)):
                    continue
                ru, rv = _round_half_away(float(x)), _round_half_away(float(y))
                if 0 <= ru < W0 and 0 <= rv < H0:
                    flags[j] = mask[rv, ru] != 0
    return reason, cs, zn, np.stack([u, v], 1), flags


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def scene():
    return synth.text_judge_planes(seed=3, n=8)


@pytest.fixture(scope="module")
def pixels(scene, oracle_lib):
    """vRefPixs of every plane: oracle.frame_box_pixels on the reference image (tool::GetBoxAllPixs), CSR."""
    off, uv, inten = [0], [], []
    for q in scene["quad"]:
        u, v, I, _ = oracle_lib.frame_box_pixels(scene["ref_img"], q, 0.0, 1.0)
        uv.append(np.stack([u, v], 1)); inten.append(I.astype(np.uint8)); off.append(off[-1] + len(u))
    return np.array(off, np.int32), np.concatenate(uv).astype(np.int16), np.concatenate(inten)


@pytest.fixture(scope="module")
def cur_frame(scene):
    from textslam_amd.frame import Frame
    fr = Frame(0); fr.GetPyrMat(scene["cur_img"], 2)
    return fr


def _call(fr, S, pix, sel=None, level=0, K=None, cos_min=0.0, margin=6, zncc_min=0.1, dete=True):
    off, uv, inten = pix
    sel = list(range(len(S["kind"]))) if sel is None else list(sel)
    o2, uv2, in2 = [0], [], []
    for i in sel:
        uv2.append(uv[off[i]:off[i + 1]]); in2.append(inten[off[i]:off[i + 1]]); o2.append(o2[-1] + off[i + 1] - off[i])
    uv2 = np.concatenate(uv2) if uv2 else np.zeros((0, 2), np.int16); in2 = np.concatenate(in2) if in2 else np.zeros(0, np.uint8)
    return fr.TextJudgeBatch(level, S["theta"][sel], S["Tcr"][sel], S["box_ray"][sel], np.array(o2, np.int32), uv2, in2, S["K"],
                             S["K"] if K is None else K, cos_min=cos_min, out_margin=margin, zncc_min=zncc_min, dete_xy=S["dete_xy"] if dete else None)


def _check_against_ref(out, S, pix, cur, sel=None, K=None, cos_min=0.0, margin=6, zncc_min=0.1, dete=True, w0h0=(640, 480)):
    off, uv, inten = pix
    sel = list(range(len(S["kind"]))) if sel is None else list(sel)
    reasons = []
    for k, i in enumerate(sel):
        pu, pv, pin = uv[off[i]:off[i + 1], 0], uv[off[i]:off[i + 1], 1], inten[off[i]:off[i + 1]]
        r, cs, zn, box, fl = judge_ref(cur, w0h0, S["theta"][i], S["Tcr"][i], S["box_ray"][i], pu, pv, pin, S["K"], S["K"] if K is None else K,
                                       cos_min, margin, zncc_min, S["dete_xy"] if dete else None)
        tag = (S["kind"][i], cos_min, margin, zncc_min)
        assert out["reason"][k] == r, tag
        assert out["pass"][k] == (r == PASS), tag
        assert np.array_equal(out["box_uv"][k].view(np.uint64), box.view(np.uint64)), tag
        assert np.array_equal(np.array([out["cos"][k]]).view(np.uint64), np.array([cs]).view(np.uint64)), tag
        if np.isnan(zn):
            assert np.isnan(out["zncc"][k]), tag
        else:
            assert abs(out["zncc"][k] - zn) <= 1e-12, (tag, out["zncc"][k], zn)
            assert abs(zn - zncc_min) > 1e-9, tag                          # no case sits on its threshold
        if dete:
            assert np.array_equal(out["dete"][k], fl), (tag, np.nonzero(out["dete"][k]), np.nonzero(fl))
        reasons.append(r)
    return reasons


# ------------------------------------------------------------------------------------------------ tests
def test_entry_point_declared_exported_and_bound():
    from textslam_amd import frame
    hdr = open(os.path.join(ROOT, "include", "tsframe.h")).read()
    assert re.search(r"\bint\s+tsframe_text_judge\s*\(void \*ctx, int level, int n, const double \*theta, const double \*Tcr, const double \*box_ray,", hdr)
    for name, val in (("PASS", 0), ("ORIENT", 1), ("DEPTH", 2), ("BOX", 3), ("ZNCC", 4)):
        assert re.search(r"#define TSFRAME_JUDGE_%s %d\b" % (name, val), hdr), name
    assert "tsframe_text_judge" in frame.EXPORTED_SYMBOLS
    L = frame._load()
    assert L.tsframe_text_judge.argtypes is not None and len(L.tsframe_text_judge.argtypes) == 22
    assert L.tsframe_text_judge.restype is C.c_int
    assert hasattr(frame.Frame, "TextJudgeBatch")


def test_synthetic_set_covers_the_cases(oracle_lib):
    S = synth.text_judge_planes(seed=3, n=8)
    kinds = S["kind"]
    for k in ("true", "perturbed", "oblique", "behind", "margin", "constant", "huge") + tuple("tiny%d" % i for i in range(6)):
        assert k in kinds, k
    i = kinds.index("margin")
    u, _, _ = synth._judge_corners(S["theta"][i], S["Tcr"][i], S["box_ray"][i], S["K"])
    assert u[0] == 6.0
    counts = {k: len(oracle_lib.frame_box_pixels(S["ref_img"], q, 0.0, 1.0)[0]) for k, q in zip(kinds, S["quad"])}
    assert [counts["tiny%d" % i] for i in range(6)] == [0, 1, 2, 3, 4, 5]
    assert counts["huge"] > 4800                                      # beyond the kernel's LDS sample cache: the recomputing path
    assert all(500 <= c <= 5000 for k, c in counts.items() if k == "true")


@pytest.mark.gpu
def test_ref_pixels_match_frame_box_pixels(scene, pixels):
    from textslam_amd.frame import Frame
    fr = Frame(0); fr.GetPyrMat(scene["ref_img"], 1)
    off, uv, inten = pixels
    for i, q in enumerate(scene["quad"]):
        got = fr.GetBoxAllPixs(0, q, 0.0, 1.0)
        assert np.array_equal(got["u"], uv[off[i]:off[i + 1], 0]) and np.array_equal(got["v"], uv[off[i]:off[i + 1], 1]), i
        assert np.array_equal(got["featureInten"], inten[off[i]:off[i + 1]].astype(np.float64)), i


@pytest.mark.gpu
@pytest.mark.parametrize("cos_min,margin,zncc_min,dete", [(0.0, 6, 0.1, True), (0.5, 6, 0.1, True), (0.0, 3, -3.0, False),
                                                          (0.0, 6, 0.8, True), (0.0, 5, 0.1, True)])
def test_judge_matches_restatement(scene, pixels, cur_frame, cos_min, margin, zncc_min, dete):
    out = _call(cur_frame, scene, pixels, cos_min=cos_min, margin=margin, zncc_min=zncc_min, dete=dete)
    reasons = _check_against_ref(out, scene, pixels, scene["cur_img"], cos_min=cos_min, margin=margin, zncc_min=zncc_min, dete=dete)
    by = dict(zip(scene["kind"], reasons))
    zn = dict(zip(scene["kind"], out["zncc"]))
    assert by["behind"] == DEPTH
    assert by["oblique"] == (ORIENT if cos_min == 0.5 else by["oblique"]) and (cos_min == 0.5 or by["oblique"] != ORIENT)
    assert by["margin"] == (BOX if margin == 6 else by["margin"]) and (margin == 6 or by["margin"] != BOX)
    if zncc_min <= -2:
        assert all(np.isnan(out["zncc"])) and by["constant"] == PASS and by["tiny0"] == PASS
    else:
        assert by["constant"] == ZNCC and zn["constant"] == -100.0
        assert by["tiny0"] == ZNCC and by["tiny1"] == ZNCC and np.isnan(zn["tiny0"]) and np.isnan(zn["tiny1"])
        assert all(not np.isnan(zn["tiny%d" % k]) for k in range(2, 6))
        assert not np.isnan(zn["huge"])
    if zncc_min == 0.1:
        assert sum(by[k] == PASS for k in by if k == "true") >= 1 and by["true"] == PASS
    if dete:
        assert out["dete"].any()
        assert out["dete_bits"].shape == (len(scene["kind"]), (len(scene["dete_xy"]) + 31)//32)


@pytest.mark.gpu
def test_planes_independent_and_deterministic(scene, pixels, cur_frame):
    n = len(scene["kind"])
    a = _call(cur_frame, scene, pixels)
    b = _call(cur_frame, scene, pixels)
    rev = _call(cur_frame, scene, pixels, sel=list(range(n))[::-1])
    keys = ("pass", "reason", "cos", "zncc", "box_uv", "dete_bits")
    for k in keys:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    for i in range(n):
        one = _call(cur_frame, scene, pixels, sel=[i])
        mixed = _call(cur_frame, scene, pixels, sel=[(i + 3) % n, i, (i + 7) % n])
        for k in keys:
            assert np.asarray(one[k])[0].tobytes() == np.asarray(a[k])[i].tobytes(), (i, k)
            assert np.asarray(rev[k])[n - 1 - i].tobytes() == np.asarray(a[k])[i].tobytes(), (i, k)
            assert np.asarray(mixed[k])[1].tobytes() == np.asarray(a[k])[i].tobytes(), (i, k)


@pytest.mark.gpu
def test_level_one(scene, pixels, cur_frame, oracle_lib):
    K1 = scene["K"]/2.0                                                # vK_scale[1] = K / 2 with K(2, 2) = 1
    cur1 = oracle_lib.frame_pyramid(scene["cur_img"], 2)[1][0]
    assert np.array_equal(cur_frame.level(1), cur1)
    for margin, zncc_min in ((3, 0.1), (3, -3.0)):
        out = _call(cur_frame, scene, pixels, level=1, K=K1, margin=margin, zncc_min=zncc_min)
        reasons = _check_against_ref(out, scene, pixels, cur1, K=K1, margin=margin, zncc_min=zncc_min)
        assert PASS in reasons


@pytest.mark.gpu
def test_resident_planes_unchanged_and_argument_errors(scene, pixels):
    from textslam_amd.frame import Frame, FrameError
    fr = Frame(0)
    off, uv, inten = pixels
    th, T, ray, K = scene["theta"][:2], np.ascontiguousarray(scene["Tcr"][:2]).reshape(2, 12), scene["box_ray"][:2], scene["K"]
    o2 = off[:3].copy(); uv2, in2 = uv[:off[2]], inten[:off[2]]
    L = fr.lib
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def raw(ctx=None, level=0, n=2, theta=th, Tcr=T, box=ray, poff=o2, puv=uv2, pin=in2, Kr=K, Kc=K, margin=6, n_dete=0, dete=None, keep_out=True):
        outs = [np.full(max(n, 1), 0x5a, np.uint8), np.full(max(n, 1), 77, np.int32), np.full(max(n, 1), 7.0), np.full(max(n, 1), 7.0), np.full((max(n, 1), 8), 7.0)]
        rc = L.tsframe_text_judge(fr.ctx if ctx is None else ctx, level, n, None if theta is None else dp(theta), None if Tcr is None else dp(Tcr),
                                  None if box is None else dp(box), None if poff is None else poff.ctypes.data_as(C.POINTER(C.c_int32)),
                                  None if puv is None else puv.ctypes.data_as(C.POINTER(C.c_int16)), None if pin is None else pin.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  None if Kr is None else dp(Kr), None if Kc is None else dp(Kc), 0.0, margin, 0.1, n_dete, None if dete is None else dp(dete),
                                  outs[0].ctypes.data_as(C.POINTER(C.c_uint8)), outs[1].ctypes.data_as(C.POINTER(C.c_int32)), dp(outs[2]), dp(outs[3]), dp(outs[4]), None)
        untouched = np.all(outs[0] == 0x5a) and np.all(outs[1] == 77) and np.all(outs[2] == 7.0) and np.all(outs[3] == 7.0) and np.all(outs[4] == 7.0)
        return rc, untouched

    rc, same = raw(); assert rc == -3 and same                                 # no image set: TSFRAME_ERR_STATE
    assert "no image" in L.tsframe_last_error(fr.ctx).decode()
    with pytest.raises(FrameError):
        _call(fr, scene, pixels)
    fr.GetPyrMat(scene["cur_img"], 2)
    before = [fr.level(l, k).copy() for l in range(2) for k in range(4)]
    rc, same = raw(n=0, theta=None, Tcr=None, box=None, poff=None, puv=None, pin=None, Kr=None, Kc=None)
    assert rc == 0 and same                                                    # n == 0: nothing to do
    bad_off = o2.copy(); bad_off[0] = 1
    dec_off = o2.copy(); dec_off[1] = dec_off[2] + 1
    nanK = K.copy(); nanK[2] = np.nan
    zeroK = K.copy(); zeroK[0] = 0.0
    cases = [("n < 0", dict(n=-1)), ("level < 0", dict(level=-1)), ("theta NULL", dict(theta=None)), ("Tcr NULL", dict(Tcr=None)),
             ("box NULL", dict(box=None)), ("pix_off NULL", dict(poff=None)), ("pix_uv NULL", dict(puv=None)), ("pix_inten NULL", dict(pin=None)),
             ("K_ref NULL", dict(Kr=None)), ("K NULL", dict(Kc=None)), ("pix_off[0]", dict(poff=bad_off)), ("pix_off decreasing", dict(poff=dec_off)),
             ("K not finite", dict(Kc=nanK)), ("K_ref zero focal", dict(Kr=zeroK)), ("margin < 0", dict(margin=-1)),
             ("n_dete < 0", dict(n_dete=-1)), ("dete NULL", dict(n_dete=3))]
    for name, kw in cases:
        rc, same = raw(**kw)
        assert rc == -1 and same, name
        assert "tsframe_text_judge" in L.tsframe_last_error(fr.ctx).decode(), name
    rc, same = raw(level=2); assert rc == -3 and same                          # level not built
    rc = L.tsframe_text_judge(None, 0, 0, None, None, None, None, None, None, None, None, 0.0, 6, 0.1, 0, None, None, None, None, None, None, None)
    assert rc == -1
    _call(fr, scene, pixels); _call(fr, scene, pixels, level=1, K=K/2.0)
    after = [fr.level(l, k) for l in range(2) for k in range(4)]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def _write_cxx_input(path, S, pix, sel):
    """The C++ driver's input: current image, poses (T_cw of the reference keyframe and the frame), K, detection centres, and the planes."""
    off, uv, inten = pix
    Tr = np.eye(4); Tc = np.eye(4)
    Tc[:3, :] = S["Tcr"][sel[0]]                                       # the reference keyframe at the origin: T_cw(frame) = T_cr
    with open(path, "wb") as f:
        img = S["cur_img"]
        f.write(struct.pack("<iiii", img.shape[1], img.shape[0], len(sel), len(S["dete_xy"])))
        f.write(img.tobytes()); f.write(Tr.tobytes()); f.write(Tc.tobytes()); f.write(np.asarray(S["K"], np.float64).tobytes())
        f.write(np.asarray(S["dete_xy"], np.float64).tobytes())
        for i in sel:
            m = int(off[i + 1] - off[i])
            f.write(struct.pack("<i", m)); f.write(S["theta"][i].astype(np.float64).tobytes()); f.write(S["box_ray"][i].astype(np.float64).tobytes())
            f.write(uv[off[i]:off[i + 1]].astype(np.int16).tobytes()); f.write(inten[off[i]:off[i + 1]].astype(np.uint8).tobytes())


@pytest.mark.gpu
def test_adapter_pack_text_judge_from_cxx(tmp_path, scene, pixels, cur_frame):
    exe = str(tmp_path / "text_judge_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "text_judge_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsframe", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    sel = [i for i, k in enumerate(scene["kind"]) if k in ("true", "perturbed", "constant", "tiny1", "tiny3", "huge")]
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    _write_cxx_input(inp, scene, pixels, sel)
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "text judge from C++: ok" in res.stdout, res.stdout
    n, nd = len(sel), len(scene["dete_xy"]); words = (nd + 31)//32
    raw = open(outp, "rb").read()
    dt = np.dtype([("Tcr", "<f8", (n, 12)), ("reason", "<i4", (n,)), ("pass", "u1", (n,)), ("cos", "<f8", (n,)), ("zncc", "<f8", (n,)),
                   ("box", "<f8", (n, 8)), ("bits", "<u4", (n, words))])
    got = np.frombuffer(raw, dt, count=1)[0]
    for sub in ("Tcr",):                                              # T_cw(frame) * T_wc(ref) with the reference keyframe at the origin: T_cr itself
        np.testing.assert_allclose(got[sub], np.ascontiguousarray(scene["Tcr"][sel]).reshape(n, 12), rtol=0, atol=1e-15)
    S2 = dict(scene); S2["Tcr"] = np.array(scene["Tcr"]); S2["Tcr"][sel] = got["Tcr"].reshape(n, 3, 4)
    out = _call(cur_frame, S2, pixels, sel=sel)
    assert np.array_equal(out["reason"], got["reason"]) and np.array_equal(out["pass"].astype(np.uint8), got["pass"])
    assert out["cos"].tobytes() == got["cos"].tobytes() and out["zncc"].tobytes() == got["zncc"].tobytes()
    assert out["box_uv"].reshape(n, 8).tobytes() == got["box"].tobytes() and out["dete_bits"].tobytes() == got["bits"].tobytes()
    assert PASS in list(got["reason"]) and ZNCC in list(got["reason"])

"""Files of the two stand-alone programs of the two-view reconstruction tests, and the comparisons the host test, the GPU test and
tools/diag/gpu_two_view_reconstruct.py share: tests/cxx/two_view_reconstruct_host.hip (the device's __host__ __device__ arithmetic on the CPU) and
tests/cxx/two_view_reconstruct_from_cxx.cpp (adapter/tsorb_two_view.hpp's reconstruct over mock types)."""
import os
import struct
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- two_view_reconstruct_host
def build_host(exe, sanitize=True):
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "two_view_reconstruct_host.hip")])
    return exe


def write_host(path, w):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", len(w["xy1"]), int(w["model"]), int(w["min_triangulated"])))
        f.write(np.ascontiguousarray(w["M21"], F32).tobytes()); f.write(np.asarray(w["K"], F32).tobytes())
        f.write(struct.pack("<ff", float(w["sigma"]), float(w["min_parallax"])))
        f.write(np.ascontiguousarray(w["xy1"], F32).tobytes()); f.write(np.ascontiguousarray(w["xy2"], F32).tobytes())
        f.write(np.asarray(w["inlier"], np.uint8).tobytes())


def _taker(raw):
    off = [0]

    def take(dt, k):
        a = np.frombuffer(raw, dt, k, off[0]); off[0] += a.nbytes
        return a
    return take, off


def read_host(path, n):
    raw = open(path, "rb").read(); take, off = _taker(raw)
    out = dict(result=take(np.int32, 6), R21=take(F32, 9).reshape(3, 3), t21=take(F32, 3), p3d=take(F32, 3*n).reshape(n, 3), triangulated=take(np.uint8, n).astype(bool),
               hyp_good=take(np.int32, 8), hyp_cos=take(F32, 8), hyp_parallax=take(F32, 8), hyp_pose=take(F32, 96).reshape(8, 3, 4),
               hyp_state=take(np.uint8, 8*n).reshape(8, n), hyp_p3d=take(F32, 24*n).reshape(8, n, 3))
    assert off[0] == len(raw)
    return out


# ---- what both comparisons (host program, device) assert
def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_floats(a, b):
    """Equal as bit patterns, NaNs in the same places (a NaN's sign and payload are the processor's)."""
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def ulps(a, b):
    """The distance of two finite float32 arrays in float steps."""
    ia = bits(a).astype(np.int64); ib = bits(b).astype(np.int64)
    ia = np.where(ia & 0x80000000, 0x80000000 - ia, ia); ib = np.where(ib & 0x80000000, 0x80000000 - ib, ib)
    return np.abs(ia - ib)


def check_bits(R, got, w):
    """1. Bit for bit, no conditions needed: from the implementation's OWN float hyp_pose and hyp_p3d the restatement's CheckRT arithmetic gives its hyp_state, hyp_good and
    hyp_cos as bit patterns; hyp_parallax within 4 float steps (acosf is the platform's); the keep logic over its counts and ITS parallaxes gives result, and R21, t21,
    p3d and triangulated follow."""
    d = R.derive(w, got["hyp_pose"], got["hyp_p3d"])
    assert np.array_equal(got["hyp_state"], d["hyp_state"]), "hyp_state differs from the restatement's CheckRT on the same float points: %s" % (
        np.argwhere(got["hyp_state"] != d["hyp_state"])[:5].tolist(),)
    assert np.array_equal(got["hyp_good"], d["hyp_good"]), (got["hyp_good"], d["hyp_good"])
    assert same_floats(got["hyp_cos"], d["hyp_cos"]), (got["hyp_cos"], d["hyp_cos"])
    fin = np.isfinite(d["hyp_parallax"])
    assert np.array_equal(fin, np.isfinite(got["hyp_parallax"])) and (ulps(got["hyp_parallax"][fin], d["hyp_parallax"][fin]) <= 4).all(), (got["hyp_parallax"], d["hyp_parallax"])
    sv = w["model"] == 0 and not np.asarray(got["hyp_pose"]).any() and R.hypotheses_h(w["M21"], w["K"])[2]
    k = R.decide(w, d, got["hyp_pose"], got["hyp_p3d"], sv, got["hyp_parallax"])
    assert np.array_equal(got["result"], k["result"]), (got["result"], k["result"])
    assert same_floats(got["R21"], k["R21"]) and same_floats(got["t21"], k["t21"]) and same_floats(got["p3d"], k["p3d"])
    assert np.array_equal(got["triangulated"], k["triangulated"])
    if not got["result"][0]:
        assert not got["R21"].any() and not got["t21"].any() and not got["p3d"].any() and not got["triangulated"].any() and got["result"][1] == -1
    if got["result"][5] & R.EXIT_SV:
        assert not any(np.asarray(got[key]).any() for key in ("hyp_good", "hyp_cos", "hyp_parallax", "hyp_pose", "hyp_state", "hyp_p3d"))
    if w["model"] == 1:
        assert not any(np.asarray(got[key][4:]).any() for key in ("hyp_good", "hyp_cos", "hyp_parallax", "hyp_pose", "hyp_state", "hyp_p3d"))
    out = ~np.asarray(w["inlier"], bool)
    assert not got["hyp_state"][:, out].any() and not got["hyp_p3d"][:, out].any()


def check_hypotheses(R, got, ref, sens):
    """2. Every hyp_pose entry within the larger of 1000 x the restatement's sensitivity and one float ulp of the hypothesis' largest entry.  Returns the largest
    difference in units of the tolerance."""
    a, b = np.asarray(got["hyp_pose"], F32), ref["hyp_pose"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    tol = R.tolerance(ref, sens)["pose"]
    with np.errstate(invalid="ignore"):
        r = np.abs(a.astype(np.float64) - b.astype(np.float64))/tol
    worst = float(np.nanmax(r)) if np.isfinite(r).any() else 0.0
    assert worst <= 1.0, "a hypothesis entry is %.3g tolerances from the restatement's" % worst
    return worst


def check_points(R, got, w, sens_point):
    """3. Every hyp_p3d point within the larger of 1000 x its own sensitivity and one float ulp of its largest coordinate -- of the restatement's triangulation from the
    SAME float hypothesis (the implementation's own hyp_pose: a hypothesis that differs in its last bit moves every point by far more than the fp64 stage does, and
    comparison 2 is what holds the hypotheses).  Non-finite points in the same places.  Returns the largest difference in units of the tolerance."""
    n = len(w["xy1"]); inl = np.asarray(w["inlier"], bool); worst = 0.0
    nh = 0 if not np.asarray(got["hyp_pose"]).any() else (8 if w["model"] == 0 else 4)
    for h in range(nh):
        P2, _ = R.camera(got["hyp_pose"][h, :, :3], got["hyp_pose"][h, :, 3], w["K"])
        X = np.zeros((n, 3)); X[inl] = R.triangulate64(R.system(P2, w["K"], w["xy1"][inl], w["xy2"][inl]))
        Xf = R._to_f32(X); a = got["hyp_p3d"][h]
        fin = np.isfinite(Xf).all(axis=1)
        assert np.array_equal(fin, np.isfinite(a).all(axis=1)), "non-finite points differ in hypothesis %d" % h
        big = np.abs(Xf[fin]).max(axis=1, keepdims=True)
        tol = np.maximum(1000.0*sens_point[h][fin, None]*big, np.spacing(big).astype(np.float64))
        if fin.any():
            worst = max(worst, float((np.abs(a[fin].astype(np.float64) - Xf[fin].astype(np.float64))/np.maximum(tol, 1e-300)).max()))
    assert worst <= 1.0, "a point is %.3g tolerances from the restatement's" % worst
    return worst


def check_decisions(R, got, ref, mg, model):
    """4. On a world that meets its conditions: ok, sel, N, the exit bits (and F's nsimilar) and the kept hypothesis' triangulated mask and hyp_good equal the
    restatement's outright; every other hyp_good -- and the best and second best counts where they are a non-kept hypothesis' -- within +- its low-margin pairs."""
    r, g = np.asarray(got["result"]), ref["result"]; low = mg["low"].astype(int); kept = int(g[1])
    assert r[[0, 1, 2, 5]].tolist() == g[[0, 1, 2, 5]].tolist(), (r, g)
    slack = int(np.delete(low, kept).max()) if kept >= 0 else int(low.max())
    assert abs(int(r[3]) - int(g[3])) <= (0 if kept >= 0 else slack), (r, g)                 # the best count: the kept hypothesis' own, or a non-kept one's
    assert abs(int(r[4]) - int(g[4])) <= (slack if model == 0 else 0), (r, g)                # H: the second best count (never the kept one's); F: nsimilar
    assert np.array_equal(got["triangulated"], ref["triangulated"])
    for h in range(8):
        assert abs(int(got["hyp_good"][h]) - int(ref["hyp_good"][h])) <= (0 if h == kept else low[h]), (h, got["hyp_good"], ref["hyp_good"], low)


# ---- two_view_reconstruct_from_cxx
def build_driver(tmp_path):
    exe = str(tmp_path / "two_view_reconstruct_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "two_view_reconstruct_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_scene(path, w, given=None):
    """The initializer's members around world w: mvKeys1, mvKeys2, mvMatches12, the mask, the model and mK; given = the call's outputs for --host."""
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiii", len(w["keys1"]), len(w["keys2"]), len(w["matches"]), int(w["model"]), int(w["min_triangulated"])))
        f.write(struct.pack("<ff", float(w["sigma"]), float(w["min_parallax"]))); f.write(np.ascontiguousarray(w["M21"], F32).tobytes()); f.write(np.asarray(w["K"], F32).tobytes())
        f.write(np.ascontiguousarray(w["keys1"], F32).tobytes()); f.write(np.ascontiguousarray(w["keys2"], F32).tobytes())
        f.write(np.ascontiguousarray(w["matches"], np.int32).tobytes()); f.write(np.asarray(w["inlier"], np.uint8).tobytes())
        if given is not None:
            f.write(np.asarray(given["result"], np.int32).tobytes()); f.write(np.ascontiguousarray(given["R21"], F32).tobytes()); f.write(np.asarray(given["t21"], F32).tobytes())
            f.write(np.ascontiguousarray(given["p3d"], F32).tobytes()); f.write(np.asarray(given["triangulated"], np.uint8).tobytes())


def read_scene(path, host):
    raw = open(path, "rb").read(); take, off = _taker(raw)
    n = int(take(np.int32, 1)[0])
    out = dict(n=n, xy1=take(F32, 2*n).reshape(n, 2), xy2=take(F32, 2*n).reshape(n, 2), inlier=take(np.uint8, n).astype(bool), M21=take(F32, 9).reshape(3, 3), K=take(F32, 4))
    out["ret"], out["hasR"], out["hasT"] = [int(x) for x in take(np.int32, 3)]
    out["R"] = take(F32, 9).reshape(3, 3); out["t"] = take(F32, 3); k = int(take(np.int32, 1)[0])
    out["vP3D"] = take(F32, 3*k).reshape(k, 3); out["vbTriangulated"] = take(np.uint8, k).astype(bool)
    if not host:
        out.update(result=take(np.int32, 6), R21=take(F32, 9).reshape(3, 3), t21=take(F32, 3), p3d=take(F32, 3*n).reshape(n, 3), triangulated=take(np.uint8, n).astype(bool))
    assert off[0] == len(raw)
    return out


def check_scene(o, w, given):
    """The driver's outputs against a plain scatter of the call's."""
    assert o["xy1"].tobytes() == np.ascontiguousarray(w["xy1"], F32).tobytes() and o["xy2"].tobytes() == np.ascontiguousarray(w["xy2"], F32).tobytes()
    assert np.array_equal(o["inlier"], np.asarray(w["inlier"], bool)) and o["M21"].tobytes() == np.ascontiguousarray(w["M21"], F32).tobytes()
    assert o["K"].tobytes() == np.asarray(w["K"], F32).tobytes()
    ok = bool(given["result"][0])
    assert o["ret"] == int(ok) and o["hasR"] == int(ok) and o["hasT"] == int(ok)
    if not ok:
        assert len(o["vP3D"]) == 0 and not o["R"].any() and not o["t"].any()
        return
    assert o["R"].tobytes() == np.ascontiguousarray(given["R21"], F32).tobytes() and o["t"].tobytes() == np.asarray(given["t21"], F32).tobytes()
    P = np.zeros((len(w["keys1"]), 3), F32); B = np.zeros(len(w["keys1"]), bool)
    P[w["matches"][:, 0]] = given["p3d"]; B[w["matches"][:, 0]] = given["triangulated"]
    assert o["vP3D"].tobytes() == P.tobytes() and np.array_equal(o["vbTriangulated"], B)

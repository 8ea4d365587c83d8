"""Files of the two stand-alone programs of the new-points tests, shared by the host test, the GPU test and tools/diag/gpu_new_points.py:
tests/cxx/new_points_host.hip (the device's __host__ __device__ decisions and arithmetic on the CPU, over the candidate lists the restatement forms) and
tests/cxx/new_points_from_cxx.cpp (adapter/tsorb_new_points.hpp's two bodies over mock types); and the comparisons the host test and the GPU test both assert."""
import os
import struct
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I32, U8 = np.float32, np.float64, np.int32, np.uint8


def _taker(raw):
    off = [0]

    def take(dt, k):
        a = np.frombuffer(raw, dt, k, off[0]); off[0] += a.nbytes
        return a
    return take, off


# ---- new_points_host
def build_host(exe, sanitize=True):
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "new_points_host.hip")])
    return exe


def write_host(path, w, cands):
    """The world and every query's candidate list (index, distance; GetFeaturesInArea's order, before the eligibility and vMatchDist tests)."""
    nq, n2 = len(w["qxy"]), len(w["kp6"])
    elig = np.ones(n2, U8) if w.get("elig2") is None else (np.asarray(w["elig2"]).reshape(-1) != 0).astype(U8)
    cnt = np.array([len(c) for c, _ in cands], I32)
    idx = np.concatenate([c for c, _ in cands]).astype(I32) if nq else np.zeros(0, I32)
    dist = np.concatenate([d for _, d in cands]).astype(I32) if nq else np.zeros(0, I32)
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiiid", nq, n2, int(w["th_low"]), int(bool(w["use_ratio"])), int(w["th_reproj"]), float(w["ratio"])))
        f.write(np.ascontiguousarray(np.asarray(w["Trw"], F64).reshape(-1, 4)[:3]).tobytes()); f.write(np.ascontiguousarray(np.asarray(w["Tcw"], F64).reshape(-1, 4)[:3]).tobytes())
        f.write(np.asarray(w["K"], F64).tobytes())
        f.write(np.ascontiguousarray(w["q_px"], F32).tobytes()); f.write(np.ascontiguousarray(np.asarray(w["kp6"], F32).reshape(-1, 6)[:, :2]).tobytes())
        f.write(elig.tobytes()); f.write(cnt.tobytes()); f.write(idx.tobytes()); f.write(dist.tobytes())


def read_host(path, nq):
    raw = open(path, "rb").read(); take, off = _taker(raw)
    out = dict(match12=take(I32, nq), match_dist=take(I32, nq), p3d=take(F32, 3*nq).reshape(nq, 3), good=take(U8, nq).astype(bool))
    out["n_match"], out["n_good"] = [int(v) for v in take(I32, 2)]
    assert off[0] == len(raw)
    return out


# ---- what both comparisons (host program, device) assert
def check_matches(got, ref):
    """1. match12, match_dist (where the call gives it) and n_match equal the restatement's, unconditionally."""
    assert np.array_equal(got["match12"], ref["match12"]), "match12 differs: first at %s" % np.flatnonzero(np.asarray(got["match12"]) != ref["match12"])[:5].tolist()
    if "match_dist" in got:
        assert np.array_equal(got["match_dist"], ref["match_dist"])
    assert got["n_match"] == ref["n_match"] == int((ref["match12"] >= 0).sum())


def check_points(R, got, ref, sens):
    """2. Every point within the larger of one float ulp of its largest coordinate and 1000 x the restatement's own sensitivity; non-finite points in the same places;
    rows without a match are zero.  Returns the largest difference in units of the tolerance and whether every point equals the restatement's in every bit."""
    X = ref["p3d"]; a = np.asarray(got["p3d"], F32); has = ref["match12"] >= 0
    assert not a[~has].any() and not np.asarray(got["good"])[~has].any()
    fin = np.isfinite(X).all(axis=1)
    assert np.array_equal(fin, np.isfinite(a).all(axis=1)), "non-finite points differ"
    worst = 0.0; rows = fin & has
    if rows.any():
        big = np.abs(X[rows]).max(axis=1, keepdims=True)
        tol = np.maximum(1000.0*sens["rel"][rows, None]*big.astype(F64), np.spacing(big).astype(F64))
        worst = float((np.abs(a[rows].astype(F64) - X[rows].astype(F64))/tol).max())
    assert worst <= 1.0, "a point is %.3g tolerances from the restatement's" % worst
    return worst, R.same32(a, X)


def check_verdicts(R, w, got, ref, same):
    """3. good and n_good are the restatement's check applied to the implementation's OWN points, bit for bit; 4. where the points are the restatement's in every
    bit, they are the restatement's full answer outright."""
    own = R.run(w, p3d=got["p3d"])
    assert np.array_equal(np.asarray(got["good"], bool), own["good"]) and got["n_good"] == own["n_good"] == int(own["good"].sum())
    if same:
        assert np.array_equal(np.asarray(got["good"], bool), ref["good"]) and got["n_good"] == ref["n_good"], "the points are the restatement's but a verdict is not"


# ---- new_points_from_cxx
def build_driver(tmp_path):
    exe = str(tmp_path / "new_points_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "new_points_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def frame1_of(w, mode):
    """The keyframe (mode 'track') or first frame ('init') around world w: feature i1 of it is query k = i1//2 for even i1; the odd ones are features the reference's
    loop skips (a map point already, a text feature, or -- for the initializer -- an octave above 0).  Returns per feature: pixel, octave, descriptor, vMatches2D3D,
    vTextObjInfo, and the query number it stands for (-1: skipped)."""
    nq = len(w["qxy"]); n1 = 2*nq
    px = np.zeros((n1, 2), F32); octv = np.zeros(n1, I32); desc = np.zeros((n1, 32), U8); m3d = np.full(n1, -1, I32); tobj = np.full(n1, -1, I32); qn = np.full(n1, -1, I32)
    px[0::2] = w["q_px"]; desc[0::2] = w["qdesc"]; qn[0::2] = np.arange(nq)
    octv[0::2] = 0 if w.get("qlev") is None or mode == "init" else np.asarray(w["qlev"])[:, 0]
    px[1::2] = np.asarray(w["q_px"], F32) + F32(1.5); desc[1::2] = w["qdesc"]
    if mode == "init":
        octv[1::2] = 1 + np.arange(nq) % 3
    else:
        octv[1::2] = octv[0::2]; m3d[1::4] = 7; tobj[3::4] = 2
    return px, octv, desc, m3d, tobj, qn


def write_scene(path, w, mode):
    """mode 'track': cfLastKeyframe / cfCurrentFrame for search_for_triangular_and_get; 'init': F1 / F2 for search_for_initializ."""
    px, octv, desc, m3d, tobj, _ = frame1_of(w, mode); n1, n2 = len(px), len(w["kp6"])
    m3d2 = np.full(n2, -1, I32) if w.get("elig2") is None else np.where(np.asarray(w["elig2"]).reshape(-1) != 0, -1, 5).astype(I32)
    T1 = np.eye(4); T1[:3] = np.asarray(w["Trw"], F64).reshape(-1, 4)[:3]; T2 = np.eye(4); T2[:3] = np.asarray(w["Tcw"], F64).reshape(-1, 4)[:3]
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", 0 if mode == "track" else 1, n1, n2, int(round(float(w["qr"][0]) if mode == "init" else 80)) if len(w["qr"]) else 80))
        f.write(np.asarray(w["K"], F64).tobytes()); f.write(T1.tobytes()); f.write(T2.tobytes()); f.write(np.asarray(w["bounds"], F64).tobytes())
        f.write(px.tobytes()); f.write(octv.tobytes()); f.write(desc.tobytes()); f.write(m3d.tobytes()); f.write(tobj.tobytes())
        f.write(np.ascontiguousarray(w["kp6"], F32).tobytes()); f.write(np.ascontiguousarray(w["desc2"], U8).tobytes()); f.write(m3d2.tobytes())


def read_scene(path, n1):
    raw = open(path, "rb").read(); take, off = _taker(raw)
    rc, n_match, n_new = [int(v) for v in take(I32, 3)]
    out = dict(rc=rc, n_match=n_match, match12=take(I32, n1), newpts=take(F64, 3*n_new).reshape(n_new, 3), newmatch=take(I32, 2*n_new).reshape(n_new, 2))
    assert off[0] == len(raw)
    return out


def check_scene(o, w, mode, got, host=False):
    """The driver's vMatchIdx12 / vNewpts / vNewptsMatch and returned count against `got`: the call's outputs on the queries the adapter must have gathered.  host: the
    driver's --host mode covers the search only (no points, the count is nMatches)."""
    _, _, _, _, _, qn = frame1_of(w, mode); feat_of = np.flatnonzero(qn >= 0)
    m12 = np.full(len(qn), -1, I32); m12[feat_of] = got["match12"]
    assert o["rc"] == 0 and np.array_equal(o["match12"], m12)
    if mode == "track" and not host:
        rows = np.flatnonzero(got["good"]) if got["n_match"] else np.zeros(0, np.int64)
        assert o["n_match"] == (got["n_good"] if got["n_match"] else 0)                # iNewScene: GetForTriangular's count, asked only when there is a match
        assert np.array_equal(o["newmatch"], np.column_stack([feat_of[rows], got["match12"][rows]]).astype(I32).reshape(-1, 2))
        assert o["newpts"].tobytes() == got["p3d"][rows].astype(F64).tobytes()
    else:
        assert o["n_match"] == got["n_match"] and len(o["newpts"]) == 0

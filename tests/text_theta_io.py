"""Files of the two stand-alone programs of the text-theta tests, shared by the host test, the GPU test and tools/diag/gpu_text_theta.py:
tests/cxx/text_theta_host.hip (the device's __host__ __device__ arithmetic on the CPU) and tests/cxx/text_theta_from_cxx.cpp (adapter/tsorb_text_theta.hpp's two
bodies over mock types)."""
import os
import struct
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, I32 = np.float32, np.float64, np.int32


def _taker(raw):
    off = [0]

    def take(dt, k):
        a = np.frombuffer(raw, dt, k, off[0]); off[0] += a.nbytes
        return a
    return take, off


# ---- text_theta_host
def build_host(exe, sanitize=True):
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "text_theta_host.hip")])
    return exe


def write_host(path, w):
    rho = w.get("rho")
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", len(w["off"]) - 1, int(rho is not None)))
        f.write(np.asarray(w["off"], I32).tobytes()); f.write(np.asarray(w["hyp_off"], I32).tobytes())
        f.write(np.ascontiguousarray(np.asarray(w["Tcr"], F64)[:3, :4]).tobytes()); f.write(np.asarray(w["K"], F64).tobytes())
        f.write(np.ascontiguousarray(w["host_xy"], F32).tobytes()); f.write(np.ascontiguousarray(w["targ_xy"], F32).tobytes())
        if rho is not None:
            f.write(np.asarray(rho, F64).tobytes())
        f.write(np.ascontiguousarray(w["triple"], I32).tobytes())


def read_host(path, w):
    P, N, H = len(w["off"]) - 1, int(w["off"][-1]), int(w["hyp_off"][-1])
    raw = open(path, "rb").read(); take, off = _taker(raw)
    out = dict(sel=take(I32, P), theta=take(F64, 3*P).reshape(P, 3), score=take(F64, P), p3d=take(F32, 3*N).reshape(N, 3), rho=take(F64, N), hyp_score=take(F64, H),
               hyp_theta=take(F64, 3*H).reshape(H, 3))
    assert off[0] == len(raw)
    return out


# ---- what both comparisons (host program, device) assert
def check_bits(R, got, w):
    """1. Bit for bit, unconditional: from the implementation's OWN rho the restatement gives its hyp_theta, hyp_score, sel, theta and score as bit patterns, NaN
    (in the same places) and -0.0 included."""
    d = R.run(w, rho=got["rho"])
    for k in ("hyp_theta", "hyp_score", "theta", "score"):
        assert R.same64(got[k], d[k]), "%s differs from the restatement's on the same rho: first at %s" % (
            k, np.argwhere(np.atleast_1d(~((got[k] == d[k]) | (np.isnan(got[k]) & np.isnan(d[k])))))[:3].tolist())
    assert np.array_equal(got["sel"], d["sel"]), (got["sel"], d["sel"])


def check_points(R, got, w, sens):
    """2. Every triangulated point within the larger of one float ulp of its largest coordinate and 1000 x the restatement's own sensitivity; non-finite points in the
    same places; rho = 1.0/(double)z of the implementation's own point, bit for bit.  Returns the largest difference in units of the tolerance and whether every
    point equals the restatement's in every bit."""
    X, _ = R.triangulate(w); a = np.asarray(got["p3d"], F32)
    fin = np.isfinite(X).all(axis=1)
    assert np.array_equal(fin, np.isfinite(a).all(axis=1)), "non-finite points differ"
    worst = 0.0
    if fin.any():
        big = np.abs(X[fin]).max(axis=1, keepdims=True)
        tol = np.maximum(1000.0*sens["rel"][fin, None]*big.astype(F64), np.spacing(big).astype(F64))
        worst = float((np.abs(a[fin].astype(F64) - X[fin].astype(F64))/tol).max())
    assert worst <= 1.0, "a point is %.3g tolerances from the restatement's" % worst
    with np.errstate(divide="ignore", invalid="ignore"):
        assert R.same64(got["rho"], 1.0/a[:, 2].astype(F64))
    return worst, R.same32(a, X)


# ---- text_theta_from_cxx
def build_driver(tmp_path):
    exe = str(tmp_path / "text_theta_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "text_theta_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


SEED = 20261
MAX_IT = 200


def scene_detections(w, mode):
    """The world's planes as a keyframe's detections: (cormap, first feature, last) each.  Tracking: every fourth detection is a map object already (skipped), and
    the planes below 8 features are skipped by the reference's threshold."""
    P = len(w["off"]) - 1
    return [(3 if (mode == "track" and p % 4 == 1) else -1, int(w["off"][p]), int(w["off"][p + 1])) for p in range(P)]


def write_scene(path, w, mode, rho=None):
    """mode 'track': cfLastKeyframe / cfCurrentFrame around world w (Trw = I, Tcw = Tcr); 'init': F1, F2 and the TextKeys.  rho [N]: TextKeys3D(2), or what --host
    uses where the device would triangulate."""
    rho = np.zeros(int(w["off"][-1])) if rho is None else np.asarray(rho, F64)
    T = np.eye(4); T[:3] = np.asarray(w["Tcr"], F64)[:3, :4]
    with open(path, "wb") as f:
        dets = scene_detections(w, mode)
        f.write(struct.pack("<iiiI", 0 if mode == "track" else 1, MAX_IT, len(dets), SEED))
        f.write(np.asarray(w["K"], F64).tobytes()); f.write(np.eye(4).tobytes()); f.write(T.tobytes())
        for cor, a, b in dets:
            f.write(struct.pack("<ii", cor, b - a))
            f.write(np.ascontiguousarray(w["host_xy"][a:b], F32).tobytes()); f.write(np.ascontiguousarray(w["targ_xy"][a:b], F32).tobytes()); f.write(rho[a:b].tobytes())


def read_scene(path):
    raw = open(path, "rb").read(); take, off = _taker(raw)
    rc, P, N, H = [int(x) for x in take(I32, 4)]
    out = dict(rc=rc, det=take(I32, P), off=take(I32, P + 1), hyp_off=take(I32, P + 1), triple=take(I32, 3*H).reshape(H, 3), host_xy=take(F32, 2*N).reshape(N, 2),
               targ_xy=take(F32, 2*N).reshape(N, 2), rho=take(F64, N), Tcr=take(F64, 12).reshape(3, 4), K=take(F64, 4), sel=take(I32, P), theta=take(F64, 3*P).reshape(P, 3),
               score=take(F64, P))
    nobj = int(take(I32, 1)[0]); out["mNcr"] = take(F64, 3*nobj).reshape(nobj, 3); out["vNGOOD"] = take(np.uint8, nobj).astype(bool)
    assert off[0] == len(raw)
    return out


def scene_call(w, mode, o):
    """The batch the adapter formed, as the arguments of the call."""
    return dict(off=o["off"], hyp_off=o["hyp_off"], host_xy=o["host_xy"], targ_xy=o["targ_xy"], triple=o["triple"], Tcr=o["Tcr"], K=o["K"], rho=o["rho"] if mode == "init" else None)


def _lcg_triples(plan):
    """The driver's generator (g = g*1664525 + 1013904223 mod 2^32; lo + (g >> 8) % (hi - lo + 1)) through tool::GetRANSACIdx for every (n, H) of plan."""
    g = SEED; out = []
    for n, H in plan:
        for _ in range(H):
            avail = list(range(n))
            for _j in range(3):
                g = (g*1664525 + 1013904223) & 0xffffffff
                r = (g >> 8) % len(avail); out.append(avail[r]); avail[r] = avail[-1]; avail.pop()
    return np.array(out, I32).reshape(-1, 3)


def check_scene(o, w, mode, d, got):
    """The driver's gather against the reference's rules, its draws against the generator, and mNcr / vNGOOD against `got`: the call's outputs on batch d."""
    dets = scene_detections(w, mode)
    keep = [i for i, (cor, a, b) in enumerate(dets) if mode == "init" or (cor < 0 and b - a >= 8)]
    assert o["rc"] == 0 and o["det"].tolist() == keep
    sizes = [dets[i][2] - dets[i][1] for i in keep]
    assert o["off"].tolist() == np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
    idx = np.concatenate([np.arange(dets[i][1], dets[i][2]) for i in keep]) if keep else np.zeros(0, int)
    assert o["host_xy"].tobytes() == np.ascontiguousarray(w["host_xy"][idx], F32).tobytes() and o["targ_xy"].tobytes() == np.ascontiguousarray(w["targ_xy"][idx], F32).tobytes()
    assert o["Tcr"].tobytes() == np.ascontiguousarray(np.asarray(w["Tcr"], F64)[:3, :4]).tobytes() and o["K"].tobytes() == np.asarray(w["K"], F64).tobytes()
    # tracking: 200 triples per plane; the initializer: drawn from 4 features on, (0, 0, 0) for exactly 3, none below
    hyps = [MAX_IT if n >= 3 else 0 for n in sizes]
    assert o["hyp_off"].tolist() == np.concatenate([[0], np.cumsum(hyps)]).astype(int).tolist()
    drawn = _lcg_triples([(n, MAX_IT) for n in sizes if n >= (4 if mode == "init" else 3)]); at = 0
    for k, n in enumerate(sizes):
        t = o["triple"][o["hyp_off"][k]:o["hyp_off"][k + 1]]
        if n >= (4 if mode == "init" else 3):
            assert np.array_equal(t, drawn[at:at + MAX_IT]); at += MAX_IT
        else:
            assert not t.any()
    assert np.array_equal(o["sel"], got["sel"]) and o["theta"].tobytes() == got["theta"].tobytes() and o["score"].tobytes() == got["score"].tobytes()
    mN = np.full((len(dets), 3), np.nan); good = np.zeros(len(dets), bool)
    for k, i0 in enumerate(keep):
        if got["sel"][k] >= 0:
            mN[i0] = got["theta"][k]; good[i0] = True
    assert np.array_equal(o["vNGOOD"], good) and np.array_equal(np.isnan(o["mNcr"]), np.isnan(mN)) and o["mNcr"][good].tobytes() == mN[good].tobytes()

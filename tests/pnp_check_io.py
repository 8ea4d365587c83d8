"""The scene files of tests/cxx/pnp_check_from_cxx.cpp (adapter/tsorb_pnp_check.hpp over mock types), shared by the host test and the GPU test: a world of
tests/pnp_ransac_ref.py turned into CheckMatch's arguments (map points as reference keyframe + ray + inverse depth, a frame's keypoints, vMatch3D2D with gaps),
the gather restated in numpy, the driver's build and the reading of its output."""
import os
import struct
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "pnp_check_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "pnp_check_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def scene(w, seed=0, n_kf=3, gaps=0.25):
    """CheckMatch's arguments around world w: every match of w becomes a map point seen from one of n_kf reference keyframes, the keypoints are w's pixels in a
    shuffled order among others, and vMatch3D2D has a share of unmatched (-1) entries in between."""
    g = np.random.default_rng(1000 + seed)
    n = len(w["Pw"])
    Twc = np.zeros((n_kf, 4, 4))
    for k in range(n_kf):
        q = g.normal(size=4); q /= np.linalg.norm(q); a, b, c, d = q
        Twc[k, :3, :3] = [[1 - 2*(c*c + d*d), 2*(b*c - a*d), 2*(b*d + a*c)], [2*(b*c + a*d), 1 - 2*(b*b + d*d), 2*(c*d - a*b)], [2*(b*d - a*c), 2*(c*d + a*b), 1 - 2*(b*b + c*c)]]
        Twc[k, :3, 3] = g.uniform(-1, 1, 3); Twc[k, 3, 3] = 1.0
    n_pts = n + int(round(gaps*n))
    slot = np.sort(g.permutation(n_pts)[:n])                            # where the matched map points stand, in the world's order
    kf = g.integers(0, n_kf, n_pts).astype(np.int32)
    rho = g.uniform(0.1, 0.6, n_pts)
    ray = g.normal(size=(n_pts, 3))
    P = w["Pw"].astype(np.float64)
    for i, s in enumerate(slot):
        T = Twc[kf[s]]
        ray[s] = (T[:3, :3].T @ (P[i] - T[:3, 3]))*rho[s]
    n_keys = n + 37
    key_of = g.permutation(n_keys)[:n]
    keys = g.uniform(0, 640, (n_keys, 2)).astype(np.float32)
    keys[key_of] = w["uv"]
    match = np.full(n_pts, -1, np.int32); match[slot] = key_of
    mK = np.array([[w["K"][0], 0, w["K"][2]], [0, w["K"][1], w["K"][3]], [0, 0, 1.0]])
    return dict(Twc=Twc, kf=kf, ray=ray, rho=rho, match=match, keys=keys, mK=mK, reproj=np.float32(w["reproj_err"]), slot=slot)


def gather(s):
    """pw = (Twr.block<3,3>(0,0) * ray / rho + Twr.block<3,1>(0,3)) in doubles, in the adapter's order of operations, then float; the matches' keypoints; K through floats."""
    m = np.flatnonzero(s["match"] >= 0)
    T = s["Twc"][s["kf"][m]]; ray = s["ray"][m]; rho = s["rho"][m]
    Pw = np.stack([((T[:, r, 0]*ray[:, 0] + T[:, r, 1]*ray[:, 1]) + T[:, r, 2]*ray[:, 2])/rho + T[:, r, 3] for r in range(3)], axis=1).astype(np.float32)
    uv = s["keys"][s["match"][m]]
    K = np.array([s["mK"][0, 0], s["mK"][1, 1], s["mK"][0, 2], s["mK"][1, 2]]).astype(np.float32).astype(np.float64)
    return Pw, uv, K


def write(path, s, mask=None, ok=True):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", len(s["Twc"]), len(s["match"]), len(s["keys"]))); f.write(s["mK"].astype(np.float64).tobytes()); f.write(struct.pack("<f", float(s["reproj"])))
        f.write(s["Twc"].astype(np.float64).tobytes())
        for i in range(len(s["match"])):
            f.write(struct.pack("<i", int(s["kf"][i]))); f.write(s["ray"][i].astype(np.float64).tobytes()); f.write(struct.pack("<d", float(s["rho"][i])))
        f.write(s["match"].astype(np.int32).tobytes()); f.write(s["keys"].astype(np.float32).tobytes())
        if mask is not None:
            f.write(struct.pack("<ii", int(ok), len(mask))); f.write(np.asarray(mask, np.uint8).tobytes())


def read(path, n_pts, host):
    raw = open(path, "rb").read(); off = 0

    def take(dt, k):
        nonlocal off
        a = np.frombuffer(raw, dt, k, off); off += a.nbytes
        return a
    n = int(take(np.int32, 1)[0])
    out = dict(n=n, Pw=take(np.float32, 3*n).reshape(n, 3), uv=take(np.float32, 2*n).reshape(n, 2), K=take(np.float64, 4))
    H = int(take(np.int32, 1)[0]); out["subset"] = take(np.int32, 5*H).reshape(H, 5)
    if host:
        out["ret"] = int(take(np.int32, 1)[0])
    else:
        out["called"], out["ret"] = [int(x) for x in take(np.int32, 2)]
        if out["called"]:
            out["result"] = take(np.int32, 4); out["pose"] = take(np.float64, 12); out["hyp_count"] = take(np.int32, H); out["inlier"] = take(np.uint8, n)
    out["match"] = take(np.int32, n_pts)
    assert off == len(raw)
    return out

"""Files of the two stand-alone programs of the two-view tests, shared by the host test, the GPU test and tools/diag/gpu_two_view.py: tests/cxx/two_view_host.hip
(the device's __host__ __device__ arithmetic on the CPU) and tests/cxx/two_view_from_cxx.cpp (adapter/tsorb_two_view.hpp over mock types)."""
import os
import struct
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- two_view_host
def build_host(exe, sanitize=True):
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cxx", "two_view_host.hip")])
    return exe


def write_host(path, w):
    n, H = len(w["xy1"]), len(w["subsets"])
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", n, H)); f.write(np.asarray(w["norm1"], F32).tobytes()); f.write(np.asarray(w["norm2"], F32).tobytes())
        f.write(struct.pack("<f", float(w["sigma"]))); f.write(np.ascontiguousarray(w["xy1"], F32).tobytes()); f.write(np.ascontiguousarray(w["xy2"], F32).tobytes())
        f.write(np.ascontiguousarray(w["subsets"], np.int32).tobytes())


def read_host(path, n, H):
    raw = open(path, "rb").read(); off = 0

    def take(dt, k):
        nonlocal off
        a = np.frombuffer(raw, dt, k, off); off += a.nbytes
        return a
    out = dict(hyp_model=take(F32, 18*H).reshape(2, H, 3, 3), hyp_score=take(F32, 2*H).reshape(2, H), sel=take(np.int32, 2), score=take(F32, 2))
    k = take(F32, 18); out["H21"], out["F21"] = k[:9].reshape(3, 3), k[9:].reshape(3, 3)
    out["inlier_h"] = take(np.uint8, n).astype(bool); out["inlier_f"] = take(np.uint8, n).astype(bool)
    assert off == len(raw)
    return out


# ---- what both comparisons (host program, device) assert
def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_floats(a, b):
    """Equal as bit patterns, NaNs in the same places (a NaN's sign and payload are the processor's)."""
    a = np.ascontiguousarray(a, F32); b = np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def check_scoring(R, got, w):
    """Bit for bit, no conditions needed: the restatement's scoring, keep loops and masks from the implementation's OWN float models."""
    d = R.derive(got["hyp_model"], w["xy1"], w["xy2"], w["sigma"])
    assert same_floats(got["hyp_score"], d["hyp_score"]), "hyp_score differs from the restatement's scoring of the same float models"
    assert np.array_equal(np.asarray(got["sel"]), d["sel"]), (got["sel"], d["sel"])
    assert same_floats(got["score"], d["score"])
    assert same_floats(got["H21"], d["H21"]) and same_floats(got["F21"], d["F21"])
    assert np.array_equal(got["inlier_h"], d["inlier_h"]) and np.array_equal(got["inlier_f"], d["inlier_f"])
    for m, k in enumerate(("inlier_h", "inlier_f")):
        if d["sel"][m] < 0:
            assert not got[k].any() and not np.asarray(got[("H21", "F21")[m]]).any() and got["score"][m] == 0


def check_models(R, got, ref, sens):
    """Every hyp_model entry within the larger of 1000 x model_sensitivity and one float ulp of the matrix's largest entry; degenerate hypotheses NaN in both.
    Returns the largest difference in units of the tolerance."""
    a, b = np.asarray(got["hyp_model"], F32), ref["hyp_model"]
    assert np.array_equal(np.isnan(a), np.isnan(b)), "degenerate hypotheses differ"
    tol = R.model_tolerance(b, sens)
    with np.errstate(invalid="ignore"):
        r = np.abs(a.astype(np.float64) - b.astype(np.float64))/tol
    worst = float(np.nanmax(r)) if np.isfinite(r).any() else 0.0
    assert worst <= 1.0, "a model entry is %.3g tolerances from the restatement's" % worst
    return worst


def check_decisions(R, got, ref):
    assert np.array_equal(np.asarray(got["sel"]), ref["sel"]), (got["sel"], ref["sel"])
    assert np.array_equal(got["inlier_h"], ref["inlier_h"]) and np.array_equal(got["inlier_f"], ref["inlier_f"])
    if (ref["sel"] >= 0).all():
        assert (R.RH(got) > 0.40) == (R.RH(ref) > 0.40)


# ---- two_view_from_cxx
def build_driver(tmp_path):
    exe = str(tmp_path / "two_view_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "two_view_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_scene(path, w, given=None):
    """The initializer's members around world w: mvKeys1, mvKeys2, mvMatches12, mvSets; given = the call's outputs for --host."""
    with open(path, "wb") as f:
        f.write(struct.pack("<iiiif", len(w["keys1"]), len(w["keys2"]), len(w["matches"]), len(w["subsets"]), float(w["sigma"])))
        f.write(np.ascontiguousarray(w["keys1"], F32).tobytes()); f.write(np.ascontiguousarray(w["keys2"], F32).tobytes())
        f.write(np.ascontiguousarray(w["matches"], np.int32).tobytes()); f.write(np.ascontiguousarray(w["subsets"], np.int32).tobytes())
        if given is not None:
            f.write(np.asarray(given["sel"], np.int32).tobytes()); f.write(np.asarray(given["score"], F32).tobytes())
            f.write(np.ascontiguousarray(given["H21"], F32).tobytes()); f.write(np.ascontiguousarray(given["F21"], F32).tobytes())
            f.write(np.asarray(given["inlier_h"], np.uint8).tobytes()); f.write(np.asarray(given["inlier_f"], np.uint8).tobytes())


def read_scene(path, host):
    raw = open(path, "rb").read(); off = 0

    def take(dt, k):
        nonlocal off
        a = np.frombuffer(raw, dt, k, off); off += a.nbytes
        return a
    out = dict(norm1=take(F32, 4), norm2=take(F32, 4)); n = int(take(np.int32, 1)[0])
    out.update(n=n, xy1=take(F32, 2*n).reshape(n, 2), xy2=take(F32, 2*n).reshape(n, 2)); H = int(take(np.int32, 1)[0])
    out["subset"] = take(np.int32, 8*H).reshape(H, 8); out["ret"] = int(take(np.int32, 1)[0]); out["SH"], out["SF"] = take(F32, 2)
    out["hasH"], out["hasF"] = [int(x) for x in take(np.int32, 2)]; out["H"] = take(F32, 9).reshape(3, 3); out["F"] = take(F32, 9).reshape(3, 3)
    out["inlH"] = take(np.uint8, n).astype(bool); out["inlF"] = take(np.uint8, n).astype(bool)
    if not host:
        out["sel"] = take(np.int32, 2)
    assert off == len(raw)
    return out

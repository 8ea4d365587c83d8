"""tsorb_match_text_theta_ransac on the GPU: the planes of a keyframe's new text detections in one call (include/tsorb.h, textslam_amd/csrc/tstexttheta.h) against
the numpy restatement (tests/text_theta_ref.py, docs/texttheta_recalled.md).  Per world:

  1. bit for bit, unconditional: from the device's OWN rho_out the restatement gives the device's hyp_theta, hyp_score, sel, theta and score as bit patterns, -0.0
     included, NaNs in the same places;
  2. points: every p3d within the larger of one float ulp of its largest coordinate and 1000 x the restatement's own sensitivity (the 4 x 4 moved at the 1e-13
     relative level in double), and rho_out = 1.0/(double)z of the device's own point;
  3. where p3d equals the restatement's in every bit, EVERY output equals the restatement's full answer outright -- and that holds on all committed worlds but at most
     one, so the comparison cannot quietly skip.

n = 3, 8, 63, 64, 65, 257, 1024 features per plane, 1, 64, 65, 200, 257 hypotheses, 1, 9 and 33 planes per call (mixed sizes, a plane without hypotheses, a plane of two
features); degenerate triples; rho given; a batch equals its planes one by one; every argument error with the outputs untouched; the resident frame and its grid
undisturbed; the adapter from C++ byte for byte."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_theta_ref as R                                            # noqa: E402
import text_theta_io as IO                                            # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("sel", "theta", "score", "p3d", "rho", "hyp_score", "hyp_theta")


@pytest.fixture(autouse=True)
def time_limit():
    """Each test under its own limit: a call that does not return ends the process with a traceback instead of holding the device."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ex():
    from textslam_amd.orbextractor import ORBextractor
    return ORBextractor()


@pytest.fixture(scope="module")
def worlds():
    """Every world, the restatement's answer and the triangulation's sensitivity -- computed once, read-only."""
    out = {}
    for name in R.ALL + R.GIVEN:
        w = R.make(name)
        out[name] = (w, R.answer(name) if name in R.ALL else R.run(w), R.sensitivity(w) if w.get("rho") is None else None)
    return out


def call(ex, w, **kw):
    g = lambda k: kw.get(k, w.get(k))
    return ex.match_text_theta_ransac(g("off"), g("host_xy"), g("targ_xy"), g("Tcr"), g("K"), g("hyp_off"), g("triple"), rho=g("rho"))


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def compare(ex, w, ref, sens):
    """Comparisons 1 - 3 of one world; returns whether the points equalled the restatement's in every bit."""
    got = call(ex, w)
    IO.check_bits(R, got, w)                                             # 1.
    if w.get("rho") is None:
        worst, same = IO.check_points(R, got, w, sens)                   # 2.
        print("points: largest difference %.3g of the tolerance, sensitivity %.2e, floats that differ %d of %d" % (
            worst, float(sens["rel"].max()) if len(sens["rel"]) else 0.0, int((got["p3d"].view(np.uint32) != ref["p3d"].view(np.uint32)).sum()), ref["p3d"].size))
    else:
        same = not got["p3d"].any() and R.same64(got["rho"], w["rho"])
        assert same
    if same:                                                             # 3.
        assert R.same_answer(got, ref), "the points are the restatement's but an output is not"
    return same


@pytest.mark.parametrize("name", R.ALL + R.GIVEN)
def test_against_the_restatement(ex, worlds, name):
    w, ref, sens = worlds[name]
    same = compare(ex, w, ref, sens)
    print(name, "sel", ref["sel"].tolist(), "points equal in every bit:", same)


def test_full_equality_on_all_worlds_but_one(ex, worlds):
    equal = {name: compare(ex, *worlds[name]) for name in R.ALL}
    print("worlds whose points differ somewhere:", [n for n, s in equal.items() if not s])
    assert sum(equal.values()) >= len(R.ALL) - 1


# ------------------------------------------------------------------ degenerate inputs
def _with(w, **kw):
    out = dict(w); out.update(kw)
    return out


def test_degenerate_triples(ex, worlds):
    """A third feature at x == cx exactly (m3[0] = 0: A and B are infinite, theta is NaN), the same feature first (m1[0] = 0 divides nothing: theta is finite), a
    repeated-index triple and a collinear one: whatever the closed form gives, the device gives the same bits, and a NaN score is never kept."""
    w = worlds["n8_h64"][0]; cx = float(w["K"][2])
    host = w["host_xy"].copy(); host[5, 0] = np.float32(cx); assert float(host[5, 0]) == cx
    host[0, 1] = host[1, 1] = host[2, 1]                                  # features 0, 1, 2 on one image row: collinear rays
    tri = w["triple"].copy(); tri[0] = (1, 2, 5); tri[1] = (5, 1, 2); tri[2] = (0, 0, 0); tri[3] = (0, 1, 2); tri[4] = (3, 3, 4)
    d = _with(w, host_xy=host, triple=tri)
    got = call(ex, d); IO.check_bits(R, got, d)
    ref = R.run(d, rho=got["rho"])
    assert np.isnan(got["hyp_theta"][0]).all() and np.isnan(got["hyp_score"][0])
    assert np.isfinite(got["hyp_theta"][1]).all() and np.isfinite(got["hyp_score"][1])
    assert R.same64(got["hyp_theta"][2:5], ref["hyp_theta"][2:5]) and R.same64(got["hyp_score"][2:5], ref["hyp_score"][2:5])
    assert got["sel"][0] == ref["sel"][0] and got["sel"][0] >= 0 and not np.isnan(got["hyp_score"][got["sel"][0]])
    assert got["sel"][0] not in (0,)


def test_outliers_only_and_all_nan(ex, worlds):
    """Every target 500 px away: every score is 0.0 and `-1.0 < 0.0` keeps hypothesis 0.  Every triple ending at x == cx: every score is NaN, nothing is kept."""
    w = worlds["n20_h200"][0]
    far = _with(w, targ_xy=w["targ_xy"] + np.float32(500.0))
    got = call(ex, far); IO.check_bits(R, got, far)
    assert not got["hyp_score"].any() and not np.signbit(got["hyp_score"]).any() and got["sel"].tolist() == [0] and got["score"][0] == 0.0
    assert R.same64(got["theta"][0], got["hyp_theta"][0]) and np.isfinite(got["theta"]).all()
    host = w["host_xy"].copy(); host[7, 0] = np.float32(w["K"][2])
    tri = w["triple"].copy(); tri[:, 0] = 1; tri[:, 1] = 2; tri[:, 2] = 7
    nan = _with(w, host_xy=host, triple=tri)
    got = call(ex, nan); IO.check_bits(R, got, nan)
    assert np.isnan(got["hyp_score"]).all() and got["sel"].tolist() == [-1] and not got["theta"].any() and not got["score"].any()


def test_rho_given(ex, worlds):
    """Feeding a call's rho_out back reproduces its thetas and scores; p3d is then zero.  The initializer's world gives the restatement's answer."""
    for name in ("n65_h257", "mixed_9"):
        w = worlds[name][0]; got = call(ex, w)
        again = call(ex, w, rho=got["rho"])
        assert all(np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes() for k in KEYS if k != "p3d") and not again["p3d"].any()


def test_batch_equals_its_planes_and_call_is_a_function(ex, worlds):
    w = worlds["mixed_9"][0]; got = call(ex, w)
    for p in range(len(w["off"]) - 1):
        s = call(ex, R.plane_world(w, p))
        a, b, h0, h1 = w["off"][p], w["off"][p + 1], w["hyp_off"][p], w["hyp_off"][p + 1]
        assert s["sel"].tobytes() == got["sel"][p:p + 1].tobytes() and s["theta"].tobytes() == got["theta"][p:p + 1].tobytes() and s["score"].tobytes() == got["score"][p:p + 1].tobytes()
        assert s["p3d"].tobytes() == got["p3d"][a:b].tobytes() and s["rho"].tobytes() == got["rho"][a:b].tobytes()
        assert s["hyp_score"].tobytes() == got["hyp_score"][h0:h1].tobytes() and s["hyp_theta"].tobytes() == got["hyp_theta"][h0:h1].tobytes()
    assert got["sel"][2] == -1 and got["sel"][5] == -1 and not got["theta"][[2, 5]].any() and not got["hyp_score"][w["hyp_off"][2]:w["hyp_off"][3]].any()
    assert same_bytes(call(ex, w), got)
    other = call(ex, worlds["batch_33"][0]); assert len(other["sel"]) == 33
    assert same_bytes(call(ex, w), got) and same_bytes(call(ex, worlds["batch_33"][0]), other)


# ------------------------------------------------------------------ argument errors
F32, F64, I32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
NAME = "tsorb_match_text_theta_ransac"
_OUT = dict(sel=(I32, -77), theta=(F64, 7.0), score=(F64, 7.0), p3d=(F32, 7.0), rho_out=(F64, 7.0), hyp_score=(F64, 7.0), hyp_theta=(F64, 7.0))
_IN = dict(off=I32, host_xy=F32, targ_xy=F32, rho=F64, Tcr=F64, K=F64, hyp_off=I32, triple=I32)


def _raw(ex, w, n_plane=None, null=(), ctx=True, mutate=None):
    a = dict(off=np.asarray(w["off"], np.int32).copy(), host_xy=np.ascontiguousarray(w["host_xy"], np.float32).copy(), targ_xy=np.ascontiguousarray(w["targ_xy"], np.float32).copy(),
             rho=None if w.get("rho") is None else np.asarray(w["rho"], np.float64).copy(), Tcr=np.ascontiguousarray(np.asarray(w["Tcr"], np.float64)[:3, :4]).copy(),
             K=np.asarray(w["K"], np.float64).copy(), hyp_off=np.asarray(w["hyp_off"], np.int32).copy(), triple=np.ascontiguousarray(w["triple"], np.int32).copy())
    if mutate:
        mutate(a)
    P, N, H = len(a["off"]) - 1, len(a["host_xy"]), len(a["triple"])
    shape = dict(sel=P, theta=(P, 3), score=P, p3d=(N, 3), rho_out=N, hyp_score=H, hyp_theta=(H, 3))
    o = {k: np.full(shape[k], v, {I32: np.int32, F32: np.float32, F64: np.float64}[t]) for k, (t, v) in _OUT.items()}
    pi = lambda k: None if (k in null or a[k] is None) else a[k].ctypes.data_as(_IN[k])
    po = lambda k: None if k in null else o[k].ctypes.data_as(_OUT[k][0])
    rc = ex.lib.tsorb_match_text_theta_ransac(ex.ctx if ctx else None, P if n_plane is None else n_plane, pi("off"), pi("host_xy"), pi("targ_xy"), pi("rho"), pi("Tcr"), pi("K"),
                                              pi("hyp_off"), pi("triple"), *[po(k) for k in _OUT])
    return rc, all(bool((o[k] == v).all()) for k, (_, v) in _OUT.items()), o


def test_arguments(ex, worlds):
    w = worlds["mixed_9"][0]
    ref = call(ex, w)

    def refused(named=True, world=w, **kw):
        rc, untouched, _ = _raw(ex, world, **kw)
        assert rc == -1 and untouched, kw
        if named:
            assert NAME in ex.lib.tsorb_last_error(ex.ctx).decode()

    refused(ctx=False, named=False)
    refused(n_plane=-1)
    for k in ("off", "host_xy", "targ_xy", "Tcr", "K", "hyp_off", "triple", "sel", "theta", "score"):
        refused(null=(k,))

    def mut(key, idx, val):
        def m(a): a[key][idx] = val
        return m
    h1 = int(w["hyp_off"][1])
    refused(mutate=mut("triple", (0, 0), 8)); refused(mutate=mut("triple", (0, 2), -1)); refused(mutate=mut("triple", (h1, 1), 63))      # planes 0 and 1 have 8 and 63 features
    refused(mutate=mut("triple", (len(w["triple"]) - 1, 2), 12))
    assert "plane 1" in ex.lib.tsorb_last_error(ex.ctx).decode() or "plane 8" in ex.lib.tsorb_last_error(ex.ctx).decode()
    refused(mutate=mut("off", 0, 1)); refused(mutate=mut("hyp_off", 0, 1)); refused(mutate=mut("off", 3, 0)); refused(mutate=mut("hyp_off", 2, 10**6))
    big = R.batch_world(5, [8, 1025], [4, 4])                             # above TSORB_THETA_MAX_FEAT
    refused(world=big)
    assert "plane 1" in ex.lib.tsorb_last_error(ex.ctx).decode() and "TSORB_THETA_MAX_FEAT" in ex.lib.tsorb_last_error(ex.ctx).decode()
    rc, untouched, _ = _raw(ex, w, n_plane=0)                             # no plane: nothing is launched, nothing is written
    assert rc == 0 and untouched
    # the optional outputs may be NULL, and the context still answers
    name_of = lambda k: "rho" if k == "rho_out" else k
    same = lambda o, keys: all(np.asarray(o[k]).reshape(-1).tobytes() == np.asarray(ref[name_of(k)]).reshape(-1).tobytes() for k in keys)
    rc, untouched, o = _raw(ex, w)
    assert rc == 0 and not untouched and same(o, _OUT)
    opt = ("p3d", "rho_out", "hyp_score", "hyp_theta")
    for null in (opt, ("p3d",), ("rho_out", "hyp_theta"), ("hyp_score",), ("p3d", "rho_out", "hyp_theta")):
        rc, _, o = _raw(ex, w, null=null)
        assert rc == 0 and same(o, [k for k in _OUT if k not in null]) and all((o[k] == _OUT[k][1]).all() for k in null), null
    assert same_bytes(call(ex, w), ref)


def test_resident_frame_not_disturbed(worlds):
    """A call between tsorb_match_set_frame and tsorb_match_search leaves the resident batch, the grid and the search results as they were."""
    from textslam_amd.orbextractor import ORBextractor, synthetic_frame
    w, ref, sens = worlds["batch_33"]
    ex2 = ORBextractor()
    ex2.extract_batch(np.stack([synthetic_frame(2, 320, 240), synthetic_frame(3, 320, 240)]))
    rng = np.random.default_rng(11)
    before = ex2.download()
    q = rng.choice(len(before[1][0]), 40, replace=False)
    args = (before[1][0][q, :2] + rng.uniform(-3, 3, (40, 2)).astype(np.float32), np.full(40, 12.0, np.float32), None, before[1][1][q])
    ex2.match_set_frame(1, (0.0, 320.0, 0.0, 240.0))
    m0 = ex2.match_search(*args)
    assert (m0["cand_cnt"] > 0).any()
    ex2.match_set_frame(1, (0.0, 320.0, 0.0, 240.0))
    got = call(ex2, w)
    m1 = ex2.match_search(*args)
    IO.check_bits(R, got, w); IO.check_points(R, got, w, sens)
    after = ex2.download()
    assert all(b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes() for b, a in zip(before, after))
    assert all(m0[k].tobytes() == m1[k].tobytes() for k in m0)


def test_adapter_from_cxx(tmp_path, ex, worlds):
    """adapter/tsorb_text_theta.hpp's two bodies over the driver's mock types: the gather, the draws and ONE call; mNcr and vNGOOD byte for byte what the Python mirror
    gives on the same arrays and triples."""
    exe = IO.build_driver(tmp_path)
    for name, mode in (("mixed_9", "track"), ("batch_33", "track"), ("init_9", "init")):
        w = worlds[name][0]
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w, mode, w.get("rho"))
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "text theta from C++: ok" in r.stdout, r.stdout + r.stderr
        o = IO.read_scene(outp)
        d = IO.scene_call(w, mode, o)                                    # the batch the adapter must have formed, with the triples it drew
        got = call(ex, d)
        IO.check_scene(o, w, mode, d, got)

"""tsorb_match_search_claim and tsorb_match_new_points on the GPU: the stateful window search of a new keyframe (and of the initializer) and the new scene points in one
call (include/tsorb.h, textslam_amd/csrc/tsclaim.h) against the numpy restatement (tests/new_points_ref.py, docs/newpoints_recalled.md).  Per world:

  1. match12, match_dist and n_match equal the restatement's, unconditionally;
  2. every p3d within the larger of one float ulp of its largest coordinate and 1000 x the restatement's own sensitivity (the 4 x 4 moved at the 1e-13 relative level
     in double);
  3. good and n_good equal the restatement's check applied to the device's OWN points, bit for bit;
  4. where the points equal the restatement's in every bit, good and n_good equal the restatement's full answer outright -- and that holds on all committed worlds
     but at most one, so the comparison cannot quietly skip.

Searched sets of 1, 63, 64, 65, 1000 and 5000 features; 0, 1, 4, 5, 255, 256, 257 and 3000 queries; windows of 0, 1, 64, 65, 129 and 600 candidates (600: above the
row a query's list has in scratch), a window that leaves the grid and queries outside it; the level filter on and off; elig2 NULL and half zero; queries that contend
for a few features; 0, 1, 64, 65 and 257 matches entering the triangulation.  The two calls agree; a fresh chain's first query is tsorb_match_search's; the resident
batch, the grid and a following search undisturbed; every argument error with the outputs untouched; the adapter from C++ byte for byte."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import new_points_ref as R                                            # noqa: E402
import new_points_io as IO                                            # noqa: E402

pytestmark = pytest.mark.gpu


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


def set_grid(ex, w):
    ex.match_set_features(w["kp6"], w["desc2"], w["bounds"])


def search(ex, w, **kw):
    g = lambda k: kw.get(k, w.get(k))
    return ex.match_search_claim(g("qxy"), g("qr"), g("qlev"), g("qdesc"), elig2=g("elig2"), th_low=g("th_low"), use_ratio=g("use_ratio"), ratio=g("ratio"))


def points(ex, w, **kw):
    g = lambda k: kw.get(k, w.get(k))
    return ex.match_new_points(g("qxy"), g("qr"), g("qlev"), g("qdesc"), g("q_px"), g("Trw"), g("Tcw"), g("K"), elig2=g("elig2"), th_low=g("th_low"), use_ratio=g("use_ratio"),
                               ratio=g("ratio"), th_reproj=g("th_reproj"))


def compare(ex, name):
    """Comparisons 1 - 4 of one world; returns whether the points equalled the restatement's in every bit."""
    w, ref, sens = R.make(name), R.answer(name), R.sens(name)
    set_grid(ex, w)
    s = search(ex, w); IO.check_matches(s, ref)                          # 1.
    got = points(ex, w); IO.check_matches(got, ref)
    assert got["match12"].tobytes() == s["match12"].tobytes() and got["n_match"] == s["n_match"]       # the two calls agree byte for byte
    worst, same = IO.check_points(R, got, ref, sens)                     # 2.
    print("%s: n_match %d n_good %d; points: largest difference %.3g of the tolerance, sensitivity %.2e, floats that differ %d of %d" % (
        name, got["n_match"], got["n_good"], worst, float(sens["rel"].max()) if len(sens["rel"]) else 0.0,
        int((got["p3d"].view(np.uint32) != ref["p3d"].view(np.uint32)).sum()), ref["p3d"].size))
    IO.check_verdicts(R, w, got, ref, same)                              # 3. and 4.
    return same


@pytest.mark.parametrize("name", R.ALL)
def test_against_the_restatement(ex, name):
    compare(ex, name)


def test_full_equality_on_all_worlds_but_one(ex):
    equal = {name: compare(ex, name) for name in R.ALL}
    print("worlds whose points differ somewhere:", [n for n, s in equal.items() if not s])
    assert sum(equal.values()) >= len(R.ALL) - 1


def test_chain_variants_on_one_grid(ex):
    """The same queries with the level filter off, with half the set not eligible, with the ratio test and with other thresholds: the restatement's answer each time,
    and the first call's answer again afterwards (a call is a function of its arguments)."""
    w = R.make("s1000_q256"); set_grid(ex, w); first = search(ex, w)
    half = (np.arange(len(w["kp6"])) % 2 == 1).astype(np.uint8)
    for kw in (dict(qlev=None), dict(elig2=None), dict(elig2=half), dict(use_ratio=True, ratio=0.9), dict(use_ratio=True, ratio=0.5), dict(th_low=20), dict(th_low=0), dict(th_low=256),
               dict(qr=np.full(len(w["qr"]), 300.0, np.float32), qlev=None)):
        d = dict(w); d.update(kw)
        IO.check_matches(search(ex, d), R.run(d))
    again = search(ex, w)
    assert all(np.asarray(again[k]).tobytes() == np.asarray(first[k]).tobytes() for k in first)


def test_first_query_of_a_fresh_chain_is_match_search(ex):
    """With a 40-px radius and elig2 = NULL the first query of a fresh chain sees what tsorb_match_search sees: best_idx, and best_dist when it is accepted."""
    w = R.make("s1000_q256"); set_grid(ex, w); n = 0
    for q in range(0, 60):
        one = {k: w[k][q:q + 1] for k in ("qxy", "qlev", "qdesc")}; r40 = np.full(1, 40.0, np.float32)
        m = ex.match_search(one["qxy"], r40, one["qlev"], one["qdesc"], max_cand=4)
        s = ex.match_search_claim(one["qxy"], r40, one["qlev"], one["qdesc"], th_low=256)
        assert s["match12"][0] == m["best_idx"][0] and s["match_dist"][0] == (m["best_dist"][0] if m["best_idx"][0] >= 0 else -1)
        n += int(m["best_idx"][0] >= 0)
    assert n >= 10


def test_large_set_takes_the_large_lds(ex):
    """65536 features: vMatchDist takes 128 KB of LDS, above what a launch gets without asking."""
    w = R.scene_world(77, 65536, 40, bad_every=7)
    set_grid(ex, w); ref = R.run(w)
    got = points(ex, w); IO.check_matches(got, ref)
    _, same = IO.check_points(R, got, ref, R.sensitivity(w, ref["match12"])); IO.check_verdicts(R, w, got, ref, same)
    assert ref["n_match"] >= 20


# ------------------------------------------------------------------ undisturbed
def test_resident_frame_grid_and_search_not_disturbed():
    from textslam_amd.orbextractor import ORBextractor, synthetic_frame
    ex2 = ORBextractor()
    ex2.extract_batch(np.stack([synthetic_frame(2, 320, 240), synthetic_frame(3, 320, 240)]))
    rng = np.random.default_rng(11)
    before = ex2.download(); kp, desc = before[1]
    q = rng.choice(len(kp), 40, replace=False)
    args = (kp[q, :2] + rng.uniform(-3, 3, (40, 2)).astype(np.float32), np.full(40, 12.0, np.float32), None, desc[q])
    ex2.match_set_frame(1, (0.0, 320.0, 0.0, 240.0))
    m0 = ex2.match_search(*args)
    assert (m0["cand_cnt"] > 0).any()
    # the calls search the RESIDENT frame's grid: the restatement on the downloaded features
    w = dict(kp6=kp, desc2=desc, bounds=(0.0, 320.0, 0.0, 240.0), qxy=args[0], qr=np.full(40, 30.0, np.float32), qlev=None, qdesc=args[3], elig2=None, th_low=50, use_ratio=False,
             ratio=0.9, q_px=args[0], Trw=R.make("pairs_64")["Trw"], Tcw=R.make("pairs_64")["Tcw"], K=R.make("pairs_64")["K"], th_reproj=9)
    ref = R.run(w)
    got = points(ex2, w); s = search(ex2, w)
    IO.check_matches(got, ref); IO.check_matches(s, ref); assert ref["n_match"] >= 10
    m1 = ex2.match_search(*args)
    after = ex2.download()
    assert all(b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes() for b, a in zip(before, after))
    assert all(m0[k].tobytes() == m1[k].tobytes() for k in m0)


# ------------------------------------------------------------------ argument errors
FP, DP, IP, UP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
_IN = dict(qxy=(FP, np.float32), qr=(FP, np.float32), qlev=(IP, np.int32), qdesc=(UP, np.uint8), elig2=(UP, np.uint8), q_px=(FP, np.float32), Trw=(DP, np.float64),
           Tcw=(DP, np.float64), K=(DP, np.float64))


def _raw(ex, w, fn, nq=None, null=(), ctx=True, mutate=None, **kw):
    a = {k: (None if w.get(k) is None else np.ascontiguousarray(w[k] if k not in ("Trw", "Tcw") else np.asarray(w[k])[:3, :4], dt).copy()) for k, (_, dt) in _IN.items()}
    if mutate:
        mutate(a)
    n = len(a["qxy"]) if nq is None else nq; m = max(len(a["qxy"]), 1)
    o = dict(match12=np.full(m, -77, np.int32), match_dist=np.full(m, -77, np.int32), n_match=np.full(1, -77, np.int32), p3d=np.full((m, 3), 7.0, np.float32),
             good=np.full(m, 77, np.uint8), n_good=np.full(1, -77, np.int32))
    pi = lambda k: None if (k in null or a[k] is None) else a[k].ctypes.data_as(_IN[k][0])
    po = lambda k, t: None if k in null else o[k].ctypes.data_as(t)
    g = lambda k: kw.get(k, w[k])
    head = (ex.ctx if ctx else None, n, pi("qxy"), pi("qr"), pi("qlev"), pi("qdesc"), pi("elig2"), int(g("th_low")), int(g("use_ratio")), float(g("ratio")))
    if fn == "search":
        rc = ex.lib.tsorb_match_search_claim(*head, po("match12", IP), po("match_dist", IP), po("n_match", IP)); keys = ("match12", "match_dist", "n_match")
    else:
        rc = ex.lib.tsorb_match_new_points(*head, pi("q_px"), pi("Trw"), pi("Tcw"), pi("K"), int(w["th_reproj"]), po("match12", IP), po("n_match", IP), po("p3d", FP),
                                           po("good", UP), po("n_good", IP)); keys = ("match12", "n_match", "p3d", "good", "n_good")
    fill = dict(match12=-77, match_dist=-77, n_match=-77, p3d=7.0, good=77, n_good=-77)
    return rc, all(bool((o[k] == fill[k]).all()) for k in keys), o


@pytest.mark.parametrize("fn", ["search", "points"])
def test_arguments(ex, fn):
    w = R.make("s63_q4"); set_grid(ex, w); name = "tsorb_match_search_claim" if fn == "search" else "tsorb_match_new_points"

    def refused(named=True, world=w, on=ex, **kw):
        rc, untouched, _ = _raw(on, world, fn, **kw)
        assert rc == -1 and untouched, kw
        if named:
            assert name in on.lib.tsorb_last_error(on.ctx).decode(), on.lib.tsorb_last_error(on.ctx)

    refused(ctx=False, named=False)
    refused(nq=-1)
    required = ("qxy", "qr", "qdesc", "match12", "n_match") + (("q_px", "Trw", "Tcw", "K", "p3d", "good", "n_good") if fn == "points" else ())
    for k in required:
        refused(null=(k,))

    def mut(key, idx, val):
        def m(a): a[key][idx] = val
        return m
    for val in (np.nan, np.inf, -np.inf):
        refused(mutate=mut("qxy", (1, 0), val)); refused(mutate=mut("qxy", (3, 1), val)); refused(mutate=mut("qr", 2, val))
    refused(mutate=mut("qr", 0, -1.0))
    refused(th_low=-1); refused(th_low=257)
    refused(use_ratio=1, ratio=np.nan); refused(use_ratio=1, ratio=np.inf); refused(use_ratio=1, ratio=-0.5)
    rc, untouched, _ = _raw(ex, w, fn, use_ratio=0, ratio=np.nan)        # the ratio is not looked at without use_ratio
    assert rc == 0 and not untouched
    from textslam_amd.orbextractor import ORBextractor
    fresh = ORBextractor()
    refused(on=fresh)                                                     # no grid set
    big = R.scene_world(78, 65537, 2)
    fresh.match_set_features(big["kp6"], big["desc2"], big["bounds"])
    refused(on=fresh, world=big); assert "TSORB_BRUTE_MAX_FEAT" in fresh.lib.tsorb_last_error(fresh.ctx).decode()
    # no query: OK, the counts are zero, nothing else is written; the optional pointers may be NULL
    rc, _, o = _raw(ex, w, fn, nq=0)
    assert rc == 0 and o["n_match"][0] == 0 and (o["match12"] == -77).all() and (fn == "search" or (o["n_good"][0] == 0 and (o["good"] == 77).all()))
    ref = R.answer("s63_q4")
    for null in ((), ("qlev",), ("match_dist",) if fn == "search" else ("elig2",)):
        d = dict(w, qlev=None) if "qlev" in null else w
        rc, _, o = _raw(ex, d, fn, null=null)
        r = R.run(d) if "qlev" in null else ref
        assert rc == 0 and np.array_equal(o["match12"], r["match12"]) and o["n_match"][0] == r["n_match"]
        if "match_dist" in null:
            assert (o["match_dist"] == -77).all()


def test_adapter_from_cxx(tmp_path, ex):
    """adapter/tsorb_new_points.hpp's two bodies over the driver's mock types: the gather of the queries, ONE call, the scatter; vMatchIdx12, vNewpts and vNewptsMatch
    byte for byte what the Python mirror gives on the queries the adapter must have formed."""
    exe = IO.build_driver(tmp_path)
    for name, mode in (("s1000_q256", "track"), ("pairs_65", "track"), ("s64_q5_none", "track"), ("init_s1000_q257", "init")):
        w = R.make(name)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w, mode)
        r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "new points from C++: ok" in r.stdout, r.stdout + r.stderr
        o = IO.read_scene(outp, 2*len(w["qxy"]))
        set_grid(ex, w)
        got = points(ex, w) if mode == "track" else dict(search(ex, w), n_good=0, good=np.zeros(len(w["qxy"]), bool), p3d=np.zeros((len(w["qxy"]), 3), np.float32))
        IO.check_scene(o, w, mode, got)

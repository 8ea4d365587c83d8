"""The restatement of a keyframe's new scene points (tests/new_points_ref.py, docs/newpoints_recalled.md) on its own, and the device's __host__ __device__ decisions
and arithmetic on the CPU against it -- no GPU:

  * hand examples of the chain with descriptors crafted to exact bit counts: a steal, a steal of a steal, a candidate hidden by vMatchDist == dist, a tie won by the
    candidate earlier in CELL order although its index is higher, the th_low and ratio boundaries, a lone candidate, an ineligible nearest candidate;
  * a hand triangulation in dyadic rationals between two non-identity cameras; the check function on given points;
  * the worlds cover the sizes the kernels branch on;
  * tests/cxx/new_points_host.hip, built with the address and undefined-behaviour sanitizers, bit-equal to the restatement on every committed world, with the full
    comparison holding on all of them but at most one;
  * adapter/tsorb_new_points.hpp's two bodies over mock types in --host mode against a plain transcription of the reference's loops."""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import new_points_ref as R                                            # noqa: E402
import new_points_io as IO                                            # noqa: E402

F32, F64 = np.float32, np.float64


def bits(k, start=0):
    """A descriptor with exactly k bits set, from bit `start` on."""
    b = np.zeros(256, np.uint8); b[start:start + k] = 1
    return np.packbits(b)


def hand(feat, queries, elig2=None, th_low=50, use_ratio=False, ratio=0.9, r=20.0):
    """feat: (x, y, bits set) per feature of the frame; queries: (x, y, bits set) -- all descriptors are prefixes of ones, so the distance is the difference of the
    counts.  One octave, no level filter."""
    kp6 = np.zeros((len(feat), 6), F32); kp6[:, :2] = [f[:2] for f in feat]
    return dict(kp6=kp6, desc2=np.stack([bits(f[2]) for f in feat]), bounds=R.BOUNDS, qxy=np.array([q[:2] for q in queries], F32), qr=np.full(len(queries), r, F32), qlev=None,
                qdesc=np.stack([bits(q[2]) for q in queries]), elig2=elig2, th_low=th_low, use_ratio=use_ratio, ratio=ratio)


def test_hamming_and_candidate_order():
    assert R.hamming(bits(7), np.stack([bits(7), bits(0), bits(256), bits(3, 5)])).tolist() == [0, 7, 249, 5 + 1]
    # features 0 and 1 in one cell (index order inside it), feature 2 in the column to the LEFT: the window walks column by column, so 2 comes first
    w = hand([(107.0, 100.0, 0), (108.0, 101.0, 0), (96.0, 100.0, 0)], [(100.0, 100.0, 0)])
    c, d = R.lists(w)[0]
    assert c.tolist() == [2, 0, 1] and d.tolist() == [0, 0, 0]
    assert len(R.lists(hand([(105.0, 100.0, 0)], [(100.0, 100.0, 0)], r=5.0))[0][0]) == 0          # |dx| < r is strict


def test_chain_hand_examples():
    A, B = (100.0, 100.0), (300.0, 300.0)
    # a steal: query 1 is closer to the feature than query 0 was
    m, d, n = R.chain(hand([A + (10,)], [A + (20,), A + (14,)]))
    assert m.tolist() == [-1, 0] and d.tolist() == [-1, 4] and n == 1
    # a steal of a steal; then a query that is no closer gets nothing
    m, d, n = R.chain(hand([A + (10,)], [A + (20,), A + (14,), A + (11,), A + (11,)]))
    assert m.tolist() == [-1, -1, 0, -1] and d.tolist() == [-1, -1, 1, -1] and n == 1
    # hidden by vMatchDist == dist (`<=`): query 1 at the same distance does not take the feature, and falls back to the farther one
    m, d, n = R.chain(hand([A + (10,), A + (40,)], [A + (14,), A + (14,)]))
    assert m.tolist() == [0, 1] and d.tolist() == [4, 26] and n == 2
    # a tie in distance: the candidate earlier in CELL order wins although its index is higher (feature 1 lies a column to the left)
    m, d, n = R.chain(hand([(107.0, 100.0, 10), (96.0, 100.0, 10)], [A + (13,)]))
    assert m.tolist() == [1] and d.tolist() == [3]
    # best == 50 is accepted, 51 is not
    assert R.chain(hand([A + (0,)], [A + (50,)]))[0].tolist() == [0] and R.chain(hand([A + (0,)], [A + (51,)]))[0].tolist() == [-1]
    # the ratio: 44 against 50 is accepted (44 < 45.0), 45 against 50 is not (45 < 45.0 is false)
    assert R.chain(hand([A + (0,), A + (94,)], [A + (44,)], use_ratio=True))[0].tolist() == [0]
    assert R.chain(hand([A + (0,), A + (95,)], [A + (45,)], use_ratio=True))[0].tolist() == [-1]
    assert R.chain(hand([A + (0,), A + (95,)], [A + (45,)], use_ratio=False))[0].tolist() == [0]
    # a lone candidate: the runner-up is INT_MAX, so the ratio accepts it
    assert R.chain(hand([A + (0,)], [A + (50,)], use_ratio=True))[0].tolist() == [0]
    # a hidden candidate is no runner-up either: after query 0 took feature 0 at distance 0, query 1 sees feature 1 alone
    m, d, n = R.chain(hand([A + (0,), A + (40,)], [A + (0,), A + (2,)], use_ratio=True))
    assert m.tolist() == [0, 1] and d.tolist() == [0, 38]
    # an ineligible nearest candidate: the next one is taken; with nothing else there is no match
    assert R.chain(hand([A + (10,), A + (30,)], [A + (12,)], elig2=np.array([0, 1], np.uint8)))[0].tolist() == [1]
    assert R.chain(hand([A + (10,)], [A + (12,)], elig2=np.array([0], np.uint8)))[0].tolist() == [-1]
    # queries elsewhere do not interfere
    m, d, n = R.chain(hand([A + (10,), B + (10,)], [A + (12,), B + (13,)]))
    assert m.tolist() == [0, 1] and n == 2


def _hand_cameras():
    """K = (2, 2, 1, 1); Trw = [I | (1, 0, 0)], Tcw = [I | (-1, 0, 0)]; the point (1, 2, 4) is (2, 2, 4) in camera 1 -> rays (0.5, 0.5) -> pixel (2, 2), and
    (0, 2, 4) in camera 2 -> rays (0, 0.5) -> pixel (1, 2)."""
    return dict(K=np.array([2.0, 2, 1, 1]), Trw=np.array([[1, 0, 0, 1.0], [0, 1, 0, 0], [0, 0, 1, 0]]), Tcw=np.array([[1, 0, 0, -1.0], [0, 1, 0, 0], [0, 0, 1, 0]]), th_reproj=9)


def test_hand_triangulation():
    w = _hand_cameras(); pt1 = np.array([[2, 2]], F32); pt2 = np.array([[1, 2]], F32)
    A = R.system(w, pt1, pt2)
    # x1 = y1 = 0.5, x2 = 0, y2 = 0.5: rows x*P[2] - P[0], y*P[2] - P[1] of both cameras
    assert np.array_equal(A[0], np.array([[-1, 0, .5, -1], [0, -1, .5, 0], [-1, 0, 0, 1], [0, -1, .5, 0]]))
    assert not (A[0] @ np.array([1, 2, 4, 1.0])).any()                   # (1, 2, 4, 1) in its null space exactly
    X = R.triangulate(w, pt1, pt2)
    assert (np.abs(X.astype(F64) - np.array([[1, 2, 4.0]])) <= np.spacing(F32(4))).all()
    assert R.check(w, X, pt1, pt2).tolist() == [True]


def test_check_on_given_points():
    w = _hand_cameras(); P = lambda *x: np.array([x], F32)
    one = lambda X, p1=(2, 2), p2=(1, 2): bool(R.check(w, X, np.array([p1], F32), np.array([p2], F32))[0])
    assert one(P(1, 2, 4))
    assert not one(P(np.inf, 2, 4)) and not one(P(1, np.nan, 4)) and not one(P(1, 2, -np.inf))
    # u1 = 2 (X + 1)/Z + 1 < 0 for X = -4: refused whatever the pixels
    assert not one(P(-4, 2, 4), p1=(-0.5, 2), p2=(-1.5, 2))
    # first error: the point is exact; pixel 1 moved by 3 px -> 9 is not > 9; by 3 + 2^-10 -> 9.0059 refused; by 3 - 2^-10 -> 8.9941 kept
    eps = 2.0**-10
    assert one(P(1, 2, 4), p1=(5, 2)) and not one(P(1, 2, 4), p1=(5 + eps, 2)) and one(P(1, 2, 4), p1=(5 - eps, 2))
    # second error likewise
    assert one(P(1, 2, 4), p2=(1, 5)) and not one(P(1, 2, 4), p2=(1, 5 + eps)) and one(P(1, 2, 4), p2=(1, 5 - eps))
    # the error is rounded to FLOAT before the comparison: 9 + 2^-30 in double is 9 in float
    assert float(F32(9.0 + 2.0**-30)) == 9.0
    # Z = 0: u1 = 4/0 = inf, (inf - 2)^2 = inf > 9 refuses; but the camera's own centre gives 0/0 = NaN, and a NaN passes `< 0` and `> 9` alike, as written
    assert not one(P(1, 2, 0))
    assert one(P(-1, 0, 0))                                              # image 1: NaN; image 2: (-inf - 1)^2 + NaN^2 = NaN as well: kept, as written
    assert not one(P(-1, 1, 0))                                          # image 1: NaN^2 + inf = NaN passes; image 2: inf + inf = inf refuses
    # behind both cameras: (-3, -2, -4) is (-2, -2, -4) in camera 1 -> pixel (2, 2) and (-4, -2, -4) in camera 2 -> pixel (3, 2); there is no depth test
    assert one(P(-3, -2, -4), p1=(2, 2), p2=(3, 2))


def test_worlds_cover_the_shapes():
    n2s, nqs, cnts, nms, lev, el = set(), set(), set(), set(), set(), set()
    for name in R.ALL:
        w = R.make(name); a = R.answer(name); cl = R.cand_lists(name)
        n2s.add(len(w["kp6"])); nqs.add(len(w["qxy"])); nms.add(a["n_match"]); lev.add(w["qlev"] is None); el.add(w["elig2"] is None)
        elig = np.ones(len(w["kp6"]), bool) if w["elig2"] is None else w["elig2"] != 0
        cnts |= {int(elig[c].sum()) for c, _ in cl}
        s = R.sens(name)
        assert 1000.0*float(s["rel"].max() if len(s["rel"]) else 0.0) < 6e-8 and not (s["ulp"] > 0).any(), name      # the fp64 stage is defined far below a float step
    assert {1, 63, 64, 65, 1000, 5000} <= n2s and {0, 1, 4, 5, 255, 256, 257, 3000} <= nqs and {0, 1, 64, 65, 129, 600} <= cnts and {0, 1, 64, 65, 257} <= nms
    assert lev == {True, False} and el == {True, False}
    assert int((R.make("s1000_q256")["elig2"] == 0).sum()) == 500
    tr = {}; R.chain(R.make("contend_255"), R.cand_lists("contend_255"), tr)
    assert tr["steals"] >= 50 and tr["hidden"] >= 5000                   # long steal chains: 255 queries for 65 features
    w = R.make("windows"); cl = R.cand_lists("windows")
    assert [len(c) for c, _ in cl[-3:]] == [0, 0, 0] and (np.asarray(w["qxy"])[-2:, 0] < 0).any() and (np.asarray(w["qxy"])[-2:, 1] > 480).any()
    assert max(len(c) for c, _ in cl) == 600 > 256                     # above the row a query's list has in the device's scratch
    for name in ("s1000_q256", "s5000_q3000", "contend_255"):            # CheckTriangular refuses some and keeps some
        assert 0 < R.answer(name)["n_good"] < R.answer(name)["n_match"]
    assert 0 < R.answer("init_s1000_q257")["n_match"] < 257              # the ratio test and th_low refuse some


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return IO.build_host(str(tmp_path_factory.mktemp("np_host") / "new_points_host"))


def _host(host_exe, tmp_path, w, cands):
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    IO.write_host(inp, w, cands)
    r = subprocess.run([host_exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "new points host: ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return IO.read_host(outp, len(w["qxy"]))


_EQUAL = {}


def _compare_host(host_exe, tmp_path, name):
    w, ref = R.make(name), R.answer(name)
    got = _host(host_exe, tmp_path, w, R.cand_lists(name))
    IO.check_matches(got, ref)
    worst, same = IO.check_points(R, got, ref, R.sens(name))
    IO.check_verdicts(R, w, got, ref, same)
    _EQUAL[name] = same


@pytest.mark.parametrize("name", R.ALL)
def test_host_program_under_sanitizers(host_exe, tmp_path, name):
    """The device's own decisions and arithmetic, compiled for the CPU with -fsanitize=address,undefined: the chain on 64 lanes with the 16-bit vMatchDist gives the
    restatement's matches, the Jacobi null vector rounds to the float np.linalg.svd's rounds to, and the check agrees."""
    _compare_host(host_exe, tmp_path, name)


def test_host_program_full_equality_on_all_worlds_but_one(host_exe, tmp_path):
    for name in R.ALL:
        if name not in _EQUAL:
            _compare_host(host_exe, tmp_path, name)
    print("worlds whose points differ somewhere:", [n for n, s in _EQUAL.items() if not s])
    assert sum(_EQUAL.values()) >= len(R.ALL) - 1


def test_host_program_on_the_hand_examples(host_exe, tmp_path):
    cam = _hand_cameras(); A = (100.0, 100.0)
    for w in (hand([A + (10,)], [A + (20,), A + (14,), A + (11,), A + (11,)]), hand([A + (10,), A + (40,)], [A + (14,), A + (14,)]),
              hand([(107.0, 100.0, 10), (96.0, 100.0, 10)], [A + (13,)]), hand([A + (0,), A + (95,)], [A + (45,)], use_ratio=True),
              hand([A + (0,), A + (94,)], [A + (44,)], use_ratio=True), hand([A + (0,)], [A + (50,)], use_ratio=True), hand([A + (0,)], [A + (51,)]),
              hand([A + (10,), A + (30,)], [A + (12,)], elig2=np.array([0, 1], np.uint8))):
        w = dict(w, q_px=w["qxy"], **cam)
        got = _host(host_exe, tmp_path, w, R.lists(w)); ref = R.run(w)
        IO.check_matches(got, ref)
        IO.check_verdicts(R, w, got, ref, False)


def test_adapter_host_mode(tmp_path):
    """adapter/tsorb_new_points.hpp over the driver's mock types, no device: the driver itself holds vMatchIdx12 / vNewpts / vNewptsMatch to a plain transcription of
    the reference's loops over ALL features (its own grid walk, its own skip conditions); here the result is held to the restatement on the gathered queries."""
    exe = IO.build_driver(tmp_path)
    for name, mode in (("s1000_q256", "track"), ("pairs_65", "track"), ("s64_q5_none", "track"), ("init_s1000_q257", "init")):
        w = R.make(name); ref = R.answer(name)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        IO.write_scene(inp, w, mode)
        r = subprocess.run([exe, "--host", inp, outp], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "new points from C++ (host): ok" in r.stdout, r.stdout + r.stderr
        o = IO.read_scene(outp, 2*len(w["qxy"]))
        IO.check_scene(o, w, mode, ref, host=True)

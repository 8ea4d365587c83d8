"""tsorb_match_brute_text / tsorb_match_brute_scene on the device: every output (indices, distances, flags, counts) bit for bit what the CPU restatement
(tests/loop_match_ref.py) gives -- at the shapes where the kernels take another path, with the candidates of a call independent of each other, the resident
batch and match grid untouched, every argument error refused with the outputs untouched, and the adapter's two functions from C++.

k_brute_scene runs BR_T = 256 threads per candidate and keeps BR_T * BR_SLOTS = 1024 candidate features in registers: n2 = 37 is below a wave, 256 + 37 just
above one pass of the workgroup, 1024 + 37 just above what the registers hold (the rest is read from memory at every step)."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_match_ref as L                                            # noqa: E402

pytestmark = pytest.mark.gpu
BR_T, BR_SLOTS = 256, 4


# ------------------------------------------------------------------ the fixture builder
def _flip(rng, row, nbits):
    row = row.copy()
    for b in rng.choice(256, nbits, replace=False):
        row[b >> 3] ^= np.uint8(1 << (b & 7))
    return row


def _keypoints(rng, n, w, h):
    xy = np.stack([rng.uniform(0, w - 1, n), rng.uniform(0, h - 1, n)], 1).astype(np.float32)
    for i in rng.choice(n, max(n // 20, min(n, 2)), replace=False):   # a few exactly at .5
        xy[i] = np.floor(xy[i]) + 0.5
    for i in rng.choice(n, max(n // 25, min(n, 2)), replace=False):   # a few outside the image
        xy[i] += [(-w, w)[int(rng.integers(2))], (-h, h)[int(rng.integers(2))]]
    return xy


def _quads(rng, nq, w, h):
    q = np.zeros((nq, 4, 2))
    for k in range(nq):
        cx, cy = rng.uniform(0.1 * w, 0.9 * w), rng.uniform(0.1 * h, 0.9 * h)
        hw, hh = rng.uniform(0.04, 0.1) * w, rng.uniform(0.04, 0.1) * h
        q[k] = np.array([[cx - hw, cy - hh], [cx + hw, cy - hh], [cx + hw, cy + hh], [cx - hw, cy + hh]]) + rng.uniform(-0.03 * w, 0.03 * w, (4, 2))
    return q


def make_current(seed, n1, w, h):
    """The current keyframe: random descriptors, a tenth of them a copy of an earlier row with up to 20 bits flipped (two features that want the same
    candidate feature: steals and hidden candidates), has3d about 80 % ones."""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    for i in rng.choice(np.arange(1, n1), n1 // 10, replace=False) if n1 > 10 else []:
        desc[i] = _flip(rng, desc[int(rng.integers(0, i))], int(rng.integers(0, 21)))
    return dict(xy=_keypoints(rng, n1, w, h), desc=desc, has3d=(rng.uniform(size=n1) < 0.8).astype(np.uint8))


def make_candidate(seed, cur, n2, nq, w, h):
    """A candidate of n2 features: the current set permuted with 0 .. 60 bits flipped per row; a tenth of the rows then a duplicate of another row, a tenth
    fresh random rows; nq boxes per label image."""
    rng = np.random.default_rng(seed)
    n1 = len(cur["desc"])
    desc = np.zeros((n2, 32), np.uint8)
    src = rng.permutation(n1)
    for i in range(n2):
        desc[i] = _flip(rng, cur["desc"][src[i % n1]], int(rng.integers(0, 61))) if n1 else rng.integers(0, 256, 32, dtype=np.uint8)
    if n2 >= 10:
        sel = rng.choice(n2, 2 * (n2 // 10), replace=False)
        for i in sel[:n2 // 10]:
            desc[i] = desc[int(rng.integers(0, n2))]
        for i in sel[n2 // 10:]:
            desc[i] = rng.integers(0, 256, 32, dtype=np.uint8)
    return dict(xy=_keypoints(rng, n2, w, h), desc=desc, has3d=(rng.uniform(size=n2) < 0.8).astype(np.uint8),
                quad_cur=_quads(rng, nq, w, h), quad_can=_quads(rng, nq, w, h))


def assert_valid(ref, n1):
    """A degenerate fixture must not pass silently: the restatement alone has to exercise every branch."""
    for k, r in enumerate(ref):
        print("candidate %d: matches %d, steals %d, hidden %d, ratio rejections %d, th_low rejections %d, ineligible by a box %d"
              % (k, r["n_match"], r["steals"], r["hidden"], r["ratio_rej"], r["th_rej"], r["box_inelig"]))
        assert r["n_match"] >= n1 / 4 and r["n_match"] == int((r["match12"] >= 0).sum())
        assert r["steals"] >= 3 and r["hidden"] >= 3 and r["ratio_rej"] >= 3 and r["th_rej"] >= 3 and r["box_inelig"] >= 3


def _same_scene(got, ref, what):
    m12, nm = got
    assert m12.dtype == np.int32 and nm.dtype == np.int32 and m12.shape[0] == len(ref) == len(nm), what
    for k, r in enumerate(ref):
        bad = int((m12[k] != r["match12"]).sum())
        print("%s candidate %d: n_match %d (restatement %d), rows differing %d of %d" % (what, k, nm[k], r["n_match"], bad, len(r["match12"])))
        assert np.array_equal(m12[k], r["match12"]), (what, k)
        assert int(nm[k]) == r["n_match"], (what, k)


@pytest.fixture(scope="module")
def ex():
    from textslam_amd.orbextractor import ORBextractor
    return ORBextractor()


# the shared fixture: a current keyframe of 300 features on 1280 x 720 and three candidates (n2 just above one pass, just above the registers, and equal to n1)
W, H, N1 = 1280, 720, 300
N2S = (BR_T + 37, BR_T * BR_SLOTS + 37, 300)


@pytest.fixture(scope="module")
def shared():
    cur = make_current(3, N1, W, H)
    cands = [make_candidate(100 + k, cur, n2, 3, W, H) for k, n2 in enumerate(N2S)]
    ref = L.match_scene(W, H, cur["xy"], cur["desc"], cur["has3d"], cands)
    return cur, cands, ref


def _call(ex, w, h, cur, cands, **kw):
    return ex.match_brute_scene(w, h, cur["xy"], cur["desc"], cur["has3d"], cands, **kw)


# ------------------------------------------------------------------ scene
def test_scene_fixture_is_valid_and_matches(ex, shared):
    cur, cands, ref = shared
    assert_valid(ref, N1)
    _same_scene(_call(ex, W, H, cur, cands), ref, "1280 x 720,")


def test_scene_below_a_wave_small_image(ex):
    cur = make_current(5, 200, 96, 72)
    cands = [make_candidate(7, cur, 37, 2, 96, 72)]
    ref = L.match_scene(96, 72, cur["xy"], cur["desc"], cur["has3d"], cands)
    assert ref[0]["n_match"] >= 5 and ref[0]["box_inelig"] >= 3
    _same_scene(_call(ex, 96, 72, cur, cands), ref, "96 x 72, n2 = 37,")


def test_scene_edge_shapes(ex, shared):
    cur, cands, sref = shared
    j = int(np.flatnonzero(sref[0]["match12"] >= 0)[0])                # a feature that has a match in candidate 0
    one = {k: v[j:j + 1] for k, v in cur.items()}; one["has3d"] = np.ones(1, np.uint8); one["xy"] = np.array([[-5.0, -5.0]], np.float32)      # n1 = 1, eligible (outside: never covered)
    none = dict(cur, has3d=np.zeros(N1, np.uint8))                                                                                    # every feature of the current keyframe ineligible
    empty = dict(xy=np.zeros((0, 2), np.float32), desc=np.zeros((0, 32), np.uint8), has3d=np.zeros(0, np.uint8), quad_cur=cands[0]["quad_cur"], quad_can=cands[0]["quad_can"])
    nobox = dict(cands[2], quad_cur=np.zeros((0, 4, 2)), quad_can=np.zeros((0, 4, 2)))
    for what, c1, cs in (("n1 = 1,", one, cands[:2]), ("nothing eligible,", none, cands), ("n2 = 0 between two,", cur, [cands[0], empty, cands[2]]),
                         ("no boxes,", cur, [nobox, cands[1]]), ("only n2 = 0,", cur, [empty])):
        ref = L.match_scene(W, H, c1["xy"], c1["desc"], c1["has3d"], cs)
        _same_scene(_call(ex, W, H, c1, cs), ref, what)
    ref = L.match_scene(W, H, one["xy"], one["desc"], one["has3d"], cands[:2])
    assert ref[0]["n_match"] == 1                                      # (the one feature does match: the case is not vacuous)
    ref = L.match_scene(W, H, cur["xy"], cur["desc"], cur["has3d"], [nobox])
    assert ref[0]["box_inelig"] == 0 and ref[0]["n_match"] >= N1 / 4
    m12, nm = ex.match_brute_scene(W, H, np.zeros((0, 2)), np.zeros((0, 32)), np.zeros(0), cands)                                     # n1 = 0: counts 0, nothing launched
    assert m12.shape == (3, 0) and nm.tolist() == [0, 0, 0]
    m12, nm = ex.match_brute_scene(W, H, cur["xy"], cur["desc"], cur["has3d"], [])
    assert m12.shape == (0, N1) and nm.shape == (0,)


def test_scene_thresholds_are_arguments(ex, shared):
    cur, cands, _ = shared
    for th, ratio in ((50, 0.6), (30, 0.9), (256, 1.0), (0, 0.9)):
        ref = []
        for c in cands[:1]:
            el1, _ = L.eligibility(W, H, cur["xy"], cur["has3d"], c["quad_cur"]); el2, _ = L.eligibility(W, H, c["xy"], c["has3d"], c["quad_can"])
            m, n, _ = L.scan(cur["desc"], el1, c["desc"], el2, th, ratio)
            ref.append(dict(match12=m, n_match=n))
        _same_scene(_call(ex, W, H, cur, cands[:1], th_low=th, ratio=ratio), ref, "th_low %d ratio %.1f," % (th, ratio))


def test_candidates_are_independent(ex, shared):
    cur, cands, ref = shared
    all3 = _call(ex, W, H, cur, cands)
    for k in range(3):                                                 # three candidates in one call = three calls of one
        m, n = _call(ex, W, H, cur, cands[k:k + 1])
        assert np.array_equal(m[0], all3[0][k]) and n[0] == all3[1][k], k
    rev = _call(ex, W, H, cur, cands[::-1])                            # the order can be reversed
    assert np.array_equal(rev[0][::-1], all3[0]) and np.array_equal(rev[1][::-1], all3[1])
    more = _call(ex, W, H, cur, cands + cands[:2])                     # more candidates than the last call (scratch grows), then fewer (scratch reused)
    assert np.array_equal(more[0][:3], all3[0]) and np.array_equal(more[0][3:], all3[0][:2]) and np.array_equal(more[1], np.r_[all3[1], all3[1][:2]])
    _same_scene(_call(ex, W, H, cur, cands[1:2]), ref[1:2], "after a larger call,")


# ------------------------------------------------------------------ text
def _text_pairs():
    rng = np.random.default_rng(21)
    r = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    near = lambda rows, lo, hi: np.stack([_flip(rng, x, int(rng.integers(lo, hi))) for x in rows]) if len(rows) else np.zeros((0, 32), np.uint8)
    b60 = r(60); a60 = near(b60[rng.permutation(60)], 0, 50)
    b60[40] = b60[3]; b60[41] = b60[3]; b60[20] = b60[7]               # duplicated rows: ties, the first index wins
    b7 = r(7); a300 = near(b7[rng.integers(0, 7, 300)], 5, 70); b7[5] = b7[1]
    b2 = r(2); b2[1] = b2[0]
    return [(near(b2[:1], 3, 4), b2), (a60, b60), (a300, b7), (r(0), r(5)), (r(5), r(0))]


def _edge_pairs():
    """min_dist = 0: 29 is good, 30 is not; min_dist = 20: 39 is good, 40 is not (every query has one near row, the other train rows are random)."""
    rng = np.random.default_rng(22)
    out = []
    for dists in ((0, 29, 30, 31), (20, 39, 40, 41)):
        b = rng.integers(0, 256, (len(dists) + 3, 32), dtype=np.uint8)
        a = np.stack([_flip(rng, b[i], d) for i, d in enumerate(dists)])
        out.append((a, b, dists))
    return out


def _same_text(got, ref, what):
    assert len(got) == len(ref)
    for p, (g, r) in enumerate(zip(got, ref)):
        print("%s pair %d: %d queries, good %d (restatement %d)" % (what, p, len(r["dist"]), int(g["good"].sum()), int(r["good"].sum())))
        for k in ("train_idx", "dist", "good"):
            assert g[k].dtype == r[k].dtype and np.array_equal(g[k], r[k]), (what, p, k)


def test_text_pairs(ex):
    pairs = _text_pairs()
    assert [(len(a), len(b)) for a, b in pairs] == [(1, 2), (60, 60), (300, 7), (0, 5), (5, 0)]
    ref = L.match_text(pairs)
    got = ex.match_brute_text(pairs)
    _same_text(got, ref, "five pairs,")
    assert got[0]["train_idx"][0] == 0 and got[0]["dist"][0] == 3      # two equal train rows: the first
    assert set(got[1]["train_idx"].tolist()).isdisjoint({40, 41}) and 3 in got[1]["train_idx"] and 20 not in got[1]["train_idx"]
    assert 5 not in got[2]["train_idx"] and 1 in got[2]["train_idx"]
    assert got[4]["train_idx"].tolist() == [-1] * 5 and got[4]["dist"].tolist() == [L.INT_MAX] * 5 and not got[4]["good"].any()
    for p in range(5):                                                 # each pair equals a call of its own
        _same_text(ex.match_brute_text(pairs[p:p + 1]), ref[p:p + 1], "pair %d alone," % p)
    assert ex.match_brute_text([]) == []


def test_text_threshold_edges(ex):
    edges = _edge_pairs()
    got = ex.match_brute_text([(a, b) for a, b, _ in edges])
    _same_text(got, L.match_text([(a, b) for a, b, _ in edges]), "edges,")
    for g, (_, _, dists) in zip(got, edges):
        assert g["dist"].tolist() == list(dists) and g["train_idx"].tolist() == [0, 1, 2, 3]
        assert g["good"].tolist() == [1, 1, 0, 0]


def test_text_more_queries_than_a_tile(ex):
    """A pair of 2 BR_T + 9 queries spans three tiles: the pair's minimum is taken over all of them; a train set of BR_T + 5 rows takes two passes."""
    rng = np.random.default_rng(23)
    b = rng.integers(0, 256, (BR_T + 5, 32), dtype=np.uint8)
    a = np.stack([_flip(rng, b[int(rng.integers(0, len(b)))], int(rng.integers(8, 60))) for _ in range(2 * BR_T + 9)])
    a[2 * BR_T + 4] = _flip(rng, b[BR_T + 2], 2)                       # the minimum in the last tile, its row in the second pass
    pairs = [(a[:5], b[:9]), (a, b)]
    ref = L.match_text(pairs)
    assert ref[1]["dist"].min() == 2 and ref[1]["train_idx"][2 * BR_T + 4] == BR_T + 2 and 0 < ref[1]["good"].sum() < len(a)
    _same_text(ex.match_brute_text(pairs), ref, "three tiles,")


# ------------------------------------------------------------------ resident state
def test_resident_batch_and_grid_unchanged(shared):
    from textslam_amd.orbextractor import ORBextractor, synthetic_frame
    cur, cands, ref = shared
    ex2 = ORBextractor()
    ex2.extract_batch(synthetic_frame(2, 320, 240))
    rng = np.random.default_rng(11)
    before = ex2.download()[0]
    ex2.match_set_frame(0, (0.0, 320.0, 0.0, 240.0))
    q = rng.choice(len(before[0]), 40, replace=False)
    args = (before[0][q, :2] + rng.uniform(-3, 3, (40, 2)).astype(np.float32), np.full(40, 12.0, np.float32), None, before[1][q])
    m0 = ex2.match_search(*args)
    lev0 = [ex2.debug_level(0, l).copy() for l in range(8)]
    _same_scene(_call(ex2, W, H, cur, cands), ref, "beside a resident batch,")
    ex2.match_brute_text(_text_pairs())
    m1 = ex2.match_search(*args)
    after = ex2.download()[0]
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert all(m0[k].tobytes() == m1[k].tobytes() for k in m0)
    assert all(np.array_equal(a, ex2.debug_level(0, l)) for l, a in enumerate(lev0))


# ------------------------------------------------------------------ argument errors
I32, U8, F32, F64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _raw_text(ex, n_pair=2, off1=(0, 3, 5), off2=(0, 2, 6), desc1=True, desc2=True, train=True, dist=True, good=True, ctx=True):
    off1 = None if off1 is None else np.array(off1, np.int32); off2 = None if off2 is None else np.array(off2, np.int32)
    d1 = np.full((8, 32), 3, np.uint8); d2 = np.full((8, 32), 5, np.uint8)
    o = [np.full(8, -77, np.int32), np.full(8, -78, np.int32), np.full(8, 0x5a, np.uint8)]
    rc = ex.lib.tsorb_match_brute_text(ex.ctx if ctx else None, n_pair, _p(off1, I32), _p(d1 if desc1 else None, U8), _p(off2, I32), _p(d2 if desc2 else None, U8),
                                       _p(o[0] if train else None, I32), _p(o[1] if dist else None, I32), _p(o[2] if good else None, U8))
    return rc, (o[0] == -77).all() and (o[1] == -78).all() and (o[2] == 0x5a).all()


def _raw_scene(ex, w=64, h=48, n1=4, n_cand=2, off2=(0, 3, 5), qoff=(0, 1, 2), th_low=50, ratio=0.9, xy1=None, xy2=None, quad=None, null=(), ctx=True):
    a = dict(xy1=np.full((4, 2), 5.0, np.float32) if xy1 is None else np.array(xy1, np.float32), desc1=np.zeros((4, 32), np.uint8), has3d1=np.ones(4, np.uint8),
             off2=None if off2 is None else np.array(off2, np.int32), xy2=np.full((5, 2), 7.0, np.float32) if xy2 is None else np.array(xy2, np.float32),
             desc2=np.zeros((5, 32), np.uint8), has3d2=np.ones(5, np.uint8), qoff=None if qoff is None else np.array(qoff, np.int32),
             quad_cur=np.zeros((2, 4, 2)) if quad is None else np.array(quad, np.float64), quad_can=np.zeros((2, 4, 2)),
             match12=np.full((2, 4), -77, np.int32), n_match=np.full(2, -78, np.int32))
    g = lambda k, t: None if k in null else _p(a[k], t)
    rc = ex.lib.tsorb_match_brute_scene(ex.ctx if ctx else None, w, h, n1, g("xy1", F32), g("desc1", U8), g("has3d1", U8), n_cand, g("off2", I32), g("xy2", F32), g("desc2", U8),
                                        g("has3d2", U8), g("qoff", I32), g("quad_cur", F64), g("quad_can", F64), th_low, ratio, g("match12", I32), g("n_match", I32))
    return rc, (a["match12"] == -77).all() and (a["n_match"] == -78).all()


def test_argument_errors(ex, shared):
    big = 65536 + 1
    text_bad = [dict(n_pair=-1), dict(off1=None), dict(off2=None), dict(desc1=False), dict(desc2=False), dict(train=False), dict(dist=False), dict(good=False),
                dict(off1=(1, 3, 5)), dict(off2=(0, 4, 2)), dict(off1=(0, 5, 3)), dict(off1=(0, big, big)), dict(off2=(0, 2, 2 + big))]
    for kw in text_bad:
        rc, untouched = _raw_text(ex, **kw)
        assert rc == -1 and untouched, kw
        assert ex.lib.tsorb_last_error(ex.ctx).decode().startswith("tsorb_match_brute_text:"), kw
    assert _raw_text(ex, ctx=False) == (-1, True)
    assert _raw_text(ex, n_pair=0, off1=None, off2=None, desc1=False, desc2=False, train=False, dist=False, good=False) == (0, True)
    rc, untouched = _raw_text(ex)
    assert rc == 0 and not untouched
    nan, inf = float("nan"), float("inf")
    q_ok = np.zeros((2, 4, 2))
    q_nan = q_ok.copy(); q_nan[1, 2, 0] = nan
    q_far = q_ok.copy(); q_far[0, 1, 1] = 2.0 ** 30 + 1024
    xy_bad = np.full((4, 2), 5.0); xy_bad[3, 1] = inf
    xy2_bad = np.full((5, 2), 7.0); xy2_bad[0, 0] = nan
    scene_bad = [dict(n1=-1), dict(n_cand=-1), dict(off2=(1, 3, 5)), dict(off2=(0, 4, 3)), dict(qoff=(0, 2, 1)), dict(qoff=(1, 1, 2)), dict(w=0), dict(h=0), dict(w=8193), dict(h=8193),
                 dict(xy1=xy_bad), dict(xy2=xy2_bad), dict(quad=q_nan), dict(quad=q_far), dict(th_low=-1), dict(th_low=257), dict(ratio=nan), dict(ratio=inf), dict(ratio=-0.5),
                 dict(n1=big), dict(off2=(0, big, big + 1))]
    scene_bad += [dict(null=(k,)) for k in ("xy1", "desc1", "has3d1", "off2", "xy2", "desc2", "has3d2", "qoff", "quad_cur", "quad_can", "match12", "n_match")]
    for kw in scene_bad:
        rc, untouched = _raw_scene(ex, **kw)
        assert rc == -1 and untouched, kw
        assert ex.lib.tsorb_last_error(ex.ctx).decode().startswith("tsorb_match_brute_scene:"), kw
    assert _raw_scene(ex, ctx=False) == (-1, True)
    assert _raw_scene(ex, n_cand=0, null=("xy1", "desc1", "has3d1", "off2", "xy2", "desc2", "has3d2", "qoff", "quad_cur", "quad_can", "match12", "n_match")) == (0, True)
    rc, untouched = _raw_scene(ex)
    assert rc == 0 and not untouched
    cur, cands, ref = shared                                           # the context still answers
    _same_scene(_call(ex, W, H, cur, cands[:1]), ref[:1], "after the errors,")


# ------------------------------------------------------------------ the adapter from C++
def test_adapter_from_cxx(tmp_path, ex):
    import loop_match_world as IO
    exe = str(tmp_path / "loop_match_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "loop_match_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsorb", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    world = IO.make_world(31)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    IO.write_world(inp, world)
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "loop match from C++: ok" in res.stdout, res.stdout
    expect = IO.expected_bytes(world, ex)                              # the same gathering in Python, through the Python mirror
    raw = open(outp, "rb").read()
    assert len(raw) > 1000 and raw == expect

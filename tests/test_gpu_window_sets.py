"""tsorb_match_search_sets on the device against the existing oracle.orb_match called once per set: every array key equal (np.array_equal) -- candidates in the
reference's order, Hamming distances, the first minimum, the runner-up.  Features are synthetic (random keypoints, random descriptors with planted duplicates)."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_fuse_io as IO                                             # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("cand_cnt", "best_idx", "best_dist", "best_dist2", "cand_idx", "cand_dist")
B0 = (0.0, 640.0, 0.0, 480.0)
B5 = (-8.5, 331.25, -4.0, 244.0)
SIZES = (0, 1, 70, 300, 1500)                       # 1500: more than one placement chunk of 256
CHUNK_EDGE = (256, 257)                              # exactly one placement chunk, and one feature past it
N_DENSE, DENSE_X, DENSE_Y = 150, (326.0, 334.0), (236.0, 244.0)       # 150 features of one further set inside the cell (33, 24) of a 10 x 10-px grid
FIXED = [[-500.0, -500.0], [5.0, 5.0], [639.0, 479.0], [320.0, 240.0], [2000.0, 100.0], [0.0, 479.0], [639.0, 0.0], [320.0, -30.0]]     # tests/test_gpu_orb.py's


def _features(rng, n, bounds, dense=0):
    x0, x1, y0, y1 = bounds
    kp = np.zeros((n, 6), np.float32)
    kp[:, 0] = rng.uniform(x0 - 4, x1 + 4, n); kp[:, 1] = rng.uniform(y0 - 4, y1 + 4, n)        # (a few outside the grid: in no cell)
    kp[:, 2] = 31.0; kp[:, 3] = rng.uniform(0, 360, n); kp[:, 4] = rng.uniform(1, 200, n); kp[:, 5] = rng.integers(0, 8, n)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fixed = np.zeros(n, bool)
    if dense:                                                                                     # spread over the index range: the cell's list crosses chunks of the placement
        at = np.sort(rng.choice(n, dense, replace=False)); fixed[at] = True
        kp[at, 0] = rng.uniform(*DENSE_X, dense); kp[at, 1] = rng.uniform(*DENSE_Y, dense)
    for i in range(0, n - 1, 5):                                                                  # planted duplicates: a neighbour with the same descriptor
        if fixed[i] or fixed[i + 1]:
            continue
        kp[i + 1, :2] = kp[i, :2] + rng.uniform(-2, 2, 2).astype(np.float32); kp[i + 1, 5] = kp[i, 5]; desc[i + 1] = desc[i]
    return kp, desc


def _flip(rng, row, nbits):
    row = row.copy()
    for b in rng.choice(256, nbits, replace=False):
        row[b >> 3] ^= np.uint8(1 << (b & 7))
    return row


@pytest.fixture(scope="module")
def ex():
    from textslam_amd.orbextractor import ORBextractor
    return ORBextractor()


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(2024)
    sets = [(*_features(rng, n, B0), B0) for n in SIZES]
    sets.append((*_features(rng, 400, B5), B5))
    sets.append((*_features(rng, 350, B0, dense=N_DENSE), B0))
    sets += [(*_features(rng, n, B0), B0) for n in CHUNK_EDGE]
    qset, qxy, qr, qlev, qd = [], [], [], [], []
    for s, (kp, desc, b) in enumerate(sets):
        n = len(kp)
        for k in range(200):
            r = (15.0, 40.0, 300.0)[k % 3]
            if n and k % 8 != 7:
                i = int(rng.integers(0, n))
                xy = kp[i, :2] + rng.normal(0, 3.0, 2); lev = (int(kp[i, 5]) - 1, int(kp[i, 5]) + 1); d = _flip(rng, desc[i], int(rng.integers(0, 40)))
            else:
                xy = np.array([rng.uniform(b[0] - 30, b[1] + 30), rng.uniform(b[2] - 30, b[3] + 30)]); lev = (int(rng.integers(-1, 4)), int(rng.integers(-1, 8)))
                d = rng.integers(0, 256, 32, dtype=np.uint8)
            qset.append(s); qxy.append(xy); qr.append(r); qlev.append(lev); qd.append(d)
    for s in (4, 5):                                                                              # the fixed queries of the existing match test, the grid left on every side
        for k, xy in enumerate(FIXED):
            qset.append(s); qxy.append(np.array(xy)); qr.append((15.0, 300.0)[k % 2] if s == 4 else 40.0); qlev.append((-1, -1)); qd.append(rng.integers(0, 256, 32, dtype=np.uint8))
    qset.append(6); qxy.append(np.array([330.0, 240.0])); qr.append(15.0); qlev.append((-1, -1)); qd.append(sets[6][1][3].copy())      # the window over the dense cell
    nq = len(qset)
    order = rng.permutation(nq)                                                                   # neighbouring queries hit different sets
    qset = np.array(qset, np.int32)[order]; qxy = np.array(qxy, np.float32)[order]; qr = np.array(qr, np.float32)[order]
    qlev = np.array(qlev, np.int32)[order]; qd = np.array(qd, np.uint8)[order]
    perm = rng.permutation(nq)                                                                    # the descriptor table is the queries' descriptors in another order
    table = np.ascontiguousarray(qd[perm]); qdi = np.argsort(perm).astype(np.int32)
    assert np.array_equal(table[qdi], qd)
    return dict(sets=sets, qset=qset, qxy=qxy, qr=qr, qlev=qlev, qd=qd, table=table, qdi=qdi, nq=nq, refs={})


def _ref(oracle, w, with_lev, max_cand):
    """oracle.orb_match once per set, scattered to the queries' positions; computed once per (level check, max_cand)."""
    key = (with_lev, max_cand)
    if key not in w["refs"]:
        nq = w["nq"]
        out = dict(cand_idx=np.full((nq, max_cand), -7, np.int32), cand_dist=np.full((nq, max_cand), -7, np.int32), cand_cnt=np.full(nq, -7, np.int32),
                   best_idx=np.full(nq, -7, np.int32), best_dist=np.full(nq, -7, np.int32), best_dist2=np.full(nq, -7, np.int32))
        for s, (kp, desc, b) in enumerate(w["sets"]):
            m = np.flatnonzero(w["qset"] == s)
            lev = w["qlev"][m] if with_lev else np.full((len(m), 2), -1, np.int32)
            r = oracle.orb_match(kp, desc, b, w["qxy"][m], w["qr"][m], lev, w["qd"][m], max_cand=max_cand)
            for k in KEYS:
                out[k][m] = r[k]
        for k in KEYS:
            out[k].setflags(write=False)
        w["refs"][key] = out
    return w["refs"][key]


def _same(got, ref, what):
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))


def test_fixture_is_loud(world, oracle_lib):
    """On the oracle's own output: the properties an ordering bug needs to show itself."""
    w = world
    ref = _ref(oracle_lib, w, False, 256)
    cnt = ref["cand_cnt"]
    assert (cnt > 0).mean() > 0.5
    assert cnt.max() > 128
    full = cnt <= 256
    at_best = (ref["cand_dist"] == ref["best_dist"][:, None]) & (ref["cand_idx"] >= 0)
    ties = full & (cnt > 0) & (at_best.sum(1) >= 2)
    assert ties.any()
    q = int(np.flatnonzero(ties)[0]); tied = ref["cand_idx"][q][at_best[q]]
    assert len(set(tied.tolist())) >= 2 and ref["best_idx"][q] == tied[0]                          # the first of them in the reference's order wins
    kp6 = w["sets"][6][0]
    dense = np.flatnonzero((kp6[:, 0] >= DENSE_X[0]) & (kp6[:, 0] <= DENSE_X[1]) & (kp6[:, 1] >= DENSE_Y[0]) & (kp6[:, 1] <= DENSE_Y[1]))
    assert len(dense) >= N_DENSE
    cx = np.rint(kp6[dense, 0].astype(np.float64) * 0.1); cy = np.rint(kp6[dense, 1].astype(np.float64) * 0.1)
    assert (cx == 33).all() and (cy == 24).all()                                                   # one cell
    over = [q for q in np.flatnonzero((w["qset"] == 6) & full) if set(dense.tolist()) <= set(ref["cand_idx"][q][:cnt[q]].tolist())]
    assert over
    nonempty = np.isin(w["qset"], [s for s, t in enumerate(w["sets"]) if len(t[0])])
    assert (nonempty & (cnt == 0)).any()
    empty = w["qset"] == 0
    assert empty.sum() >= 200 and (cnt[empty] == 0).all() and (ref["best_idx"][empty] == -1).all() and (ref["best_dist"][empty] == 2 ** 31 - 1).all()
    assert (ref["best_dist2"][empty] == 2 ** 31 - 1).all()
    assert (w["qset"][1:] != w["qset"][:-1]).mean() > 0.5


@pytest.mark.parametrize("with_lev", [False, True])
@pytest.mark.parametrize("max_cand", [0, 4, 256])
def test_all_shapes_in_one_call(ex, world, oracle_lib, with_lev, max_cand):
    w = world
    got = ex.match_search_sets(w["sets"], w["qset"], w["qxy"], w["qr"], w["table"], qdi=w["qdi"], qlev=w["qlev"] if with_lev else None, max_cand=max_cand)
    _same(got, _ref(oracle_lib, w, with_lev, max_cand), (with_lev, max_cand))


@pytest.mark.parametrize("max_cand", [256, 4])
def test_every_set_as_the_single_grid(ex, world, oracle_lib, max_cand):
    """The context's grid is built by the same chunked builder: every set of the world through match_set_features + match_search against the oracle's rows of that set
    (the empty grid, a grid smaller than a chunk, the chunk boundary, a cell whose list crosses chunks, features outside the grid, an origin off zero)."""
    w = world
    ref = _ref(oracle_lib, w, True, max_cand)
    for s, (kp, desc, b) in enumerate(w["sets"]):
        m = np.flatnonzero(w["qset"] == s)
        ex.match_set_features(kp, desc, b)
        got = ex.match_search(w["qxy"][m], w["qr"][m], w["qlev"][m], w["qd"][m], max_cand=max_cand)
        _same(got, {k: ref[k][m] for k in KEYS}, (s, max_cand))


def test_descriptors_by_index_or_expanded(ex, world, oracle_lib):
    w = world
    got = ex.match_search_sets(w["sets"], w["qset"], w["qxy"], w["qr"], w["table"][w["qdi"]], qdi=None, qlev=w["qlev"], max_cand=4)
    _same(got, _ref(oracle_lib, w, True, 4), "expanded")


def test_sets_sharing_a_table_equal_separate_calls(ex, world):
    w = world
    rng = np.random.default_rng(5)
    use = [2, 3, 4, 5]
    P = 120
    table = np.ascontiguousarray(w["table"][:P])
    xy = np.stack([rng.uniform(0, 640, (P,)), rng.uniform(0, 480, (P,))], 1).astype(np.float32)
    sets = [w["sets"][s] for s in use]
    qset = np.repeat(np.arange(len(use), dtype=np.int32), P); qdi = np.tile(np.arange(P, dtype=np.int32), len(use))
    qxy = np.tile(xy, (len(use), 1)); qr = np.full(len(use) * P, 40.0, np.float32)
    got = ex.match_search_sets(sets, qset, qxy, qr, table, qdi=qdi, max_cand=16)
    assert (got["cand_cnt"] > 0).mean() > 0.5
    for k, st in enumerate(sets):
        one = ex.match_search_sets([st], np.zeros(P, np.int32), xy, qr[:P], table, qdi=np.arange(P, dtype=np.int32), max_cand=16)
        _same({key: got[key][k * P:(k + 1) * P] for key in KEYS}, one, ("set", use[k]))


def test_one_set_is_the_single_set_pair_of_calls(ex, world):
    w = world
    m = np.flatnonzero(w["qset"] == 4)
    kp, desc, b = w["sets"][4]
    got = ex.match_search_sets([w["sets"][4]], np.zeros(len(m), np.int32), w["qxy"][m], w["qr"][m], w["qd"][m], qlev=w["qlev"][m], max_cand=32)
    ex.match_set_features(kp, desc, b)
    single = ex.match_search(w["qxy"][m], w["qr"][m], w["qlev"][m], w["qd"][m], max_cand=32)
    assert all(got[k].tobytes() == single[k].tobytes() for k in KEYS)


def test_resident_batch_and_grid_unchanged(world, oracle_lib):
    from textslam_amd.orbextractor import ORBextractor, synthetic_frame
    w = world
    ex2 = ORBextractor()
    ex2.extract_batch(np.stack([synthetic_frame(2, 320, 240), synthetic_frame(3, 320, 240)]))
    rng = np.random.default_rng(11)
    before = ex2.download()
    ex2.match_set_frame(1, (0.0, 320.0, 0.0, 240.0))
    q = rng.choice(len(before[0][0]), 40, replace=False)
    args = (before[0][0][q, :2] + rng.uniform(-3, 3, (40, 2)).astype(np.float32), np.full(40, 12.0, np.float32), None, before[0][1][q])
    m0 = ex2.match_search(*args)
    assert (m0["cand_cnt"] > 0).any()
    got = ex2.match_search_sets(w["sets"], w["qset"], w["qxy"], w["qr"], w["table"], qdi=w["qdi"], max_cand=4)
    _same(got, _ref(oracle_lib, w, False, 4), "beside a resident batch,")
    m1 = ex2.match_search(*args)
    after = ex2.download()
    assert all(b[0].tobytes() == a[0].tobytes() and b[1].tobytes() == a[1].tobytes() for b, a in zip(before, after))
    assert all(m0[k].tobytes() == m1[k].tobytes() for k in m0)


# ------------------------------------------------------------------ argument errors
I32, U8, F32, F64 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _raw(ex, n_set=2, foff=(0, 3, 5), bounds=None, n_qdesc=4, nq=4, qset=(0, 1, 1, 0), qdi=(3, 2, 1, 0), qxy=None, qr=None, max_cand=2, null=(), ctx=True, lev=True):
    a = dict(foff=np.array(foff, np.int32), kp6=np.full((5, 6), 9.0, np.float32), desc=np.zeros((5, 32), np.uint8),
             bounds=np.array([B0, B0] if bounds is None else bounds, np.float64), qdesc=np.zeros((4, 32), np.uint8), qset=np.array(qset, np.int32),
             qdi=None if qdi is None else np.array(qdi, np.int32), qxy=np.full((4, 2), 9.0, np.float32) if qxy is None else np.array(qxy, np.float32),
             qr=np.full(4, 15.0, np.float32) if qr is None else np.array(qr, np.float32), qlev=np.full((4, 2), -1, np.int32) if lev else None)
    o = [np.full((4, 2), -77, np.int32), np.full((4, 2), -77, np.int32)] + [np.full(4, -77, np.int32) for _ in range(4)]
    g = lambda k, t: None if k in null or a[k] is None else _p(a[k], t)
    rc = ex.lib.tsorb_match_search_sets(ex.ctx if ctx else None, n_set, g("foff", I32), g("kp6", F32), g("desc", U8), g("bounds", F64), n_qdesc, g("qdesc", U8), nq,
                                        g("qset", I32), g("qdi", I32), g("qxy", F32), g("qr", F32), g("qlev", I32), max_cand, *[_p(x, I32) for x in o])
    return rc, all((x == -77).all() for x in o)


def test_argument_errors(ex):
    nan, inf, big = float("nan"), float("inf"), 65536 + 1
    xy_nan = np.full((4, 2), 9.0); xy_nan[2, 1] = nan
    xy_inf = np.full((4, 2), 9.0); xy_inf[0, 0] = inf
    bad = [dict(null=(k,)) for k in ("foff", "kp6", "desc", "bounds", "qdesc", "qset", "qxy", "qr")]
    bad += [dict(n_set=-1), dict(nq=-1), dict(n_qdesc=-1), dict(n_set=1025), dict(foff=(1, 3, 5)), dict(foff=(0, 4, 3)), dict(foff=(0, big, big)), dict(foff=(0, 2, 2 + big)),
            dict(bounds=[B0, (640.0, 640.0, 0.0, 480.0)]), dict(bounds=[(0.0, 640.0, 480.0, 0.0), B0]), dict(bounds=[B0, (0.0, nan, 0.0, 480.0)]), dict(bounds=[(-inf, 640.0, 0.0, 480.0), B0]),
            dict(bounds=[B0, (0.0, 640.0, 0.0, inf)]), dict(qset=(0, 1, 2, 0)), dict(qset=(0, -1, 1, 0)), dict(qdi=(0, 1, 2, 4)), dict(qdi=(-1, 1, 2, 3)), dict(qdi=None, n_qdesc=3),
            dict(qxy=xy_nan), dict(qxy=xy_inf), dict(qr=[15.0, nan, 15.0, 15.0]), dict(qr=[15.0, 15.0, 15.0, inf]), dict(max_cand=-1)]
    for kw in bad:
        rc, untouched = _raw(ex, **kw)
        assert rc == -1 and untouched, kw
        assert ex.lib.tsorb_last_error(ex.ctx).decode().startswith("tsorb_match_search_sets:"), kw
    assert _raw(ex, ctx=False) == (-1, True)
    every = ("foff", "kp6", "desc", "bounds", "qdesc", "qset", "qxy", "qr", "qdi", "qlev")
    assert _raw(ex, n_set=0, null=every) == (0, True)                                           # nothing to search: no pointer is read
    assert _raw(ex, nq=0, null=every) == (0, True)
    rc, untouched = _raw(ex)
    assert rc == 0 and not untouched
    rc, untouched = _raw(ex, qdi=None, lev=False)                                               # both optional inputs NULL
    assert rc == 0 and not untouched
    got = ex.match_search_sets([(np.zeros((0, 6), np.float32), np.zeros((0, 32), np.uint8), B0)], [0, 0], [[5.0, 5.0], [700.0, 9.0]], [15.0, 300.0], np.zeros((2, 32), np.uint8), max_cand=3)
    assert (got["cand_cnt"] == 0).all() and (got["best_idx"] == -1).all() and (got["best_dist"] == 2 ** 31 - 1).all() and (got["best_dist2"] == 2 ** 31 - 1).all()
    assert (got["cand_idx"] == -1).all() and (got["cand_dist"] == -1).all()


# ------------------------------------------------------------------ the adapter from C++, the searches on the device
def test_adapter_from_cxx(tmp_path, ex):
    exe = IO.build(tmp_path)
    dev_path, host_path = str(tmp_path / "dev.bin"), str(tmp_path / "host.bin")
    c = IO.run(exe, dev_path, host=False)
    IO.check_counters(c)
    assert IO.run(exe, host_path, host=True) == c
    assert open(dev_path, "rb").read() == open(host_path, "rb").read()             # window_best_host is the device's search
    rec = IO.read_records(dev_path)
    for pre in ("fuse_", "more_"):                                                 # the same arrays through the Python mirror
        foff = rec[pre + "foff"]; kp6 = rec[pre + "kp6"].reshape(-1, 6); desc = rec[pre + "desc"].reshape(-1, 32); b = rec[pre + "bounds"].reshape(-1, 4)
        sets = [(kp6[foff[s]:foff[s + 1]], desc[foff[s]:foff[s + 1]], tuple(b[s])) for s in range(len(foff) - 1)]
        got = ex.match_search_sets(sets, rec[pre + "qset"], rec[pre + "qxy"].reshape(-1, 2), rec[pre + "qr"], rec[pre + "qdesc"].reshape(-1, 32), qdi=rec[pre + "qdi"])
        for k in ("best_idx", "best_dist", "cand_cnt"):
            assert np.array_equal(got[k], rec[pre + k]), (pre, k)

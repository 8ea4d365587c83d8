"""tsloop_detect_loop on the GPU: loopClosing::DetectLoop's string scan, match lists, keyframe vote and candidates (include/tsloop.h, textslam_amd/csrc/tsloop_detect.h)
against the restatement of tests/detect_loop_ref.py.  Every comparison is integer or byte equality, scores as bit patterns: all arithmetic is on integers apart from one
fp64 quotient per pair and the fp64 threshold, which both sides evaluate in the reference's order, so no tolerance is needed.

  * seeded worlds of at most 8 queries, 300 map texts (more than one 256-lane tile, the last one partial) and 40 keyframes over a 4-letter alphabet;
  * fixed cases, each also held to values written here: string lengths at the 64-bit word's edges, bytes >= 0x80, the 11 / 2 / 5 rounding case, every exit;
  * a query's lists byte-equal whatever other queries are in the call; outputs poisoned before the call and untouched where the contract says so; the max_match
    overflow; every argument error; the empty inputs;
  * the adapter (adapter/tsloop_detect.hpp) from C++ over mock types, beside a plain restatement of the reference's loop, byte for byte the Python call."""
import ctypes as C
import os
import struct
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_loop_ref as R                                           # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = (-77, 7.0)
EDGE = (0, 1, 31, 32, 33, 63, 64)
WORLDS = [(11, 8, 300, 40), (12, 5, 257, 7), (13, 8, 256, 40), (14, 3, 1, 1), (15, 8, 300, 0)]      # (seed, queries, map texts, keyframes)


@pytest.fixture(scope="module")
def lo():
    from textslam_amd.loop import LoopOptimizer
    return LoopOptimizer(0)


@pytest.fixture(scope="module")
def worlds():
    """Every seeded world and the restatement's answers -- computed once, read-only."""
    out = {}
    for c in WORLDS:
        w = R.world(c[0], n_query=c[1], n_map=c[2], n_kf=c[3])
        out[c] = (w, {(mmw, th): R.detect_loop(min_matched_words=mmw, score_thresh_min=th, **w) for mmw in (0, 1, 2) for th in (0.51, 0.35)})
    return out


def W(queries, map_texts, obs_rows=None, n_kf=1, q_self=None, m_skip=None):
    return {"queries": list(queries), "q_self": np.full(len(queries), -1, np.int32) if q_self is None else np.asarray(q_self, np.int32), "map_texts": list(map_texts),
            "m_skip": np.zeros(len(map_texts), np.uint8) if m_skip is None else np.asarray(m_skip, np.uint8),
            "obs_rows": [[0]]*len(map_texts) if obs_rows is None else obs_rows, "n_kf": n_kf}


def both(lo, w, **kw):
    """The device's answer, held equal to the restatement's."""
    kw.setdefault("max_match", max(len(w["map_texts"]), 1))
    got = lo.DetectLoop(w["queries"], w["q_self"], w["map_texts"], w["m_skip"], w["obs_rows"], w["n_kf"], **kw)
    kw.pop("max_match")
    ref = R.detect_loop(**w, **kw)
    assert got["status"] == 0 and R.same(got, ref) is None, R.same(got, ref)
    return got


@pytest.mark.parametrize("case", WORLDS, ids=lambda c: "seed%d_q%d_m%d_k%d" % c)
def test_seeded_worlds(lo, worlds, case):
    w, refs = worlds[case]
    seen = 0
    for (mmw, th), ref in refs.items():
        got = lo.DetectLoop(w["queries"], w["q_self"], w["map_texts"], w["m_skip"], w["obs_rows"], w["n_kf"], min_matched_words=mmw, score_thresh_min=th, max_match=300)
        print(case, mmw, th, "cnt", got["match_cnt"].tolist(), "cand", got["cand"].tolist())
        assert got["status"] == 0 and R.same(got, ref) is None, R.same(got, ref)
        seen += int(got["match_cnt"].sum())
    assert seen > 0 or case[2] == 1
    if case == WORLDS[0]:                                              # the world is worth its name: ties inside a list, several candidates, both thresholds differ
        r0, r1 = refs[(0, 0.51)], refs[(0, 0.35)]
        assert any(len(s) > 1 and len(set(s.tolist())) < len(s) for s in r0["match_score"]) and r0["n_cand"] > 1
        assert int(r1["match_cnt"].sum()) > int(r0["match_cnt"].sum())


def test_lengths_at_the_word_edges(lo):
    """Lengths 0, 1, 31, 32, 33, 63, 64 on either side: a^i against a^j is |i - j| edits; against random bytes it is the DP's value.  Both strings empty: not scored."""
    g = np.random.default_rng(7)
    for lm in EDGE:
        qs = [b"a"*l for l in EDGE]
        got = both(lo, W(qs, [b"a"*lm]), min_str_score=-1.0, score_thresh_min=0.0, min_matched_words=0)
        for l, cnt, d, s in zip(EDGE, got["match_cnt"], got["match_dist"], got["match_score"]):
            if l == 0 and lm == 0:
                assert cnt == 0
            else:
                assert cnt == 1 and d.tolist() == [abs(l - lm)] and s.tobytes() == (np.float64(max(l, lm) - abs(l - lm))/np.float64(max(l, lm))).tobytes()
        qs = [bytes(g.integers(0, 3, l).tolist()) for l in EDGE]
        both(lo, W(qs, [bytes(g.integers(0, 3, lm).tolist()), bytes(g.integers(0, 256, lm).tolist())]), min_str_score=-1.0, score_thresh_min=0.0, min_matched_words=0)
    got = both(lo, W([b"", b""], [b"", b"ab", b""]), min_str_score=-1.0, score_thresh_min=0.0)      # "" against "ab": distance 2, score 0
    assert got["match_cnt"].tolist() == [1, 1] and got["match_idx"][0].tolist() == [1] and got["match_dist"][1].tolist() == [2] and got["match_score"][0].tolist() == [0.0]
    got = both(lo, W([b""], [b"", b""]))
    assert got["match_cnt"].tolist() == [0] and got["n_cand"] == 0


def test_bytes_above_0x7f_and_the_self_skip(lo):
    texts = [b"\xff\x7f", b"\x80\xff\x80", b"\x00\x7f\x00"]
    got = both(lo, W([b"\x80\xff\x80"], texts), min_matched_words=0)
    assert got["match_idx"][0].tolist() == [1] and got["match_dist"][0].tolist() == [0] and got["match_score"][0].tolist() == [1.0] and got["kf_score"].tolist() == [1]
    got = both(lo, W([b"\x80\xff\x80"], texts, q_self=[1]), min_matched_words=0, score_thresh_min=0.0)      # its own object skipped: 1/3 and 0 remain, threshold 2/9
    assert got["match_idx"][0].tolist() == [0] and got["match_dist"][0].tolist() == [2] and got["match_score"][0].tobytes() == (np.float64(1)/np.float64(3)).tobytes()
    got = both(lo, W([b"\x80\xff\x80"], texts, q_self=[1]), min_matched_words=0)                            # threshold 0.51: none
    assert got["match_cnt"].tolist() == [0]


@pytest.mark.parametrize("thresh_min", [0.51, 0.35])
def test_the_rounding_case(lo, thresh_min):
    """11 bytes, distances 2 and 5: 6/11 ties (9/11)*2/3 in rationals and is below it in the reference's doubles -- the second text is no match."""
    got = both(lo, R.rounding_world(), min_matched_words=0, score_thresh_min=thresh_min)
    assert got["match_cnt"].tolist() == [1] and got["match_idx"][0].tolist() == [0] and got["match_dist"][0].tolist() == [2]
    assert got["match_score"][0].tobytes() == (np.float64(9)/np.float64(11)).tobytes()
    assert got["kf_score"].tolist() == [1, 0] and got["kf_nobj"].tolist() == [1, 0] and got["cand"].tolist() == [0]


def test_exits_of_a_query(lo):
    got = both(lo, W([b"abcdefghij"], [b"abxxxxxxxx", b"yyyyyyyyyy"]), min_matched_words=0)         # best score 0.2 < 0.3
    assert got["match_cnt"].tolist() == [0] and got["kf_score"].tolist() == [0] and got["n_cand"] == 0
    got = both(lo, W([b"abcdefghij"], [b"abcxxxxxxx"]), min_matched_words=0, score_thresh_min=0.0)  # 0.3 is not below 0.3
    assert got["match_cnt"].tolist() == [1] and got["match_dist"][0].tolist() == [7]
    got = both(lo, W([b"abcd", b"ab"], [b"abcd", b"ab", b"abcd"], m_skip=[1, 1, 1]), min_matched_words=0)       # every map text skipped
    assert got["match_cnt"].tolist() == [0, 0] and got["kf_score"].tolist() == [0] and got["n_cand"] == 0
    got = both(lo, W([b"abcd"], [b"abcd", b"abcx", b"abcd", b"abc", b"abcd"], m_skip=[0, 0, 0, 0, 1]), min_matched_words=0)     # ScoreMax == 1.0: exact copies only
    assert got["match_idx"][0].tolist() == [0, 2] and got["kf_score"].tolist() == [2] and got["kf_nobj"].tolist() == [2]
    got = both(lo, W([b"abcd"], [b"abxd", b"abcx", b"xbcd", b"ab"], q_self=[-1]), min_matched_words=0)         # equal scores keep the map's order
    assert got["match_idx"][0].tolist() == [0, 1, 2] and got["match_dist"][0].tolist() == [1, 1, 1]


def test_votes_and_candidates(lo):
    # two queries matching one object: score 2, one object; an object nobody observes votes for nobody
    w = W([b"abcd", b"abcd", b"zzzz"], [b"abcd", b"zzzz"], obs_rows=[[0], []], n_kf=2)
    got = both(lo, w, min_matched_words=0)
    assert got["match_cnt"].tolist() == [1, 1, 1] and got["kf_score"].tolist() == [2, 0] and got["kf_nobj"].tolist() == [1, 0] and got["cand"].tolist() == [0]
    got = both(lo, w, min_matched_words=1)
    assert got["kf_score"].tolist() == [2, 0] and got["n_cand"] == 0
    # a high score from too few objects is passed over, and the walk goes on to the valid keyframe behind it
    w = W([b"aaaa", b"aaaa", b"aaaa", b"bbbb", b"cccc"], [b"aaaa", b"bbbb", b"cccc"], obs_rows=[[0], [1], [1]], n_kf=2)
    got = both(lo, w, min_matched_words=1)
    assert got["kf_score"].tolist() == [3, 2] and got["kf_nobj"].tolist() == [1, 2] and got["cand"].tolist() == [1]
    # more valid keyframes than top_n, with tied scores; then n_kf < top_n
    w = W([b"aaaa", b"bbbb", b"cccc"], [b"aaaa", b"bbbb", b"cccc"], obs_rows=[[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [2, 4]], n_kf=6)
    got = both(lo, w, min_matched_words=1, top_n=3)
    assert got["kf_score"].tolist() == [2, 2, 3, 2, 3, 2] and got["cand"].tolist() == [2, 4, 0]
    got = both(lo, w, min_matched_words=1, top_n=1)
    assert got["cand"].tolist() == [2]
    got = both(lo, w, min_matched_words=1)
    assert got["n_cand"] == 6 and got["cand"].tolist() == [2, 4, 0, 1, 3, 5]
    got = both(lo, w, min_matched_words=2)
    assert got["cand"].tolist() == [2, 4]


def test_independence_of_the_queries(lo, worlds):
    """A query's lists do not depend on what other queries are in the call, nor on where it stands; the votes are the sums."""
    w, refs = worlds[WORLDS[0]]
    nq = len(w["queries"])
    call = lambda order: lo.DetectLoop([w["queries"][q] for q in order], w["q_self"][order], w["map_texts"], w["m_skip"], w["obs_rows"], w["n_kf"], min_matched_words=0, max_match=300)
    sig = lambda r, q: (int(r["match_cnt"][q]), r["match_idx"][q].tobytes(), r["match_dist"][q].tobytes(), r["match_score"][q].tobytes())
    full = call(list(range(nq)))
    assert R.same(full, refs[(0, 0.51)]) is None
    rev = call(list(range(nq))[::-1])
    assert [sig(rev, q) for q in range(nq)] == [sig(full, q) for q in range(nq)][::-1]
    assert np.array_equal(rev["kf_score"], full["kf_score"]) and np.array_equal(rev["kf_nobj"], full["kf_nobj"]) and np.array_equal(rev["cand"], full["cand"])
    tot = np.zeros(w["n_kf"], np.int64)
    for q in range(nq):
        one = call([q])
        assert sig(one, 0) == sig(full, q)
        tot += one["kf_score"]
    assert np.array_equal(tot, full["kf_score"])


def _raw(lo, w, mutate=None, ctx=True, **kw):
    """The C call with sentinel-filled outputs: returns (rc, struct, arrays)."""
    from textslam_amd import loop
    p, A = loop.make_detect_problem(w["queries"], w["q_self"], w["map_texts"], w["m_skip"], w["obs_rows"], w["n_kf"], fill=FILL, **kw)
    if mutate is not None:
        mutate(p, A)
    return lo.lib.tsloop_detect_loop(lo.ctx if ctx else None, C.byref(p)), p, A


OUT_I = ("match_cnt", "match_idx", "match_dist", "kf_score", "kf_nobj", "n_cand", "cand")


def _untouched(A):
    return bool(all(np.all(A[k] == FILL[0]) for k in OUT_I) and np.all(A["match_score"] == FILL[1]))


def test_poisoned_outputs_and_overflow(lo):
    w = W([b"aaaa", b"bbbb", b"abab"], [b"aaaa", b"aaaa", b"bbbb", b"aaaa", b"abab"], obs_rows=[[0], [0, 1], [1], [], [2]], n_kf=3)
    ref = R.detect_loop(min_matched_words=0, **w)
    assert ref["match_cnt"].tolist() == [3, 1, 1]
    # everything fits: entries past a list's count, and cand past n_cand, stay as they were
    rc, p, A = _raw(lo, w, min_matched_words=0, max_match=4, top_n=5)
    assert rc == 0
    from textslam_amd import loop
    assert R.same(loop.detect_result(p, A), ref) is None
    for q, n in enumerate(ref["match_cnt"]):
        assert np.all(A["match_idx"][q, n:] == FILL[0]) and np.all(A["match_dist"][q, n:] == FILL[0]) and np.all(A["match_score"][q, n:] == FILL[1])
    assert ref["n_cand"] == 3 and np.all(A["cand"][3:] == FILL[0])
    # max_match = 2: query 0 does not fit -- counts, votes and candidates complete, its list unwritten, the other lists written, the error says so
    rc, p, A = _raw(lo, w, min_matched_words=0, max_match=2)
    msg = lo.lib.tsloop_last_error(lo.ctx).decode()
    assert rc == -1 and "tsloop_detect_loop" in msg and "max_match" in msg
    assert A["match_cnt"][:3].tolist() == [3, 1, 1]
    assert np.array_equal(A["kf_score"][:3], ref["kf_score"]) and np.array_equal(A["kf_nobj"][:3], ref["kf_nobj"]) and A["n_cand"][0] == ref["n_cand"]
    assert np.array_equal(A["cand"][:ref["n_cand"]], ref["cand"])
    assert np.all(A["match_idx"][0] == FILL[0]) and np.all(A["match_dist"][0] == FILL[0]) and np.all(A["match_score"][0] == FILL[1])
    for q in (1, 2):
        assert A["match_idx"][q, :1].tolist() == ref["match_idx"][q].tolist() and A["match_score"][q, :1].tobytes() == ref["match_score"][q].tobytes()
    got = lo.DetectLoop(w["queries"], w["q_self"], w["map_texts"], w["m_skip"], w["obs_rows"], w["n_kf"], min_matched_words=0, max_match=2)
    assert got["status"] == -1 and got["match_idx"][0] is None and got["match_idx"][1].tolist() == [2] and got["match_cnt"].max() == 3
    # max_match = 3 is exactly enough
    both(lo, w, min_matched_words=0, max_match=3)


def test_lists_beyond_the_default_capacity(lo):
    """More matches in all than n_query x 64: the lists come back in two pieces, the seam inside the first query's list."""
    w = W([b"taxi", b"taxis"], [b"taxi"]*150 + [b"taxis"]*100, obs_rows=[[0]]*150 + [[1]]*100, n_kf=2)
    got = both(lo, w, min_matched_words=0)
    assert got["match_cnt"].tolist() == [150, 100] and got["match_idx"][0].tolist() == list(range(150)) and got["match_idx"][1].tolist() == list(range(150, 250))
    assert set(got["match_dist"][0].tolist()) == {0} and got["kf_score"].tolist() == [150, 100] and got["cand"].tolist() == [0, 1]
    got = both(lo, w, min_matched_words=0, score_thresh_min=0.0, min_str_score=-1.0, max_match=250)
    assert got["match_cnt"].tolist() == [150, 100]


def test_arguments(lo):
    w = W([b"aaaa", b"bbbb"], [b"aaaa", b"aaab", b"bbbb"], obs_rows=[[0, 2], [1], [0, 1, 2]], n_kf=3, q_self=[-1, 2])

    def refused(mutate=None, ww=w, named=True, **kw):
        rc, p, A = _raw(lo, ww, mutate=mutate, **kw)
        assert rc == -1 and _untouched(A)
        if named:
            assert "tsloop_detect_loop" in lo.lib.tsloop_last_error(lo.ctx).decode()

    refused(ctx=False, named=False)                                    # a NULL context
    assert lo.lib.tsloop_detect_loop(lo.ctx, None) == -1
    for name in ("q_off", "q_str", "q_self", "m_off", "m_str", "m_skip", "obs_off", "obs_kf", "match_cnt", "match_idx", "match_dist", "match_score", "kf_score",
                 "kf_nobj", "n_cand", "cand"):
        refused(lambda p, A, name=name: setattr(p, name, None))
    for name in ("n_query", "n_map", "n_kf"):                          # a negative count
        refused(lambda p, A, name=name: setattr(p, name, -1))
    refused(top_n=0); refused(max_match=0); refused(min_matched_words=-1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(min_str_score=bad); refused(score_thresh_min=bad)
    for key in ("q_off", "m_off", "obs_off"):                          # offsets that do not start at 0, or decrease
        def first(p, A, key=key): A[key][0] = 1
        def dec(p, A, key=key): A[key][1] = A[key][2] + 1
        refused(first); refused(dec)
    refused(ww=W([b"a"*65], [b"aaaa"]))                                # a string longer than TSLOOP_TEXT_MAX_LEN
    refused(ww=W([b"aaaa"], [b"aaaa", b"b"*65]))
    def self_hi(p, A): A["q_self"][0] = 3
    def self_lo(p, A): A["q_self"][1] = -2
    def kf_hi(p, A): A["obs_kf"][1] = 3
    def kf_lo(p, A): A["obs_kf"][2] = -1
    def kf_eq(p, A): A["obs_kf"][4] = A["obs_kf"][3]
    def kf_dec(p, A): A["obs_kf"][3], A["obs_kf"][4] = 1, 0
    for m in (self_hi, self_lo, kf_hi, kf_lo, kf_eq, kf_dec):
        refused(m)
    # a row may start below the end of the row before it; 64 bytes are allowed; and the context still answers
    both(lo, w, min_matched_words=0)
    both(lo, W([b"a"*64], [b"a"*64, b"a"*63 + b"b"]), min_matched_words=0)


def test_empty_inputs(lo):
    from textslam_amd import loop
    p = loop.TsloopDetectProblem(); lo.lib.tsloop_default_options_detect(C.byref(p))
    assert lo.lib.tsloop_detect_loop(lo.ctx, C.byref(p)) == 0            # n_query == 0: no pointer is read
    rc, p, A = _raw(lo, W([], [b"aaaa"], n_kf=2, obs_rows=[[0, 1]]))
    assert rc == 0 and A["kf_score"].tolist() == [0, 0] and A["kf_nobj"].tolist() == [0, 0] and A["n_cand"][0] == 0
    assert all(np.all(A[k] == FILL[0]) for k in ("match_cnt", "match_idx", "match_dist", "cand")) and np.all(A["match_score"] == FILL[1])
    rc, p, A = _raw(lo, W([b"aaaa", b""], [], n_kf=2, obs_rows=[]))      # n_map == 0
    assert rc == 0 and A["match_cnt"].tolist() == [0, 0] and A["kf_score"].tolist() == [0, 0] and A["kf_nobj"].tolist() == [0, 0] and A["n_cand"][0] == 0
    assert all(np.all(A[k] == FILL[0]) for k in ("match_idx", "match_dist", "cand")) and np.all(A["match_score"] == FILL[1])
    got = lo.DetectLoop([], [], [b"aaaa"], [0], [[0]], 1)
    assert got["n_cand"] == 0 and got["kf_score"].tolist() == [0] and len(got["match_idx"]) == 0


# ------------------------------------------------------------------------------------------------ the adapter
def mock_world(double_check, long_string=False):
    """A map of 12 keyframes (11 is the current one) and text objects with '#' recognitions, TEXTBAD objects, co-visible and connected keyframes, an object observed
    by nobody, 70 copies of one word (more than the first max_match) -- and, for the fallback, a 65-byte string."""
    g = np.random.default_rng(21)
    nk, cur = 12, 11
    vkfs = [k for k in range(nk) if k not in (cur, 5)]                 # keyframe 5 is in the map and not in vKFs
    cov = np.zeros((3, nk), np.int32); cov[0, 9] = 4; cov[1, 8] = 1; cov[2, 8] = 6; cov[0, 10] = 2; cov[1, 10] = 2; cov[2, 10] = 9
    connect = [7, 3]
    words = [b"exit", b"exit", b"exlt", b"cafe", b"caffe", b"c#fe", b"", b"open", b"opem", b"0pen", b"exit!", b"ex"] + [b"taxi"]*70 + [b"tax1", b"taxis"]
    if long_string:
        words.append(b"x"*65)
    objs = []
    for i, wd in enumerate(words):
        state = 2 if i in (1, 8, 20) else int(g.integers(0, 2))
        obs = sorted(set(int(k) for k in g.integers(0, nk, int(g.integers(0, 5)))))
        if i == 3:
            obs = []
        objs.append((100 + i, state, wd, obs))
    view = [0, 3, 5, 7, 12, 6, 9]                                      # exit, cafe, c#fe (skipped), open, taxi (ScoreMax 1.0: its 68 live exact copies, more than 64), "", 0pen
    for i in view:                                                     # the observed objects are observed by the current keyframe too
        objs[i] = (objs[i][0], objs[i][1], objs[i][2], sorted(set(objs[i][3] + [cur])))
    return {"nk": nk, "cur": cur, "vkfs": vkfs, "connect": connect, "cov": cov, "objs": objs, "view": view, "mmw": 1, "double_check": int(double_check),
            "thresh": 0.35 if double_check else 0.51}


def write_world(f, m):
    f.write(struct.pack("<iii", m["nk"], m["cur"], len(m["vkfs"]))); f.write(np.asarray(m["vkfs"], np.int32).tobytes())
    f.write(struct.pack("<i", len(m["connect"]))); f.write(np.asarray(m["connect"], np.int32).tobytes()); f.write(np.ascontiguousarray(m["cov"], np.int32).tobytes())
    f.write(struct.pack("<i", len(m["objs"])))
    for mnid, state, wd, obs in m["objs"]:
        f.write(struct.pack("<iii", mnid, state, len(wd))); f.write(wd); f.write(struct.pack("<i", len(obs))); f.write(np.asarray(obs, np.int32).tobytes())
    f.write(struct.pack("<i", len(m["view"]))); f.write(np.asarray(m["view"], np.int32).tobytes())
    f.write(struct.pack("<ii", m["mmw"], m["double_check"])); f.write(struct.pack("<d", m["thresh"]))


def gather(m):
    """The adapter's gather restated: the arguments of the call for a mock world, and the observation each query stands for."""
    elig = {}
    for i, k in enumerate(m["vkfs"]):
        if k == m["cur"] or m["cov"][:, k].any() or (m["double_check"] and k in m["connect"]):
            continue
        elig[k] = i
    rows = [sorted(elig[k] for k in obs if k in elig) for _, _, _, obs in m["objs"]]
    qs, q_self, q_obs = [], [], []
    for i, v in enumerate(m["view"]):
        if b"#" in m["objs"][v][2]:
            continue
        qs.append(m["objs"][v][2]); q_self.append(v); q_obs.append(i)
    return {"queries": qs, "q_self": np.array(q_self, np.int32), "map_texts": [o[2] for o in m["objs"]], "m_skip": np.array([o[1] == 2 for o in m["objs"]], np.uint8),
            "obs_rows": rows, "n_kf": len(m["vkfs"])}, q_obs


def test_adapter_from_cxx(tmp_path, lo):
    exe = str(tmp_path / "loop_detect_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "loop_detect_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsloop", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    ms = [mock_world(False), mock_world(True), mock_world(True, long_string=True)]
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", len(ms)))
        for m in ms:
            write_world(f, m)
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "detect loop from C++: ok" in res.stdout, res.stdout
    raw = open(outp, "rb").read(); off = 0

    def arr(dt):
        nonlocal off
        (n,) = struct.unpack_from("<i", raw, off); off += 4
        a = np.frombuffer(raw, dt, n, off); off += n*np.dtype(dt).itemsize
        return a

    calls = []
    for m in ms:
        ok, ncall = struct.unpack_from("<ii", raw, off); off += 8
        if any(len(o[2]) > 64 for o in m["objs"]):
            assert ok == 0                                             # the fallback: the reference's loop is left to the caller
            continue
        assert ok == 1
        calls.append(ncall)
        w, q_obs = gather(m)
        from textslam_amd import loop
        _, A = loop.make_detect_problem(w["queries"], w["q_self"], w["map_texts"], w["m_skip"], w["obs_rows"], w["n_kf"])
        nq, nm = len(w["queries"]), len(w["map_texts"])
        for key, dt, n in (("q_off", np.int32, nq + 1), ("q_str", np.uint8, A["q_off"][-1]), ("q_self", np.int32, nq), ("m_off", np.int32, nm + 1),
                           ("m_str", np.uint8, A["m_off"][-1]), ("m_skip", np.uint8, nm), ("obs_off", np.int32, nm + 1), ("obs_kf", np.int32, A["obs_off"][-1])):
            assert arr(dt).tobytes() == A[key][:n].tobytes(), key      # the flat arrays, byte for byte the Python call's
        assert arr(np.int32).tolist() == q_obs
        got = lo.DetectLoop(w["queries"], w["q_self"], w["map_texts"], w["m_skip"], w["obs_rows"], w["n_kf"], min_matched_words=m["mmw"], score_thresh_min=m["thresh"],
                            max_match=nm)
        assert R.same(got, R.detect_loop(min_matched_words=m["mmw"], score_thresh_min=m["thresh"], **w)) is None
        assert arr(np.int32).tobytes() == got["match_cnt"].tobytes()
        for q in range(nq):
            assert arr(np.int32).tobytes() == got["match_idx"][q].tobytes() and arr(np.int32).tobytes() == got["match_dist"][q].tobytes()
            assert arr(np.float64).tobytes() == got["match_score"][q].tobytes()
        assert arr(np.int32).tobytes() == got["kf_score"].tobytes() and arr(np.int32).tobytes() == got["kf_nobj"].tobytes() and arr(np.int32).tobytes() == got["cand"].tobytes()
        assert arr(np.int32).tolist() == [m["vkfs"][k] for k in got["cand"]]                        # the returned keyframes
        lists = {i: q for q, i in enumerate(q_obs)}
        for i in range(len(m["view"])):                                # vAllMatchTextRes: a skipped observation keeps an empty entry
            (n,) = struct.unpack_from("<i", raw, off); off += 4
            if i not in lists:
                assert n == 0
                continue
            q = lists[i]
            assert n == got["match_cnt"][q]
            for j in range(n):
                mnid, d, s = struct.unpack_from("<idd", raw, off); off += 20
                assert mnid == m["objs"][got["match_idx"][q][j]][0] and d == float(got["match_dist"][q][j]) and struct.pack("<d", s) == got["match_score"][q][j:j + 1].tobytes()
        print("world", m["double_check"], "cnt", got["match_cnt"].tolist(), "cand", got["cand"].tolist(), "calls", ncall)
        assert got["match_cnt"].max() > 64 and got["n_cand"] >= 1
    assert off == len(raw) and calls == [2, 2]                         # a list longer than the first max_match: the adapter called again, once

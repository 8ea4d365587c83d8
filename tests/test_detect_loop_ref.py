"""The restatement of loopClosing::DetectLoop (tests/detect_loop_ref.py) checked against itself on the CPU: the bit-vector recurrence the kernel runs against the
literal DP, the fp64 threshold at the case where doubles and rationals decide differently, and the filter-then-top-N form against the walk as it is written."""
import os
import sys
from fractions import Fraction
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_loop_ref as R                                           # noqa: E402

EDGE = (0, 1, 31, 32, 33, 63, 64)


def test_bitvector_equals_the_dp_at_the_word_edges():
    g = np.random.default_rng(1)
    for alphabet in (np.array([97, 98]), np.array([0, 0x7f, 0x80, 0xfe, 0xff]), np.arange(256)):
        for lq in EDGE:
            for lm in EDGE:
                a = bytes(g.choice(alphabet, lq).tolist()); b = bytes(g.choice(alphabet, lm).tolist())
                assert R.levenshtein_bitvec(a, b) == R.levenshtein_dp(a, b), (a, b)
    assert R.levenshtein_bitvec(b"", b"") == 0 and R.levenshtein_bitvec(b"", b"abc") == 3 and R.levenshtein_bitvec(b"abc", b"") == 3
    assert R.levenshtein_dp(b"kitten", b"sitting") == R.levenshtein_bitvec(b"kitten", b"sitting") == 3
    assert R.levenshtein_bitvec(b"\x80\xff\x80", b"\xff\x7f") == R.levenshtein_dp(b"\x80\xff\x80", b"\xff\x7f") == 2      # bytes >= 0x80 are bytes, not signed chars


def test_bitvector_equals_the_dp_on_random_pairs():
    g = np.random.default_rng(2)
    for _ in range(1500):
        k = int(g.integers(2, 6))
        a = bytes(g.integers(0, k, int(g.integers(0, 65))).tolist()); b = bytes(g.integers(0, k, int(g.integers(0, 65))).tolist())
        assert R.levenshtein_bitvec(a, b) == R.levenshtein_dp(a, b), (a, b)
    w = R.world(5, n_query=4, n_map=40, n_kf=6)
    assert R.same(R.detect_loop(dist=R.levenshtein_bitvec, **w), R.detect_loop(**w)) is None


@pytest.mark.parametrize("thresh_min", [0.51, 0.35])
def test_the_threshold_is_the_doubles(thresh_min):
    w = R.rounding_world()
    assert [R.levenshtein_dp(w["queries"][0], t) for t in w["map_texts"]] == [2, 5, 0]
    assert Fraction(9, 11)*2/3 == Fraction(6, 11)                      # a tie in exact arithmetic ...
    th = R.score_threshold(np.float64(9)/np.float64(11), thresh_min)
    assert np.float64(6)/np.float64(11) < th                           # ... and below the threshold in the reference's doubles
    r = R.detect_loop(score_thresh_min=thresh_min, min_matched_words=0, **w)
    assert r["match_cnt"].tolist() == [1] and r["match_idx"][0].tolist() == [0] and r["match_dist"][0].tolist() == [2]
    assert r["kf_score"].tolist() == [1, 0] and r["cand"].tolist() == [0]


def test_an_exact_copy_keeps_only_exact_copies():
    texts = [b"abcd", b"abcx", b"abcd", b"abc", b"abcd"]
    r = R.detect_loop([b"abcd"], [-1], texts, [0, 0, 0, 0, 1], [[0]]*5, 1, min_matched_words=0)
    assert r["match_idx"][0].tolist() == [0, 2] and r["match_score"][0].tolist() == [1.0, 1.0] and r["kf_score"].tolist() == [2] and r["kf_nobj"].tolist() == [2]
    r = R.detect_loop([b"abcd"], [0], texts[:2] + [b"abxd"], [0, 0, 0], [[0]]*3, 1, min_matched_words=0)      # without a copy: 0.75 -> threshold 0.51
    assert r["match_idx"][0].tolist() == [1, 2] and r["match_dist"][0].tolist() == [1, 1]


def test_filter_then_top_n_is_the_walk():
    g = np.random.default_rng(3)
    for _ in range(400):
        n_kf = int(g.integers(0, 30))
        score = g.integers(0, 6, n_kf); nobj = np.minimum(score, g.integers(0, 6, n_kf))
        for mmw in (0, 1, 2):
            for top_n in (1, 3, 10, 40):
                assert R.filter_top_n(score, nobj, mmw, top_n) == R.walk_candidates(score, nobj, mmw, top_n)
    # a keyframe with a high score and too few objects is passed over; the walk goes on to the next one
    assert R.walk_candidates([5, 3, 3, 1], [1, 2, 3, 1], 1, 10) == [1, 2] == R.filter_top_n([5, 3, 3, 1], [1, 2, 3, 1], 1, 10)

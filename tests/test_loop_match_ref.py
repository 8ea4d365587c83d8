"""The CPU restatement of loop closing's two matchers (tests/loop_match_ref.py) against what can be known without it: a naive all-pairs computation for the
text matcher, hand-built cases with known answers for the scene scan, and the literal double loop for the vectorised scan.  No GPU."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_match_ref as L                                            # noqa: E402

ZERO = np.zeros(32, np.uint8)


def bits(n, start=0):
    """A descriptor with n bits set, from bit `start` on: Hamming distance n to ZERO."""
    d = np.zeros(32, np.uint8)
    for b in range(start, start + n):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def naive_text(d1, d2):
    pop = lambda a, b: sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))
    ti, di = [], []
    for q in d1:
        best, bi = L.INT_MAX, -1
        for j, t in enumerate(d2):
            d = pop(q, t)
            if d < best:
                best, bi = d, j
        ti.append(bi); di.append(best)
    cut = max(2.0 * min(di), 30.0) if di else 0.0
    return ti, di, [int(len(d2) > 0 and d < cut) for d in di]


# ------------------------------------------------------------------ text
def test_text_against_naive_all_pairs_with_ties():
    rng = np.random.default_rng(1)
    for n1, n2 in ((1, 2), (17, 9), (40, 40), (0, 3), (4, 0)):
        d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
        if n2 >= 9:
            d2[7] = d2[2]; d2[8] = d2[2]                               # duplicated rows: a tie goes to the first index
        d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
        if n1 >= 17 and n2 >= 9:
            d1[5] = d2[2]; d1[6] = d2[7] ^ bits(3)
        r = L.match_text([(d1, d2)])[0]
        ti, di, good = naive_text(d1, d2)
        assert r["train_idx"].tolist() == ti and r["dist"].tolist() == di and r["good"].tolist() == good, (n1, n2)
        if n1 >= 17 and n2 >= 9:
            assert r["train_idx"][5] == 2 and r["dist"][5] == 0 and r["train_idx"][6] == 2 and r["dist"][6] == 3
    r = L.match_text([(np.zeros((4, 32), np.uint8), np.zeros((0, 32), np.uint8))])[0]
    assert r["train_idx"].tolist() == [-1] * 4 and r["dist"].tolist() == [L.INT_MAX] * 4 and r["good"].tolist() == [0] * 4


def test_text_threshold_edges():
    far = np.full(32, 0xff, np.uint8)
    for dists, good in (((0, 29, 30), [1, 1, 0]), ((20, 39, 40), [1, 1, 0])):
        d1 = np.stack([bits(d) for d in dists])
        r = L.match_text([(d1, np.stack([ZERO, far]))])[0]
        assert r["dist"].tolist() == list(dists) and r["train_idx"].tolist() == [0, 0, 0] and r["good"].tolist() == good, dists


# ------------------------------------------------------------------ scene: the scan
def _scan(d1, d2, **kw):
    d1 = np.stack(d1); d2 = np.stack(d2)
    m, n, cnt = L.scan(d1, np.ones(len(d1), bool), d2, np.ones(len(d2), bool), **kw)
    m2, n2 = L.scan_loops(d1, np.ones(len(d1), bool), d2, np.ones(len(d2), bool), **kw)
    assert m.tolist() == m2.tolist() and n == n2
    return m.tolist(), n, cnt


def test_scene_steal():
    """Two current descriptors want the one candidate row; the later one is closer: it wins, the earlier goes back to -1, the count stays 1."""
    m, n, cnt = _scan([bits(4), bits(2)], [ZERO])
    assert m == [-1, 0] and n == 1 and cnt["steals"] == 1
    m, n, cnt = _scan([bits(2), bits(2)], [ZERO])                       # identical: vMatchDist[0] = 2 <= 2 hides the row from the second one
    assert m == [0, -1] and n == 1 and cnt["steals"] == 0 and cnt["hidden"] == 1


def test_scene_runner_up_hidden_by_the_filter():
    """Candidate rows A = ZERO and B = bits(8).  Feature 0 = bits(1) claims A at distance 1.  Feature 1 = bits(8, start=4) is at 8 from B (bits 4 .. 7 shared)
    and 8 from A: A is hidden (vMatchDist[A] = 1 <= 8), so B stands alone and is accepted; without the filter 8 against 8 fails the ratio test."""
    A, B = ZERO, bits(8)
    f1 = bits(8, start=4)
    assert L.hamming_rows(f1, np.stack([A, B])).tolist() == [8, 8]
    m, n, cnt = _scan([bits(1), f1], [A, B])
    assert m == [0, 1] and n == 2 and cnt["hidden"] == 1 and cnt["ratio_rej"] == 0
    m, n, cnt = _scan([f1], [A, B])                                    # the same feature without the earlier claim: rejected
    assert m == [-1] and n == 0 and cnt["ratio_rej"] == 1


def test_scene_ratio_boundary():
    far = bits(50, start=100)
    assert _scan([bits(45)], [ZERO, bits(45) ^ far])[0] == [-1]        # 45 against 50: 45 < 45.0 is false
    assert L.hamming_rows(bits(45), (bits(45) ^ far).reshape(1, 32)).tolist() == [50]
    assert _scan([bits(44)], [ZERO, bits(44) ^ far])[0] == [0]         # 44 against 50
    assert _scan([bits(45)], [ZERO])[0] == [0]                         # a single eligible candidate: the runner-up is INT_MAX


def test_scene_th_low():
    assert _scan([bits(50)], [ZERO])[0] == [0]
    m, n, cnt = _scan([bits(51)], [ZERO])
    assert m == [-1] and cnt["th_rej"] == 1
    assert _scan([bits(51)], [ZERO], th_low=51)[0] == [0]


def test_scene_scan_against_the_literal_loops():
    rng = np.random.default_rng(4)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    flip = lambda r, n: r ^ np.bitwise_or.reduce([bits(1, int(b)) for b in rng.choice(256, n, replace=False)] + [ZERO])
    d1 = np.stack([flip(base[i % 40], int(rng.integers(0, 30))) for i in range(70)])
    d2 = np.stack([flip(base[i % 40], int(rng.integers(0, 60))) for i in rng.permutation(60)])
    e1 = rng.uniform(size=70) < 0.8; e2 = rng.uniform(size=60) < 0.8
    m, n, cnt = L.scan(d1, e1, d2, e2)
    m2, n2 = L.scan_loops(d1, e1, d2, e2)
    assert m.tolist() == m2.tolist() and n == n2 == int((m >= 0).sum()) and n >= 10 and cnt["steals"] >= 1 and cnt["hidden"] >= 1
    assert (m[~e1] == -1).all() and not set(m[m >= 0].tolist()) & set(np.flatnonzero(~e2).tolist())


# ------------------------------------------------------------------ scene: eligibility
def test_scene_eligibility():
    w, h = 64, 48
    box = np.array([[10.9, 10.2], [30.7, 10.9], [30.1, 20.8], [10.3, 20.5]])           # truncated: the rectangle (10, 10) .. (30, 20), boundary included
    xy = np.array([[20, 15], [10, 15], [9, 15], [30, 20], [31, 20], [20, 21],           # inside, on the left edge, one pixel outside it, the corner, one outside, below
                   [9.5, 15], [10.5, 9.4], [9.49, 15], [30.5, 15],                      # 9.5 rounds to 10 (covered), 10.5 to 11 / 9.4 to 9 (not), 9.49 to 9 (not), 30.5 to 31 (not)
                   [-3, 15], [20, 48], [64.2, 15], [1e9, -1e9]], np.float32)            # outside the image: not covered
    has = np.ones(len(xy), np.uint8); has[0] = 1
    el, nbox = L.eligibility(w, h, xy, has, box[None])
    assert (~el).tolist() == [True, True, False, True, False, False, True, False, False, False, False, False, False, False]
    assert nbox == 4
    assert L.roundf(10.5) == 11 and L.roundf(-0.5) == -1 and L.roundf(0.49999997) == 0 and L.roundf(2.5) == 3
    el, nbox = L.eligibility(w, h, xy, np.zeros(len(xy), np.uint8), box[None])          # has3d = 0: out whatever the boxes say
    assert not el.any() and nbox == 0
    el, nbox = L.eligibility(w, h, xy, has, np.zeros((0, 4, 2)))                        # no box: has3d alone
    assert el.all() and nbox == 0
    # the current keyframe's eligibility depends on the candidate (its label image does)
    d = np.stack([bits(3), bits(5)]); c = dict(xy=np.array([[40, 40]], np.float32), desc=ZERO[None], has3d=[1], quad_can=np.zeros((0, 4, 2)))
    r = L.match_scene(w, h, xy[:2], d, [1, 1], [dict(c, quad_cur=box[None]), dict(c, quad_cur=np.zeros((0, 4, 2)))])
    assert r[0]["match12"].tolist() == [-1, -1] and r[0]["n_match"] == 0 and r[0]["box_inelig"] == 2
    assert r[1]["match12"].tolist() == [0, -1] and r[1]["n_match"] == 1

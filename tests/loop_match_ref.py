"""CPU restatement of the two matchers of loopClosing::SearchMatch as include/tsorb.h states them (tsorb_match_brute_text, tsorb_match_brute_scene),
written from that description and independently of the kernels (textslam_amd/csrc/tsbrute.h).  numpy / plain Python; integers and flags only.

  match_text(pairs)        FeatureMatch_brute(.., USETHRESH = true): docs/bfmatcher_recalled.md's nearest neighbour (first index on a tie) and the
                           max(2 min_dist, 30.0) cut, per pair
  match_scene(...)         SearchMatch_Other: eligibility (has3d, not covered by a text box of the candidate's label image) and the sequential claim scan,
                           per candidate, with the counters the tests need
  match_scene_loops(...)   the same scan as the literal double loop (slow: small cases), to check the vectorised one against

The fill of a box is tests/cvorb_ref.py's mask_quad (cv::fillPoly of a quad, corners truncated like cv::Point)."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvorb_ref as R                                                  # noqa: E402

INT_MAX = 2147483647
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming_rows(d, rows):
    """Hamming distances of the 32-byte descriptor d to every row of rows [n, 32]."""
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    return _POP[np.bitwise_xor(rows, np.asarray(d, np.uint8).reshape(1, 32))].sum(axis=1)


def roundf(v):
    """(int)roundf(v) for an fp32 v: halves away from zero (the fraction of an fp32 is exact in a double)."""
    v = float(np.float32(v))
    a = abs(v)
    f = np.floor(a)
    r = int(f) + (1 if a - f >= 0.5 else 0)
    return -r if v < 0 else r


# ------------------------------------------------------------------ text pairs
def match_text(pairs):
    """pairs: list of (desc1 [n1, 32], desc2 [n2, 32]).  Returns a list of dicts: train_idx [n1] int32 (relative to the pair), dist [n1] int32, good [n1] uint8."""
    out = []
    for d1, d2 in pairs:
        d1 = np.asarray(d1, np.uint8).reshape(-1, 32); d2 = np.asarray(d2, np.uint8).reshape(-1, 32)
        n1, n2 = len(d1), len(d2)
        ti = np.full(n1, -1, np.int32); di = np.full(n1, INT_MAX, np.int32)
        if n2 > 0:
            for q in range(n1):
                d = hamming_rows(d1[q], d2)
                j = int(np.argmin(d))                                  # the first index of the minimum
                ti[q], di[q] = j, d[j]
        good = np.zeros(n1, np.uint8)
        if n1 > 0 and n2 > 0:                                          # (an empty set 2: no match, never good)
            cut = max(2.0 * float(di.min()), 30.0)
            good = (di.astype(np.float64) < cut).astype(np.uint8)
        out.append(dict(train_idx=ti, dist=di, good=good))
    return out


# ------------------------------------------------------------------ scene features
def label_mask(w, h, quads):
    """True where a text label >= 0 was painted: the union of the boxes' fills on a w x h image."""
    m = np.zeros((h, w), bool)
    for q in np.asarray(quads, np.float64).reshape(-1, 4, 2):
        m |= R.mask_quad(w, h, q).astype(bool)
    return m


def covered(mask, xy):
    """Per keypoint: its rounded pixel lies inside the image and carries a label."""
    h, w = mask.shape
    out = np.zeros(len(xy), bool)
    for i, (x, y) in enumerate(np.asarray(xy, np.float32).reshape(-1, 2)):
        u, v = roundf(x), roundf(y)
        out[i] = 0 <= u < w and 0 <= v < h and bool(mask[v, u])
    return out


def eligibility(w, h, xy, has3d, quads):
    """(eligible [n] bool, number of features a box alone made ineligible)."""
    has = np.asarray(has3d).reshape(-1).astype(bool)
    cov = covered(label_mask(w, h, quads), xy) if len(has) else np.zeros(0, bool)
    return has & ~cov, int((has & cov).sum())


def _two_smallest(d, idx):
    """(best, first index of best, runner-up) of the distances d at the indices idx (both in index order); INT_MAX / -1 where absent."""
    if len(d) == 0:
        return INT_MAX, -1, INT_MAX
    k = int(np.argmin(d))
    best = int(d[k])
    rest = np.delete(d, k)
    return best, int(idx[k]), (int(rest.min()) if len(rest) else INT_MAX)


def scan(desc1, el1, desc2, el2, th_low=50, ratio=0.9):
    """The claim scan of one candidate.  Returns match12 [n1] int32, n_match and the counters:
    steals (an accepted i1 took an i2 that had an owner), hidden (steps at which the vMatchDist filter changed best / index / runner-up against the
    unfiltered scan), ratio_rej (best <= th_low, ratio test failed), th_rej (there was a best, above th_low)."""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    n1, n2 = len(desc1), len(desc2)
    m12 = np.full(n1, -1, np.int32); m21 = np.full(n2, -1, np.int64); md = np.full(n2, INT_MAX, np.int64)
    cnt = dict(steals=0, hidden=0, ratio_rej=0, th_rej=0)
    n_match = 0
    e2 = np.flatnonzero(el2)
    for i1 in range(n1):
        if not el1[i1]:
            continue
        d = hamming_rows(desc1[i1], desc2[e2]) if len(e2) else np.zeros(0, np.int64)
        keep = ~(md[e2] <= d)
        best, bi, second = _two_smallest(d[keep], e2[keep])
        if (best, bi, second) != _two_smallest(d, e2):
            cnt["hidden"] += 1
        if bi < 0:
            continue
        if best <= th_low:
            if best < float(second) * ratio:
                if m21[bi] >= 0:
                    m12[m21[bi]] = -1; n_match -= 1; cnt["steals"] += 1
                m12[i1] = bi; m21[bi] = i1; md[bi] = best; n_match += 1
            else:
                cnt["ratio_rej"] += 1
        else:
            cnt["th_rej"] += 1
    return m12, n_match, cnt


def scan_loops(desc1, el1, desc2, el2, th_low=50, ratio=0.9):
    """The scan as the literal double loop with its if / else-if chain."""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32); desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    n1, n2 = len(desc1), len(desc2)
    dist = [[int(_POP[np.bitwise_xor(desc1[a], desc2[b])].sum()) for b in range(n2)] for a in range(n1)]
    m12 = [-1] * n1; m21 = [-1] * n2; md = [INT_MAX] * n2
    n_match = 0
    for i1 in range(n1):
        if not el1[i1]:
            continue
        best, second, bi = INT_MAX, INT_MAX, -1
        for i2 in range(n2):
            if not el2[i2]:
                continue
            d = dist[i1][i2]
            if md[i2] <= d:
                continue
            if d < best:
                second = best; best = d; bi = i2
            elif d < second:
                second = d
        if best <= th_low and best < float(second) * ratio:
            if m21[bi] >= 0:
                m12[m21[bi]] = -1; n_match -= 1
            m12[i1] = bi; m21[bi] = i1; md[bi] = best; n_match += 1
    return np.array(m12, np.int32).reshape(n1), n_match


def match_scene(w, h, xy1, desc1, has3d1, cands, th_low=50, ratio=0.9):
    """cands: list of dicts xy [n2, 2], desc [n2, 32], has3d [n2], quad_cur [nq, 4, 2], quad_can [nq, 4, 2].
    Returns per candidate a dict: match12 [n1] int32, n_match, the scan's counters, box_inelig (features with 3-D information a box took out, both sides),
    el1 / el2 (the eligibility flags)."""
    out = []
    for c in cands:
        el1, b1 = eligibility(w, h, xy1, has3d1, c["quad_cur"])
        el2, b2 = eligibility(w, h, c["xy"], c["has3d"], c["quad_can"])
        m12, n, cnt = scan(desc1, el1, c["desc"], el2, th_low, ratio)
        out.append(dict(match12=m12, n_match=n, box_inelig=b1 + b2, el1=el1, el2=el2, **cnt))
    return out

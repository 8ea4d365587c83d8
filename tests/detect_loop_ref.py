"""loopClosing::DetectLoop (src/loopClosing.cc:119-304) restated in plain Python / numpy over the flat arguments of tsloop_detect_loop (include/tsloop.h).

  levenshtein_dp      the DP of tool::LevenshteinDist (src/tool.cc:281-296), literally, over bytes
  levenshtein_bitvec  the bit-vector recurrence the kernel runs (textslam_amd/csrc/tsloop_detect.h: td_myers), on Python integers masked to 64 bits
  detect_loop         scores with one float64 division, a stable sort per query, the threshold in float64 in the reference's order of operations, the votes,
                      a stable sort of the keyframes and the walk of :277-300 as it is written
  world               a seeded world: a small alphabet, so ties and near-threshold scores are common

The two stated differences from the reference are the interface's: a pair of two empty strings is not scored (the reference divides 0 by 0), and equal scores keep
their index order (the reference's std::sort leaves them in an unspecified order)."""
import numpy as np

TEXT_MAX_LEN = 64
M64 = (1 << 64) - 1


def levenshtein_dp(a, b):
    a = bytes(a); b = bytes(b)
    l1, l2 = len(a), len(b)
    dp = [[0]*(l2 + 1) for _ in range(l1 + 1)]
    for i in range(1, l1 + 1):
        dp[i][0] = i
    for j in range(1, l2 + 1):
        dp[0][j] = j
    for i in range(1, l1 + 1):
        for j in range(1, l2 + 1):
            if a[i - 1] == b[j - 1]:
                dp[i][j] = dp[i - 1][j - 1]
            else:
                dp[i][j] = min(dp[i - 1][j - 1], min(dp[i][j - 1], dp[i - 1][j])) + 1
    return dp[l1][l2]


def levenshtein_bitvec(pattern, text):
    """The kernel's path: the pattern (the query, at most 64 bytes) as 256 match masks, one 64-bit column state walked along the text."""
    pattern = bytes(pattern); text = bytes(text)
    m = len(pattern)
    assert m <= TEXT_MAX_LEN
    if m == 0:
        return len(text)
    peq = [0]*256
    for i, ch in enumerate(pattern):
        peq[ch] |= 1 << i
    Pv, Mv, top, score = M64, 0, 1 << (m - 1), m
    for ch in text:
        Eq = peq[ch]
        Xv = Eq | Mv
        Xh = ((((Eq & Pv) + Pv) & M64) ^ Pv) | Eq
        Ph = Mv | (~(Xh | Pv) & M64)
        Mh = Pv & Xh
        if Ph & top:
            score += 1
        if Mh & top:
            score -= 1
        Ph = ((Ph << 1) | 1) & M64
        Mh = (Mh << 1) & M64
        Pv = Mh | (~(Xv | Ph) & M64)
        Mv = Ph & Xv
    return score


def pair_score(len_q, len_m, dist):
    maxlen = max(len_q, len_m)
    return np.float64(maxlen - dist)/np.float64(maxlen)


def score_threshold(score_max, score_thresh_min):
    """:207-210 in float64: a multiplication, then a division, each rounded once, then std::max."""
    score_max = np.float64(score_max)
    if score_max == np.float64(1.0):
        return score_max
    third = (score_max*np.float64(2.0))/np.float64(3.0)
    return third if third > np.float64(score_thresh_min) else np.float64(score_thresh_min)


def walk_candidates(kf_score, kf_nobj, min_matched_words, top_n):
    """:269-300 as written: the keyframes sorted by descending score (stable: equal scores keep their index order), then break / continue / break."""
    n_kf = len(kf_score)
    order = sorted(range(n_kf), key=lambda k: -int(kf_score[k]))
    thresh_top = min(top_n, n_kf)
    out = []
    for k in order:
        if kf_score[k] <= min_matched_words:
            break
        if kf_nobj[k] <= min_matched_words:
            continue
        if len(out) >= thresh_top:
            break
        out.append(k)
    return out


def filter_top_n(kf_score, kf_nobj, min_matched_words, top_n):
    """What the kernel does: the keyframes that pass both tests, by (descending score, ascending index), the first min(top_n, n_kf)."""
    ok = [k for k in range(len(kf_score)) if kf_score[k] > min_matched_words and kf_nobj[k] > min_matched_words]
    ok.sort(key=lambda k: (-int(kf_score[k]), k))
    return ok[:min(top_n, len(kf_score))]


def detect_loop(queries, q_self, map_texts, m_skip, obs_rows, n_kf, min_matched_words=1, score_thresh_min=0.51, min_str_score=0.3, top_n=10, dist=levenshtein_dp):
    """Returns the dict LoopOptimizer.DetectLoop returns (lists never overflow here)."""
    nq, nm = len(queries), len(map_texts)
    out = {"match_cnt": np.zeros(nq, np.int32), "match_idx": [], "match_dist": [], "match_score": []}
    kf_score = np.zeros(n_kf, np.int32); objs = [set() for _ in range(n_kf)]
    for q in range(nq):
        scored = []                                                   # (m, dist, score) of the pairs the reference scores
        for m in range(nm):
            if m_skip[m] or m == q_self[q]:
                continue
            if max(len(queries[q]), len(map_texts[m])) == 0:
                continue
            d = dist(queries[q], map_texts[m])
            scored.append((m, d, pair_score(len(queries[q]), len(map_texts[m]), d)))
        scored.sort(key=lambda t: -t[2])                              # stable
        matches = []
        if scored and not (scored[0][2] < np.float64(min_str_score)):
            th = score_threshold(scored[0][2], score_thresh_min)
            for t in scored:
                if t[2] < th:
                    break
                matches.append(t)
        out["match_cnt"][q] = len(matches)
        out["match_idx"].append(np.array([t[0] for t in matches], np.int32)); out["match_dist"].append(np.array([t[1] for t in matches], np.int32))
        out["match_score"].append(np.array([t[2] for t in matches], np.float64))
        for m, _, _ in matches:
            for k in obs_rows[m]:
                kf_score[k] += 1; objs[k].add(m)
    kf_nobj = np.array([len(s) for s in objs], np.int32).reshape(n_kf)
    cand = walk_candidates(kf_score, kf_nobj, min_matched_words, top_n)
    out.update({"kf_score": kf_score, "kf_nobj": kf_nobj, "n_cand": len(cand), "cand": np.array(cand, np.int32), "status": 0})
    return out


def world(seed, n_query=8, n_map=300, n_kf=40, alphabet=b"abcd", len_lo=3, len_hi=9, skip_frac=0.1, obs_max=6):
    """A seeded world.  Map texts are random words over a small alphabet, many of them edits of a few stems; the queries are edits of map texts, some of them the
    map's own objects (q_self).  Keyframe rows are random increasing subsets, some of them empty."""
    g = np.random.default_rng(seed)
    A = np.frombuffer(alphabet, np.uint8)

    def word():
        return bytes(g.choice(A, int(g.integers(len_lo, len_hi + 1))).tolist())

    def edit(w):
        w = bytearray(w)
        for _ in range(int(g.integers(0, 3))):
            op = int(g.integers(0, 3)); at = int(g.integers(0, len(w) + 1))
            if op == 0 and len(w) < TEXT_MAX_LEN:
                w.insert(at, int(g.choice(A)))
            elif op == 1 and len(w) > 1:
                del w[min(at, len(w) - 1)]
            elif len(w) > 0:
                w[min(at, len(w) - 1)] = int(g.choice(A))
        return bytes(w)

    stems = [word() for _ in range(max(4, n_map//12))]
    map_texts = [edit(stems[int(g.integers(len(stems)))]) if g.random() < 0.7 else word() for _ in range(n_map)]
    m_skip = (g.random(n_map) < skip_frac).astype(np.uint8)
    obs_rows = []
    for _ in range(n_map):
        n = int(g.integers(0, min(obs_max, n_kf) + 1)) if n_kf else 0
        obs_rows.append(np.sort(g.choice(n_kf, n, replace=False)).astype(np.int32) if n else np.zeros(0, np.int32))
    queries, q_self = [], []
    for q in range(n_query):
        m = int(g.integers(n_map))
        if q % 3 == 0:
            queries.append(map_texts[m]); q_self.append(m)            # the query's own object: skipped, its copies and near copies remain
        else:
            queries.append(edit(map_texts[m])); q_self.append(-1)
    return {"queries": queries, "q_self": np.array(q_self, np.int32), "map_texts": map_texts, "m_skip": m_skip, "obs_rows": obs_rows, "n_kf": n_kf}


def rounding_world():
    """A query of 11 bytes, its best match at distance 2, another map text at distance 5: 6/11 == (9/11)*2/3 in rationals, below it in doubles."""
    q = b"abcdefghijk"
    texts = [b"abcdefghixx", b"abcdefxxxxx", b"abcdefghijk"]           # distances 2, 5 and 0 (the last one the query's own object: skipped)
    return {"queries": [q], "q_self": np.array([2], np.int32), "map_texts": texts, "m_skip": np.zeros(3, np.uint8),
            "obs_rows": [np.array([0], np.int32), np.array([0, 1], np.int32), np.array([1], np.int32)], "n_kf": 2}


def same(a, b):
    """Two result dicts equal as integers, bytes and bit patterns.  Returns the name of the first difference or None."""
    if not np.array_equal(a["match_cnt"], b["match_cnt"]):
        return "match_cnt"
    for key in ("match_idx", "match_dist", "match_score"):
        for q, (x, y) in enumerate(zip(a[key], b[key])):
            if (x is None) != (y is None) or (x is not None and (x.dtype != y.dtype or x.tobytes() != y.tobytes())):
                return "%s[%d]" % (key, q)
    for key in ("kf_score", "kf_nobj", "cand"):
        if not np.array_equal(a[key], b[key]):
            return key
    return None if a["n_cand"] == b["n_cand"] else "n_cand"

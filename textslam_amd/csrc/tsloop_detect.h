// tsloop_detect.h -- loopClosing::DetectLoop's string scan and keyframe vote (tsloop_detect_loop, include/tsloop.h).  Included by tsloop.hip.
// Three launches, none of which waits for another workgroup; every number that leaves them is an integer or one fp64 quotient of two integers.
//   k_td_scan  grid (tiles of TD_T map texts) x n_query, a lane per map text.  The query's 256 per-byte match masks (bit i = "query byte i is this byte") are built
//              once per workgroup in LDS, thread c the mask of byte value c; the tile's string bytes are staged into LDS as aligned dwords.  Each lane runs the
//              bit-vector recurrence (Myers 1999 in Hyyro's form for the global distance) over its map text: 64-bit word operations, no array.  With the query
//              as the pattern, bit len_q - 1 of the horizontal deltas carries the last DP row's steps, so the running value ends as tool::LevenshteinDist's
//              dp[len1][len2].  The distance goes out as one byte per pair, TD_SKIP for a pair the reference does not score.
//              Bounds: the query's length (<= TSLOOP_TEXT_MAX_LEN) for the masks, the tile's bytes for the staging, the map text's length for the recurrence.
//   k_td_pick  one workgroup per query.  Pass 1 folds ScoreMax over the query's row of distances (the maximum of the scores' bit patterns: scores are >= 0, so
//              their unsigned order is their order -- a maximum, whatever the order it is taken in).  Scoreth is evaluated in fp64 exactly as the reference
//              writes it: ScoreMax*2.0 rounded, then /3.0 rounded (contraction is off for this library; nothing is reassociated).  Pass 2 ballot-compacts the
//              matches in index order, counts them, and adds 1 to each matched map text's hit count (integer atomics).  If the list fits max_match, pass 3 places
//              each match at its rank: the number of matches with a larger score, or an equal score and a smaller index -- the order of a stable sort.
//              The ranked list is a row of 16-byte records in scratch.
//              Bounds: n_map for passes 1 and 2, the query's match count (<= max_match) squared for pass 3.
//   k_td_vote  one workgroup.  First the lists that fit are packed one behind the other into the download block (rec_off: the prefix sums of their counts), so that
//              what crosses the bus is what was matched, not n_query x max_match.  Then every matched map text adds its hit count to kf_score and 1 to kf_nobj of
//              each keyframe in its row of obs_kf (integer atomics, so the sums do not depend on scheduling; a row is strictly increasing, so a map text counts
//              once per keyframe).  Then at most min(top_n, n_kf)
//              rounds, each taking the largest remaining (kf_score, smaller index first) among the keyframes that pass both tests.
//              Bounds: n_query and the matches in all for the packing, n_map and the rows' lengths for the vote, min(top_n, n_kf) rounds of n_kf for the selection.
#pragma once

#define TD_T 256                  // threads of every workgroup here, map texts of a scan tile, and the number of byte values
#define TD_NW (TD_T/64)
#define TD_SKIP 255               // a pair that is not scored (a distance is at most TSLOOP_TEXT_MAX_LEN)
static_assert(TSLOOP_TEXT_MAX_LEN == 64, "one 64-bit word holds a query's column of the DP");

struct TdRec { int32_t idx, dist; double score; };                // one match: the map text, the distance, the score

struct TdDev {
    int32_t n_query, n_map, n_kf, top_n, n_tile, max_match, min_matched_words;
    const int32_t *q_off; const uint8_t *q_str; const int32_t *q_self;
    const int32_t *m_off; const uint8_t *m_str; const uint8_t *m_skip;
    const int32_t *obs_off, *obs_kf;
    double min_str_score, score_thresh_min;
    uint8_t *dist;                // [n_query][n_map] scratch
    int32_t *hit;                 // [n_map] scratch: the number of queries that matched the map text
    int32_t *tmp_idx; double *tmp_score;          // [n_query][max_match] scratch: a query's matches in index order
    TdRec *rank_rec;              // [n_query][max_match] scratch: a query's matches in the list's order
    int32_t *match_cnt, *rec_off; // [n_query], [n_query + 1]: where each list that fits starts in out_rec
    TdRec *out_rec;               // the lists that fit, packed
    int32_t *kf_score, *kf_nobj, *n_cand, *cand;
};

// the score of a scored pair: one IEEE division of two exactly converted integers (loopClosing.cc:192; maxlen - dist is exact in doubles either way round)
__device__ __forceinline__ double td_score(int maxlen, int dist) { return (double)(maxlen - dist)/(double)maxlen; }

// Levenshtein distance of the pattern behind peq (length m, 1 <= m <= 64) to the n bytes at txt
__device__ __forceinline__ int td_myers(const unsigned long long *peq, int m, const uint8_t *txt, int n) {
    unsigned long long Pv = ~0ull, Mv = 0ull; const unsigned long long top = 1ull << (m - 1);
    int score = m;
#pragma unroll 1
    for (int j = 0; j < n; j++) {
        const unsigned long long Eq = peq[txt[j]];
        const unsigned long long Xv = Eq | Mv, Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        unsigned long long Ph = Mv | ~(Xh | Pv), Mh = Pv & Xh;
        score += (Ph & top) ? 1 : 0; score -= (Mh & top) ? 1 : 0;
        Ph = (Ph << 1) | 1ull; Mh <<= 1;                               // | 1: the DP's first row counts up (dp[0][j] = j)
        Pv = Mh | ~(Xv | Ph); Mv = Ph & Xv;
    }
    return score;
}

__global__ __launch_bounds__(TD_T) void k_td_scan(TdDev D) {
    __shared__ unsigned long long s_peq[256];
    __shared__ uint32_t s_tile[TD_T*TSLOOP_TEXT_MAX_LEN/4 + 4];
    __shared__ uint8_t s_q[TSLOOP_TEXT_MAX_LEN];
    const int tid = threadIdx.x, q = (int)(blockIdx.x/(unsigned)D.n_tile), tile = (int)(blockIdx.x % (unsigned)D.n_tile);
    const int qa = D.q_off[q], len_q = D.q_off[q + 1] - qa;
    if (tid < len_q) s_q[tid] = D.q_str[qa + tid];
    const int t0 = tile*TD_T, t1 = min(t0 + TD_T, D.n_map);
    const int b0 = D.m_off[t0], b1 = D.m_off[t1], a0 = b0 & ~3;       // [a0, b1) as aligned dwords: at most TD_T*64 + 3 bytes (the device copy of m_str is padded)
    const uint32_t *src = (const uint32_t *)(D.m_str + a0);
    for (int w = tid; 4*w < b1 - a0; w += TD_T) s_tile[w] = src[w];
    __syncthreads();
    {   unsigned long long e = 0ull;
        for (int i = 0; i < len_q; i++) e |= (unsigned long long)(s_q[i] == (uint8_t)tid) << i;
        s_peq[tid] = e; }
    __syncthreads();
    const int m = t0 + tid;
    if (m >= t1) return;
    if (q == 0) D.hit[m] = 0;
    const int ma = D.m_off[m], len_m = D.m_off[m + 1] - ma, maxlen = max(len_q, len_m);
    int d = TD_SKIP;
    if (!D.m_skip[m] && m != D.q_self[q] && maxlen > 0)
        d = len_q == 0 ? len_m : td_myers(s_peq, len_q, (const uint8_t *)s_tile + (ma - a0), len_m);
    D.dist[(size_t)q*(size_t)D.n_map + (size_t)m] = (uint8_t)d;
}

// the maximum of one value per thread, returned to every thread (s_red: TD_NW words; two barriers)
__device__ __forceinline__ unsigned long long td_block_max(unsigned long long v, unsigned long long *s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = s_red[0];
#pragma unroll
    for (int w = 1; w < TD_NW; w++) r = s_red[w] > r ? s_red[w] : r;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(TD_T) void k_td_pick(TdDev D) {
    __shared__ unsigned long long s_red[TD_NW];
    __shared__ int s_cnt[TD_NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
    const int len_q = D.q_off[q + 1] - D.q_off[q];
    const uint8_t *row = D.dist + (size_t)q*(size_t)D.n_map;
    auto score_of = [&](int m, int d) { return td_score(max(len_q, D.m_off[m + 1] - D.m_off[m]), d); };
    // pass 1: ScoreMax as (bit pattern + 1), 0 = nothing scored
    unsigned long long best = 0ull;
    for (int m = tid; m < D.n_map; m += TD_T) {
        const int d = row[m];
        if (d != TD_SKIP) { const unsigned long long b = (unsigned long long)__double_as_longlong(score_of(m, d)) + 1ull; best = b > best ? b : best; }
    }
    best = td_block_max(best, s_red);
    const double ScoreMax = best ? __longlong_as_double((long long)(best - 1ull)) : -1.0;
    if (best == 0ull || ScoreMax < D.min_str_score) { if (tid == 0) D.match_cnt[q] = 0; return; }
    double Scoreth;
    if (ScoreMax == 1.0) Scoreth = ScoreMax;
    else { const double twice = ScoreMax*2.0, third = twice/3.0; Scoreth = third > D.score_thresh_min ? third : D.score_thresh_min; }   // std::max(a, b): a < b ? b : a
    // pass 2: the matches in index order
    int32_t *t_idx = D.tmp_idx + (size_t)q*(size_t)D.max_match; double *t_sc = D.tmp_score + (size_t)q*(size_t)D.max_match;
    int base = 0;
    for (int m0 = 0; m0 < D.n_map; m0 += TD_T) {
        const int m = m0 + tid;
        bool is = false; double s = 0.0;
        if (m < D.n_map) { const int d = row[m]; if (d != TD_SKIP) { s = score_of(m, d); is = !(s < Scoreth); } }
        const unsigned long long bal = __ballot(is);
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int at = base + __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
#pragma unroll
        for (int w = 0; w < TD_NW; w++) { at += w < wave ? s_cnt[w] : 0; tot += s_cnt[w]; }
        if (is) {
            atomicAdd(&D.hit[m], 1);
            if (at < D.max_match) { t_idx[at] = m; t_sc[at] = s; }
        }
        base += tot;
        __syncthreads();
    }
    const int cnt = base;
    if (tid == 0) D.match_cnt[q] = cnt;
    if (cnt > D.max_match) return;                                     // the list does not fit: the count and the votes are complete, the list stays unwritten
    __threadfence_block();
    __syncthreads();
    // pass 3: each match to its rank
    const volatile double *v_sc = t_sc; const volatile int32_t *v_idx = t_idx;
    for (int i = tid; i < cnt; i += TD_T) {
        const double si = v_sc[i];
        int rank = 0;
        for (int j = 0; j < cnt; j++) { const double sj = v_sc[j]; rank += (sj > si || (sj == si && j < i)) ? 1 : 0; }
        const int m = v_idx[i];
        TdRec r; r.idx = m; r.dist = row[m]; r.score = si;
        D.rank_rec[(size_t)q*(size_t)D.max_match + (size_t)rank] = r;
    }
}

__global__ __launch_bounds__(TD_T) void k_td_vote(TdDev D) {
    __shared__ unsigned long long s_red[TD_NW];
    const int tid = threadIdx.x;
    // the lists that fit, one behind the other
    if (tid == 0) {
        int o = 0;
        for (int q = 0; q < D.n_query; q++) { D.rec_off[q] = o; const int c = D.match_cnt[q]; o += c <= D.max_match ? c : 0; }
        D.rec_off[D.n_query] = o;
    }
    __threadfence_block();
    __syncthreads();
    {   const volatile int32_t *v_off = D.rec_off;
        for (int q = 0; q < D.n_query; q++) {
            const int a = v_off[q], n = v_off[q + 1] - a;
            for (int i = tid; i < n; i += TD_T) D.out_rec[(size_t)a + (size_t)i] = D.rank_rec[(size_t)q*(size_t)D.max_match + (size_t)i];
        } }
    // the sums live in L2 for the whole kernel: zeroed, added to and read back with device-scope atomics only, never through this CU's L1
    for (int k = tid; k < D.n_kf; k += TD_T) {
        __hip_atomic_store(&D.kf_score[k], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(&D.kf_nobj[k], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __threadfence();
    __syncthreads();
    for (int m = tid; m < D.n_map; m += TD_T) {
        const int h = D.hit[m];
        if (h <= 0) continue;
        for (int e = D.obs_off[m]; e < D.obs_off[m + 1]; e++) { const int k = D.obs_kf[e]; atomicAdd(&D.kf_score[k], h); atomicAdd(&D.kf_nobj[k], 1); }
    }
    __threadfence();
    __syncthreads();
    // the walk of loopClosing.cc:277-300 as filter-then-top-N: a key orders by score, then by smaller index
    const int nsel = min(D.top_n, D.n_kf);
    unsigned long long last = ~0ull; int n = 0;
    for (int r = 0; r < nsel; r++) {
        unsigned long long best = 0ull;
        for (int k = tid; k < D.n_kf; k += TD_T) {
            const int s = __hip_atomic_load(&D.kf_score[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), o = __hip_atomic_load(&D.kf_nobj[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s > D.min_matched_words && o > D.min_matched_words) {
                const unsigned long long key = ((unsigned long long)(uint32_t)s << 32) | (unsigned long long)(0xffffffffu - (uint32_t)k);
                if (key < last && key > best) best = key;
            }
        }
        best = td_block_max(best, s_red);
        if (best == 0ull) break;                                       // (a valid keyframe's score is at least 1: its key is not 0)
        if (tid == 0) D.cand[n] = (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
        n++; last = best;
    }
    if (tid == 0) *D.n_cand = n;
}

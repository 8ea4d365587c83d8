// TEST DRIVER: loopClosing::DetectLoop from C++ -- adapter/tsloop_detect.hpp over the mock types of mock_loop_detect.hpp, beside a plain restatement of the reference's
// loop (std::string texts, the DP, std::stable_sort) on a copy of the same world.  Usage: loop_detect_from_cxx <in.bin> <out.bin>
//   in : int32 n_world; per world: int32 imapkfs, cur_id, n_vkfs, vkfs_id[n_vkfs], n_connect, connect_id[n_connect], cov[3][imapkfs] (the co-visibility counts with
//        the current keyframe), n_obj, per object (mnId, state, len, bytes[len], n_obs, kf_id[n_obs]), n_view, view_obj[n_view] (object positions the current keyframe
//        observes), MinMatchedWords, DoubleCheck_Visible, double ScoreThresh_min
//   out: per world: int32 ok, calls; if ok the call's flat arrays, each as int32 count + data: q_off, q_str, q_self, m_off, m_str, m_skip, obs_off, obs_kf, q_obs,
//        match_cnt, per query match_idx / match_dist / match_score [match_cnt], kf_score, kf_nobj, cand; then the returned keyframes' mnId, then per observation
//        int32 n and n x (int32 mapObj->mnId, double dist, double score)
// The driver itself fails unless detect_loop's vAllMatchTextRes and candidates equal the restatement's; tests/test_gpu_text_loop.py holds the arrays equal to Python's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "loop_detect_plain.hpp"
#include "tsloop_detect.hpp"

using namespace mockdetect;

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { const int32_t c = (int32_t)n; fwrite(&c, 4, 1, f); if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "loop_detect_from_cxx: %s\n", msg); return 1; } while (0)


static bool read_world(FILE *f, World &W) {
    int32_t nk = 0, cur = 0, nv = 0, nc = 0, no = 0, nview = 0;
    if (!rd(f, &nk, 1) || !rd(f, &cur, 1) || !rd(f, &nv, 1) || nk <= 0 || cur < 0 || cur >= nk) return false;
    W.kfs.assign((size_t)nk, keyframe()); for (int k = 0; k < nk; k++) W.kfs[(size_t)k].mnId = (long unsigned int)k;
    W.cur = &W.kfs[(size_t)cur]; W.M.resize_kfs(nk);
    std::vector<int32_t> ids((size_t)nv); if (!rd(f, ids.data(), ids.size())) return false;
    for (int i = 0; i < nv; i++) W.vKFs.push_back(&W.kfs[(size_t)ids[(size_t)i]]);
    if (!rd(f, &nc, 1)) return false;
    ids.assign((size_t)nc, 0); if (!rd(f, ids.data(), ids.size())) return false;
    for (int i = 0; i < nc; i++) W.vConnects[&W.kfs[(size_t)ids[(size_t)i]]] = 1;
    for (int w = 0; w < 3; w++) { std::vector<int32_t> col((size_t)nk); if (!rd(f, col.data(), col.size())) return false;
        for (int k = 0; k < nk; k++) W.M.M[w][(size_t)k*(size_t)nk + (size_t)cur] = (double)col[(size_t)k]; }
    if (!rd(f, &no, 1)) return false;
    W.objs.assign((size_t)no, mapText());
    for (int o = 0; o < no; o++) {
        int32_t h[3], n = 0; if (!rd(f, h, 3)) return false;
        mapText &T = W.objs[(size_t)o]; T.mnId = (long unsigned int)h[0]; T.STATE = (TextStatus)h[1];
        T.TextMean.mean.assign((size_t)h[2], '\0'); if (!rd(f, &T.TextMean.mean[0], (size_t)h[2])) return false;
        if (!rd(f, &n, 1)) return false;
        ids.assign((size_t)n, 0); if (!rd(f, ids.data(), ids.size())) return false;
        for (int i = 0; i < n; i++) T.vObvkeyframe[&W.kfs[(size_t)ids[(size_t)i]]] = std::vector<int>(1, i);
        W.M.vMapTextObjs.push_back(&T);
    }
    if (!rd(f, &nview, 1)) return false;
    ids.assign((size_t)nview, 0); if (!rd(f, ids.data(), ids.size())) return false;
    W.obs.assign((size_t)nview, TextObservation());
    for (int i = 0; i < nview; i++) { W.obs[(size_t)i].obj = &W.objs[(size_t)ids[(size_t)i]]; W.obs[(size_t)i].idx.assign(1, i); W.obs[(size_t)i].cos = 1.0; W.cur->vObvText.push_back(&W.obs[(size_t)i]); }
    int32_t t[2]; if (!rd(f, t, 2) || !rd(f, &W.ScoreThresh_min, 1)) return false;
    W.MinMatchedWords = t[0]; W.DoubleCheck = t[1];
    return true;
}

int main(int argc, char **argv) {
    if (argc != 3) FAIL("usage: loop_detect_from_cxx in.bin out.bin");
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    FILE *g = fopen(argv[2], "wb"); if (!g) FAIL("cannot open output");
    int32_t nw = 0; if (!rd(f, &nw, 1)) FAIL("short input");
    void *ctx = 0;
    if (tsloop_create(0, &ctx) != TSLOOP_OK) FAIL("tsloop_create");
    for (int w = 0; w < nw; w++) {
        World W; if (!read_world(f, W)) FAIL("short input");
        AllRes got(3), want;                                          // (detect_loop resizes what it is given)
        tsloop_adapter::PackedDetect P; bool ok = true;
        const std::vector<keyframe *> cand = tsloop_adapter::detect_loop<Traits>(ctx, W.cur, W.vKFs, &W.M, W.MinMatchedWords, W.vConnects, W.ScoreThresh_min, W.DoubleCheck != 0, got, ok, &P);
        const int32_t head[2] = { ok ? 1 : 0, P.calls }; fwrite(head, 4, 2, g);
        if (!ok) { if (got.size() != 3 || !cand.empty()) FAIL("fallback: outputs touched"); continue; }
        const std::vector<keyframe *> cand_want = plain_detect(W, want);
        if (cand != cand_want) FAIL("candidates differ from the restatement");
        if (got.size() != want.size()) FAIL("vAllMatchTextRes: size");
        for (size_t i = 0; i < got.size(); i++) {
            if (got[i].size() != want[i].size()) FAIL("vAllMatchTextRes: a list's size");
            for (size_t j = 0; j < got[i].size(); j++)
                if (got[i][j].mapObj != want[i][j].mapObj || got[i][j].dist != want[i][j].dist || got[i][j].score != want[i][j].score) FAIL("vAllMatchTextRes: an entry");
        }
        const size_t nq = (size_t)P.p.n_query, nm = (size_t)P.p.n_map, mm = (size_t)P.p.max_match;
        wr(g, P.q_off.data(), nq + 1); wr(g, P.q_str.data(), P.q_str.size()); wr(g, P.q_self.data(), nq); wr(g, P.m_off.data(), nm + 1); wr(g, P.m_str.data(), P.m_str.size());
        wr(g, P.m_skip.data(), nm); wr(g, P.obs_off.data(), nm + 1); wr(g, P.obs_kf.data(), P.obs_kf.size()); wr(g, P.q_obs.data(), nq); wr(g, P.match_cnt.data(), nq);
        for (size_t q = 0; q < nq; q++) { const size_t n = (size_t)P.match_cnt[q]; wr(g, &P.match_idx[q*mm], n); wr(g, &P.match_dist[q*mm], n); wr(g, &P.match_score[q*mm], n); }
        wr(g, P.kf_score.data(), (size_t)P.p.n_kf); wr(g, P.kf_nobj.data(), (size_t)P.p.n_kf); wr(g, P.cand.data(), (size_t)P.n_cand);
        std::vector<int32_t> ids; for (size_t i = 0; i < cand.size(); i++) ids.push_back((int32_t)cand[i]->mnId);
        wr(g, ids.data(), ids.size());
        for (size_t i = 0; i < got.size(); i++) {
            const int32_t n = (int32_t)got[i].size(); fwrite(&n, 4, 1, g);
            for (size_t j = 0; j < got[i].size(); j++) { const int32_t id = (int32_t)got[i][j].mapObj->mnId; fwrite(&id, 4, 1, g); fwrite(&got[i][j].dist, 8, 1, g); fwrite(&got[i][j].score, 8, 1, g); }
        }
    }
    fclose(f); fclose(g);
    tsloop_destroy(ctx);
    printf("detect loop from C++: ok\n");
    return 0;
}

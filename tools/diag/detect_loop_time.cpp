// DIAGNOSTIC (not a test): tsloop_detect_loop timed beside a single-thread restatement of the reference's loop on the same worlds and the same machine.
// Usage: detect_loop_time <calls>; compiled and run by tools/diag/gpu_detect_loop.py.  The worlds, the mock types and the restatement are the test suite's
// (tests/cxx/loop_detect_plain.hpp); the two sides' match counts and candidates are compared on every shape, and every shape is reported.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "loop_detect_plain.hpp"
#include "tsloop_detect.hpp"

using namespace mockdetect;
#define FAIL(msg) do { fprintf(stderr, "detect_loop_time: %s\n", msg); return 1; } while (0)

static uint32_t g_lcg = 12345u;
static uint32_t lcg(uint32_t n) { g_lcg = g_lcg*1664525u + 1013904223u; return (g_lcg >> 8) % n; }
static std::string word() { std::string s((size_t)(3 + lcg(14)), 'a'); for (size_t i = 0; i < s.size(); i++) s[i] = (char)('a' + lcg(26)); return s; }     // 3 - 16 bytes
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int time_mode(int calls) {
    void *ctx = 0;
    if (tsloop_create(0, &ctx) != TSLOOP_OK) FAIL("tsloop_create");
    printf("# per call, copies included, max_match = 64 (the default; no shape overflows it), the adapter's gather not included; device = the median of %d calls after a\n"
           "# warm-up with their 10th and 90th percentiles; host = a single-thread restatement of the reference's loop (std::string texts, the DP, a stable sort per query;\n"
           "# this binary, g++ -O2) on the same machine, the median of at least 5 runs and 0.3 s, with the fastest and the slowest run\n"
           "# queries x map texts (3 - 16 bytes, 300 keyframes)   device_ms (p10 - p90)         host_ms (min - max)             host/device\n", calls);
    const int NQ[3] = { 8, 16, 32 }, NM[3] = { 500, 5000, 20000 };
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
        World W; const int nk = 301, nq = NQ[a], nm = NM[b];
        W.kfs.assign((size_t)nk, keyframe()); for (int k = 0; k < nk; k++) W.kfs[(size_t)k].mnId = (long unsigned int)k;
        W.cur = &W.kfs[(size_t)nk - 1]; W.M.resize_kfs(nk);
        for (int k = 0; k + 1 < nk; k++) W.vKFs.push_back(&W.kfs[(size_t)k]);
        for (int k = nk - 21; k + 1 < nk; k++) W.M.M[0][(size_t)k*(size_t)nk + (size_t)nk - 1] = 5.0;                   // the last 20 keyframes are co-visible
        W.objs.assign((size_t)nm, mapText());
        for (int o = 0; o < nm; o++) { mapText &T = W.objs[(size_t)o]; T.mnId = (long unsigned int)o; T.STATE = lcg(20) == 0 ? TEXTBAD : TEXTGOOD;
            T.TextMean.mean = o >= 4 && lcg(4) == 0 ? W.objs[(size_t)lcg((uint32_t)o)].TextMean.mean : word();                // a quarter repeats an earlier word
            const int n = 1 + (int)lcg(5), k0 = (int)lcg((uint32_t)(nk - 6)); for (int i = 0; i < n; i++) T.vObvkeyframe[&W.kfs[(size_t)(k0 + i)]] = std::vector<int>(1, i);
            W.M.vMapTextObjs.push_back(&T); }
        W.obs.assign((size_t)nq, TextObservation());
        for (int i = 0; i < nq; i++) { W.obs[(size_t)i].obj = &W.objs[(size_t)lcg((uint32_t)nm)]; W.obs[(size_t)i].idx.assign(1, i); W.obs[(size_t)i].cos = 1.0; W.cur->vObvText.push_back(&W.obs[(size_t)i]); }
        W.MinMatchedWords = 1; W.DoubleCheck = 0; W.ScoreThresh_min = 0.51;
        tsloop_adapter::PackedDetect P; std::vector<mapText *> vObjs;
        if (!tsloop_adapter::pack_detect_loop<Traits>(W.cur, W.vKFs, &W.M, W.MinMatchedWords, W.vConnects, W.ScoreThresh_min, false, P, vObjs)) FAIL("pack");
        std::vector<double> td, th;
        for (int it = 0; it < calls + 5; it++) { const double t0 = now_ms(); if (tsloop_detect_loop(ctx, &P.p) != TSLOOP_OK) FAIL(tsloop_last_error(ctx)); if (it >= 5) td.push_back(now_ms() - t0); }
        AllRes want; std::vector<keyframe *> cand; double spent = 0.0;
        while (th.size() < 5 || spent < 300.0) { const double t0 = now_ms(); cand = plain_detect(W, want); th.push_back(now_ms() - t0); spent += th.back(); }
        long n_match = 0;
        for (int q = 0; q < nq; q++) { if ((size_t)P.match_cnt[(size_t)q] != want[(size_t)P.q_obs[(size_t)q]].size()) FAIL("time: match counts differ"); n_match += P.match_cnt[(size_t)q]; }
        if ((size_t)P.n_cand != cand.size()) FAIL("time: candidates differ");
        for (size_t j = 0; j < cand.size(); j++) if (W.vKFs[(size_t)P.cand[j]] != cand[j]) FAIL("time: candidates differ");
        std::sort(td.begin(), td.end()); std::sort(th.begin(), th.end());
        const double d = td[td.size()/2], h = th[th.size()/2];
        printf("%3d x %-6d                                          %9.3f (%.3f - %.3f)     %9.3f (%.3f - %.3f, %d runs) %9.1f     (matches %ld, candidates %d)\n", nq, nm, d,
               td[td.size()/10], td[td.size()*9/10], h, th.front(), th.back(), (int)th.size(), h/d, n_match, (int)P.n_cand);
    }
    tsloop_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) FAIL("usage: detect_loop_time calls");
    return time_mode(std::max(1, atoi(argv[1])));
}

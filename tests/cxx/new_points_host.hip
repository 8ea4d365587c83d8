// TEST / DIAGNOSTICS PROGRAM: the __host__ __device__ decisions and arithmetic of textslam_amd/csrc/tsclaim.h on the CPU, one thread, no device call.
// Usage: new_points_host <in.bin> <out.bin> [reps]
//   in : int32 nq, n2, th_low, use_ratio, th_reproj; double ratio, Trw[12], Tcw[12], K[4]; float q_px[nq][2], xy2[n2][2]; uint8 elig[n2]; int32 cnt[nq];
//        int32 idx[sum cnt], dist[sum cnt]: every query's candidates in GetFeaturesInArea's order with their Hamming distances (what k_claim_walk leaves in scratch,
//        before the eligibility test)
//   out: int32 match12[nq], match_dist[nq]; float p3d[nq][3]; uint8 good[nq]; int32 n_match, n_good
// The chain runs the device's way -- a query's candidates on 64 lanes, 64 at a time, cl_offer / cl_merge per lane, the butterfly of cl_merge, cl_accept, the 16-bit
// vMatchDist with 0 for "not eligible" -- and beside it a plain transcription of the reference's loop on ints; the two must agree at every step or the program fails.
//   reps > 0: additionally times `reps` runs of the reference's loop (the chain over the given lists, then the point and the check of every match) and prints
//   "loop_ms <mean>".  The window walk and the Hamming distances are NOT in that time: the lists are given.
// tests/test_new_points_ref.py builds it with the host sanitizers and compares it with the numpy restatement; tools/diag/gpu_new_points.py builds it with -O2 as the
// host baseline.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <chrono>
#include <vector>
#include "../../include/tsorb.h"
#define TSCLAIM_HOST_ONLY
#include "../../textslam_amd/csrc/tsclaim.h"

template <class V> static bool rd(FILE *f, V *p, size_t n) { return n == 0 || fread(p, sizeof(V), n, f) == n; }
template <class V> static void wr(FILE *f, const V *p, size_t n) { if (n) fwrite(p, sizeof(V), n, f); }
#define FAIL(msg) do { fprintf(stderr, "new_points_host: %s\n", msg); return 1; } while (0)
typedef std::chrono::steady_clock Clock;

// one step the device's way: the first minimum in candidate order and the runner-up over what vMatchDist does not hide
static void step_lanes(const int32_t *idx, const int32_t *dist, int cnt, const std::vector<uint16_t> &md, int &k1, int &s2) {
    int lk[64], ls[64];
    for (int l = 0; l < 64; l++) { lk[l] = CL_NONE; ls[l] = CL_NO2; }
    for (int c0 = 0; c0 < cnt; c0 += 64)
        for (int l = 0; l < 64 && c0 + l < cnt; l++) cl_merge(lk[l], ls[l], cl_offer((int)md[(size_t)idx[c0 + l]], dist[c0 + l], c0 + l), CL_NO2);
    for (int o = 32; o > 0; o >>= 1) { int nk[64], ns[64];
        for (int l = 0; l < 64; l++) { nk[l] = lk[l]; ns[l] = ls[l]; cl_merge(nk[l], ns[l], lk[l ^ o], ls[l ^ o]); }
        for (int l = 0; l < 64; l++) { lk[l] = nk[l]; ls[l] = ns[l]; } }
    k1 = lk[0]; s2 = ls[0];
    for (int l = 1; l < 64; l++) if (lk[l] != k1 || ls[l] != s2) { k1 = -1; return; }      // (every lane ends with the same pair)
}

int main(int argc, char **argv) {
    if (argc < 3) FAIL("usage: new_points_host in.bin out.bin [reps]");
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *f = fopen(argv[1], "rb"); if (!f) FAIL("cannot open input");
    int32_t hd[5]; double ratio, Trw[12], Tcw[12], K[4];
    if (!rd(f, hd, 5) || !rd(f, &ratio, 1) || !rd(f, Trw, 12) || !rd(f, Tcw, 12) || !rd(f, K, 4)) FAIL("bad header");
    const int nq = hd[0], n2 = hd[1], th_low = hd[2], use_ratio = hd[3], th_reproj = hd[4];
    if (nq < 0 || n2 < 0 || n2 > TSORB_BRUTE_MAX_FEAT || th_low < 0 || th_low > 256) FAIL("bad sizes");
    std::vector<float> q_px(2*(size_t)nq), xy2(2*(size_t)n2); std::vector<uint8_t> elig((size_t)n2); std::vector<int32_t> cnt((size_t)nq), off((size_t)nq + 1, 0);
    if (!rd(f, q_px.data(), q_px.size()) || !rd(f, xy2.data(), xy2.size()) || !rd(f, elig.data(), elig.size()) || !rd(f, cnt.data(), cnt.size())) FAIL("short input");
    for (int q = 0; q < nq; q++) { if (cnt[(size_t)q] < 0 || cnt[(size_t)q] > n2) FAIL("bad count"); off[(size_t)q + 1] = off[(size_t)q] + cnt[(size_t)q]; }
    const size_t tot = (size_t)off[(size_t)nq];
    std::vector<int32_t> idx(tot), dist(tot);
    if (!rd(f, idx.data(), tot) || !rd(f, dist.data(), tot)) FAIL("short input");
    fclose(f);
    for (size_t e = 0; e < tot; e++) if (idx[e] < 0 || idx[e] >= n2 || dist[e] < 0 || dist[e] > 256) FAIL("bad candidate");
    std::vector<int32_t> m12((size_t)nq), mdist((size_t)nq), own((size_t)n2); std::vector<uint16_t> md((size_t)n2); std::vector<float> p3d(3*(size_t)nq); std::vector<uint8_t> good((size_t)nq);
    std::vector<int> vMatchDist((size_t)n2), vMatchIdx21((size_t)n2), vMatchIdx12((size_t)nq);
    int32_t n_match = 0, n_good = 0; double loop_ms = 0.0;
    for (int rep = 0; rep < (reps > 0 ? reps + 1 : 1); rep++) {             // run 0 is the one that is checked and written (and the warm-up of the timed ones)
        const Clock::time_point t0 = Clock::now();
        // the reference's loop (tracking.cc:1354-1407 / :1056-1106) on the given lists
        int nMatches = 0;
        for (int i = 0; i < n2; i++) { vMatchDist[(size_t)i] = 2147483647; vMatchIdx21[(size_t)i] = -1; }
        for (int q = 0; q < nq; q++) vMatchIdx12[(size_t)q] = -1;
        if (rep == 0) for (int i = 0; i < n2; i++) { md[(size_t)i] = elig[(size_t)i] ? CL_FREE : 0; own[(size_t)i] = -1; }
        for (int i1 = 0; i1 < nq; i1++) {
            const int32_t *ci = idx.data() + off[(size_t)i1], *cd = dist.data() + off[(size_t)i1]; const int n = cnt[(size_t)i1];
            int bestDist = 2147483647, bestDist2 = 2147483647, bestIdx2 = -1;
            for (int j = 0; j < n; j++) { const int i2 = ci[j], d = cd[j];
                if (!elig[(size_t)i2]) continue;
                if (vMatchDist[(size_t)i2] <= d) continue;
                if (d < bestDist) { bestDist2 = bestDist; bestDist = d; bestIdx2 = i2; } else if (d < bestDist2) bestDist2 = d; }
            const bool take = bestDist <= th_low && (!use_ratio || (double)bestDist < (double)bestDist2*ratio);
            if (rep == 0) {                                                // the device's way to the same step
                int k1, s2, best; step_lanes(ci, cd, n, md, k1, s2);
                if (k1 < 0) FAIL("the lanes end a butterfly with different pairs");
                const bool acc = cl_accept(k1, s2, th_low, use_ratio, ratio, best);
                const int i2 = k1 == CL_NONE ? -1 : ci[k1 & 0xffff];
                if (acc != take || (take && (i2 != bestIdx2 || best != bestDist))) FAIL("a step of the lanes differs from the reference's loop");
                if ((k1 == CL_NONE) != (bestIdx2 < 0) || (k1 != CL_NONE && (s2 == CL_NO2 ? 2147483647 : s2) != bestDist2)) FAIL("the lanes' runner-up differs from the reference's loop");
                if (acc) { md[(size_t)i2] = (uint16_t)best; own[(size_t)i2] = i1; }
            }
            if (take) {
                if (vMatchIdx21[(size_t)bestIdx2] >= 0) { vMatchIdx12[(size_t)vMatchIdx21[(size_t)bestIdx2]] = -1; nMatches--; }
                vMatchIdx12[(size_t)i1] = bestIdx2; vMatchIdx21[(size_t)bestIdx2] = i1; vMatchDist[(size_t)bestIdx2] = bestDist; nMatches++; }
        }
        int ng = 0;
        for (int q = 0; q < nq; q++) { float X[3] = { 0.f, 0.f, 0.f }; bool g = false; const int m = vMatchIdx12[(size_t)q];
            if (m >= 0) g = cl_new_point(Trw, Tcw, K, &q_px[2*(size_t)q], &xy2[2*(size_t)m], th_reproj, X);
            p3d[3*(size_t)q] = X[0]; p3d[3*(size_t)q + 1] = X[1]; p3d[3*(size_t)q + 2] = X[2]; good[(size_t)q] = g ? 1 : 0; ng += g ? 1 : 0; }
        const Clock::time_point t1 = Clock::now();
        if (rep > 0) { loop_ms += std::chrono::duration<double, std::milli>(t1 - t0).count(); continue; }
        // vMatchIdx12 the device's way: from vMatchIdx21 at the end
        for (int q = 0; q < nq; q++) { m12[(size_t)q] = -1; mdist[(size_t)q] = -1; }
        for (int i = 0; i < n2; i++) if (own[(size_t)i] >= 0) { m12[(size_t)own[(size_t)i]] = i; mdist[(size_t)own[(size_t)i]] = (int32_t)md[(size_t)i]; n_match++; }
        for (int q = 0; q < nq; q++) if (m12[(size_t)q] != vMatchIdx12[(size_t)q]) FAIL("vMatchIdx12 from vMatchIdx21 differs from the reference's loop");
        if (n_match != nMatches) FAIL("nMatches differs");
        n_good = ng;
        FILE *o = fopen(argv[2], "wb"); if (!o) FAIL("cannot open output");
        wr(o, m12.data(), m12.size()); wr(o, mdist.data(), mdist.size()); wr(o, p3d.data(), p3d.size()); wr(o, good.data(), good.size()); wr(o, &n_match, 1); wr(o, &n_good, 1);
        fclose(o);
    }
    if (reps > 0) printf("loop_ms %.6f (queries %d)\n", loop_ms/reps, nq);
    printf("new points host: ok\n");
    return 0;
}

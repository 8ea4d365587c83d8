// tswindow.h -- window searches in many feature sets at once (loopClosing::SearchAndFuse_Scene, src/loopClosing.cc:1168-1288, once per keyframe of the loop window; and
// loopClosing::MatchMore, :1398-1489), included by tsorb.hip after the single-grid kernels whose arithmetic it shares (mg_cell_of, match_walk).
//   k_ws_grid   <- frame::AssignFeaturesToGrid (frame.cc:372-407) for EVERY set in one launch, a workgroup per set: the cell counts, their scan and the running cursors of
//                  the stable placement stay in LDS
//   k_ws_match  <- keyframe::GetFeaturesInArea (keyframe.cc:217-256) + DescriptorDistance + the best scan for every query in one launch, a wave per query: the query's
//                  set and descriptor row are looked up, the walk is match_walk
// Every loop below is bounded by a set's feature count, the cell count or a constant; a workgroup of k_ws_grid writes only its own set's rows of off and list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define WS_T 256                      /* threads per workgroup of both kernels; k_ws_grid places WS_T features at a time */
#define WS_PER (MG_CELLS/WS_T)        /* cells a thread of k_ws_grid scans: 12 */
static_assert(WS_PER*WS_T == MG_CELLS, "the scan gives every thread the same number of cells");

struct WindowSets {
    int n_set, nq, max_cand;
    const int *foff;                  // [n_set + 1] first feature row of a set
    const double *grid;               // [n_set][4] min_x, min_y, 1/cell width, 1/cell height (frame.cc:124-125)
    const float *kp; const uint8_t *desc, *qdesc;         // [foff[n_set]][6], [foff[n_set]][32], [n_qdesc][32]: device memory
    int *off, *list;                  // [n_set][MG_CELLS + 1], [foff[n_set]] (feature indices relative to the set)
    // the pinned block: queries in, results out
    const float *qxy, *qr; const int *qlev, *qset, *qdi;  // qlev: -1, -1 = no level check;  qdi: the query's row of qdesc
    int *cand_idx, *cand_dist, *cand_cnt, *best_idx, *best_dist, *best_dist2;
};

// A cell lists its features in index order (the reference's push_back).  Features are taken WS_T at a time in index order: a feature's place is its cell's cursor (the
// features of the cell in earlier chunks) plus the features of the cell before it in the chunk, counted through LDS; the cursors then advance by the chunk's counts
// (integer adds: their order does not matter).
__global__ __launch_bounds__(WS_T) void k_ws_grid(WindowSets W) {
    __shared__ int s_cnt[MG_CELLS], s_part[WS_T]; __shared__ __attribute__((aligned(16))) int s_cell[WS_T];
    const int s = blockIdx.x, t = threadIdx.x, f0 = W.foff[s], n = W.foff[s + 1] - f0;
    const double min_x = W.grid[4*s], min_y = W.grid[4*s + 1], iw = W.grid[4*s + 2], ih = W.grid[4*s + 3];
    const float *kp = W.kp + 6*(size_t)f0;
    int *off = W.off + (size_t)s*(MG_CELLS + 1), *list = W.list + f0;
    for (int c = t; c < MG_CELLS; c += WS_T) s_cnt[c] = 0;
    __syncthreads();
    for (int i = t; i < n; i += WS_T) { const int c = mg_cell_of(kp[6*(size_t)i], kp[6*(size_t)i + 1], min_x, min_y, iw, ih); if (c >= 0) atomicAdd(&s_cnt[c], 1); }
    __syncthreads();
    // inclusive scan of the counts: WS_PER consecutive cells a thread, the threads' sums through LDS
    int v[WS_PER], sum = 0;
#pragma unroll
    for (int k = 0; k < WS_PER; k++) { v[k] = s_cnt[WS_PER*t + k]; sum += v[k]; }
    s_part[t] = sum; __syncthreads();
    for (int d = 1; d < WS_T; d <<= 1) { const int a = t >= d ? s_part[t - d] : 0; __syncthreads(); s_part[t] += a; __syncthreads(); }
    int run = s_part[t] - sum;
    if (t == 0) off[0] = 0;
#pragma unroll
    for (int k = 0; k < WS_PER; k++) { s_cnt[WS_PER*t + k] = run; run += v[k]; off[1 + WS_PER*t + k] = run; }      // s_cnt: from here the cell's cursor
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += WS_T) {
        const int i = i0 + t;
        const int c = i < n ? mg_cell_of(kp[6*(size_t)i], kp[6*(size_t)i + 1], min_x, min_y, iw, ih) : -1;
        s_cell[t] = c;
        __syncthreads();
        if (c >= 0) {
            int before = 0;
            for (int j = 0; j < t; j += 8) {                                   // eight entries a step, two 16-byte LDS reads; the entries from t on do not count
                const int4 a = *(const int4 *)&s_cell[j], b = *(const int4 *)&s_cell[j + 4];
                before += ((a.x == c) & (j < t)) + ((a.y == c) & (j + 1 < t)) + ((a.z == c) & (j + 2 < t)) + ((a.w == c) & (j + 3 < t))
                        + ((b.x == c) & (j + 4 < t)) + ((b.y == c) & (j + 5 < t)) + ((b.z == c) & (j + 6 < t)) + ((b.w == c) & (j + 7 < t));
            }
            list[s_cnt[c] + before] = i;
        }
        __syncthreads();                                                   // (every cursor has been read)
        if (c >= 0) atomicAdd(&s_cnt[c], 1);
        __syncthreads();
    }
}

__global__ __launch_bounds__(WS_T) void k_ws_match(WindowSets W) {
    __shared__ int s_inc[WS_T/64][64], s_o0[WS_T/64][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x*(WS_T/64) + wv;
    if (q >= W.nq) return;                                   // (a whole wave)
    const int s = W.qset[q], f0 = W.foff[s];
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; k++) qd[k] = ((const uint32_t *)W.qdesc)[8*(size_t)W.qdi[q] + k];
    MatchGrid G; G.kp = W.kp + 6*(size_t)f0; G.desc = W.desc + 32*(size_t)f0; G.off = W.off + (size_t)s*(MG_CELLS + 1); G.list = W.list + f0;
    G.min_x = W.grid[4*s]; G.min_y = W.grid[4*s + 1]; G.iw = W.grid[4*s + 2]; G.ih = W.grid[4*s + 3];
    match_walk(G, lane, s_inc[wv], s_o0[wv], W.qxy[2*q], W.qxy[2*q + 1], W.qr[q], W.qlev[2*q], W.qlev[2*q + 1], qd, W.max_cand,
               W.cand_idx + (size_t)q*W.max_cand, W.cand_dist + (size_t)q*W.max_cand, W.cand_cnt + q, W.best_idx + q, W.best_dist + q, W.best_dist2 + q);
}

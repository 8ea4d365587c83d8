// tswindow.h -- the reference's 64 x 48 feature grid and the window search in it, stated once: how a grid is built (frame::AssignFeaturesToGrid / PosInGrid,
// frame.cc:372-407), what describes a built grid (MatchGrid) and how one query walks it (frame::GetFeaturesInArea, frame.cc:415-468, tracking::DescriptorDistance,
// tracking.cc:2762-2778).  Every window search of libtsorb goes through here: the context's single grid (tracking::SearchFrom3D*: tsorb_match_set_frame /
// tsorb_match_set_features / tsorb_fuse_frame build it, tsorb_match_search and tsclaim.h's kernels search it) and the per-set grids of loop fusion
// (loopClosing::SearchAndFuse_Scene, src/loopClosing.cc:1168-1288, once per keyframe of the loop window; loopClosing::MatchMore, :1398-1489).  Included by tsorb.hip
// before tsclaim.h, which walks the context's grid.
//   grid_build     one workgroup builds one grid: the cell counts, their scan and the running cursors of the stable placement stay in LDS
//   k_grid         grid_build for the context's grid, one workgroup
//   k_ws_grid      grid_build for EVERY set of tsorb_match_search_sets in one launch, a workgroup per set
//   match_walk     the walk of one query by one wave (GetFeaturesInArea + DescriptorDistance + the best scan)
//   k_match        match_walk per query in the context's grid
//   k_ws_match     match_walk per query of tsorb_match_search_sets: the query's set and descriptor row are looked up
// Every loop below is bounded by a grid's feature count, the cell count or a constant; a workgroup of grid_build writes only its own grid's off and list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MG_COLS 64
#define MG_ROWS 48
#define MG_CELLS (MG_COLS*MG_ROWS)
#define WS_T 256                      /* threads per workgroup of the kernels here; grid_build places WS_T features at a time */
#define WS_PER (MG_CELLS/WS_T)        /* cells a thread of grid_build scans: 12 */
static_assert(WS_PER*WS_T == MG_CELLS, "the scan gives every thread the same number of cells");

// A built grid: the features of cell c are list[off[c]] .. list[off[c + 1] - 1], in index order (the reference's push_back).
struct MatchGrid {
    const float *kp; const uint8_t *desc;             // [n][6], [n][32]
    int *off, *list;                                  // [MG_CELLS + 1], [n]
    double min_x, min_y, iw, ih;                      // the grid's origin, 1/cell width, 1/cell height
};
// frame.cc:124-125: g = min_x, min_y, 1/cell width, 1/cell height of the grid over the image bounds
static inline void grid_scale(const double min_x, const double max_x, const double min_y, const double max_y, double g[4]) {
    g[0] = min_x; g[1] = min_y; g[2] = (double)MG_COLS/(max_x - min_x); g[3] = (double)MG_ROWS/(max_y - min_y);
}
// frame::PosInGrid (frame.cc:395-407) in the reference's doubles: the feature's cell (column-major, as the window walk counts them), -1 outside the grid
__device__ __forceinline__ int mg_cell_of(const float fx, const float fy, const double min_x, const double min_y, const double iw, const double ih) {
    const int px = (int)round(((double)fx - min_x)*iw), py = (int)round(((double)fy - min_y)*ih);
    return (px < 0 || px >= MG_COLS || py < 0 || py >= MG_ROWS) ? -1 : px*MG_ROWS + py;
}

// One workgroup of WS_T threads builds the grid of kp[n][6]: a stable counting sort.  Features are taken WS_T at a time in index order: a feature's place is its cell's
// cursor (the features of the cell in earlier chunks) plus the features of the cell before it in the chunk, counted through LDS; the cursors then advance by the chunk's
// counts (integer adds: their order does not matter).  n = 0 leaves off all zero.
__device__ __forceinline__ void grid_build(const float *kp, const int n, const double min_x, const double min_y, const double iw, const double ih, int *off, int *list) {
    __shared__ int s_cnt[MG_CELLS], s_part[WS_T]; __shared__ __attribute__((aligned(16))) int s_cell[WS_T];
    const int t = threadIdx.x;
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
__global__ __launch_bounds__(WS_T) void k_grid(MatchGrid G, int n) { grid_build(G.kp, n, G.min_x, G.min_y, G.iw, G.ih, G.off, G.list); }

struct WindowSets {
    int n_set, nq, max_cand;
    const int *foff;                  // [n_set + 1] first feature row of a set
    const double *grid;               // [n_set][4] grid_scale of a set's bounds
    const float *kp; const uint8_t *desc, *qdesc;         // [foff[n_set]][6], [foff[n_set]][32], [n_qdesc][32]: device memory
    int *off, *list;                  // [n_set][MG_CELLS + 1], [foff[n_set]] (feature indices relative to the set)
    // the pinned block: queries in, results out
    const float *qxy, *qr; const int *qlev, *qset, *qdi;  // qlev: -1, -1 = no level check;  qdi: the query's row of qdesc
    int *cand_idx, *cand_dist, *cand_cnt, *best_idx, *best_dist, *best_dist2;
};
// set s of W as a grid
__device__ __forceinline__ MatchGrid ws_grid_of(const WindowSets &W, const int s) {
    const int f0 = W.foff[s];
    MatchGrid G; G.kp = W.kp + 6*(size_t)f0; G.desc = W.desc + 32*(size_t)f0; G.off = W.off + (size_t)s*(MG_CELLS + 1); G.list = W.list + f0;
    G.min_x = W.grid[4*s]; G.min_y = W.grid[4*s + 1]; G.iw = W.grid[4*s + 2]; G.ih = W.grid[4*s + 3];
    return G;
}
__global__ __launch_bounds__(WS_T) void k_ws_grid(WindowSets W) {
    const int s = blockIdx.x;
    const MatchGrid G = ws_grid_of(W, s);
    grid_build(G.kp, W.foff[s + 1] - W.foff[s], G.min_x, G.min_y, G.iw, G.ih, G.off, G.list);
}

// One WAVE per query (until round 6: one thread per query walking its window's cells one after the other -- two dependent loads per cell, two more per feature, 81 cells for a
// 40-px radius: 289 us for 1000 queries, 0.37 ms per call of tracking::SearchFrom3D's search).  The window's cells on the lanes in the reference's order (column by column,
// frame.cc:415-468), their feature counts as a wave scan; then the window's features on the lanes, again in that order (a lane finds its feature's cell in the scan), the
// reference's filters and the Hamming distance per lane; the survivors keep their order through a ballot, best / second best as the two smallest of the multiset with the
// first minimum's index (what the reference's sequential scan ends with).
// The walk of one query by one wave, stated once: k_match (the context's single grid), k_ws_match (a grid per set) and tsclaim.h's kernels call it.  M is the searched
// grid by value; inc / o0s are the wave's 64-entry LDS scratch; cand_idx / cand_dist are the query's own rows (max_cand entries, unused slots included).
// keep(i, d): a further test of a feature that passed the window and the octave, asked with its index and distance (tsclaim.h: eligibility, the running vMatchDist);
// MwAll keeps every one.
struct MwAll { __device__ __forceinline__ bool operator()(int, int) const { return true; } };
template <class Keep = MwAll>
__device__ __forceinline__ void match_walk(const MatchGrid M, const int lane, int *inc, int *o0s, const float x, const float y, const float r, const int minLevel, const int maxLevel,
                                           const uint32_t (&qd)[8], const int max_cand, int *cand_idx, int *cand_dist, int *cand_cnt, int *best_idx, int *best_dist, int *best_dist2, const Keep keep = Keep()) {
    int nc = 0, bi = -1, bd = 2147483647, bd2 = 2147483647;
    const int c0x = max(0, (int)floor(((double)x - M.min_x - (double)r)*M.iw)), c1x = min(MG_COLS - 1, (int)ceil(((double)x - M.min_x + (double)r)*M.iw));
    const int c0y = max(0, (int)floor(((double)y - M.min_y - (double)r)*M.ih)), c1y = min(MG_ROWS - 1, (int)ceil(((double)y - M.min_y + (double)r)*M.ih));
    if (!(c0x >= MG_COLS || c1x < 0 || c0y >= MG_ROWS || c1y < 0)) {
        const bool check = (minLevel > 0) || (maxLevel >= 0);
        const int ny = c1y - c0y + 1, ncell = (c1x - c0x + 1)*ny;
        const unsigned long long lt = (1ull << lane) - 1ull;
        for (int e0 = 0; e0 < ncell; e0 += 64) {             // 64 cells of the window at a time
            const int e = e0 + lane; int o0 = 0, cnt = 0;
            if (e < ncell) { const int ix = c0x + e/ny, iy = c0y + e - (e/ny)*ny, c = ix*MG_ROWS + iy; o0 = M.off[c]; cnt = M.off[c+1] - o0; }
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
            const int tot = __shfl(incl, 63, 64);
            inc[lane] = incl; o0s[lane] = o0 - (incl - cnt);                                 // (list position of the cell's first feature minus the features before the cell)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int j0 = 0; j0 < tot; j0 += 64) {            // 64 features of those cells at a time, in order
                const int j = j0 + lane; bool pass = false; int i = 0, d = 0;
                if (j < tot) {
                    int lo = 0;                                // the first cell whose inclusive count exceeds j
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1) if (inc[lo + step - 1] <= j) lo += step;
                    i = M.list[o0s[lo] + j];
                    const float fx = M.kp[6*i], fy = M.kp[6*i+1]; const int oct = (int)M.kp[6*i+5];
                    const uint32_t *fd = (const uint32_t *)(M.desc + 32*(size_t)i);
                    uint32_t f8[8];
#pragma unroll
                    for (int w = 0; w < 8; w++) f8[w] = fd[w];
                    pass = true;
                    if (check) { if (oct < minLevel) pass = false; if (maxLevel >= 0 && oct > maxLevel) pass = false; }
                    const float dx = fx - x, dy = fy - y;
                    if (!(fabsf(dx) < r && fabsf(dy) < r)) pass = false;
#pragma unroll
                    for (int w = 0; w < 8; w++) d += __popc(qd[w] ^ f8[w]);
                    if (pass) pass = keep(i, d);
                }
                const unsigned long long pm = __ballot(pass);
                if (pm) {
                    const int rank = nc + __popcll(pm & lt);
                    if (pass && rank < max_cand) { cand_idx[rank] = i; cand_dist[rank] = d; }
                    nc += __popcll(pm);
                    // the chunk's two smallest distances and the first lane of the smallest
                    int m1 = pass ? d : 2147483647;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) m1 = min(m1, __shfl_xor(m1, o, 64));
                    const unsigned long long at1 = __ballot(pass && d == m1);
                    const int first = __ffsll((long long)at1) - 1;
                    int m2 = (pass && lane != first) ? d : 2147483647;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) m2 = min(m2, __shfl_xor(m2, o, 64));
                    const int i1 = __shfl(i, first, 64);
                    // merged behind what came before (a later equal minimum does not take the index: strict < in the reference)
                    if (m1 < bd) { bd2 = min(bd, m2); bd = m1; bi = i1; } else bd2 = min(bd2, m1);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");      // (the next 64 cells overwrite the scan)
        }
    }
    for (int k = nc + lane; k < max_cand; k += 64) { cand_idx[k] = -1; cand_dist[k] = -1; }     // unused slots
    if (lane == 0) { *cand_cnt = nc; *best_idx = bi; *best_dist = bd; *best_dist2 = bd2; }
}
__global__ __launch_bounds__(WS_T) void k_match(MatchGrid G, int nq, const float *qxy, const float *qr, const int *qlev, const uint8_t *qdesc, int max_cand,
                                                int *cand_idx, int *cand_dist, int *cand_cnt, int *best_idx, int *best_dist, int *best_dist2) {
    __shared__ int s_inc[WS_T/64][64], s_o0[WS_T/64][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x*(WS_T/64) + wv;
    if (q >= nq) return;                                     // (a whole wave)
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; k++) qd[k] = ((const uint32_t *)qdesc)[8*(size_t)q + k];
    match_walk(G, lane, s_inc[wv], s_o0[wv], qxy[2*q], qxy[2*q+1], qr[q], qlev ? qlev[2*q] : -1, qlev ? qlev[2*q+1] : -1, qd, max_cand,
               cand_idx + (size_t)q*max_cand, cand_dist + (size_t)q*max_cand, cand_cnt + q, best_idx + q, best_dist + q, best_dist2 + q);
}
__global__ __launch_bounds__(WS_T) void k_ws_match(WindowSets W) {
    __shared__ int s_inc[WS_T/64][64], s_o0[WS_T/64][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x*(WS_T/64) + wv;
    if (q >= W.nq) return;                                   // (a whole wave)
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; k++) qd[k] = ((const uint32_t *)W.qdesc)[8*(size_t)W.qdi[q] + k];
    match_walk(ws_grid_of(W, W.qset[q]), lane, s_inc[wv], s_o0[wv], W.qxy[2*q], W.qxy[2*q + 1], W.qr[q], W.qlev[2*q], W.qlev[2*q + 1], qd, W.max_cand,
               W.cand_idx + (size_t)q*W.max_cand, W.cand_dist + (size_t)q*W.max_cand, W.cand_cnt + q, W.best_idx + q, W.best_dist + q, W.best_dist2 + q);
}

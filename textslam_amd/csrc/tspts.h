// tspts.h -- tool::GetPyramidPts on the device (included by tsframe.hip after bilinear and GridDev): k_pts_batch serves the feature sets of a frame
// in ONE launch, one workgroup per (set, level) job, for tsframe_pyramid_pts (one set) and tsframe_pyramid_pts_batch alike; this is the only device
// code of the function.  A job is independent of every other: level l of set i writes at most n_i entries from out0 = xy_off[i]*L + l*n_i and
// leaves its count in cnt[job]; the host's copy-out closes the gaps, so no workgroup waits for another.
// Level 0 copies the raw features.  Level l >= 1 lays the reference's cell grid over the box (text, tool.cc:599-616) or the level image (scene,
// tool.cc:898-907); the host computes it (pts_grid).  A cell keeps one feature: the reference's search (tool.cc:678-685) compares each gradient
// with MAX, but MAX is never updated, so the last feature of the cell whose gradient passes (> 0 text, >= 0 scene) wins: the max index.  The grid
// lives in LDS up to PTS_LDS_CELLS cells, above that in the job's own region of the device scratch; either way this workgroup initialises it,
// so nothing is left over from an earlier call.  The cells are then emitted in the reference's visiting order (x outer, y inner) by an ordered
// compaction: wave ballot + popcount, and a sum over the PTS_NT/64 wave totals per chunk of PTS_NT cells.  Every loop bound (n, cw*ch) comes
// from the host's job.
#ifndef TSPTS_H
#define TSPTS_H

#define PTS_LDS_CELLS 8192                                       /* ints: 32 KB of LDS; mirrored by textslam_amd/frame.py for the tests */
#define PTS_NT 1024

struct PtsJob {
    GridDev G; const uint8_t *img, *grad; int w, h;              // the level's grid (unused at level 0) and resident planes
    int level, xy0, n, out0; long long sel_off;                  // sel_off < 0: the grid fits LDS; else the offset (ints) of its scratch region
};

__device__ __forceinline__ void pts_emit_one(const uint8_t *__restrict__ img, int w, int h, double pu, double pv, int j, int at,
                                             double *u, double *v, int *idx, double *inten, uint8_t *in) {
    u[at] = pu; v[at] = pv; idx[at] = j;
    double I; in[at] = bilinear(img, w, h, pu, pv, I) ? 1 : 0; inten[at] = I;
}

// sel: LDS or global (the address space is resolved after inlining); returns the number of entries written from J.out0
__device__ __forceinline__ int pts_level(int *sel, int *s_w, const PtsJob &J, const float *__restrict__ xy,
                                         double *u, double *v, int *idx, double *inten, uint8_t *in) {
    const int tid = threadIdx.x, w = J.w, h = J.h;
    const uint8_t *__restrict__ img = J.img, *__restrict__ grad = J.grad;
    const GridDev &G = J.G;
    const int ncell = G.cw*G.ch;
    for (int k = tid; k < ncell; k += PTS_NT) sel[k] = -1;
    __syncthreads();
    // per raw feature (tool.cc:620-637): the gradient sample at the level position, the cell by round() with the max edge folded into the last cell
    // (m == cw), and the cell's max qualifying index.  A feature outside the grid, where the reference would index past CellIdx, takes no cell.
    for (int j = tid; j < J.n; j += PTS_NT) {
        const double pu = (double)xy[2*j]*G.s, pv = (double)xy[2*j + 1]*G.s;
        double g; bilinear(grad, w, h, pu, pv, g);
        int m = (int)round(G.mode == 0 ? (pu - G.x0)/G.fx : pu/G.fx), q = (int)round(G.mode == 0 ? (pv - G.y0)/G.fy : pv/G.fy);
        if (m == G.cw) m = G.cw - 1;
        if (q == G.ch) q = G.ch - 1;
        if (m < 0 || q < 0 || m >= G.cw || q >= G.ch) continue;
        if (G.mode == 0 ? (g > 0.0) : (g >= 0.0)) atomicMax(&sel[q*G.cw + m], j);
    }
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < ncell; c0 += PTS_NT) {
        const int o = c0 + tid;                                // visiting order: o = i3 * ch + i4
        int j = -1;
        if (o < ncell) { const int i3 = o / G.ch, i4 = o - i3*G.ch; j = sel[i4*G.cw + i3]; }
        const int slot = wg_ordered_slot<PTS_NT/64>(j >= 0, s_w, base);
        if (j >= 0)                                            // a feature sits in one cell only: at most J.n entries in all
            pts_emit_one(img, w, h, (double)xy[2*j]*G.s, (double)xy[2*j + 1]*G.s, j, J.out0 + slot, u, v, idx, inten, in);
    }
    return base;
}

__global__ __launch_bounds__(PTS_NT) void k_pts_batch(const PtsJob *__restrict__ jobs, const float *__restrict__ xy_all, int *sel_glob, int *cnt,
                                                      double *u, double *v, int *idx, double *inten, uint8_t *in) {
    __shared__ int s_sel[PTS_LDS_CELLS], s_w[PTS_NT/64];
    const PtsJob J = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    const float *xy = xy_all + 2*(size_t)J.xy0;
    int total;
    if (J.level == 0) {
        for (int j = tid; j < J.n; j += PTS_NT) pts_emit_one(J.img, J.w, J.h, xy[2*j], xy[2*j + 1], j, J.out0 + j, u, v, idx, inten, in);
        total = J.n;
    } else if (J.n == 0) {
        total = 0;
    } else if (J.sel_off < 0) {
        total = pts_level(s_sel, s_w, J, xy, u, v, idx, inten, in);
    } else {
        total = pts_level(sel_glob + J.sel_off, s_w, J, xy, u, v, idx, inten, in);
    }
    if (tid == 0) cnt[blockIdx.x] = total;
}

#endif

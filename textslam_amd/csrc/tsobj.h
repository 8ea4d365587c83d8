// tsobj.h -- tsframe_text_object_info's kernel (included by tsframe.hip after bilinear, NB_DX / NB_DY, tsraster.h and tsquadstat.h): mapText::GetObjectInfo
// (src/mapText.cc:64-107) for all new text objects of a keyframe in ONE launch, one workgroup per (object, level) job.
//   tool::CalTextinfo   (src/tool.cc:1178-1262): mu / sigma of the detection quad on the level image, from the integer histogram of the masked pixels
//                       (quad_moments, csrc/tsquadstat.h -- the function libtsba's musigma_core calls: mu exact, sigma from the 256 bins in a fixed order);
//   tool::CalNormvec    (src/tool.cc:1342-1355): the level's features, thread = (feature, tap) with k_neighbours' expressions;
//   tool::GetBoxAllPixs (src/tool.cc:1264-1337): at level 0 the pixels of the SAME mask, ordered compaction as k_box_pixels (ballot + wave counts with
//                       a running base: wg_ordered_slot) into the object's own region of the pixel arrays.
// The host truncates the corners and clamps the bounding box (quad_box, as tsframe_box_pixels); the region of object i is sized by its clamped
// level-0 box, so its place is known before the launch and no workgroup waits for another: the host's copy-out closes the gaps.
// The quad mask lives in LDS (MS_MASK_WORDS).  quad_moments rasters every level with raster_quad_rows in bands of B = MS_MASK_WORDS*32 / w rows from the box's
// first row: a level of at most 640 x 480 pixels is one band whatever the box (B >= h), a larger one takes ceil(box rows / B).  raster_quad_rows is the one
// fill (raster_quad is its window of all rows), the histogram does not depend on the banding, and the pixels leave band after band: row-major order.  With one
// band quad_moments leaves the mask of the moments there for the pixels; with more, the bands are rastered a second time (mu and sigma are needed first).
// Every loop bound is a size of the job: box rows and columns, bands, features.
#ifndef TSOBJ_H
#define TSOBJ_H

#define OBJ_NT 1024

struct ObjJob {
    const uint8_t *img; int w, h;                                // the level's resident image
    int xy[8];                                                   // truncated corners (cv::Point)
    int x0, x1, y0, y1;                                          // clamped bounding box, inclusive
    int f0, nf;                                                  // the level's features in the packed feature arrays
    long long pix0;                                              // level 0 with pixel output: first slot of the object's region; else -1
};
struct ObjOut { double mu, sigma; int ok, npix; };

__global__ __launch_bounds__(OBJ_NT) void k_object_info(const ObjJob *__restrict__ jobs, const double *__restrict__ fu, const double *__restrict__ fv,
                                                        const double *__restrict__ fI, ObjOut *__restrict__ out,
                                                        double *__restrict__ ninten, double *__restrict__ inten8, double *__restrict__ ninten8, uint8_t *__restrict__ in,
                                                        int *__restrict__ pu, int *__restrict__ pv, double *__restrict__ pI, double *__restrict__ pN) {
    __shared__ unsigned s_mask[MS_MASK_WORDS];
    __shared__ unsigned s_hist[256];
    __shared__ double s_red[OBJ_NT];
    __shared__ int s_xy[8], s_w[OBJ_NT/64];
    const int tid = threadIdx.x;
    const ObjJob J = jobs[blockIdx.x];
    const uint8_t *__restrict__ img = J.img;
    const int w = J.w, h = J.h;
    if (tid < 8) s_xy[tid] = jobs[blockIdx.x].xy[tid];             // (from memory: indexing the register copy by tid would put the job in scratch)
    const int bw = J.x1 - J.x0 + 1, bh = J.y1 - J.y0 + 1;
    const int B = (MS_MASK_WORDS*32)/w;                          // rows of a band (the host refuses w > MS_MASK_WORDS*32)
    const bool one_band = bh <= B;
    __syncthreads();
    // 1. + 2. the histogram of the masked pixels of the clamped box, band after band, and its moments (quad_moments, tsquadstat.h): mu is exact
    const QuadMoments M = quad_moments<OBJ_NT>(img, w, h, s_xy, J.x0, J.x1, J.y0, J.y1, s_mask, s_hist, s_red
#ifdef MID_STAMPS
                                               , nullptr, 0
#endif
                                               );
    const double n = M.n, mu = M.mu, sigma = M.sigma;
    const bool ok = n >= 2.0 && sigma != 0.0;
    if (tid == 0) { ObjOut o; o.mu = mu; o.sigma = sigma; o.ok = ok ? 1 : 0; o.npix = (int)n; out[blockIdx.x] = o; }
    // 3. tool::CalNormvec -> GetNeighbour(INTERVAL8): thread = (feature, tap), as k_neighbours; ok = 0: the raw values, the normalised ones 0.0
    for (int e = tid; e < 8*J.nf; e += OBJ_NT) {
        const int j = J.f0 + (e >> 3), k = e & 7;
        double I; const bool inside = bilinear(img, w, h, fu[j] + NB_DX[k], fv[j] + NB_DY[k], I);
        inten8[8*(size_t)J.f0 + e] = I; ninten8[8*(size_t)J.f0 + e] = ok ? (I - mu)/sigma : 0.0;
        if (k == 7) in[j] = inside ? 1 : 0;
        if (k == 0) ninten[j] = ok ? (fI[j] - mu)/sigma : 0.0;
    }
    // 4. tool::GetBoxAllPixs (level 0): ordered compaction of the box, band after band, in tiles of OBJ_NT pixels
    if (J.pix0 < 0 || bw <= 0) return;
    int base = 0;
    for (int yb = J.y0; yb <= J.y1; yb += B) {
        const int ye = min(yb + B, J.y1 + 1), nr = ye - yb;
        if (!one_band) {
            __syncthreads();
            for (int k = tid; k < (nr*w + 31) >> 5; k += OBJ_NT) s_mask[k] = 0;
            __syncthreads();
            raster_quad_rows(s_mask, s_xy, w, h, yb, ye, tid, OBJ_NT);
            __syncthreads();
        }
        const int npx = bw*nr;
        for (int k0 = 0; k0 < npx; k0 += OBJ_NT) {
            const int k = k0 + tid;
            int x = 0, y = 0; bool hit = false;
            if (k < npx) { const int r = k/bw; x = J.x0 + (k - r*bw); y = yb + r; const int bit = r*w + x; hit = (s_mask[bit >> 5] >> (bit & 31)) & 1u; }
            const int slot = wg_ordered_slot<OBJ_NT/64>(hit, s_w, base);
            if (hit) {                                           // at most the masked pixels of the box: inside the region of bw*bh slots
                const size_t at = (size_t)J.pix0 + (size_t)slot;
                const double I = (double)img[(size_t)y*w + x];
                pu[at] = x; pv[at] = y; pI[at] = I; pN[at] = ok ? (I - mu)/sigma : 0.0;
            }
        }
    }
}

#endif

// The quad fill (csrc/tsraster.h) as host code behind tests/cxx/host_shim, against the oracle's cv::fillPoly restatement (tsba_oracle_fillpoly4).
// Above the LDS mask (648 x 480 and larger): the union of the row bands of raster_quad_rows at every pixel.  Bands as the kernels take them: MS_MASK_WORDS*32 / w
// rows each, from the clamped yMin of the corners' bounding box to its yMax; the mask is a heap block of exactly MS_MASK_WORDS words, so a sanitizer build sees any
// bit outside it.  Also, at sampled pixels, quad_covers against the same fill.
// At and below the mask (2 x 2 ... 640 x 480, B == hh there): raster_quad itself at every pixel, raster_quad_rows on windows [y0, y1) against the same rows of the
// fill (one row, first row, last row, sweeps), each mask block sized to exactly the window's words; quad_covers at every pixel up to 97 x 61; 4 and 256 "threads"
// (with 4, one thread owns a whole edge and the interior stride equals the edge count); the QUADS table and quads from a fixed-seed generator with corners up
// to one image size outside on every side, some corners repeated.
// Prints one line per size and "raster rows host: ok"; exit status 1 on the first difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
#include "tsraster.h"
extern "C" void tsba_oracle_fillpoly4(int w, int h, const int *xy, uint8_t *mask);

struct Quad { const char *name; double f[8]; int d[8]; };          // corner = f * (w, h) + d

static const Quad QUADS[] = {
    {"inside",                 {0.20, 0.30, 0.60, 0.25, 0.70, 0.60, 0.25, 0.70}, {0}},
    {"inside, full height",    {0.20, 0.00, 0.45, 0.00, 0.47, 1.00, 0.18, 1.00}, {0, 2, 0, 3, 0, -3, 0, -4}},
    {"inside, one row high",   {0.30, 0.50, 0.60, 0.50, 0.61, 0.50, 0.29, 0.50}, {0, 0, 0, 0, 0, 1, 0, 1}},
    {"whole image",            {0.00, 0.00, 1.00, 0.00, 1.00, 1.00, 0.00, 1.00}, {0, 0, -1, 0, -1, -1, 0, -1}},
    {"left corner outside",    {-0.20, 0.40, 0.40, 0.30, 0.45, 0.70, 0.10, 0.75}, {0}},
    {"right corner outside",   {0.60, 0.30, 1.25, 0.45, 0.90, 0.80, 0.55, 0.70}, {0}},
    {"top corner outside",     {0.30, 0.20, 0.50, -0.35, 0.70, 0.25, 0.50, 0.60}, {0}},
    {"bottom corner outside",  {0.30, 0.70, 0.55, 0.40, 0.75, 0.75, 0.50, 1.40}, {0}},
    {"all corners outside",    {-0.30, -0.30, 1.30, -0.25, 1.35, 1.30, -0.25, 1.20}, {0}},
    {"far outside, over it",   {-3.00, -2.00, 4.00, -2.50, 3.50, 3.00, -2.50, 3.50}, {0}},
    {"diamond through sides",  {0.50, -0.40, 1.40, 0.50, 0.50, 1.40, -0.40, 0.50}, {0}},
    {"outside, not over it",   {1.10, 0.20, 1.50, 0.25, 1.45, 0.60, 1.15, 0.55}, {0}},
    {"above, not over it",     {0.20, -0.50, 0.60, -0.45, 0.55, -0.10, 0.25, -0.15}, {0}},
    {"two equal corners",      {0.20, 0.20, 0.20, 0.20, 0.70, 0.45, 0.30, 0.90}, {0}},
    {"zero height",            {0.10, 0.50, 0.40, 0.50, 0.90, 0.50, 0.60, 0.50}, {0}},
    {"zero height, outside x", {-0.30, 0.75, 0.40, 0.75, 1.30, 0.75, 0.60, 0.75}, {0}},
    {"zero width",             {0.50, 0.05, 0.50, 0.40, 0.50, 0.95, 0.50, 0.60}, {0}},
    {"one point",              {0.50, 0.50, 0.50, 0.50, 0.50, 0.50, 0.50, 0.50}, {0}},
    {"bow tie",                {0.20, 0.10, 0.80, 0.90, 0.80, 0.10, 0.20, 0.90}, {0}},
    {"bow tie, outside",       {-0.20, -0.10, 1.20, 1.10, 1.20, -0.10, -0.20, 1.10}, {0}},
    {"last row and column",    {0.60, 0.70, 1.00, 0.70, 1.00, 1.00, 0.60, 1.00}, {0, 0, -1, 0, -1, -1, 0, -1}},
    {"sliver",                 {0.05, 0.05, 0.95, 0.93, 0.95, 0.94, 0.05, 0.06}, {0}},
};

static uint32_t lcg_state = 20260118u;
static uint32_t lcg() { lcg_state = lcg_state*1664525u + 1013904223u; return lcg_state >> 8; }

// rows [y0, y1) of the fill with nt threads, in a block of exactly the window's words, against the same rows of ref
static bool window_equal(const int *xy, int w, int h, int y0, int y1, int nt, const std::vector<uint8_t> &ref, const char *name) {
    const size_t words = (size_t)(((y1 - y0)*w + 31) >> 5);
    unsigned *m = (unsigned *)calloc(words, sizeof(unsigned));
    for (int tid = 0; tid < nt; tid++) raster_quad_rows(m, xy, w, h, y0, y1, tid, nt);
    bool same = true;
    for (int y = y0; y < y1 && same; y++) for (int x = 0; x < w; x++) {
        const int bit = (y - y0)*w + x; const int g = (m[bit >> 5] >> (bit & 31)) & 1u, r = ref[(size_t)y*w + x] ? 1 : 0;
        if (g != r) { printf("%d x %d, quad '%s', rows [%d, %d), %d threads: pixel (%d, %d) is %d, %d in the oracle\n", w, h, name, y0, y1, nt, x, y, g, r); same = false; break; }
    }
    for (size_t b = (size_t)(y1 - y0)*w; b < 32*words && same; b++)      // the last word's bits past the window stay clear
        if ((m[b >> 5] >> (b & 31)) & 1u) { printf("%d x %d, quad '%s', rows [%d, %d), %d threads: bit %zu past the window is set\n", w, h, name, y0, y1, nt, b); same = false; }
    free(m);
    return same;
}

// one quad at a size at or below the mask; sweep: every one-row window and tiled windows of several heights, else first row, last row and three drawn windows
static bool small_quad_equal(const int *xy, int w, int h, const char *name, bool sweep, bool every_pixel, long long &n_set, long long &n_win, long long &n_cov) {
    std::vector<uint8_t> ref((size_t)w*h, 0);
    tsba_oracle_fillpoly4(w, h, xy, ref.data());
    for (uint8_t r : ref) n_set += r ? 1 : 0;
    for (int nt : {4, 256}) {
        const size_t words = (size_t)((w*h + 31) >> 5);
        unsigned *m = (unsigned *)calloc(words, sizeof(unsigned));
        for (int tid = 0; tid < nt; tid++) raster_quad(m, xy, w, h, tid, nt);
        for (int p = 0; p < w*h; p++)
            if ((int)((m[p >> 5] >> (p & 31)) & 1u) != (ref[p] ? 1 : 0)) { printf("%d x %d, quad '%s', %d threads: raster_quad differs at (%d, %d)\n", w, h, name, nt, p % w, p / w); free(m); return false; }
        free(m);
        if (!window_equal(xy, w, h, 0, 1, nt, ref, name) || !window_equal(xy, w, h, h - 1, h, nt, ref, name)) return false;
        n_win += 2;
        if (sweep) {
            for (int hgt : {1, 2, 3, h/2 + 1, h})
                for (int y0 = 0; y0 < h; y0 += hgt) { if (!window_equal(xy, w, h, y0, std::min(y0 + hgt, h), nt, ref, name)) return false; n_win++; }
        } else {
            for (int k = 0; k < 3; k++) {
                const int y0 = (int)(lcg() % (uint32_t)h), y1 = y0 + 1 + (int)(lcg() % (uint32_t)(h - y0));
                if (!window_equal(xy, w, h, y0, k == 0 ? y0 + 1 : y1, nt, ref, name)) return false;
                n_win++;
            }
        }
    }
    for (size_t p = 0; p < (size_t)w*h; p += every_pixel ? 1 : 97) {
        const int x = (int)(p % w), y = (int)(p / w);
        if (quad_covers(xy, w, h, x, y) != (ref[p] != 0)) { printf("%d x %d, quad '%s': quad_covers differs at (%d, %d)\n", w, h, name, x, y); return false; }
        n_cov++;
    }
    if (!every_pixel)
        for (int x = 0; x < w; x++) for (int y : {0, h - 1})
            if (quad_covers(xy, w, h, x, y) != (ref[(size_t)y*w + x] != 0)) { printf("%d x %d, quad '%s': quad_covers differs at (%d, %d)\n", w, h, name, x, y); return false; }
    return true;
}

int main() {
    const int small[][2] = {{2, 2}, {5, 3}, {33, 17}, {97, 61}, {640, 480}};
    for (const auto &sz : small) {
        const int w = sz[0], h = sz[1];
        const bool upto = w*h <= 97*61;                                    // every pixel and every window up to 97 x 61, the present sampling above
        const int n_rand = upto ? 1000 : 60;
        long long n_set = 0, n_win = 0, n_cov = 0;
        for (const Quad &q : QUADS) {
            int xy[8];
            for (int k = 0; k < 8; k++) xy[k] = (int)(q.f[k]*((k & 1) ? h : w)) + q.d[k];
            if (!small_quad_equal(xy, w, h, q.name, true, upto, n_set, n_win, n_cov)) return 1;
        }
        for (int i = 0; i < n_rand; i++) {
            int xy[8]; char name[32];
            for (int k = 0; k < 8; k++) { const int s = (k & 1) ? h : w; xy[k] = (int)(lcg() % (uint32_t)(3*s)) - s; }      // [-s, 2 s)
            if (i % 7 == 3) { xy[2] = xy[0]; xy[3] = xy[1]; }
            if (i % 11 == 5) { xy[6] = xy[2]; xy[7] = xy[3]; }
            if (i % 13 == 6) { xy[5] = xy[3]; }                            // (a horizontal edge)
            snprintf(name, sizeof(name), "generated %d", i);
            if (!small_quad_equal(xy, w, h, name, false, upto, n_set, n_win, n_cov)) return 1;
        }
        printf("%d x %d: %d + %d quads, 4 and 256 threads, %lld windows, %lld pixels set, %lld point tests: equal\n", w, h, (int)(sizeof(QUADS)/sizeof(QUADS[0])), n_rand, n_win, n_set, n_cov);
    }
    const int sizes[][2] = {{648, 480}, {1280, 720}, {1920, 1080}};
    const int NT = 256;
    unsigned *mask = (unsigned *)malloc(sizeof(unsigned)*MS_MASK_WORDS);
    for (const auto &sz : sizes) {
        const int w = sz[0], h = sz[1], B = (MS_MASK_WORDS*32)/w;
        std::vector<uint8_t> ref((size_t)w*h), got((size_t)w*h);
        long long n_set = 0, n_bands = 0, n_cov = 0;
        for (const Quad &q : QUADS) {
            int xy[8];
            for (int k = 0; k < 8; k++) xy[k] = (int)(q.f[k]*((k & 1) ? h : w)) + q.d[k];
            std::fill(ref.begin(), ref.end(), 0); std::fill(got.begin(), got.end(), 0);
            tsba_oracle_fillpoly4(w, h, xy, ref.data());
            int yMin = xy[1], yMax = xy[1];
            for (int b = 1; b < 4; b++) { yMin = std::min(yMin, xy[2*b+1]); yMax = std::max(yMax, xy[2*b+1]); }
            yMin = std::max(yMin, 0); yMax = std::min(yMax, h - 1);
            for (int yb = yMin; yb <= yMax; yb += B) {
                const int ye = std::min(yb + B, yMax + 1);
                memset(mask, 0, sizeof(unsigned)*(size_t)(((ye - yb)*w + 31) >> 5));
                for (int tid = 0; tid < NT; tid++) raster_quad_rows(mask, xy, w, h, yb, ye, tid, NT);
                for (int y = yb; y < ye; y++) for (int x = 0; x < w; x++) { const int bit = (y - yb)*w + x; got[(size_t)y*w + x] = (mask[bit >> 5] >> (bit & 31)) & 1u; }
                n_bands++;
            }
            for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
                const uint8_t r = ref[(size_t)y*w + x] ? 1 : 0;
                if (r != got[(size_t)y*w + x]) { printf("%d x %d, quad '%s': pixel (%d, %d) is %d in the bands, %d in the oracle\n", w, h, q.name, x, y, got[(size_t)y*w + x], r); return 1; }
                n_set += r;
            }
            for (size_t p = 0; p < (size_t)w*h; p += 97) {                 // point membership at every 97th pixel and on the image's border rows
                const int x = (int)(p % w), y = (int)(p / w);
                if (quad_covers(xy, w, h, x, y) != (ref[p] != 0)) { printf("%d x %d, quad '%s': quad_covers differs at (%d, %d)\n", w, h, q.name, x, y); return 1; }
                n_cov++;
            }
            for (int x = 0; x < w; x++) for (int y : {0, h - 1})
                if (quad_covers(xy, w, h, x, y) != (ref[(size_t)y*w + x] != 0)) { printf("%d x %d, quad '%s': quad_covers differs at (%d, %d)\n", w, h, q.name, x, y); return 1; }
        }
        printf("%d x %d: %d quads, %lld bands of up to %d rows, %lld pixels set, %lld point tests: equal\n", w, h, (int)(sizeof(QUADS)/sizeof(QUADS[0])), n_bands, B, n_set, n_cov);
    }
    free(mask);
    printf("raster rows host: ok\n");
    return 0;
}

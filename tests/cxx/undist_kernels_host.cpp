// The camera-frame kernels (csrc/tsundist.h) as host code, one "thread" at a time: k_undist_map and k_undist_grey on heap blocks of exactly the sizes the
// library allocates (the map padded to a multiple of four entries, the raw frame (h - 1) * stride + w * channels bytes), so a sanitizer build sees any access
// outside them.  tests/test_undist_kernels_host.py builds this with -fsanitize=address,undefined, compares what it writes with the numpy restatement
// (tests/camera_frame_ref.py) and so holds the kernels' arithmetic and bounds without a GPU.
//   in : int32 w, h, stride, channels, r_first, seed; double K[4], dist[5], K_new[4]; the raw frame
//   out: int16 xy[h][w][2]; uint16 frac[h][w]; uint8 grey[h][w]; uint8 colour[h][w][channels]
// After the real map the remap runs once more over a map of random entries (any short, coordinates around every border, any fraction bits): no tap may leave
// the frame whatever the map holds.  Prints "undist kernels host: ok".
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// what tsundist.h uses of the HIP language
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(n)
#define __restrict__
struct Idx3 { int x, y, z; };
static Idx3 blockIdx, threadIdx;
struct uint4 { uint32_t x, y, z, w; };
struct uint2 { uint32_t x, y; };
#include "tsundist.h"

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "undist kernels host: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static void run_map(const UndistCam &C, int16_t *xy, uint16_t *frac) {
    for (int b = 0; b < (C.h + 63)/64; b++) for (int t = 0; t < 64; t++) { blockIdx.x = b; threadIdx.x = t; k_undist_map(C, xy, frac); }
}
static void run_grey(int ch, bool colour, const uint8_t *raw, int w, int h, int stride, int r_first, const int16_t *xy, const uint16_t *frac, uint8_t *grey, uint8_t *col) {
    const int npix = w*h;
    for (int b = 0; b < (npix + 1023)/1024; b++) for (int t = 0; t < 256; t++) {
        blockIdx.x = b; threadIdx.x = t;
        if (ch == 3 && colour) k_undist_grey<3, true>(raw, w, h, stride, r_first, xy, frac, npix, grey, col);
        else if (ch == 3) k_undist_grey<3, false>(raw, w, h, stride, r_first, xy, frac, npix, grey, nullptr);
        else if (colour) k_undist_grey<1, true>(raw, w, h, stride, 0, xy, frac, npix, grey, col);
        else k_undist_grey<1, false>(raw, w, h, stride, 0, xy, frac, npix, grey, nullptr);
    }
}

int main(int argc, char **argv) {
    REQUIRE(argc == 3);
    FILE *f = fopen(argv[1], "rb"); REQUIRE(f);
    int32_t hd[6]; UndistCam C;
    REQUIRE(fread(hd, 4, 6, f) == 6 && fread(C.K, 8, 4, f) == 4 && fread(C.dist, 8, 5, f) == 5 && fread(C.Kn, 8, 4, f) == 4);
    const int w = hd[0], h = hd[1], stride = hd[2], ch = hd[3], r_first = hd[4];
    REQUIRE(w >= 2 && h >= 2 && w <= 8192 && h <= 8192 && (ch == 1 || ch == 3) && stride >= w*ch);
    C.w = w; C.h = h; C.s0 = 4096/w < 1 ? 1 : 4096/w; if (C.s0 > h) C.s0 = h;
    const size_t npix = (size_t)w*h, n4 = (npix + 3) & ~(size_t)3, raw_bytes = (size_t)(h - 1)*stride + (size_t)w*ch;
    uint8_t *raw = (uint8_t *)malloc(raw_bytes); REQUIRE(raw && fread(raw, 1, raw_bytes, f) == raw_bytes);
    fclose(f);
    int16_t *xy = (int16_t *)calloc(n4*2, sizeof(int16_t)); uint16_t *frac = (uint16_t *)calloc(n4, sizeof(uint16_t));
    uint8_t *grey = (uint8_t *)malloc(npix), *grey2 = (uint8_t *)malloc(npix), *col = (uint8_t *)malloc((npix*ch + 3) & ~(size_t)3);
    REQUIRE(xy && frac && grey && grey2 && col);
    run_map(C, xy, frac);
    run_grey(ch, true, raw, w, h, stride, r_first, xy, frac, grey, col);
    run_grey(ch, false, raw, w, h, stride, r_first, xy, frac, grey2, nullptr);
    REQUIRE(memcmp(grey, grey2, npix) == 0);                           // the instance without the colour plane stores the same level 0

    FILE *o = fopen(argv[2], "wb"); REQUIRE(o);
    fwrite(xy, sizeof(int16_t), npix*2, o); fwrite(frac, sizeof(uint16_t), npix, o); fwrite(grey, 1, npix, o); fwrite(col, 1, npix*ch, o);
    fclose(o);

    // a map of anything: the taps are tested before they are read
    srand((unsigned)hd[5]);
    for (size_t i = 0; i < n4; i++) {
        for (int c = 0; c < 2; c++) {
            const int lim = c == 0 ? w : h, r = rand() % 5;
            xy[2*i + c] = (int16_t)(r == 0 ? rand() : r == 1 ? rand() % (lim + 4) - 2 : r == 2 ? lim - 2 + rand() % 4 : r == 3 ? -2 + rand() % 4 : (rand() & 1 ? 32767 : -32768));
        }
        frac[i] = (uint16_t)rand();
    }
    run_grey(ch, true, raw, w, h, stride, r_first, xy, frac, grey, col);
    free(raw); free(xy); free(frac); free(grey); free(grey2); free(col);
    printf("undist kernels host: ok\n");
    return 0;
}

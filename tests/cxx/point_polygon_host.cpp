// TEST INFRASTRUCTURE: fuse_point_in_polygon and the two polygon builders of textslam_amd/csrc/tsfuse.h compiled by plain g++ (no device, no HIP header).
//
//   point_polygon_host <in.bin> <out.bin>
//     in:  i32 n; n x (4 x 2 i32 polygon corners, 2 f32 point)
//     out: n bytes, 1 = cv::pointPolygonTest(polygon, point, true) > 0
//   point_polygon_host --polys <in.bin> <out.bin>
//     in:  i32 n; n x (4 x 2 f64 quad corners, 4 f64 bbox, f64 win)
//     out: n x 16 i32 = the shrunk quad, the bounding box
#include <cstdio>
#include <cstring>
#include <vector>
#include "tsfuse.h"

int main(int argc, char **argv) {
    const bool polys = argc == 4 && strcmp(argv[1], "--polys") == 0;
    if (argc != 3 && !polys) { fprintf(stderr, "usage: %s [--polys] in.bin out.bin\n", argv[0]); return 2; }
    FILE *f = fopen(argv[argc - 2], "rb"); if (!f) return 2;
    int32_t n = 0; if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    FILE *o = fopen(argv[argc - 1], "wb"); if (!o) return 2;
    for (int32_t i = 0; i < n; i++) {
        if (polys) { double v[13]; if (fread(v, 8, 13, f) != 13) return 2;
            int p[16]; fuse_shrunk_quad(v, v[12], p); fuse_bbox_quad(v + 8, p + 8); fwrite(p, 4, 16, o); }
        else { int32_t p[8]; float pt[2]; if (fread(p, 4, 8, f) != 8 || fread(pt, 4, 2, f) != 2) return 2;
            const unsigned char r = fuse_point_in_polygon(p, 4, pt[0], pt[1]) ? 1 : 0; fwrite(&r, 1, 1, o); }
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 2;
}

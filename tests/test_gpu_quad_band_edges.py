"""The row bands of the quad mask at their edges (csrc/tsquadstat.h quad_moments, and the pixel stage of k_object_info that re-rasters the bands): on a
2048 x 302 image of random bytes with one level a band is 307200 // 2048 = 150 rows, and tsframe_text_object_info takes quads about 300 columns wide whose
clamped boxes are 150 rows (one full band: the mask of the moments serves the pixels), 151 (a last band of one row), 300 (two full bands), 301 (two full
bands and one row) and 301 rows from row 1 (bands that do not align with the image's rows 0, 150, 300).
Against oracle_lib.musigma and the oracle's box pixels: ok, mu and the pixel offsets exactly, sigma at rtol 1e-11 (the two sides sum the squares in
different orders: the bound of tests/test_gpu_object_info.py), the pixel coordinates and raw intensities bit for bit and in order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, BAND = 2048, 302, 150
# (rows of the clamped box, the quad): slanted sides, integer top and bottom rows so that the box's rows are the quad's
CASES = [(150, [(100.0, 0.0), (400.5, 3.0), (396.0, 149.0), (104.5, 146.0)]),
         (151, [(500.0, 0.0), (800.5, 2.0), (795.0, 150.0), (497.5, 148.0)]),
         (300, [(900.0, 0.0), (1200.5, 4.0), (1203.0, 299.0), (903.5, 296.0)]),
         (301, [(1300.0, 0.0), (1600.5, 3.0), (1596.0, 300.0), (1304.5, 298.0)]),
         (301, [(1700.0, 1.0), (2000.5, 5.0), (1997.0, 301.0), (1698.5, 299.0)])]
NO_FEATS = {"level_off": np.zeros(2, np.int32), "u": np.zeros(0), "v": np.zeros(0), "inten": np.zeros(0)}


def test_band_edges_against_the_oracle(oracle_lib):
    from textslam_amd.frame import Frame
    assert 307200//W == BAND
    img = np.random.default_rng(61).integers(0, 256, (H, W), dtype=np.uint8)
    quads = np.array([q for _, q in CASES])
    for (rows, _), q in zip(CASES, quads):
        assert int(np.ceil(q[:, 1].max())) - int(np.floor(q[:, 1].min())) + 1 == rows and q[:, 1].max() <= H - 1
        assert 290 <= q[:, 0].max() - q[:, 0].min() <= 310
    assert quads[4][:, 1].min() > 0 and [r for r, _ in CASES] == [BAND, BAND + 1, 2*BAND, 2*BAND + 1, 2*BAND + 1]
    fr = Frame(0)
    fr.GetPyrMat(img, 1)
    got = fr.GetObjectInfoBatch(quads, [1.0], [NO_FEATS]*len(quads))
    off_g, off_o = [0], [0]
    for i, (g, q) in enumerate(zip(got, quads)):
        ok_o, mu_o, sg_o = oracle_lib.musigma(img, q)
        mu, sg = float(g["statistics"][0, 0]), float(g["statistics"][0, 1])
        u, v, I, _ = oracle_lib.frame_box_pixels(img, q, mu_o, sg_o)
        p = g["vRefPixs"]
        off_g.append(off_g[-1] + len(p["u"])); off_o.append(off_o[-1] + len(u))
        print("quad %d: %d rows, %d pixels, mu %.17g, sigma %.17g (oracle %.17g, relative difference %.3e)" % (i, CASES[i][0], len(u), mu, sg, sg_o, abs(sg - sg_o)/sg_o))
        assert ok_o and bool(g["ok"][0]) == bool(ok_o), i
        assert mu == mu_o, (i, mu, mu_o)
        np.testing.assert_allclose(sg, sg_o, rtol=1e-11, atol=0)
        assert p["u"].dtype == np.int32 and p["u"].tobytes() == u.tobytes() and p["v"].tobytes() == v.tobytes(), i
        assert p["featureInten"].tobytes() == I.tobytes(), i
        assert int(p["v"].min()) == int(q[:, 1].min()) and int(p["v"].max()) == int(q[:, 1].max()) and len(u) > 250*(CASES[i][0] - 10), i      # every band's rows are there
    assert off_g == off_o

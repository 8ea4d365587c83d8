"""The quad fill (csrc/tsraster.h) on the host: tests/cxx/raster_rows_host.cpp compiles the header as plain C++ behind tests/cxx/host_shim and compares it with
the oracle's cv::fillPoly restatement.  Above the mask (648 x 480, 1280 x 720, 1920 x 1080) the union of a quad's row bands at every pixel; at and below it
(2 x 2, 5 x 3, 33 x 17, 97 x 61, 640 x 480) raster_quad itself, raster_quad_rows on windows sized to exactly their words, quad_covers, with 4 and 256 threads;
quads inside, with corners outside on each side and on all sides, degenerate, and from a fixed-seed generator.  Built with -fsanitize=address,undefined and
run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bands_equal_the_oracle_fill_under_sanitizers(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1"]
    obj, exe = str(tmp_path / "tsba_oracle.o"), str(tmp_path / "raster_rows_host")
    subprocess.check_call(["gcc", "-c", "-std=c11", "-ffp-contract=off", *san, "-o", obj, os.path.join(ROOT, "oracle", "tsba_oracle.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *san, "-I" + os.path.join(ROOT, "tests", "cxx", "host_shim"),
                           "-I" + os.path.join(ROOT, "textslam_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "raster_rows_host.cpp"), obj, "-lm"])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "raster rows host: ok" in res.stdout and res.stderr == "", res.stdout + res.stderr
    assert sum("equal" in line for line in res.stdout.splitlines()) == 8

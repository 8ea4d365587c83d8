"""tsframe_pyramid_pts_batch without a GPU: include/tsframe.h declares it, the built library exports it, the Python mirror has it with the LDS
capacity taken from the kernel's header, and the adapter's header (adapter/tsframe_pyramid_pts.hpp) compiles on its own as C++11 against mock
types."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter")]

MOCK = r"""
#include "tsframe_pyramid_pts.hpp"
namespace mockp {
struct KeyPoint { struct Pt { float x, y; } pt; };
struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat31 { double v[3]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat33 { double m[9]; double operator()(int r, int c) const { return m[3*r + c]; } };
struct TextFeature { double u, v; Vec2 feature; int level, IdxToRaw; bool INITIAL; Mat31 ray; double featureInten; bool IN; };
struct SceneFeature { double u, v; Vec2 feature; int level, IdxToRaw; };
}
using namespace mockp;
// both overloads instantiated against the mock types
int text_only(void *ctx, const std::vector<std::vector<KeyPoint> > &k, const std::vector<Vec2> &a, const std::vector<Vec2> &b, const std::vector<double> &inv,
              const Mat33 &K0, std::vector<std::vector<std::vector<TextFeature *> > > &out) {
    return tsframe_adapter::text_fea_proc(ctx, k, a, b, inv, K0, out);
}
int with_scene(void *ctx, const std::vector<std::vector<KeyPoint> > &k, const std::vector<Vec2> &a, const std::vector<Vec2> &b, const std::vector<double> &inv,
               const Mat33 &K0, std::vector<std::vector<std::vector<TextFeature *> > > &out, const std::vector<Vec2> &obs,
               std::vector<std::vector<SceneFeature *> > &scene) {
    return tsframe_adapter::text_fea_proc(ctx, k, a, b, inv, K0, out, obs, scene);
}
"""


def test_header_declares():
    text = open(os.path.join(ROOT, "include", "tsframe.h")).read()
    m = re.search(r"int\s+tsframe_pyramid_pts_batch\s*\(([^;]*)\)\s*;", text)
    assert m, "include/tsframe.h does not declare tsframe_pyramid_pts_batch"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ["void *ctx", "int n_set", "const int32_t *mode", "const int32_t *xy_off", "const float *xy", "const double *box", "const double *inv_scale",
                    "int32_t *level_off", "double *u", "double *v", "int32_t *idx", "double *inten", "uint8_t *in"]
    assert "PTS_LDS_CELLS" not in text                                                   # the capacity is the kernel's business, not the ABI's


def test_library_exports_symbol():
    import __graft_entry__ as ge
    so = os.path.join(ROOT, "textslam_amd", "libtsframe.so")
    if not os.path.exists(so):
        ge.build()
    lib = C.CDLL(so)                                                                     # symbol lookup only: no context, no device
    assert hasattr(lib, "tsframe_pyramid_pts_batch")
    assert hasattr(lib, "tsframe_pyramid_pts")                                           # the single call keeps its entry point


def test_python_mirror():
    from textslam_amd import frame
    assert "tsframe_pyramid_pts_batch" in frame.EXPORTED_SYMBOLS
    assert callable(getattr(frame.Frame, "GetPyramidPtsBatch"))
    L = frame._load()
    assert len(L.tsframe_pyramid_pts_batch.argtypes) == 13 and L.tsframe_pyramid_pts_batch.restype is C.c_int
    src = open(os.path.join(ROOT, "textslam_amd", "csrc", "tspts.h")).read()
    assert frame.PTS_LDS_CELLS == int(re.search(r"^#define\s+PTS_LDS_CELLS\s+(\d+)", src, re.M).group(1)) > 0


def test_adapter_header_compiles_as_cxx11(tmp_path):
    src = tmp_path / "pyramid_pts_mock.cpp"
    src.write_text(MOCK)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + INC + [str(src)])
    txt = open(os.path.join(ROOT, "adapter", "tsframe_pyramid_pts.hpp")).read()
    assert not re.search(r"#include\s*[<\"](opencv|Eigen)", txt)                         # header-only, no OpenCV / Eigen

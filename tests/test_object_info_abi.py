"""tsframe_text_object_info without a GPU: include/tsframe.h declares it with the agreed argument list, the built library exports it beside the
single calls it batches, the Python mirror has it, and the adapter's header (adapter/tsframe_text_object_info.hpp) compiles on its own as C++11
against mock types."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter")]

MOCK = r"""
#include "tsframe_text_object_info.hpp"
namespace mocko {
struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat31 { double v[3]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } };
struct Mat33 { double m[9]; double operator()(int r, int c) const { return m[3*r + c]; } };
struct TextFeature { double u, v; Vec2 feature; int level, IdxToRaw; bool INITIAL; Mat31 ray; double featureInten, featureNInten; bool IN;
                     std::vector<Vec2> neighbour; std::vector<Mat31> neighbourRay; std::vector<double> neighbourInten, neighbourNInten; };
struct mapText { std::vector<std::vector<Vec2> > vTextDete; std::vector<Vec2> vTextDeteRay, statistics;
                 std::vector<std::vector<TextFeature *> > vRefFeature; std::vector<TextFeature *> vRefPixs; std::vector<bool> vRefFeatureSTATE; };
}
using namespace mocko;
int new_objects(void *ctx, const std::vector<bool> &good, const std::vector<std::vector<Vec2> > &dete, const std::vector<mapText *> &objs,
                const std::vector<double> &inv, const std::vector<Mat33> &vK) {
    return tsframe_adapter::text_object_info(ctx, good, dete, objs, inv, vK);
}
"""

ARGS = ["void *ctx", "int n_obj", "const double *quad", "const double *inv_scale", "const int32_t *feat_off", "const int32_t *level_off",
        "const double *u", "const double *v", "const double *inten", "int pix_cap", "double *musigma", "uint8_t *ok", "double *ninten", "double *inten8",
        "double *ninten8", "uint8_t *in", "int32_t *pix_off", "int32_t *pix_u", "int32_t *pix_v", "double *pix_inten", "double *pix_ninten"]


def test_header_declares():
    text = open(os.path.join(ROOT, "include", "tsframe.h")).read()
    m = re.search(r"int\s+tsframe_text_object_info\s*\(([^;]*)\)\s*;", text)
    assert m, "include/tsframe.h does not declare tsframe_text_object_info"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert args == ARGS
    assert "mapText.cc:64-107" in text                                                   # the header comment names the reference lines


def test_library_exports_symbol():
    import __graft_entry__ as ge
    so = os.path.join(ROOT, "textslam_amd", "libtsframe.so")
    if not os.path.exists(so):
        ge.build()
    lib = C.CDLL(so)                                                                     # symbol lookup only: no context, no device
    assert hasattr(lib, "tsframe_text_object_info")
    for single in ("tsframe_neighbours", "tsframe_box_pixels", "tsframe_pyramid_pts_batch", "tsframe_get_level"):
        assert hasattr(lib, single), single                                              # the single calls keep their entry points


def test_python_mirror():
    from textslam_amd import frame
    assert "tsframe_text_object_info" in frame.EXPORTED_SYMBOLS
    assert callable(getattr(frame.Frame, "GetObjectInfoBatch"))
    L = frame._load()
    assert len(L.tsframe_text_object_info.argtypes) == len(ARGS) and L.tsframe_text_object_info.restype is C.c_int


def test_adapter_header_compiles_as_cxx11(tmp_path):
    src = tmp_path / "object_info_mock.cpp"
    src.write_text(MOCK)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + INC + [str(src)])
    txt = open(os.path.join(ROOT, "adapter", "tsframe_text_object_info.hpp")).read()
    assert not re.search(r"#include\s*[<\"](opencv|Eigen)", txt)                         # header-only, no OpenCV / Eigen


def test_driver_compiles_as_cxx11(tmp_path):
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + INC +
                          [os.path.join(ROOT, "tests", "cxx", "object_info_from_cxx.cpp")])

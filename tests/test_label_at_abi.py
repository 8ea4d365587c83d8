"""tsba_text_label_at without a GPU: the library exports it, include/tsba.h declares it, the Python mirror has it, and the adapter's header
(adapter/tsba_text_labels.hpp) compiles as C++11 against a mock centre type and rounds a centre as the reference does (C round)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter")]

MOCK = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include "tsba_text_labels.hpp"
namespace mockl { struct Vec2 { double v[2]; double operator()(int i) const { return v[i]; } double &operator()(int i) { return v[i]; } }; }
// both overloads instantiated against the mock centre type
int one(void *ctx, const std::vector<mockl::Vec2> &c, std::vector<float> &l) { return tsba_adapter::labels_at_centres(ctx, 3, c, l); }
int two(void *ctx, const std::vector<mockl::Vec2> &a, const std::vector<mockl::Vec2> &b, std::vector<std::vector<float> > &l) {
    std::vector<int> kfs; kfs.push_back(3); kfs.push_back(4);
    std::vector<const std::vector<mockl::Vec2> *> cs; cs.push_back(&a); cs.push_back(&b);
    return tsba_adapter::labels_at_centres(ctx, kfs, cs, l);
}
"""

ROUND_MAIN = r"""
extern "C" int tsba_text_label_at(void *, int, int, const int32_t *, const int32_t *, int32_t *) { return TSBA_ERR_STATE; }     // (never called here: no library linked)
int main() {
    const double v[] = { 0.5, -0.5, 1.5, -1.5, 2.4999, -2.4999, 2.5, -2.5, 0.0, -0.0, 0.49999999999999994, 319.5, 1e300, -1e300 };
    for (unsigned i = 0; i < sizeof v/sizeof v[0]; i++) {
        const double r = round(v[i]);
        printf("%.17g %d %.17g\n", v[i], (int)tsba_adapter::centre_px(v[i]), r);
    }
    printf("nan %d\n", (int)tsba_adapter::centre_px(std::nan("")));
    return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    so = os.path.join(ROOT, "textslam_amd", "libtsba.so")
    if not os.path.exists(so):
        ge.build()
    return C.CDLL(so)


def test_library_exports_and_header_declares(lib):
    assert hasattr(lib, "tsba_text_label_at")
    text = open(os.path.join(ROOT, "include", "tsba.h")).read()
    m = re.search(r"int\s+tsba_text_label_at\s*\(([^;]*)\)\s*;", text)
    assert m, "include/tsba.h does not declare tsba_text_label_at"
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert [a.strip() for a in args.split(",")] == ["void *ctx", "int level", "int n", "const int32_t *kf", "const int32_t *px", "int32_t *label"]
    assert re.search(r"#define\s+TSBA_ABI_VERSION\s+5\b", text)                          # no struct changed
    assert hasattr(lib, "tsba_text_label_image")                                        # the drawing half keeps its call


def test_python_mirror():
    from textslam_amd import optimizer
    assert "tsba_text_label_at" in optimizer.EXPORTED_SYMBOLS
    assert callable(getattr(optimizer.Optimizer, "TextLabelAt"))
    L = optimizer.load_library()
    assert len(L.tsba_text_label_at.argtypes) == 6 and L.tsba_text_label_at.restype is C.c_int


def test_adapter_header_compiles_as_cxx11(tmp_path):
    src = tmp_path / "labels_mock.cpp"
    src.write_text(MOCK)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + INC + [str(src)])
    txt = open(os.path.join(ROOT, "adapter", "tsba_text_labels.hpp")).read()
    assert not re.search(r"#include\s*[<\"]opencv", txt) and "cv::" not in txt           # header-only, no OpenCV


def test_adapter_rounds_like_c_round(tmp_path):
    src, exe = tmp_path / "round.cpp", tmp_path / "round"
    src.write_text(MOCK + ROUND_MAIN)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-O1"] + INC + ["-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    got = {}
    for line in out:
        f = line.split()
        if len(f) == 3:
            got[float(f[0]) if f[0] != "-0" else -0.0] = (int(f[1]), float(f[2]))
    want = {0.5: 1, -0.5: -1, 1.5: 2, -1.5: -2, 2.4999: 2, -2.4999: -2, 2.5: 3, -2.5: -3, 0.49999999999999994: 0, 319.5: 320}      # half away from zero
    for v, r in want.items():
        px, c_round = got[v]
        assert px == r == int(c_round), (v, px, c_round)
    assert got[1e300][0] == -1 and got[-1e300][0] == -1 and "nan -1" in out              # no int holds them: a pixel outside every image

"""C-ABI checks of tsloop_sim3_batch that need no GPU: include/tsloop.h declares it and TSLOOP_RANSAC_MAX_HYP, libtsloop.so exports it, the Python mirror
(textslam_amd/loop.py) names it, the mirror's struct has the header's size and offsets (gcc), and a NULL context is refused without a device."""
import ctypes as C
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "tsloop.h")
NAMES = ("tsloop_sim3_batch", "tsloop_default_options_sim3_ransac")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    so = os.path.join(ROOT, "textslam_amd", "libtsloop.so")
    if not os.path.exists(so):
        ge.build()
    return C.CDLL(so)


def test_header_declares_and_library_exports(lib):
    from textslam_amd import loop
    text = open(HDR).read()
    declared = set(re.findall(r"\b(tsloop_[a-z_0-9]+)\s*\(", text))
    for n in NAMES:
        assert n in declared, n + " not declared in include/tsloop.h"
        assert hasattr(lib, n), n + " not exported by libtsloop.so"
        assert n in loop.EXPORTED_SYMBOLS
    for n in loop.EXPORTED_SYMBOLS:
        assert n in declared and hasattr(lib, n), n
    m = re.search(r"#define\s+TSLOOP_RANSAC_MAX_HYP\s+(\d+)", text)
    assert m and int(m.group(1)) == loop.RANSAC_MAX_HYP == 64


def test_struct_layout_matches_ctypes(tmp_path):
    from textslam_amd import loop
    fields = [f for f, _ in loop.TsloopSim3BatchProblem._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "tsloop.h"\n#include <stddef.h>\nunsigned long sz_batch(void){return sizeof(tsloop_sim3_batch_problem);}\n'
                   'unsigned long sz_sim3(void){return sizeof(tsloop_sim3_problem);}\nunsigned long sz_rep(void){return sizeof(tsloop_report);}\n'
                   'unsigned long sz_opt(void){return sizeof(tsloop_options);}\n'
                   + "".join("unsigned long off_%s(void){return offsetof(tsloop_sim3_batch_problem, %s);}\n" % (f, f) for f in fields))
    so = tmp_path / "sz.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    for f in ["sz_batch", "sz_sim3", "sz_rep", "sz_opt"] + ["off_" + f for f in fields]:
        getattr(L, f).restype = C.c_ulong
    assert L.sz_batch() == C.sizeof(loop.TsloopSim3BatchProblem)
    assert L.sz_sim3() == C.sizeof(loop.TsloopSim3Problem) and L.sz_rep() == C.sizeof(loop.TsloopReport) and L.sz_opt() == C.sizeof(loop.TsloopOptions)   # unchanged
    for f in fields:
        assert getattr(L, "off_" + f)() == getattr(loop.TsloopSim3BatchProblem, f).offset, f


def test_refused_without_a_context(lib):
    """A NULL context is an argument error before anything else is looked at (no device needed)."""
    from textslam_amd import loop
    lib.tsloop_sim3_batch.argtypes = [C.c_void_p, C.POINTER(loop.TsloopSim3BatchProblem), C.POINTER(loop.TsloopOptions)]
    p = loop.TsloopSim3BatchProblem(); o = loop.TsloopOptions()
    assert lib.tsloop_sim3_batch(None, C.byref(p), C.byref(o)) == -1
    assert lib.tsloop_sim3_batch(None, None, None) == -1
    lib.tsloop_default_options_sim3_ransac.argtypes = [C.POINTER(loop.TsloopSim3BatchProblem)]; lib.tsloop_default_options_sim3_ransac.restype = None
    p.n_cand = 7
    lib.tsloop_default_options_sim3_ransac(C.byref(p))
    assert (p.min_inliers, p.max_err2, p.optimise, p.n_cand) == (20, 45.0, 1, 7)

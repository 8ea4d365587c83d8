"""C-ABI checks of tsloop_detect_loop that need no GPU: include/tsloop.h declares it, tsloop_default_options_detect and TSLOOP_TEXT_MAX_LEN, libtsloop.so exports
both names, the Python mirror (textslam_amd/loop.py) names them, the mirror's struct has the header's size and offsets (gcc), and a NULL context is refused."""
import ctypes as C
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "tsloop.h")
NAMES = ("tsloop_detect_loop", "tsloop_default_options_detect")


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
    m = re.search(r"#define\s+TSLOOP_TEXT_MAX_LEN\s+(\d+)", text)
    assert m and int(m.group(1)) == loop.TEXT_MAX_LEN == 64


def test_struct_layout_matches_ctypes(tmp_path):
    from textslam_amd import loop
    fields = [f for f, _ in loop.TsloopDetectProblem._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include "tsloop.h"\n#include <stddef.h>\nunsigned long sz_detect(void){return sizeof(tsloop_detect_problem);}\n'
                   'unsigned long sz_batch(void){return sizeof(tsloop_sim3_batch_problem);}\n'
                   + "".join("unsigned long off_%s(void){return offsetof(tsloop_detect_problem, %s);}\n" % (f, f) for f in fields))
    so = tmp_path / "sz.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    for f in ["sz_detect", "sz_batch"] + ["off_" + f for f in fields]:
        getattr(L, f).restype = C.c_ulong
    assert L.sz_detect() == C.sizeof(loop.TsloopDetectProblem)
    assert L.sz_batch() == C.sizeof(loop.TsloopSim3BatchProblem)                 # unchanged
    for f in fields:
        assert getattr(L, "off_" + f)() == getattr(loop.TsloopDetectProblem, f).offset, f


def test_refused_without_a_context(lib):
    """A NULL context is an argument error before anything else is looked at (no device needed); the defaults touch only their four fields."""
    from textslam_amd import loop
    lib.tsloop_detect_loop.argtypes = [C.c_void_p, C.POINTER(loop.TsloopDetectProblem)]
    p = loop.TsloopDetectProblem()
    assert lib.tsloop_detect_loop(None, C.byref(p)) == -1
    assert lib.tsloop_detect_loop(None, None) == -1
    lib.tsloop_default_options_detect.argtypes = [C.POINTER(loop.TsloopDetectProblem)]; lib.tsloop_default_options_detect.restype = None
    p.n_query = 7; p.n_map = 9; p.n_kf = 3; p.min_matched_words = 5
    lib.tsloop_default_options_detect(C.byref(p))
    assert (p.min_str_score, p.score_thresh_min, p.top_n, p.max_match) == (0.3, 0.51, 10, 64)
    assert (p.n_query, p.n_map, p.n_kf, p.min_matched_words) == (7, 9, 3, 5) and not p.q_off and not p.match_cnt


def test_make_detect_problem_packs_the_flat_arrays():
    from textslam_amd import loop
    p, A = loop.make_detect_problem([b"ab", b""], [-1, 0], [b"abc", b"\xff"], [0, 1], [[0, 2], []], 3, min_matched_words=2, score_thresh_min=0.35, fill=(-7, 9.0))
    assert (p.n_query, p.n_map, p.n_kf, p.top_n, p.max_match, p.min_matched_words, p.score_thresh_min, p.min_str_score) == (2, 2, 3, 10, 64, 2, 0.35, 0.3)
    assert A["q_off"].tolist() == [0, 2, 2] and A["m_off"].tolist() == [0, 3, 4] and A["m_str"][:4].tolist() == [97, 98, 99, 255]
    assert A["obs_off"].tolist() == [0, 2, 2] and A["obs_kf"][:2].tolist() == [0, 2] and A["m_skip"][:2].tolist() == [0, 1] and A["q_self"][:2].tolist() == [-1, 0]
    assert A["match_idx"].shape == (2, 64) and (A["match_idx"] == -7).all() and (A["match_score"] == 9.0).all() and A["cand"].shape == (10,)
    assert p.m_str[3] == 255 and p.obs_kf[1] == 2

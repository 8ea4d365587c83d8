"""C-ABI checks of tsorb_match_text_theta_ransac that need no GPU: include/tsorb.h declares it and TSORB_THETA_MAX_FEAT, libtsorb.so exports it, and the argument
types of the Python mirror (textslam_amd/orbextractor.py) are the header's -- gcc compiles an assignment of the function to a pointer of the mirror's type with
-Werror=incompatible-pointer-types."""
import ctypes as C
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "tsorb.h")
NAME = "tsorb_match_text_theta_ransac"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    so = os.path.join(ROOT, "textslam_amd", "libtsorb.so")
    if not os.path.exists(so):
        ge.build()
    from textslam_amd import orbextractor
    return orbextractor.load_library()


def test_header_declares_and_library_exports(lib):
    from textslam_amd import orbextractor
    text = open(HDR).read()
    declared = set(re.findall(r"\b(tsorb_[a-z_0-9]+)\s*\(", text))
    assert NAME in declared, NAME + " not declared in include/tsorb.h"
    assert hasattr(lib, NAME), NAME + " not exported by libtsorb.so"
    assert NAME in orbextractor.EXPORTED_SYMBOLS
    m = re.search(r"#define\s+TSORB_THETA_MAX_FEAT\s+(\d+)", text)
    assert m and int(m.group(1)) == 1024 == orbextractor.TEXT_THETA_MAX_FEAT
    m = re.search(r"#define\s+TSORB_THETA_MAX_HYP\s+(\d+)", text)
    assert m and int(m.group(1)) == orbextractor.TEXT_THETA_MAX_HYP
    assert hasattr(orbextractor.ORBextractor, "match_text_theta_ransac")


_CTYPE = {C.c_void_p: "void *", C.c_int: "int", C.POINTER(C.c_int32): "int32_t *", C.POINTER(C.c_float): "float *", C.POINTER(C.c_double): "double *"}
INPUTS = set(range(2, 10))                                             # the positions of the const pointers of the prototype: off .. triple


def _pointer_decl(fn, const):
    args = []
    for k, t in enumerate(fn.argtypes):
        s = _CTYPE[t]
        args.append(("const " + s) if (k in const and s.endswith("*")) else s)
    return "int (*p_%s)(%s) = %s;\n" % (NAME, ", ".join(args), NAME)


def test_mirror_argument_types_are_the_headers(lib, tmp_path):
    fn = lib.tsorb_match_text_theta_ransac
    assert fn.restype == C.c_int and len(fn.argtypes) == 17
    src = tmp_path / "sig.c"
    src.write_text('#include "tsorb.h"\n' + _pointer_decl(fn, INPUTS))
    cmd = ["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sig.o"), str(src)]
    subprocess.check_call(cmd)
    # the check has teeth: a float rho where the header has doubles does not compile
    bad = tmp_path / "bad.c"
    bad.write_text(src.read_text().replace("const double *", "const float *", 1))
    assert bad.read_text() != src.read_text()
    assert subprocess.run(cmd[:-3] + ["-o", str(tmp_path / "bad.o"), str(bad)], capture_output=True).returncode != 0


def test_refused_without_a_context(lib):
    """A NULL context is an argument error before anything else is looked at (no device needed)."""
    assert lib.tsorb_match_text_theta_ransac(None, 1, *([None]*15)) == -1

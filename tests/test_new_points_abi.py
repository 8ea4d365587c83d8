"""C-ABI checks of tsorb_match_search_claim and tsorb_match_new_points that need no GPU: include/tsorb.h declares them, libtsorb.so exports them, the argument
types of the Python mirror (textslam_amd/orbextractor.py) are the header's -- gcc compiles an assignment of each function to a pointer of the mirror's type with
-Werror=incompatible-pointer-types -- and a NULL context is refused before anything else is looked at."""
import ctypes as C
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "tsorb.h")
NAMES = ("tsorb_match_search_claim", "tsorb_match_new_points")


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
    for name in NAMES:
        assert name in declared, name + " not declared in include/tsorb.h"
        assert hasattr(lib, name), name + " not exported by libtsorb.so"
        assert name in orbextractor.EXPORTED_SYMBOLS
    assert hasattr(orbextractor.ORBextractor, "match_search_claim") and hasattr(orbextractor.ORBextractor, "match_new_points")
    m = re.search(r"#define\s+TSORB_BRUTE_MAX_FEAT\s+(\d+)", text)
    assert m and int(m.group(1)) == orbextractor.BRUTE_MAX_FEAT == 65536     # the searched set's limit: an index fits the 16 bits a staged candidate gives it


_CTYPE = {C.c_void_p: "void *", C.c_int: "int", C.c_double: "double", C.POINTER(C.c_int32): "int32_t *", C.POINTER(C.c_float): "float *", C.POINTER(C.c_double): "double *",
          C.POINTER(C.c_uint8): "uint8_t *"}
INPUTS = {"tsorb_match_search_claim": set(range(2, 7)), "tsorb_match_new_points": set(range(2, 7)) | set(range(10, 14))}      # the const pointers of the prototypes


def _pointer_decl(name, fn, const):
    args = []
    for k, t in enumerate(fn.argtypes):
        s = _CTYPE[t]
        args.append(("const " + s) if (k in const and s.endswith("*")) else s)
    return "int (*p_%s)(%s) = %s;\n" % (name, ", ".join(args), name)


@pytest.mark.parametrize("name", NAMES)
def test_mirror_argument_types_are_the_headers(lib, tmp_path, name):
    fn = getattr(lib, name)
    assert fn.restype == C.c_int and len(fn.argtypes) == (13 if name == NAMES[0] else 20)
    src = tmp_path / "sig.c"
    src.write_text('#include "tsorb.h"\n' + _pointer_decl(name, fn, INPUTS[name]))
    cmd = ["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sig.o"), str(src)]
    subprocess.check_call(cmd)
    # the check has teeth: an int32 eligibility mask where the header has bytes does not compile
    bad = tmp_path / "bad.c"
    bad.write_text(src.read_text().replace("const uint8_t *, int,", "const int32_t *, int,", 1))
    assert bad.read_text() != src.read_text()
    assert subprocess.run(cmd[:-3] + ["-o", str(tmp_path / "bad.o"), str(bad)], capture_output=True).returncode != 0


def test_refused_without_a_context(lib):
    """A NULL context is an argument error before anything else is looked at (no device needed), and no output is touched."""
    n = C.c_int32(-77)
    assert lib.tsorb_match_search_claim(None, 0, None, None, None, None, None, 50, 0, 0.9, None, None, C.byref(n)) == -1 and n.value == -77
    assert lib.tsorb_match_new_points(None, 0, None, None, None, None, None, 50, 0, 0.9, None, None, None, None, 9, None, C.byref(n), None, None, C.byref(n)) == -1
    assert n.value == -77

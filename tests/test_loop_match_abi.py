"""C-ABI checks of the loop-closing matchers that need no GPU: include/tsorb.h declares them and TSORB_BRUTE_MAX_FEAT, libtsorb.so exports them, and the
argument types of the Python mirror (textslam_amd/orbextractor.py) are the header's -- gcc compiles an assignment of each function to a pointer of the
mirror's type with -Werror=incompatible-pointer-types."""
import ctypes as C
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "tsorb.h")
NAMES = ("tsorb_match_brute_text", "tsorb_match_brute_scene")


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
    for n in NAMES:
        assert n in declared, n + " not declared in include/tsorb.h"
        assert hasattr(lib, n), n + " not exported by libtsorb.so"
        assert n in orbextractor.EXPORTED_SYMBOLS
    m = re.search(r"#define\s+TSORB_BRUTE_MAX_FEAT\s+(\d+)", text)
    assert m and int(m.group(1)) == orbextractor.BRUTE_MAX_FEAT
    # the packed key (distance << 16 | index) of the device reduction: an index fits 16 bits, the key stays a positive int32
    assert int(m.group(1)) <= 1 << 16 and (0x7fff << 16 | 0xffff) == 2 ** 31 - 1
    assert text.index("tsorb_match_search(") < text.index("tsorb_match_brute_text(") < text.index("tsorb_match_brute_scene(")


_CTYPE = {C.c_void_p: "void *", C.c_int: "int", C.c_double: "double", C.c_float: "float",
          C.POINTER(C.c_int32): "int32_t *", C.POINTER(C.c_uint8): "uint8_t *", C.POINTER(C.c_float): "float *", C.POINTER(C.c_double): "double *"}


def _pointer_decl(fn, name, const):
    """`int (*p)(<the mirror's argument types>) = name;` -- input pointers const as in the header (const-ness is not part of the mirror)."""
    args = []
    for k, t in enumerate(fn.argtypes):
        s = _CTYPE[t]
        args.append(("const " + s) if (k in const and s.endswith("*")) else s)
    return "int (*p_%s)(%s) = %s;\n" % (name, ", ".join(args), name)


def test_mirror_argument_types_are_the_headers(lib, tmp_path):
    src = tmp_path / "sig.c"
    text_in, scene_in = set(range(2, 6)), set(range(4, 7)) | set(range(8, 15))        # the input pointers' positions
    assert lib.tsorb_match_brute_text.restype == C.c_int and lib.tsorb_match_brute_scene.restype == C.c_int
    assert len(lib.tsorb_match_brute_text.argtypes) == 9 and len(lib.tsorb_match_brute_scene.argtypes) == 19
    src.write_text('#include "tsorb.h"\n' + _pointer_decl(lib.tsorb_match_brute_text, "tsorb_match_brute_text", text_in)
                   + _pointer_decl(lib.tsorb_match_brute_scene, "tsorb_match_brute_scene", scene_in))
    cmd = ["gcc", "-c", "-Wall", "-Werror", "-Werror=incompatible-pointer-types", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "sig.o"), str(src)]
    subprocess.check_call(cmd)
    # the check has teeth: a float where the header has a double does not compile
    bad = tmp_path / "bad.c"
    bad.write_text(src.read_text().replace("int, double, int32_t *, int32_t *)", "int, float, int32_t *, int32_t *)"))
    assert bad.read_text() != src.read_text()
    assert subprocess.run(cmd[:-3] + ["-o", str(tmp_path / "bad.o"), str(bad)], capture_output=True).returncode != 0


def test_refused_without_a_context(lib):
    """A NULL context is an argument error before anything else is looked at (no device needed)."""
    assert lib.tsorb_match_brute_text(None, 1, None, None, None, None, None, None, None) == -1
    assert lib.tsorb_match_brute_scene(None, 640, 480, 1, None, None, None, 1, None, None, None, None, None, None, None, 50, 0.9, None, None) == -1

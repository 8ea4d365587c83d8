"""The staging layout of the one-call entry points and the owner of their blocks (textslam_amd/csrc/tsstage.h: Span, Layout, Block) on the CPU -- no GPU, no HIP header.

tests/cxx/stage_layout_host.cpp is built with plain g++ and the address and undefined-behaviour sanitizers and run as a child process.  It checks, for the
alignments of libtsorb (16) and libtsloop (256): every span's offset is a multiple of the alignment; spans do not overlap and mark() covers them all; a
zero-length span takes no room and is a no-op in put and get, null pointers included; put then get through a heap block of exactly mark() bytes returns every
array unchanged (odd counts 1, 3, 17; element sizes 1, 4, 8, 12, 24 -- AddressSanitizer is what holds the block to "exactly"); a null source or destination
touches nothing; at() on a second base gives the same offset.

The owner of a block that only grows (Block) runs there too, over a malloc / free policy that counts its live blocks and fails on request: growing from empty; a
smaller grow keeps pointer and capacity; a larger one frees first and returns a block whose every byte can be written; capacity == max(need, room); a failed
allocation leaves null and 0 and the next grow succeeds; a context's blocks are released by its destructor alone (the leak check at exit is the judge); a block,
and a struct that holds one, is not copyable (static_assert)."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stage_layout") / "stage_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cxx", "stage_layout_host.cpp")])
    return exe


def test_layout_under_sanitizers(host_exe):
    r = subprocess.run([host_exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "stage layout host: ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_layout_header_needs_no_hip():
    """The layout half and the owner template compile with g++ alone; the two memory policies (hipMalloc / hipHostMalloc) are behind the HIP compiler's guard."""
    src = open(os.path.join(ROOT, "textslam_amd", "csrc", "tsstage.h")).read()
    head, guard, room = src.partition("#ifdef __HIPCC__")
    assert guard and "#include <hip" not in src
    assert "struct DeviceMem" in room and "struct PinnedMem" in room and "DeviceBlock" in room and "PinnedBlock" in room
    assert "struct Block" in head and "struct Layout" in head and "struct Span" in head
    assert "hipMalloc" not in head and "hipHostMalloc" not in head and "hipError_t" not in head and "hipFree" not in head and "hipHostFree" not in head
    assert "hipMalloc(" in room and "hipFree(" in room and "hipHostMalloc(" in room and "hipHostFree(" in room

"""The layout of the reduced camera system that an upload chooses -- dense or band storage, streaming or partitioned solver, number of interiors, separator
system by cyclic reduction or sequentially, ring geometry (csrc/tsba_layout.h: choose_solver_layout) -- through the host-only hook tsba_debug_solver_layout:
no GPU needed."""
import ctypes as C
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "textslam_amd", "libtsba.so")
KEYS = ("use_lds", "band", "S_up", "LDB", "band_stream", "P", "sep_cr", "partitioned", "nsepb", "ring", "ring_G", "xchg_wp")
ERR_STATE = -4


def _const(header, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(os.path.join(ROOT, "textslam_amd", "csrc", header)).read()).group(1))


BAND_BW_MAX, CH_NB, CR_SMAX = _const("tsba_band.h", "BAND_BW_MAX"), _const("tsba_chol.h", "CH_NB"), _const("tsba_bandcr.h", "CR_SMAX")
BANDP_MAXP, RING_OFF = _const("tsba_bandp.h", "BANDP_MAXP"), _const("tsba_bandp.h", "RING_OFF")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    from textslam_amd import abi
    L = C.CDLL(LIB)
    L.tsba_debug_solver_layout.argtypes = [C.c_int]*5 + [C.POINTER(abi.TsbaDebugOptions), C.POINTER(C.c_int32)]; L.tsba_debug_solver_layout.restype = C.c_int
    L.tsba_debug_bandp_part.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]; L.tsba_debug_bandp_part.restype = None
    L.tsba_debug_sv_lmax.argtypes = [C.c_int, C.c_int, C.c_int]; L.tsba_debug_sv_lmax.restype = C.c_int
    return L


def _layout(lib, n_kf, bw_rows, ring=0, ring_k0=0, multi=0, **switches):
    from textslam_amd import abi
    d = abi.TsbaDebugOptions()
    for k, v in switches.items():
        setattr(d, k, v)
    out = (C.c_int32*12)()
    rc = lib.tsba_debug_solver_layout(n_kf, bw_rows, ring, ring_k0, multi, C.byref(d) if switches else None, out)
    assert rc in (0, ERR_STATE), rc
    return rc, dict(zip(KEYS, [int(x) for x in out]))


def _shrunk(n_kf, B, P):
    """The fewest-blocks rule of the kernels: an interior holds at least 2 B + 2 pose blocks."""
    while P > 1 and (n_kf - (P - 1)*B)//P < 2*B + 2:
        P -= 1
    return P


def test_invariants_of_the_chosen_layout(lib):
    """A few hundred seeded inputs, every debug switch zero: what the solvers and their kernels rely on."""
    rng = np.random.default_rng(17)
    seen = {"dense": 0, "wide": 0, "stream1": 0, "part": 0, "cr": 0, "ring": 0, "refused": 0}
    for it in range(600):
        ring = int(it % 4 == 3); multi = int(rng.integers(0, 2))
        if ring:                                                         # as the plan builder makes one: a band the cyclic reduction takes, a loop of four interiors at least
            B = int(rng.integers(1, CR_SMAX//6 + 1)); nloop = int(rng.integers(13*B + 8, 3000)); k0 = int(rng.choice([0, 0, 47, int(rng.integers(47, 3000))])); n_kf = k0 + nloop
        else:
            B = int(rng.integers(1, BAND_BW_MAX//6 + 1)); n_kf = int(rng.choice([int(rng.integers(2, 80)), int(rng.integers(2, 6001))])); k0 = 0
        bw = 6*B; N = 6*n_kf
        rc, L = _layout(lib, n_kf, bw, ring, k0, multi)
        ctx = (n_kf, bw, ring, k0, multi, L)
        assert 1 <= L["P"] <= BANDP_MAXP, ctx
        if not L["band"]:
            assert L["band_stream"] == 0 and L["P"] == 1, ctx
        if L["use_lds"] or bw + 2*CH_NB - 1 >= N:
            assert L["band"] == 0, ctx
        assert L["partitioned"] == (L["P"] > 1), ctx
        if L["P"] > 1 and not ring:
            assert (n_kf - (L["P"] - 1)*B)//L["P"] >= 2*B + 2, ctx
        if L["sep_cr"]:
            assert L["P"] >= 4, ctx
        assert (rc == 0) == (not ring or L["ring"] == 1), ctx          # a ring plan is solved as a ring or refused
        if L["ring"]:
            G = L["ring_G"]
            assert ring and L["sep_cr"] and G >= 4 and G & (G - 1) == 0 and 0 <= L["P"] - G <= RING_OFF - 1 and (k0 > 0) == (L["P"] > G), ctx
        assert L["xchg_wp"] == (min(N, bw + 6) if multi and L["band"] else 0), ctx
        if L["band_stream"] and not ring:                                # the solve phase's LDS bound holds for the partition of the chosen P
            lmax = lib.tsba_debug_sv_lmax(n_kf, B, L["P"])
            o = (C.c_int*5)(); longest = 0
            for p in range(L["P"]):
                lib.tsba_debug_bandp_part(n_kf, B, L["P"], p, o); assert o[0] == L["P"], ctx
                longest = max(longest, o[2] - o[1])
            assert lmax >= longest, ctx
        seen["dense" if not L["band"] else "wide" if not L["band_stream"] else "stream1" if L["P"] == 1 else "part"] += 1
        seen["cr"] += L["sep_cr"]; seen["ring"] += L["ring"]; seen["refused"] += rc != 0
    assert min(seen[k] for k in ("dense", "stream1", "part", "cr", "ring")) >= 20, seen     # (bands of at most BAND_BW_MAX rows all take the streaming solver; no_band_stream: below)


def test_debug_switches_do_what_the_header_says(lib):
    """include/tsba_debug.h: band_parts, sep_solver, no_band_stream."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        B = int(rng.integers(1, CR_SMAX//6 + 1)); bw = 6*B; n_kf = int(rng.integers(200, 6001)); k = int(rng.integers(2, 300))
        if 6*n_kf <= bw + 2*CH_NB - 1:
            continue
        rc, L = _layout(lib, n_kf, bw, band_parts=k)
        assert rc == 0 and L["band_stream"] == 1 and L["P"] == _shrunk(n_kf, B, min(k, BANDP_MAXP)), (n_kf, bw, k, L)
        rc, L = _layout(lib, n_kf, bw, band_parts=1)
        assert L["band_stream"] == 1 and L["P"] == 1 and L["partitioned"] == 0 and L["sep_cr"] == 0, (n_kf, bw, L)      # the single-workgroup streaming solver
        rc, L = _layout(lib, n_kf, bw, sep_solver=1)
        assert L["sep_cr"] == 0, (n_kf, bw, L)
        for s in (2, 3, 4):
            rc, L = _layout(lib, n_kf, bw, sep_solver=s, band_parts=k)
            assert L["sep_cr"] == (L["P"] >= 4), (n_kf, bw, k, s, L)
        rc, L = _layout(lib, n_kf, bw, no_band_stream=1)
        assert L["band_stream"] == 0 and L["S_up"] == CH_NB and L["P"] == 1 and L["LDB"] == bw + 2*CH_NB - 1, (n_kf, bw, L)


# (n_kf, bw_rows, ring plan, ring_k0, multi) -> (use_lds, band, band_stream, interiors as solver_info reports them, sep_cr, ring): what the PARENT of the commit that
# introduced choose_solver_layout chose for the maps the GPU suite uploads without a band_parts override -- profiles/upload_stages_solver_info_parent_vs_branch.txt
PINNED = {
    (20, 114, 0, 0, 0): (1, 0, 0, 0, 0, 0),          # the C4 window
    (300, 48, 0, 0, 0): (0, 1, 1, 9, 1, 0),          # config_global(300, band 8)
    (700, 54, 0, 0, 0): (0, 1, 1, 17, 1, 0),         # config_global(700, band 9)
    (5000, 60, 0, 0, 0): (0, 1, 1, 129, 1, 0),       # the 5000-keyframe chain at band 10
    (500, 72, 0, 0, 0): (0, 1, 1, 13, 1, 0),         # C5 (the cost model's comment: 13 interiors)
    (600, 48, 1, 0, 0): (0, 1, 1, 16, 1, 1),         # test_loop_closure_ring_partition
    (2400, 66, 1, 0, 0): (0, 1, 1, 32, 1, 1),
    (600, 48, 1, 200, 0): (0, 1, 1, 12, 1, 1),       # test_loop_closure_with_a_tail
    (1500, 42, 1, 1000, 0): (0, 1, 1, 48, 1, 1),
    (600, 48, 0, 0, 0): (0, 1, 1, 17, 1, 0),         # the long-range map (far_solver = 2: band part + blocks outside it)
    (300, 48, 0, 0, 1): (0, 1, 1, 9, 1, 0),          # world = 2
}


@pytest.mark.parametrize("inputs", sorted(PINNED))
def test_pinned_layouts_of_the_suites_maps(lib, inputs):
    rc, L = _layout(lib, *inputs)
    assert rc == 0
    got = (L["use_lds"], L["band"], L["band_stream"], L["P"] if L["band_stream"] else 0, L["sep_cr"], L["ring"])
    assert got == PINNED[inputs], (inputs, L)

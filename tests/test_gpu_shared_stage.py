"""The one-call entry points of libtsorb share one device block and one pinned block on their context, and both only grow (textslam_amd/csrc/tsstage.h).
Different calls in turn on ONE context, so that a later call reuses a block an earlier one sized and that still holds the earlier call's bytes:

  1. match_pnp_ransac on its smallest committed world (5 matches, 1 hypothesis): the blocks are a few hundred bytes;
  2. match_two_view_reconstruct on a largest committed world (300 matches): the blocks grow;
  3. match_text_theta_ransac with rho and p3d omitted: a partial download into a block that still holds step 2's bytes;
  4. step 1 again, now in blocks far larger than it needs.

Every output of every step equals, bit for bit, the same call on a fresh context of its own, and the outputs the caller omitted keep their fill value.  The calls go
through the C ABI with raw arrays, every output pre-filled, so a byte the call did not write shows."""
import ctypes as C
import faulthandler
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ransac_ref as PNP                                          # noqa: E402
import two_view_reconstruct_ref as REC                                # noqa: E402
import text_theta_ref as TT                                           # noqa: E402

pytestmark = pytest.mark.gpu
F32, F64, I32, U8 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
_CT = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int32): I32, np.dtype(np.uint8): U8}
FILL = 77


@pytest.fixture(autouse=True)
def time_limit():
    """A call that does not return ends the process with a traceback instead of holding the device."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _p(a):
    return None if a is None else a.ctypes.data_as(_CT[a.dtype])


def _outs(shapes):
    return {k: np.full(s, FILL, t) for k, (s, t) in shapes.items()}


def pnp(ex, w):
    Pw = np.ascontiguousarray(w["Pw"], np.float32); uv = np.ascontiguousarray(w["uv"], np.float32); K = np.ascontiguousarray(w["K"], np.float64)
    sub = np.ascontiguousarray(w["subsets"], np.int32); n, H = len(Pw), len(sub)
    o = _outs(dict(inlier=(n, np.uint8), result=(4, np.int32), pose=(12, np.float64), hyp_count=(H, np.int32), hyp_pose=(12*H, np.float64)))
    rc = ex.lib.tsorb_match_pnp_ransac(ex.ctx, n, _p(Pw), _p(uv), _p(K), H, _p(sub), float(w["reproj_err"]), float(w["confidence"]),
                                       _p(o["inlier"]), _p(o["result"]), _p(o["pose"]), _p(o["hyp_count"]), _p(o["hyp_pose"]))
    assert rc == 0, ex.lib.tsorb_last_error(ex.ctx).decode()
    return o


def reconstruct(ex, w):
    xy1 = np.ascontiguousarray(w["xy1"], np.float32); xy2 = np.ascontiguousarray(w["xy2"], np.float32); inl = np.ascontiguousarray(w["inlier"], np.uint8)
    M = np.ascontiguousarray(w["M21"], np.float32).reshape(9); K = np.ascontiguousarray(w["K"], np.float32); n, H = len(xy1), 8
    o = _outs(dict(result=(6, np.int32), R21=(9, np.float32), t21=(3, np.float32), p3d=(3*n, np.float32), triangulated=(n, np.uint8), hyp_good=(H, np.int32),
                   hyp_cos=(H, np.float32), hyp_parallax=(H, np.float32), hyp_pose=(12*H, np.float32), hyp_state=(H*n, np.uint8), hyp_p3d=(3*H*n, np.float32)))
    rc = ex.lib.tsorb_match_two_view_reconstruct(ex.ctx, n, _p(xy1), _p(xy2), _p(inl), int(w["model"]), _p(M), _p(K), float(w["sigma"]), float(w["min_parallax"]),
                                                 int(w["min_triangulated"]), *[_p(o[k]) for k in o])
    assert rc == 0, ex.lib.tsorb_last_error(ex.ctx).decode()
    return o


TT_OMITTED = ("p3d", "rho_out")


def text_theta(ex, w):
    off = np.ascontiguousarray(w["off"], np.int32); hoff = np.ascontiguousarray(w["hyp_off"], np.int32); tri = np.ascontiguousarray(w["triple"], np.int32)
    hxy = np.ascontiguousarray(w["host_xy"], np.float32); txy = np.ascontiguousarray(w["targ_xy"], np.float32)
    Tcr = np.ascontiguousarray(np.asarray(w["Tcr"], np.float64)[:3, :4]); K = np.ascontiguousarray(w["K"], np.float64)
    P, N, H = len(off) - 1, len(hxy), len(tri)
    assert w.get("rho") is None                                       # rho omitted: triangulated on the device
    o = _outs(dict(sel=(P, np.int32), theta=(3*P, np.float64), score=(P, np.float64), p3d=(3*N, np.float32), rho_out=(N, np.float64), hyp_score=(H, np.float64),
                   hyp_theta=(3*H, np.float64)))
    rc = ex.lib.tsorb_match_text_theta_ransac(ex.ctx, P, _p(off), _p(hxy), _p(txy), None, _p(Tcr), _p(K), _p(hoff), _p(tri),
                                              *[None if k in TT_OMITTED else _p(o[k]) for k in o])
    assert rc == 0, ex.lib.tsorb_last_error(ex.ctx).decode()
    return o


def _same(got, ref, step):
    for k in ref:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), (step, k)


def test_calls_in_turn_on_one_context_equal_fresh_contexts():
    from textslam_amd.orbextractor import ORBextractor
    w_pnp = PNP.world(*PNP.CASES[0]); w_rec = REC.make("f_drop_300"); w_tt = TT.make("mixed_9")
    assert w_pnp["n"] == min(c[1] for c in PNP.CASES + PNP.SPECIAL) and w_rec["n"] == 300          # (300: the largest n of two_view_reconstruct_ref.WORLDS)
    steps = [("pnp", pnp, w_pnp), ("reconstruct", reconstruct, w_rec), ("text_theta", text_theta, w_tt), ("pnp again", pnp, w_pnp)]
    fresh = [f(ORBextractor(), w) for _, f, w in steps[:3]]
    fresh.append(fresh[0])
    # the fresh answers are answers: every output written, but for the two the text-theta call omitted
    for (name, _, _), o in zip(steps, fresh):
        for k, a in o.items():
            if name == "text_theta" and k in TT_OMITTED:
                assert (a == FILL).all(), (name, k)
            else:
                assert a.size == 0 or not (a == FILL).all(), (name, k)
    shared = ORBextractor()
    for (name, f, w), ref in zip(steps, fresh):
        _same(f(shared, w), ref, name)

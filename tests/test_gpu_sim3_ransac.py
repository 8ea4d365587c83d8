"""tsloop_sim3_batch on the GPU: every loop candidate's Sim3Solver RANSAC and OptimizeSim3 in one launch (include/tsloop.h, textslam_amd/csrc/tsloop_ransac.h).

  * the RANSAC against the numpy restatement (tests/sim3_ransac_ref.py): inlier counts of EVERY hypothesis, the selection, the mask equal as integers; each
    hypothesis' Sim3 to q 1e-10 / s 1e-10 relative / t 1e-9 -- derived, not tuned: two fp64 eigen-solvers differ in the eigenvector by about
    eps |N| / gap <= 1e-12 at the relative gap of 1e-3 the inputs are held to, and t carries that through |O2| <= 8 m;
  * the LM against the oracle started from the device's own selection, with the tolerances of tests/test_gpu_loop.py::test_optimize_sim3_parity;
  * the fused call bit for bit what tsloop_optimize_sim3 returns from the same start (one device function, contraction off);
  * a candidate's outputs byte-equal whatever else is in the batch, in whatever order; candidates without hypotheses or matches; every argument error;
  * the adapter (adapter/tsloop_sim3_ransac.hpp) from C++ over the mock types, byte for byte the Python call.
The inputs are held to conditions first (no error within 1e-5 relative of the threshold, eigenvalue gap >= 1e-3, no final LM residual within 1e-6 px of
4.0): with them every integer the test compares is decided by a margin far above the rounding differences of the two sides."""
import ctypes as C
import os
import struct
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ransac_ref as S                                           # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = S.CASES + S.EXTRA
_id = lambda c: "seed%d_n%d_h%d%s" % (c[0], c[1], c[3], "_k2" if len(c) > 4 else "")
FILL = (0x5a, -77, 7.0)


@pytest.fixture(scope="module")
def lo():
    from textslam_amd.loop import LoopOptimizer
    return LoopOptimizer(0)


@pytest.fixture(scope="module")
def worlds(oracle_lib):
    """Every case's world, the restatement's answer and the conditions the comparison rests on -- computed once, read-only."""
    out = {}
    for c in ALL:
        w = S.world(*c); res = S.run_world(w); cond = S.conditions(w, res, oracle_lib)
        assert cond["err_margin"] >= 1e-5, (c, cond)
        assert cond["gap"] >= 1e-3, (c, cond)
        assert cond["lm_margin"] >= 1e-6, (c, cond)
        out[c] = (w, res, cond)
    for c in S.CASES:                                                  # the table of the recipe's prototype
        counts, sel, ok, n_lm = S.EXPECT[c[0]]
        assert out[c][1]["counts"][:8] == counts and out[c][1]["sel"] == sel and out[c][1]["ok"] == ok
        assert n_lm is None or out[c][2]["lm"][0] == n_lm
    return out


def cand_of(w, triples=None):
    return {"P1": w["P1"], "P2": w["P2"], "pred1": w["pred1"], "pred2": w["pred2"], "uv1": w["uv1"], "uv2": w["uv2"],
            "triples": w["triples"] if triples is None else triples, "K2": w["K2"]}


def empty_cand(n, K, seed=0):
    """n matches and no hypothesis (n < 20: the reference's N < mRansacMinInliers exit), or no match at all."""
    w = S.world(20 + seed, max(n, 3), 0.0, H=0)
    c = cand_of(w, np.zeros((0, 3), np.int32))
    for k in ("P1", "P2", "pred1", "pred2", "uv1", "uv2"):
        c[k] = c[k][:n]
    return c


def sig(r):
    """A candidate's outputs as bytes (the report without its wall time)."""
    rep = None if r["report"] is None else tuple(r["report"][k] for k in ("iters", "accepted", "termination", "n_inlier", "cost0", "cost1"))
    return (r["ok"], r["sel"], r["n_inlier_ransac"], r["sim_ransac"].tobytes(), r["inlier"].tobytes(), r["hyp_count"].tobytes(), r["hyp_sim"].tobytes(),
            None if r["sim"] is None else r["sim"].tobytes(), rep)


@pytest.fixture(scope="module")
def singles(lo, worlds):
    """One candidate per call: (optimise = 0, optimise = 1) for every case."""
    out = {}
    for c in ALL:
        w = worlds[c][0]
        out[c] = (lo.Sim3Batch([cand_of(w)], w["K1"], w["K"], optimise=False)[0], lo.Sim3Batch([cand_of(w)], w["K1"], w["K"], optimise=True)[0])
    return out


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_ransac_against_the_restatement(worlds, singles, case):
    w, ref, _ = worlds[case]; got = singles[case][0]
    print("counts", got["hyp_count"].tolist(), "ref", ref["counts"], "sel", got["sel"], ref["sel"])
    assert got["hyp_count"].tolist() == ref["counts"]
    assert (got["sel"], got["ok"], got["n_inlier_ransac"]) == (ref["sel"], ref["ok"], ref["n_inlier"])
    assert np.array_equal(got["inlier"], ref["mask"])
    sims = np.array([h["sim"] for h in ref["hyps"]])
    dq = np.abs(got["hyp_sim"][:, :4] - sims[:, :4]).max(); dt = np.abs(got["hyp_sim"][:, 4:7] - sims[:, 4:7]).max(); ds = np.abs(got["hyp_sim"][:, 7]/sims[:, 7] - 1).max()
    print("dq %.2e dt %.2e ds %.2e" % (dq, dt, ds))
    assert (got["hyp_sim"][:, 0] >= 0).all()                           # the sign rule
    np.testing.assert_allclose(np.linalg.norm(got["hyp_sim"][:, :4], axis=1), 1.0, rtol=0, atol=1e-14)
    assert dq <= 1e-10 and ds <= 1e-10 and dt <= 1e-9
    assert np.array_equal(got["sim_ransac"], got["hyp_sim"][got["sel"]])
    assert got["sim"] is None and got["report"] is None                # optimise = 0
    # the RANSAC part of the optimise = 1 call is the same
    one = singles[case][1]
    assert sig(one)[:4] == sig(got)[:4] and sig(one)[5:7] == sig(got)[5:7]
    if not ref["ok"]:
        assert not got["inlier"].any() and one["sim"] is None and one["report"] is None


OK_CASES = [c for c in ALL if c[0] not in (6, 8, 13)]


@pytest.mark.parametrize("case", OK_CASES, ids=_id)
def test_lm_against_the_oracle(worlds, singles, oracle_lib, case):
    w = worlds[case][0]; r0, r1 = singles[case]
    assert r0["ok"] and r1["ok"]
    no, so, io, ro = oracle_lib.optimize_sim3(w["P1"], w["uv1"], w["P2"], w["uv2"], r0["inlier"].astype(np.uint8), r0["sim_ransac"], w["K"])
    rg = r1["report"]
    print("device", rg, "oracle", ro)
    assert (rg["iters"], rg["accepted"], rg["termination"]) == (ro["iters"], ro["accepted"], ro["termination"])
    assert rg["n_inlier"] == no == int(r1["inlier"].sum()) and np.array_equal(r1["inlier"], io)
    np.testing.assert_allclose(rg["cost0"], ro["cost0"], rtol=1e-12)
    np.testing.assert_allclose(rg["cost1"], ro["cost1"], rtol=1e-9)
    np.testing.assert_allclose(r1["sim"], so, rtol=0, atol=1e-8)
    if case in S.CASES:
        assert no == S.EXPECT[case[0]][3]
    assert not (r1["inlier"] & ~r0["inlier"]).any()                    # the LM only ever removes


@pytest.mark.parametrize("case", OK_CASES, ids=_id)
def test_fused_equals_unfused(lo, worlds, singles, case):
    """sim, mask and report of the optimise = 1 call, bit for bit what tsloop_optimize_sim3 returns when fed sim_ransac and the RANSAC mask."""
    w = worlds[case][0]; r0, r1 = singles[case]
    n, sim, inl, rep = lo.OptimizeSim3(w["P1"], w["uv1"], w["P2"], w["uv2"], r0["inlier"].astype(np.uint8), r0["sim_ransac"], w["K"])
    assert sim.tobytes() == r1["sim"].tobytes()
    assert np.array_equal(inl, r1["inlier"]) and n == r1["report"]["n_inlier"]
    for k in ("iters", "accepted", "termination", "n_inlier"):
        assert rep[k] == r1["report"][k], k
    for k in ("cost0", "cost1"):
        assert struct.pack("<d", rep[k]) == struct.pack("<d", r1["report"][k]), k


def test_independence_of_the_candidates(lo, worlds, singles):
    """A candidate's outputs do not depend on what else is in the batch, nor on where it stands."""
    cs = list(S.CASES) + [S.EXTRA[2]]
    w0 = worlds[cs[0]][0]
    cands = [cand_of(worlds[c][0]) for c in cs]
    want = [sig(singles[c][1]) for c in cs]
    fwd = lo.Sim3Batch(cands, w0["K1"], w0["K"])
    assert [sig(r) for r in fwd] == want
    rev = lo.Sim3Batch(cands[::-1], w0["K1"], w0["K"])
    assert [sig(r) for r in rev] == want[::-1]
    dup = lo.Sim3Batch([c for c in cands for _ in (0, 1)], w0["K1"], w0["K"])
    assert [sig(r) for r in dup] == [s for s in want for _ in (0, 1)]
    assert any(r["ok"] for r in fwd) and not all(r["ok"] for r in fwd)
    r0 = lo.Sim3Batch(cands, w0["K1"], w0["K"], optimise=False)
    assert [sig(r) for r in r0] == [sig(singles[c][0]) for c in cs]


def _raw(lo, cands, K1, K, optimise=True, ctx=True, options=True, mutate=None, **kw):
    """The C call with sentinel-filled outputs: returns (rc, arrays)."""
    from textslam_amd import loop
    p, A = loop.make_sim3_batch_problem(cands, K1, K, optimise, fill=FILL, **kw)
    if mutate is not None:
        mutate(p, A)
    o = lo.default_options_sim3()
    rc = lo.lib.tsloop_sim3_batch(lo.ctx if ctx else None, C.byref(p), C.byref(o) if options else None)
    return rc, A


def _untouched(A, rows=None):
    rep = np.frombuffer(A["rep"], np.uint8).reshape(len(A["rep"]), -1)
    if rows is None:
        return bool(all(np.all(A[k] == FILL[0]) for k in ("ok", "inlier")) and all(np.all(A[k] == FILL[1]) for k in ("sel", "n_inlier_ransac", "hyp_count"))
                    and all(np.all(A[k] == FILL[2]) for k in ("sim_ransac", "sim", "hyp_sim")) and np.all(rep == FILL[0]))
    return bool(np.all(A["sim"][rows] == FILL[2]) and np.all(rep[rows] == FILL[0]))


def test_candidates_without_hypotheses_or_matches(lo, worlds, singles):
    """ok, not ok, a candidate of 12 matches (no hypothesis: N < 20) and one without matches in one batch: the latter two are not ok, select nothing, have
    masks of 0, and sim / rep of every candidate that is not ok are not written."""
    cs = [S.CASES[0], S.CASES[5], S.CASES[1]]                          # ok, not ok, ok
    w0 = worlds[cs[0]][0]
    cands = [cand_of(worlds[cs[0]][0]), empty_cand(12, w0["K"]), cand_of(worlds[cs[1]][0]), empty_cand(0, w0["K"]), cand_of(worlds[cs[2]][0]), empty_cand(12, w0["K"], 1)]
    rc, A = _raw(lo, cands, w0["K1"], w0["K"])
    assert rc == 0
    assert A["ok"].tolist() == [1, 0, 0, 0, 1, 0] and A["sel"][[1, 3, 5]].tolist() == [-1, -1, -1] and A["n_inlier_ransac"][[1, 3, 5]].tolist() == [0, 0, 0]
    assert np.all(A["sim_ransac"][[1, 3, 5]] == 0.0)
    off = A["off"]
    for k in (1, 2, 3, 5):
        assert not A["inlier"][off[k]:off[k + 1]].any()
    assert _untouched(A, [1, 2, 3, 5]) and not _untouched(A, [0]) and not _untouched(A, [4])
    for k, c in ((0, cs[0]), (2, cs[1]), (4, cs[2])):                  # and the others are what they are alone
        one = singles[c][1]
        assert A["sim_ransac"][k].tobytes() == one["sim_ransac"].tobytes() and np.array_equal(A["inlier"][off[k]:off[k + 1]].astype(bool), one["inlier"])
        assert A["hyp_count"][A["hyp_off"][k]:A["hyp_off"][k + 1]].tolist() == one["hyp_count"].tolist()
        if one["ok"]:
            assert A["sim"][k].tobytes() == one["sim"].tobytes() and A["rep"][k].n_inlier == one["report"]["n_inlier"]
    # only candidates without hypotheses: nothing is launched, the same answers
    rc, A = _raw(lo, [empty_cand(12, w0["K"]), empty_cand(0, w0["K"])], w0["K1"], w0["K"])
    assert rc == 0 and A["ok"].tolist() == [0, 0] and A["sel"].tolist() == [-1, -1] and not A["inlier"].any() and _untouched(A, [0, 1])
    # optimise = 0: sim / rep of an ok candidate stay as they were
    rc, A = _raw(lo, [cand_of(w0)], w0["K1"], w0["K"], optimise=False)
    assert rc == 0 and A["ok"].tolist() == [1] and _untouched(A, [0])
    # the optional outputs may be NULL
    def drop(p, A):
        p.hyp_count = None; p.hyp_sim = None
    rc, A = _raw(lo, [cand_of(w0)], w0["K1"], w0["K"], mutate=drop)
    assert rc == 0 and A["sim"][0].tobytes() == singles[cs[0]][1]["sim"].tobytes() and np.all(A["hyp_count"] == FILL[1]) and np.all(A["hyp_sim"] == FILL[2])


def test_arguments(lo, worlds, singles):
    w = worlds[S.CASES[0]][0]; w2 = worlds[S.CASES[1]][0]
    base = [cand_of(w), cand_of(w2)]
    n0 = len(w["P1"])

    def refused(mutate=None, cands=base, named=True, **kw):
        rc, A = _raw(lo, cands, w["K1"], w["K"], mutate=mutate, **kw)
        assert rc == -1 and _untouched(A)
        if named:
            assert "tsloop_sim3_batch" in lo.lib.tsloop_last_error(lo.ctx).decode()

    refused(ctx=False, named=False)                                    # a NULL context
    refused(options=False)
    for name in ("off", "hyp_off", "triple", "P1", "P2", "pred1", "pred2", "uv1", "uv2", "K2", "ok", "sel", "n_inlier_ransac", "sim_ransac", "inlier", "sim", "rep"):
        refused(lambda p, A, name=name: setattr(p, name, None))
    refused(lambda p, A: setattr(p, "n_cand", -1))                     # a negative count
    for key in ("off", "hyp_off"):                                     # offsets that do not start at 0, or decrease
        def first(p, A, key=key): A[key][0] = 1
        def dec(p, A, key=key): A[key][1] = A[key][2] + 1
        refused(first); refused(dec)
    g = np.random.default_rng(0)
    many = S.draw_triples(n0, 65, lambda a, b: a + int(g.random()*(b - a + 1)))
    refused(cands=[cand_of(w, many)])                                  # more than TSLOOP_RANSAC_MAX_HYP hypotheses
    rc, A = _raw(lo, [cand_of(w, many[:64])], w["K1"], w["K"]); assert rc == 0 and len(A["hyp_count"]) == 64
    def t_hi(p, A): A["triple"][2, 1] = n0                             # a triple index outside the candidate (it exists in the next one)
    def t_lo(p, A): A["triple"][0, 0] = -1
    def t_eq(p, A): A["triple"][1, 2] = A["triple"][1, 0]
    def t_hi2(p, A): A["triple"][-1, 0] = len(w2["P1"])
    for m in (t_hi, t_lo, t_eq, t_hi2):
        refused(m)
    for key, idx in (("P1", (3, 1)), ("P2", (n0 + 2, 0)), ("pred1", (0, 0)), ("pred2", (5, 1)), ("uv1", (7, 0)), ("uv2", (n0, 1)), ("K2", (1, 2))):
        for bad in (np.nan, np.inf):
            def nf(p, A, key=key, idx=idx, bad=bad): A[key][idx] = bad
            refused(nf)
    for key in ("K1", "K"):
        def nfk(p, A, key=key): getattr(p, key)[3] = float("nan")
        refused(nfk)
    refused(min_inliers=-1)
    for bad in (float("nan"), float("inf"), -1.0):
        refused(max_err2=bad)
    # n_cand == 0 reads no pointer
    from textslam_amd import loop
    p = loop.TsloopSim3BatchProblem(); o = lo.default_options_sim3()
    assert lo.lib.tsloop_sim3_batch(lo.ctx, C.byref(p), C.byref(o)) == 0
    assert lo.Sim3Batch([], w["K1"], w["K"]) == []
    # and the context still answers
    again = lo.Sim3Batch(base, w["K1"], w["K"])
    assert [sig(r) for r in again] == [sig(singles[S.CASES[0]][1]), sig(singles[S.CASES[1]][1])]
    # the thresholds are the arguments': with min_inliers = 205 the first candidate's best count (205) is not enough, with 204 it is
    assert [r["ok"] for r in lo.Sim3Batch(base[:1], w["K1"], w["K"], min_inliers=205)] == [False]
    assert [r["ok"] for r in lo.Sim3Batch(base[:1], w["K1"], w["K"], min_inliers=204)] == [True]
    assert lo.Sim3Batch(base[:1], w["K1"], w["K"], max_err2=0.0)[0]["hyp_count"].tolist() == [0]*5


def test_adapter_from_cxx(tmp_path, lo, worlds):
    """pack_sim3_batch / scatter_sim3_batch and the caller's side of Sim3Solver over the mock types: the hypothesis counts, the triples (the driver's 32-bit LCG
    restated in Python) and every output byte for byte the Python call's."""
    exe = str(tmp_path / "sim3_ransac_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "sim3_ransac_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsloop", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    cs = list(S.CASES) + list(S.EXTRA[1:])
    ws = [worlds[c][0] for c in cs]
    K1, K = ws[0]["K1"], ws[0]["K"]
    seed = 20240917
    gen = S.Lcg32(seed)
    cands = [cand_of(w) for w in ws]
    cands.insert(2, empty_cand(12, K)); cands.insert(5, empty_cand(0, K))
    for c in cands:                                                    # the caller's rule and draws, candidate by candidate
        n = len(c["P1"]); c["triples"] = S.draw_triples(n, S.n_hypotheses(n), gen.random_int)
    assert sorted(set(len(c["triples"]) for c in cands)) == [0, 1, 3, 5]
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<iI", len(cands), seed)); f.write(np.asarray(K1, np.float64).tobytes()); f.write(np.asarray(K, np.float64).tobytes())
        for c in cands:
            f.write(struct.pack("<i", len(c["P1"]))); f.write(np.asarray(c["K2"], np.float64).tobytes())
            for k, dt in (("P1", np.float64), ("P2", np.float64), ("pred1", np.float64), ("pred2", np.float64), ("uv1", np.float32), ("uv2", np.float32)):
                f.write(np.ascontiguousarray(c[k], dt).tobytes())
    res = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "sim3 batch from C++: ok" in res.stdout, res.stdout
    got = lo.Sim3Batch(cands, K1, K)
    raw = open(outp, "rb").read(); off = 0
    for c, r in zip(cands, got):
        n = len(c["P1"])
        (H,) = struct.unpack_from("<i", raw, off); off += 4
        tri = np.frombuffer(raw, np.int32, 3*H, off).reshape(H, 3); off += 12*H
        assert H == len(c["triples"]) and np.array_equal(tri, c["triples"])
        ok, sel, ninl, nopt = struct.unpack_from("<iiii", raw, off); off += 16
        sr = raw[off:off + 64]; off += 64; sim = raw[off:off + 64]; off += 64
        ri = struct.unpack_from("<iiii", raw, off); off += 16; rd = raw[off:off + 16]; off += 16
        inl = np.frombuffer(raw, np.uint8, n, off); off += n
        hc = np.frombuffer(raw, np.int32, H, off); off += 4*H; hs = raw[off:off + 64*H]; off += 64*H
        assert (bool(ok), sel, ninl) == (r["ok"], r["sel"], r["n_inlier_ransac"]) and sr == r["sim_ransac"].tobytes()
        assert np.array_equal(inl.astype(bool), r["inlier"]) and hc.tolist() == r["hyp_count"].tolist() and hs == r["hyp_sim"].tobytes()
        if r["ok"]:
            rep = r["report"]
            assert sim == r["sim"].tobytes() and ri == (rep["iters"], rep["accepted"], rep["termination"], rep["n_inlier"]) and nopt == rep["n_inlier"]
            assert rd == struct.pack("<dd", rep["cost0"], rep["cost1"])
        else:
            assert nopt == -1
    assert off == len(raw)
    assert any(r["ok"] for r in got) and not all(r["ok"] for r in got)

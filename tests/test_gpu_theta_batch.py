"""tsba_theta_optim_batch: optimizer::ThetaOptimMultiFs for the immature planes of one frame (tracking::TextUpdate, tracking.cc:1917-1946) in one
launch -- per plane against the oracle and against tsba_theta_optim, independence of the neighbours, the singular plane, argument errors, the resident
problem of tsba_upload, and the adapter's batch from C++."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest

from textslam_amd import synth, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    from textslam_amd.optimizer import Optimizer
    return Optimizer(0)


@pytest.fixture(scope="module")
def planes():
    return synth.theta_planes(seed=5, n=12)


def _batch(gpu, probs, o=None, cov0=None):
    work = [P.copy() for P in probs]
    reps, covs = gpu.ThetaOptimMultiFsBatch(work, options=o or abi.options_theta(), cov0=cov0)
    return work, reps, covs


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _rep_key(r):
    return tuple((k, tuple(r[k]) if isinstance(r[k], list) else r[k]) for k in sorted(r) if not k.startswith("t_"))


def test_batch_entry_point_declared_exported_and_bound():
    from textslam_amd import optimizer
    hdr = open(os.path.join(ROOT, "include", "tsba.h")).read()
    assert re.search(r"\bint\s+tsba_theta_optim_batch\s*\(void \*ctx, tsba_problem \*const \*probs, int n, const tsba_options \*o,\s*double \*cov, tsba_report \*reps\)", hdr)
    assert "#define TSBA_SOLVER_THETA        9" in hdr
    assert re.search(r"#define TSBA_ABI_VERSION 5\b", hdr)
    assert "tsba_theta_optim_batch" in optimizer.EXPORTED_SYMBOLS
    L = optimizer.load_library()
    assert hasattr(L, "tsba_theta_optim_batch")
    assert L.tsba_theta_optim_batch.argtypes is not None and len(L.tsba_theta_optim_batch.argtypes) == 6
    assert L.tsba_theta_optim_batch.restype is C.c_int


@pytest.mark.gpu
def test_batch_matches_oracle_per_plane(gpu, oracle_lib, planes):
    o = abi.options_theta()
    work, reps, covs = _batch(gpu, planes, o)
    n_two = 0
    for i, P in enumerate(planes):
        R = P.copy()
        rc, rep_o, cov_o = oracle_lib.theta_optim(R, o, 0)
        r = reps[i]
        assert r["status"] == 0 and r["solver_path"] == 9, i
        assert r["iters"] == rep_o["iters"] and r["accepted"] == rep_o["accepted"] and r["termination"] == rep_o["termination"], (i, r, rep_o)
        np.testing.assert_allclose(r["cost0"], rep_o["cost0"], rtol=1e-9)
        np.testing.assert_allclose(r["cost1"], rep_o["cost1"], rtol=1e-9)
        np.testing.assert_allclose(work[i].theta, R.theta, rtol=0, atol=1e-8)
        assert r["cov_valid"] == (1 if rc == 0 else 0)
        if rc == 0:
            np.testing.assert_allclose(covs[i], cov_o, rtol=1e-7)
        n_two += rep_o["accepted"][-1] >= 2
    assert n_two >= len(planes) // 2                      # the set exercises the LM loop at level 0


@pytest.mark.gpu
def test_batch_matches_single_calls(gpu, planes):
    o = abi.options_theta()
    work, reps, covs = _batch(gpu, planes, o)
    for i, P in enumerate(planes):
        G = P.copy()
        rep_s, cov_s = gpu.ThetaOptimMultiFs(G, text=0, options=o)
        r = reps[i]
        assert r["iters"] == rep_s["iters"] and r["accepted"] == rep_s["accepted"] and r["termination"] == rep_s["termination"], (i, r, rep_s)
        assert r["n_tblock"] == rep_s["n_tblock"] and r["n_resid_evals"] == rep_s["n_resid_evals"] and r["n_passes"] == rep_s["n_passes"]
        assert r["cov_valid"] == rep_s["cov_valid"] and r["status"] == rep_s["status"]
        np.testing.assert_allclose(work[i].theta, G.theta, rtol=0, atol=1e-8)
        np.testing.assert_allclose(covs[i], cov_s, rtol=1e-7)
        assert work[i].pose.tobytes() == P.pose.tobytes()  # poses untouched


@pytest.mark.gpu
def test_batch_planes_are_independent_and_deterministic(gpu):
    probs = synth.theta_planes(seed=11, n=16)
    _, reps16, covs16 = _batch(gpu, probs)
    w16, _, _ = _batch(gpu, probs)
    th16 = [P.theta for P in w16]
    wrev, reps_rev, covs_rev = _batch(gpu, probs[::-1])
    wrep, reps_rep, covs_rep = _batch(gpu, probs)
    # images shared by pointer: the second list's problems reuse the first list's image arrays (every plane copied once per call)
    shared = [P.copy() for P in probs]
    twins = []
    for P in shared:
        Q = P.copy()
        Q.img = P.img
        twins.append(Q)
    reps_sh, covs_sh = gpu.ThetaOptimMultiFsBatch(shared + twins, options=abi.options_theta())
    for i, P in enumerate(probs):
        w1, reps1, covs1 = _batch(gpu, [P])
        for th, rep, cov in ((th16[i], reps16[i], covs16[i]), (wrev[15 - i].theta, reps_rev[15 - i], covs_rev[15 - i]),
                             (wrep[i].theta, reps_rep[i], covs_rep[i]), (shared[i].theta, reps_sh[i], covs_sh[i]),
                             (twins[i].theta, reps_sh[16 + i], covs_sh[16 + i])):
            assert _same_bits(th, w1[0].theta), i
            assert _same_bits(cov, covs1[0]), i
            assert _rep_key(rep) == _rep_key(reps1[0]), i


@pytest.mark.gpu
def test_batch_singular_plane(gpu):
    probs = synth.theta_planes(seed=5, n=6, singular=2)
    base = synth.theta_planes(seed=5, n=6)
    prev = np.tile(np.arange(9, dtype=np.float64).reshape(1, 3, 3), (6, 1, 1))
    w, reps, covs = _batch(gpu, probs, cov0=prev)
    assert reps[2]["cov_valid"] == 0 and reps[2]["status"] == 0
    assert _same_bits(covs[2], prev[2])
    others = [i for i in range(6) if i != 2]
    wb, repsb, covsb = _batch(gpu, [base[i] for i in others])
    for k, i in enumerate(others):
        assert reps[i]["cov_valid"] == 1
        assert _same_bits(w[i].theta, wb[k].theta) and _same_bits(covs[i], covsb[k]) and _rep_key(reps[i]) == _rep_key(repsb[k])


def _raw_call(gpu, probs, o, n=None):
    from textslam_amd.abi import TsbaProblem, TsbaReport
    n = len(probs) if n is None else n
    structs = [P.struct() for P in probs]
    keep = [P._keep for P in probs]
    arr = (C.POINTER(TsbaProblem) * max(len(probs), 1))(*[C.pointer(s) for s in structs])
    reps = (TsbaReport * max(len(probs), 1))()
    C.memset(reps, 0x5a, C.sizeof(reps))
    cov = np.full((max(len(probs), 1), 9), 7.0)
    rc = gpu.lib.tsba_theta_optim_batch(gpu.ctx, arr, n, C.byref(o), cov.ctypes.data_as(C.POINTER(C.c_double)), reps)
    del keep
    return rc, bytes(reps), cov


@pytest.mark.gpu
def test_batch_argument_errors(gpu):
    good = synth.theta_planes(seed=7, n=3)
    cases = []
    two = synth.landmark_refine(seed=3, n_pt=0, n_text=2)
    cases.append(("n_text", lambda: [good[0].copy(), two], abi.options_theta()))
    def bad_host():
        P = good[1].copy(); P.text_host = np.array([P.n_kf], np.int32); return [good[0].copy(), P]
    cases.append(("text_host", bad_host, abi.options_theta()))
    def with_points():
        return [good[0].copy(), synth.landmark_refine(seed=3, n_pt=20, n_text=1)]
    cases.append(("n_pt", with_points, abi.options_theta()))
    def free_pose():
        P = good[2].copy(); P.kf_initial = P.kf_initial.copy(); P.kf_initial[-1] = 0; return [good[0].copy(), P]
    cases.append(("kf_initial", free_pose, abi.options_theta()))
    def bad_tobs_text():
        P = good[1].copy(); P.tobs_text = P.tobs_text.copy(); P.tobs_text[0] = 1; return [P]
    cases.append(("tobs_text", bad_tobs_text, abi.options_theta()))
    def missing_level():
        P = good[1].copy(); P.n_levels = 2; return [good[0].copy(), P]
    cases.append(("level", missing_level, abi.options_theta()))
    for name, val in (("use_text", 0), ("filter_good", 1), ("outlier_scene", 1), ("outlier_text", 1)):
        o = abi.options_theta(); setattr(o, name, val)
        cases.append((name, lambda: [g.copy() for g in good], o))
    for name, mk, o in cases:
        probs = mk()
        before = [P.theta.copy() for P in probs]
        rc, reps, cov = _raw_call(gpu, probs, o)
        assert rc == -1, name
        assert all(np.array_equal(P.theta, b) for P, b in zip(probs, before)), name
        assert np.all(cov == 7.0) and reps == b"\x5a"*len(reps), name
        msg = gpu.lib.tsba_last_error(gpu.ctx).decode()
        assert "tsba_theta_optim_batch" in msg, (name, msg)
    rc, reps, cov = _raw_call(gpu, [good[0].copy()], abi.options_theta(), n=0)
    assert rc == 0 and np.all(cov == 7.0) and reps == b"\x5a"*len(reps)


@pytest.mark.gpu
def test_batch_leaves_resident_problem_untouched(gpu):
    P = synth.tiny(seed=21, n_kf=5, n_pt=60, n_text=4)
    o = abi.options_local()
    gpu.upload(P, o)
    r1 = gpu.solve(); A = gpu.download(P.copy())
    gpu.upload(P, o)
    _batch(gpu, synth.theta_planes(seed=5, n=5))
    r2 = gpu.solve(); B = gpu.download(P.copy())
    assert _same_bits(A.pose, B.pose) and _same_bits(A.rho, B.rho) and _same_bits(A.theta, B.theta)
    assert _rep_key(r1) == _rep_key(r2)


@pytest.mark.gpu
def test_adapter_batch_from_cxx(tmp_path):
    exe = str(tmp_path / "theta_batch_from_cxx")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "adapter"),
                           "-I" + os.path.join(ROOT, "tests", "cxx"), "-o", exe, os.path.join(ROOT, "tests", "cxx", "theta_batch_from_cxx.cpp"),
                           "-L" + os.path.join(ROOT, "textslam_amd"), "-ltsba", "-L/opt/rocm/lib",
                           "-Wl,-rpath," + os.path.join(ROOT, "textslam_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    dumps = []
    for i, P in enumerate(synth.theta_planes(seed=13, n=5)):
        path = str(tmp_path / f"plane{i}.bin")
        abi.write_dump(path, P, abi.STATE_NOTREACHWIN)
        dumps.append(path)
    out = subprocess.run([exe] + dumps, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "theta batch from C++: ok" in out.stdout, out.stdout

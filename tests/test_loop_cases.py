"""CPU guard of tests/loop_cases.py: every case of the table satisfies the admission rule (stable under one-rounding changes of the oracle's fp64 inputs,
parameter spread <= 1e-6) and does what its name says -- the padded system size and the solver it selects, the log-map branch, the exit code, a rejected
step, the connections of a pair -- asserted from the CPU oracle and from plain arithmetic.  The GPU runs of these cases are tests/test_gpu_loop_shapes.py."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_cases as LC  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built(oracle_lib):
    return oracle_lib


def n_free_of(d):
    return int((d["fixed"] == 0).sum())


def test_solver_size_rule():
    """The arithmetic of solve_lds_doubles (restated in loop_cases.py; it mirrors textslam_amd/csrc/tsba_solve.h): 192 unknowns -- 27 free keyframes, 32
    solver blocks -- are the last system the one-workgroup LDS solver takes, 198 = 96 + 96 + 6 the first the blocked Cholesky takes."""
    assert LC.rowoff(0) == 0 and LC.rowoff(1) == 2 and LC.rowoff(2) == 4 and LC.rowoff(3) == 8                     # rows padded to an even length
    assert all(LC.solver_of(n) == "lds" for n in range(6, 193, 6)) and all(LC.solver_of(n) == "chol" for n in range(198, 2400, 6))
    assert LC.solve_lds_doubles(192)*8 == 163600 and LC.solve_lds_doubles(198)*8 == 173440
    assert LC.padded_size(27) == 192 and 192//6 == 32 and LC.padded_size(28) == 198 == 2*LC.CH_NB + 6 and LC.padded_size(41) == 288 == 3*LC.CH_NB
    assert LC.padded_size(12 - 3) == 66                                                                            # the one size the suite ran before
    # every path of the row loader of solve_body<false, false> has a size in the table: n <= 70 | 70 < n <= 109 | 109 < n <= 122 | 122 < n <= 134 | beyond
    sizes = sorted({LC.padded_size(nf) for nf in LC.SHAPES if LC.solver_of(LC.padded_size(nf)) == "lds"})
    for lo, hi in ((0, 70), (70, 109), (109, 122), (122, 134), (134, 192)):
        assert any(lo < n <= hi for n in sizes), (lo, hi, sizes)
    assert sizes[-1] == 192 and [LC.padded_size(nf) for nf in LC.SHAPES] == [12, 18, 36, 42, 78, 114, 126, 144, 192, 198, 288, 1800]


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.name)
def test_case_is_admitted(case):
    s = LC.oracle_sensitivity(case)
    print("%s: stable %s, spread x %.3e cost1 %.3e, report %s" % (case.name, s["stable"], s["spread"]["x"], s["spread"]["cost1"], s["base"]["ints"]))
    assert s["stable"], s["runs"]
    assert s["spread"]["x"] <= LC.ADMIT_SPREAD
    assert len(s["runs"]) == (4 if case.kind == "pg" and 7*n_free_of(LC.inputs_of(case)) > 1000 else 8)


def test_left_out_cases_fail_the_rule():
    s = LC.oracle_sensitivity(LC.REJECTED)
    assert not s["stable"] and len(set(s["runs"])) > 2               # the report changes with the last bit of the inputs
    s = LC.oracle_sensitivity(LC.FULL28)
    assert s["stable"] and s["base"]["ints"] == (5, 4, 1) and s["spread"]["x"] > LC.ADMIT_SPREAD
    assert all(c.name not in LC.BY_NAME for c in LC.LEFT_OUT)


@pytest.mark.parametrize("case", LC.CASES, ids=lambda c: c.name)
def test_case_does_what_it_says(case):
    d, cl, base = LC.inputs_of(case), case.claims, LC.oracle_sensitivity(case)["base"]
    rep = base["rep"]
    for key in ("iters", "accepted", "termination"):
        if key in cl:
            assert rep[key] == cl[key], (key, rep)
    if case.kind == "pg":
        nf = n_free_of(d)
        assert nf >= 1 and len(d["edge_i"]) == len(d["edge_j"]) == len(d["meas"]) >= 1 and np.all(d["edge_i"] != d["edge_j"])
        n6 = LC.padded_size(nf)
        if "n_free" in cl:
            assert nf == cl["n_free"]
        if "n6" in cl:
            assert n6 == cl["n6"] and LC.solver_of(n6) == cl["solver"]
        if "padding" in cl:
            assert (n6 > 7*nf) == cl["padding"]
        if case.opts.get("max_it") == 1 and "accepted" not in cl:
            assert (rep["iters"], rep["accepted"]) == (1, 1) and np.abs(base["x"] - d["pose"]).max() > 1e-4          # a real step was taken
        if cl.get("accepted") == 0:                                  # a rejected step: the oracle hands the pose back as it went in
            assert rep["accepted"] < rep["iters"] and np.array_equal(base["x"], d["pose"]) and rep["cost1"] == rep["cost0"]
        if "branch" in cl:                                           # from the oracle's residual: res[:3] = omega, res[6] = sigma
            import oracle
            r, _, _ = oracle.pg_eval(d["pose"][0], d["pose"][1], d["meas"][0])
            w = float(np.linalg.norm(r[:3]))
            small_sigma = abs(r[6]) < 1e-5
            small_angle = w < 0.01 and np.sqrt(1 - w*w) > 1 - 1e-5   # that branch returns sin(theta) axis; the other theta axis
            if not small_angle:
                assert np.cos(w) <= 1 - 1e-5
            assert (int(small_sigma) | (int(small_angle) << 1)) == cl["branch"] == int(LC.edges()["branch"][LC.edge_index(case.name[8:-4])])
        fidx = np.cumsum(d["fixed"] == 0) - 1
        pairs, inc = {}, np.zeros(len(d["fixed"]), int)
        for a, b in zip(d["edge_i"], d["edge_j"]):
            inc[a] += 1; inc[b] += 1
            if not d["fixed"][a] and not d["fixed"][b]:
                key = (max(fidx[a], fidx[b]), min(fidx[a], fidx[b])); pairs[key] = pairs.get(key, 0) + 1
        if "pair_conn" in cl:
            assert max(pairs.values()) == cl["pair_conn"] > 2 and pairs[(fidx[4], fidx[3])] == cl["pair_conn"]
            assert sorted(pairs.values())[-2] == 3                   # the generator alone: two directions and, for 4 - 7, one loop connection
        if "leaf" in cl:
            import oracle
            r, _, _ = oracle.pg_eval(d["pose"][d["edge_i"][-1]], d["pose"][cl["leaf"]], d["meas"][-1])
            assert inc[cl["leaf"]] == 1 and d["edge_j"][-1] == cl["leaf"] and not d["fixed"][cl["leaf"]] and np.abs(r).max() > 1e-3    # and it pulls
        if cl.get("fixed_last"):
            assert d["fixed"][-1] and d["fixed"][5] and not d["fixed"][4] and not d["fixed"][6]
        if "n_edge" in cl:
            assert len(d["edge_i"]) == cl["n_edge"] > 1024 and cl["n_edge"] % 64 != 0
        if nf == 257:
            assert nf > 256                                          # k_pg_candidate: 256 keyframes per workgroup
        fx = d["fixed"].astype(bool)
        assert np.array_equal(base["x"][fx], d["pose"][fx])
    else:
        n = len(d["P1"])
        assert n == cl["n"] and d["uv1"].dtype == d["uv2"].dtype == np.float32
        if "active" in cl:
            assert int(d["inliers"].sum()) == cl["active"]
            if case.name.endswith("idle_wave"):
                assert not d["inliers"][64:128].any() and d["inliers"][:64].all() and d["inliers"][128:].all()
            if case.name.endswith("one_wave"):
                assert d["inliers"][256:320].all()
        if case.name.startswith("sim3_start"):
            assert rep["termination"] == 1 and np.abs(base["x"][4:] - d["sim0"][4:]).max() > 0.2                    # found its way back from afar

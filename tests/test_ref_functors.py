"""The CPU oracle against TextSLAM's OWN cost functors (not marked gpu).

oracle/_ref/libtsref.so holds the twelve functors of the reference tree's include/ directory, compiled unchanged against the stand-in
headers of oracle/ref_shims/ (oracle/Makefile; built only where the reference tree is present).  tests/golden/ref_functors.npz records what
they return on the cases of tests/golden/make_ref_functors.py.  Here:
  * the fixture is fresh: the compiled functors return exactly the recorded values (skipped only without the library);
  * the oracle's residuals (tsba_oracle_eval, sim3_eval, pg_eval) equal the recorded ones, family by family;
  * the oracle's tangent-space Jacobians of the scene and Sim3 blocks equal (Jet Jacobian) x (plus-Jacobian).

TOL: per family, ten times the worst deviation measured between oracle and reference on these cases (MEASURED below; the margin covers
another summation order).  The same figures are listed in oracle/RECALLED.md.  Deviation of residuals: max |a - b| / max(1, |b|); of
Jacobians: max |a - b| / max |b| over the family's blocks of one level.
A family whose measured deviation is exactly 0 is asserted EQUAL, bit for bit: there the oracle repeats the functor's operations in the
functor's order under -ffp-contract=off, so both round alike, and ten times nothing is nothing.  Should another compiler ever break that
equality, the figure to put here is the one it measures, not a floor chosen in advance."""
import os
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ref_functors as gen  # noqa: E402

# family -> the worst deviation between oracle and reference measured on the fixture's cases (python tests/test_ref_functors.py prints them;
# rounded up to two digits; the same list is in oracle/RECALLED.md)
MEASURED = {
    # residuals of the BA functors, by the functor that owns the block
    "auto_BAScene": 0.0, "auto_BASceneNW": 0.0, "auto_PoseOptimScene": 4.8e-14, "auto_IniBAScene": 0.0, "auto_RhoScene": 5.7e-14,
    "nume_BAText": 6.5e-13, "nume_PoseOptimText": 0.0, "nume_IniBAText": 0.0, "nume_thetaText": 0.0,
    # Jet Jacobian x plus-Jacobian against the oracle's tangent-space Jacobian
    "jac/auto_BAScene": 9.3e-16, "jac/auto_BASceneNW": 1.1e-15, "jac/auto_PoseOptimScene": 5.7e-16, "jac/auto_IniBAScene": 5.9e-16, "jac/auto_RhoScene": 5.2e-15,
    "auto_sim": 2.2e-13, "auto_siminv": 1.2e-13, "jac/auto_sim": 1.2e-15, "jac/auto_siminv": 6.7e-16,
    # numer_loop_ver2 / logSim3, per branch of logSim3.  small_angle (|log s| >= 1e-5, d > 1 - 1e-5) is where the reference's B ~ 1/sigma^3 makes
    # W ill-conditioned (tests/golden/make_ref_functors.py::device_samples); small_sigma holds the angles next to pi, where omega amplifies a
    # rounding of d by 1/(pi - theta)^2 = 1e6.  "device": the well-conditioned connections the device tests use.
    "numer_loop_ver2/generic": 2.6e-13, "numer_loop_ver2/small_sigma": 1.6e-9, "numer_loop_ver2/small_angle": 6.8e-8, "numer_loop_ver2/both": 3.4e-16,
    "numer_loop_ver2/device": 1.6e-11,
    "logSim3/generic": 4.2e-16, "logSim3/small_sigma": 4.3e-16, "logSim3/small_angle": 7.3e-8, "logSim3/both": 0.0,
    "TextProj/p": 5.1e-16, "TextProj/uv": 1.1e-14,      # the reference against the formula in extended precision
}


TOL = {k: 10*v for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def fix():
    return gen.load()


def dev_res(a, b, atol=0.0):
    """Deviation of residuals a from b: max (|a - b| - atol) / max(1, |b|)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max((np.abs(a - b) - atol)/np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def dev_jac(a, b, rel=0.0):
    """Deviation of Jacobians a from b: max |a - b| / max |b|, less rel."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (float(np.max(np.abs(a - b))/max(np.max(np.abs(b)), 1e-300)) if a.size else 0.0) - rel


def put(d, k, v):
    d[k] = max(d.get(k, 0.0), v)


class Tally:
    """Per family: dev, the worst deviation counted against TOL (after atol / rel were taken off), raw, the worst plain figure (absolute
    residual difference, relative Jacobian difference), and cnt, the number of blocks."""

    def __init__(self, atol=0.0, rel=0.0):
        self.atol, self.rel, self.dev, self.raw, self.cnt = atol, rel, {}, {}, {}

    def res(self, fam, a, b):
        put(self.dev, fam, dev_res(a, b, self.atol))
        put(self.raw, fam, float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if len(a) else 0.0)
        self.cnt[fam] = self.cnt.get(fam, 0) + len(a)

    def jac(self, fam, a, b):
        put(self.dev, "jac/" + fam, dev_jac(a, b, self.rel)); put(self.raw, "jac/" + fam, dev_jac(a, b))


def ba_deviations(oracle, fix, evaluate=None, cases=None, atol=0.0, rel=0.0):
    """A Tally of `evaluate(P, o, level)` (default: the CPU oracle) against the recorded reference values over every BA case and level.
    atol / rel (the device tests): what is taken off a residual's absolute difference / a Jacobian's relative difference before it counts,
    i.e. a tolerance ADDED to the family's bound."""
    evaluate = evaluate or oracle.evaluate
    t = Tally(atol, rel)
    for name in cases or gen.BA_CASES:
        P, o, levels = gen.ba_case(name)
        assert np.array_equal(gen.digest(P), fix[f"ba/{name}/digest"]), name + ": the synthetic problem is not the recorded one"
        unit = o.w_sx == 1.0 and o.w_sy == 1.0
        for l in levels:
            f = gen.ba_level(fix, name, l)
            ev = evaluate(P, o, l)
            assert (ev["ns"], ev["nt"]) == (f["ns"], f["nt"]), (name, l)
            sc, tx = oracle.ba_blocks(P, o, l); ns = f["ns"]
            rs, rt = ev["resid"][:2*ns].reshape(-1, 2), ev["resid"][2*ns:].reshape(-1, 8)
            fs, ft = f["resid"][:2*ns].reshape(-1, 2), f["resid"][2*ns:].reshape(-1, 8)
            if ns:
                frozen = np.asarray(P.pt_host)[sc[:, 1]] < 0
                Jt = oracle.scene_tangent(f["jac_scene"], P, sc)
                for fam, m in (("auto_BASceneNW" if unit else "auto_BAScene", ~frozen), ("auto_PoseOptimScene", frozen)):
                    if m.any():
                        t.res(fam, rs[m], fs[m]); t.jac(fam, ev["jac_scene"][m], Jt[m])
                if "resid_ini" in f:
                    i = f["idx_ini"]; pose = np.asarray(P.pose).reshape(-1, 7)
                    Ji = np.zeros((len(i), 2, 7))
                    for n_, b in enumerate(i):
                        Ji[n_, :, :3] = f["jac_ini"][n_, :, :4] @ oracle.quat_plus_jacobian(pose[sc[b, 0], :4]); Ji[n_, :, 3:6] = f["jac_ini"][n_, :, 4:7]; Ji[n_, :, 6] = f["jac_ini"][n_, :, 7]
                    t.res("auto_IniBAScene", rs[i], f["resid_ini"]); t.jac("auto_IniBAScene", ev["jac_scene"][i][:, :, [0, 1, 2, 3, 4, 5, 12]], Ji)
                if "resid_rho" in f:
                    i = f["idx_rho"]
                    t.res("auto_RhoScene", rs[i], f["resid_rho"]); t.jac("auto_RhoScene", ev["jac_scene"][i][:, :, 12:13], f["jac_rho"])
            if f["nt"]:
                frozen = np.asarray(P.text_host)[tx[:, 1]] < 0
                for fam, m in (("nume_BAText", ~frozen), ("nume_PoseOptimText", frozen)):
                    if m.any():
                        t.res(fam, rt[m], ft[m])
                for fam, key in (("nume_IniBAText", "ini_text"), ("nume_thetaText", "theta_text")):
                    if "resid_" + key in f:
                        t.res(fam, rt[f["idx_" + key]], f["resid_" + key])
    return t


def sim_deviations(oracle, fix):
    dev = {}
    g = lambda k: fix["sim/cpu200/" + k]
    x, n = g("x"), len(g("P1")); per = n//len(x)
    for i in range(n):
        xi = x[i//per]
        r, J = oracle.sim3_eval(xi, g("P1")[i], g("P2")[i], g("uv1")[i], g("uv2")[i], g("K"))
        Jf = np.zeros((4, 7)); Jf[:, :3] = g("jac")[i][:, :4] @ oracle.quat_plus_jacobian(xi[:4]); Jf[:, 3:] = g("jac")[i][:, 4:]
        put(dev, "auto_sim", dev_res(r[:2], g("res")[i, :2])); put(dev, "auto_siminv", dev_res(r[2:], g("res")[i, 2:]))
        put(dev, "jac/auto_sim", dev_jac(J[:2], Jf[:2])); put(dev, "jac/auto_siminv", dev_jac(J[2:], Jf[2:]))
    return dev


def loop_deviations(oracle, fix):
    dev = {}
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])
    for b in gen.LOOP_BRANCHES:
        e = {k: np.asarray(fix[f"loop/{b}/{k}"], np.float64) for k in ("meas", "x1", "x2", "res")}
        r = np.array([oracle.pg_eval(e["x1"][i], e["x2"][i], e["meas"][i])[0] for i in range(len(e["meas"]))])
        put(dev, "numer_loop_ver2/" + b, dev_res(r, e["res"]))
        D = np.concatenate([fix[f"logsim3/{b}/q"], fix[f"logsim3/{b}/t"], fix[f"logsim3/{b}/s"][:, None]], axis=1)
        r = np.array([oracle.pg_eval(ident, ident, D[i])[0] for i in range(len(D))])         # S21 o I o I^-1: logSim3 of the measurement itself, exactly
        put(dev, "logSim3/" + b, dev_res(r, fix[f"logsim3/{b}/res"]))
        e = {k: np.asarray(fix[f"loop15/{b}/{k}"], np.float64) for k in ("meas", "x1", "x2", "res")}                 # the device tests' connections
        r = np.array([oracle.pg_eval(e["x1"][i], e["x2"][i], e["meas"][i])[0] for i in range(len(e["meas"]))])
        put(dev, "numer_loop_ver2/device", dev_res(r, e["res"]))
    g = {k: fix["graph12/" + k] for k in ("pose", "edge_i", "edge_j", "meas", "res")}
    r = np.array([oracle.pg_eval(g["pose"][i], g["pose"][j], m)[0] for i, j, m in zip(g["edge_i"], g["edge_j"], g["meas"])])
    put(dev, "numer_loop_ver2/device", dev_res(r, g["res"]))
    return dev


def report(dev, cnt=None):
    for k in sorted(dev):
        print(f"  {k:32s} deviation {dev[k]:.3e}  bound {TOL.get(k, float('nan')):.3e}" + (f"  ({cnt[k]} blocks)" if cnt and k in cnt else ""))


def check(dev):
    bad = {k: (v, TOL[k]) for k, v in dev.items() if not v <= TOL[k]}
    assert not bad, bad


def test_fixture_is_fresh(oracle_lib, fix):
    """The recorded values ARE what the compiled functors return: a fresh evaluation of every case equals the fixture bit for bit, and the
    cases still meet what was demanded of them (finite values, branches as named, no residual within 1e-6 of the inlier threshold)."""
    if oracle_lib.ref_lib() is None:
        pytest.skip("oracle/_ref/libtsref.so was not built: no reference tree at build time")
    fresh = gen.reference_outputs(oracle_lib, fix)
    assert fresh, "nothing evaluated"
    for k, v in fresh.items():
        assert k in fix and v.dtype == fix[k].dtype and np.array_equal(v, fix[k]), k
    inputs = gen.compute()
    assert list(inputs) == list(fix)
    for k in fix:
        if k not in fresh and fix[k].dtype.kind != "f":
            assert np.array_equal(inputs[k], fix[k]), k
    gen.check_cases(fix)


def test_fixture_cases_are_the_demanded_ones(oracle_lib, fix):
    """Readable without the reference: every branch of logSim3 holds 200 connections on its side of both thresholds and 1e-3 clear of them, angles
    from 1e-9 to pi - 1e-3; the Sim3 set has unnormalised quaternions, scales 0.5 and 2, float32 pixels and a point of small positive depth; pixel_grid has text blocks of a frozen host."""
    gen.check_cases(fix)
    for b in gen.LOOP_BRANCHES:
        assert len(fix[f"loop/{b}/res"]) == 200 and len(fix[f"logsim3/{b}/res"]) == 200
    ang = np.arccos(np.clip(np.concatenate([fix[f"logsim3/{b}/d"] for b in gen.LOOP_BRANCHES]), -1, 1))
    assert ang.max() > np.pi - 1.1e-3 and ang.max() <= np.pi - 0.99e-3 and np.linalg.norm(fix["logsim3/both/res"][:, :3], axis=1).min() < 2e-9
    x = fix["sim/cpu200/x"]
    assert len(fix["sim/cpu200/P1"]) == 200 and np.abs(np.linalg.norm(x[:, :4], axis=1) - 1).min() > 0.05 and x[:, 7].min() < 0.51 and x[:, 7].max() > 1.99
    assert fix["sim/cpu200/uv1"].dtype == np.float32
    z = x[0, 7]*(gen.q_R(x[0, :4]) @ fix["sim/cpu200/P2"][0]) + x[0, 4:7]          # match 0 after the transform auto_sim applies: s R P2 + t
    assert 0.0 < z[2] < 0.1, z
    P, o, levels = gen.ba_case("pixel_grid")                                      # its frozen-host plane gives nume_PoseOptimText blocks at every level
    for l in levels:
        tx = np.asarray(P.text_host)[oracle_lib.ba_blocks(P, o, l)[1][:, 1]]
        assert (tx < 0).any() and (tx >= 0).any(), l
    for n in ("n9", "n300", "n257"):
        assert 0 < fix[f"sim/{n}/inlier"].sum() < len(fix[f"sim/{n}/inlier"])


def test_oracle_ba_functors_against_reference(oracle_lib, fix):
    """tsba_oracle_eval against the reference functors on every BA case and pyramid level, block by block and family by family: residuals,
    and the tangent-space Jacobian of the scene blocks against (Jet Jacobian) x (plus-Jacobian).  The plus-Jacobian is the oracle's own
    restatement of ceres::QuaternionParameterization::ComputeJacobian -- row C11 of oracle/RECALLED.md, which this test does NOT pin: it is
    still recalled.  Every one of the nine BA families must have blocks."""
    t = ba_deviations(oracle_lib, fix)
    dev, cnt = t.dev, t.cnt
    report(dev, cnt)
    for fam in ("auto_BAScene", "auto_BASceneNW", "auto_PoseOptimScene", "auto_IniBAScene", "auto_RhoScene", "nume_BAText", "nume_PoseOptimText", "nume_IniBAText", "nume_thetaText"):
        assert cnt.get(fam, 0) > 0, fam
    check(dev)


def test_pixel_grid_taps_are_where_they_were_put(oracle_lib, fix):
    """The pixel_grid case does what it was built for, judged on the reference's values: taps at exact integers on the last column / row are
    read (residual = (I - mu)/sigma - ref with I the pixel itself), taps one pixel beyond give intensity 0, and the planes seen in the
    constant image (sigma == 0) have all-zero residuals."""
    P, o, levels = gen.ba_case("pixel_grid")
    seen_edge = seen_out = seen_flat = 0
    for l in levels:
        f = gen.ba_level(fix, "pixel_grid", l)
        sc, tx = oracle_lib.ba_blocks(P, o, l)
        rt = f["resid"][2*f["ns"]:].reshape(-1, 8)
        h, w = P.img[l].shape[1:]
        for b, (kf, j, fi, t) in enumerate(tx):
            mu, sg = f["musigma"][t]
            if sg == 0:
                assert np.all(rt[b] == 0); seen_flat += 1
                continue
            u0, v0 = P.tfeat_uv[l][fi]
            for k in range(8):
                u, v = int(u0 + oracle_lib.TAP_DX[k]), int(v0 + oracle_lib.TAP_DY[k])
                inside = 0 <= u < w and 0 <= v < h
                I = float(P.img[l][kf][v, u]) if inside else 0.0
                assert rt[b, k] == ((I - mu)/sg - P.tfeat_ref[l][fi][k])*o.w_t, (l, b, k)
                seen_edge += inside and (u == w - 1 or v == h - 1); seen_out += (u == w or v == h)
    assert seen_edge > 0 and seen_out > 0 and seen_flat > 0


def test_oracle_sim3_functors_against_reference(oracle_lib, fix):
    """oracle.sim3_eval against auto_sim / auto_siminv on 200 matches (unnormalised quaternions, scales 0.5 ... 2, float32 pixels, one point
    of small positive depth): residuals, and the 7-column tangent Jacobian against (Jet Jacobian) x (the oracle's plus-Jacobian, RECALLED C11,
    still recalled)."""
    dev = sim_deviations(oracle_lib, fix)
    report(dev); check(dev)


def test_oracle_pose_graph_against_reference(oracle_lib, fix):
    """oracle.pg_eval against numer_loop_ver2, and its log map against logSim3, 200 connections in each of logSim3's four branches."""
    dev = loop_deviations(oracle_lib, fix)
    report(dev); check(dev)


def test_textproj_against_extended_precision(fix):
    """The reference's TextProj (both overloads) against the same formula in extended precision: p = R ray / rho + t with rho = -ray . theta,
    then the pinhole projection -- the sign of rho and the composition of T_cr are what this pins."""
    L = np.longdouble
    ray, T, th, K = (fix["textproj/" + k].astype(L) for k in ("ray", "Tcr", "theta", "K"))
    T = T.reshape(-1, 4, 4)
    rho = -(ray*th).sum(axis=1)
    p = np.stack([(T[:, i, :3]*ray).sum(axis=1)/rho + T[:, i, 3] for i in range(3)], axis=1)
    uv = np.stack([K[0, 0]*p[:, 0]/p[:, 2] + K[0, 2], K[1, 1]*p[:, 1]/p[:, 2] + K[1, 2]], axis=1)
    dev = {"TextProj/p": dev_res(fix["textproj/p"], p.astype(np.float64)), "TextProj/uv": dev_res(fix["textproj/uv"], uv.astype(np.float64))}
    report(dev); check(dev)


if __name__ == "__main__":
    import oracle
    f = gen.load()
    t = ba_deviations(oracle, f); report(t.dev, t.cnt)
    report(sim_deviations(oracle, f)); report(loop_deviations(oracle, f))

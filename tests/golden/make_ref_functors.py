"""Generates tests/golden/ref_functors.npz: what TextSLAM's own cost functors return on the cases below.

Run it where the reference tree was present at build time (oracle/Makefile builds oracle/_ref/libtsref.so from the tree's functor
headers against the stand-in headers of oracle/ref_shims/):  python tests/golden/make_ref_functors.py
The file holds the inputs of every case (for the synthetic BA problems: the generator's name, the parameters and a digest of all
its arrays) and the functors' residuals and Jet Jacobians -- nothing else.  tests/test_ref_functors.py checks that it is fresh and
compares the CPU oracle with it; tests/test_gpu_ref_functors.py compares the device with it, without the reference.

compute() builds everything; the cases are fixed here, by construction and by seed, never by what any implementation returns.
Every value is asserted finite."""
import hashlib
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from textslam_amd import synth, abi  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_functors.npz")
BA_CASES = ["tiny3", "tiny11", "border", "init_pair", "landmark_refine", "c3small", "init_identity", "pixel_grid"]
LOOP_BRANCHES = ["generic", "small_sigma", "small_angle", "both"]
SIM_SETS = {"cpu200": 200, "n9": 9, "n300": 300, "n257": 257}
EPS = 1e-5                                   # logSim3's two thresholds: |log s| < EPS, d > 1 - EPS


class Fixture(dict):
    """name -> array; .files as an npz has."""
    @property
    def files(self):
        return list(self.keys())


# ------------------------------------------------------------------------------------------------ BA problems
def ba_case(name):
    """-> (problem, options, levels).  The first five are the problems of tests/test_oracle.py::rule_case."""
    if name.startswith("tiny"):
        return synth.tiny(seed=int(name[4:])), abi.options_local(), (0, 1, 2)
    if name == "border":
        return synth.border_variant(), abi.options_local(), (0, 1, 2)
    if name == "init_pair":
        return synth.init_pair(seed=5), abi.options_init(), (0, 1, 2, 3)
    if name == "landmark_refine":
        return synth.landmark_refine(seed=9), abi.options_landmarker(), (0, 1, 2, 3)
    if name == "c3small":       # a pose problem of config_c3's kind: one frame, every landmark frozen, 50 points and 2 planes
        return synth.make_problem(1, 50, 2, 5, feats=(8, 6, 4), frozen_frac=1.0, n_out=2, max_targets=1, text_targets=1), abi.options_pose(), (0, 1, 2)
    if name == "init_identity":  # InitBA as the reference runs it: the host keyframe AT the identity, so that auto_IniBAScene / nume_IniBAText apply
        P = synth.init_pair(seed=6, n_pt=60, n_text=2)
        pose = np.array(P.pose, np.float64).reshape(-1, 7); pose[0] = [1, 0, 0, 0, 0, 0, 0]; P.pose = np.ascontiguousarray(pose.reshape(np.shape(P.pose)))
        return P, abi.options_init(), (0, 1, 2, 3)
    if name == "pixel_grid":
        return pixel_grid(), abi.options_local(), (0, 1, 2)
    raise KeyError(name)


def pixel_grid():
    """Text taps at EXACT integer pixels, on the image's last column / row and one pixel outside it.
    tiny(seed=3) with every pose at the identity (T_cr = I exactly), every plane theta = (0, 0, -1/2) (rho = 1/2 exactly) and
    K = (256, 256, 320, 240): a tap ray ((u + dx - cx)/fx, (v + dy - cy)/fy, 1) then projects to (u + dx, v + dy) with no rounding at any
    level (all of it is exact binary arithmetic).  Feature centres cycle through corners of the level image: (w-3, h-3) puts the dx = +2
    tap on the last column and the dy = +2 tap on the last row; (w-2, h-2) puts them at x = w / y = h (the `uc >= stride` rule: intensity 0);
    (2, 2) and (1, 1) do the same at the first column / row and at -1; then interior pixels.  Plane 2 has a frozen host (its T_wr = I):
    nume_PoseOptimText.  Keyframe 3's images are constant, so the planes it observes have sigma == 0 there: every residual is 0."""
    P = synth.tiny(seed=3)
    P.K = np.array([256.0, 256.0, 320.0, 240.0])
    pose = np.zeros((P.n_kf, 7)); pose[:, 0] = 1.0; P.pose = np.ascontiguousarray(pose.reshape(np.shape(P.pose)))
    th = np.zeros((P.n_text, 3)); th[:, 2] = -0.5; P.theta = np.ascontiguousarray(th.reshape(np.shape(P.theta)))
    eye = np.eye(4)[:3].reshape(-1)
    P.text_host_Twr = np.ascontiguousarray(np.tile(eye, (P.n_text, 1)).reshape(np.shape(P.text_host_Twr)))
    P.pt_host_Trw = np.ascontiguousarray(np.tile(eye, (P.n_pt, 1)).reshape(np.shape(P.pt_host_Trw)))
    quad = np.array([[200.0, 150.0], [440.0, 150.0], [440.0, 330.0], [200.0, 330.0]])
    box = np.tile(((quad - P.K[2:])/P.K[:2])[None], (P.n_text, 1, 1))
    P.text_box_ray = np.ascontiguousarray(box.reshape(np.shape(P.text_box_ray)))
    rng = np.random.default_rng(31)
    for l in range(P.n_levels):
        P.img[l] = np.array(P.img[l], np.uint8)
        P.img[l][3] = 128
        h, w = P.img[l].shape[1:]
        n = len(P.tfeat_uv[l]); uv = np.zeros((n, 2))
        corners = [(w - 3, h - 3), (w - 2, h - 2), (2, 2), (1, 1), (w - 3, 2), (2, h - 2)]
        for i in range(n):
            uv[i] = corners[i % 12] if i % 12 < len(corners) else (rng.integers(3, w - 3), rng.integers(3, h - 3))
        P.tfeat_uv[l] = np.ascontiguousarray(uv)
    return P.normalise()


def digest(P):
    h = hashlib.sha256()
    arrs = [P.K, P.pose, P.rho, P.theta, P.pt_ray, P.pt_host, P.pt_host_Trw, P.text_host, P.text_host_Twr, P.text_box_ray, P.kf_initial, P.sgood, P.tobs_kf,
            P.tobs_text, P.tobs_good, P.tobs_fgood_off, P.tfgood]
    for l in range(P.n_levels):
        arrs += [P.sobs_kf[l], P.sobs_pt[l], P.sobs_flag[l], P.sobs_uv0[l], P.tfeat_off[l], P.tfeat_raw[l], P.tfeat_uv[l], P.tfeat_ref[l]]
        if P.img[l] is not None:
            arrs.append(P.img[l])
    for a in arrs:
        a = np.ascontiguousarray(a); h.update(str(a.dtype).encode()); h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def compute_ba(oracle, out):
    for name in BA_CASES:
        P, o, levels = ba_case(name)
        out[f"ba/{name}/digest"] = digest(P)
        out[f"ba/{name}/pose"], out[f"ba/{name}/rho"], out[f"ba/{name}/theta"] = (np.array(v, np.float64).reshape(-1) for v in (P.pose, P.rho, P.theta))
        pairs, jacs = {}, []
        for l in levels:
            ms = oracle.evaluate(P, o, l, jac=False)["musigma"]         # mu / sigma are inputs of the text functors (tool::CalTextinfo, not a functor)
            ev = oracle.ref_ba_eval(P, o, l, ms)
            out[f"ba/{name}/L{l}/musigma"] = ms
            # a scene functor's Jacobian does not depend on the observed pixel, and the levels observe the same (keyframe, point) pairs:
            # one Jacobian per pair and problem, an index per block and level (checked bit for bit here)
            idx = np.zeros(ev["ns"], np.int32)
            for i, (kf, pt, _) in enumerate(ev["scene_blocks"]):
                key = (int(kf), int(pt))
                if key not in pairs:
                    pairs[key] = len(jacs); jacs.append(ev["jac_scene"][i])
                assert np.array_equal(jacs[pairs[key]], ev["jac_scene"][i]), (name, l, key)
                idx[i] = pairs[key]
            out[f"ba/{name}/L{l}/jac_scene_idx"] = idx
            for k, v in ev.items():
                if k in ("ns", "nt", "scene_blocks", "text_blocks", "jac_scene"):
                    continue
                out[f"ba/{name}/L{l}/{k}"] = np.asarray(v)
            out[f"ba/{name}/L{l}/nblk"] = np.array([ev["ns"], ev["nt"]], np.int64)
        out[f"ba/{name}/jac_scene_pairs"] = np.array(jacs, np.float64).reshape(-1, 2, 15)


def ba_level(fix, name, l):
    """One level of one BA case out of the loaded fixture -> dict(ns, nt, resid, jac_scene [ns,2,15], musigma, and the other families' values)."""
    pre = f"ba/{name}/L{l}/"
    d = {k[len(pre):]: fix[k] for k in fix.files if k.startswith(pre)}
    d["ns"], d["nt"] = (int(v) for v in d.pop("nblk"))
    d["jac_scene"] = fix[f"ba/{name}/jac_scene_pairs"][d.pop("jac_scene_idx")].reshape(-1, 2, 15)
    return d


# ------------------------------------------------------------------------------------------------ Sim3 algebra (numpy, inputs only)
def q_mul(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def q_R(q):
    w, x, y, z = q/np.linalg.norm(q)
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)], [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)], [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]])


def sim_mul(A, B):
    """(q | t | s) of A o B, x -> s_A R_A (s_B R_B x + t_B) + t_A."""
    return np.concatenate([q_mul(A[:4]/np.linalg.norm(A[:4]), B[:4]/np.linalg.norm(B[:4])), A[7]*(q_R(A[:4]) @ B[4:7]) + A[4:7], [A[7]*B[7]]])


def sim_inv(A):
    q = A[:4]/np.linalg.norm(A[:4]); qi = np.array([q[0], -q[1], -q[2], -q[3]])
    return np.concatenate([qi, -(q_R(qi) @ A[4:7])/A[7], [1.0/A[7]]])


def q_axis_angle(axis, ang):
    axis = axis/np.linalg.norm(axis)
    return np.concatenate([[np.cos(ang/2)], np.sin(ang/2)*axis])


def branch_samples(branch, n, rng):
    """(angle, log-scale) of the residual transform handed to logSim3, n of them, for one of its four branches.
    Thresholds: |sigma| < EPS and d = cos(angle) > 1 - EPS, that is 1 - cos(angle) < EPS.  Every sample keeps at least 1e-3 relative distance
    from a threshold (in sigma, and in 1 - d); the first samples of every branch sit right at that distance, on this branch's side, and the
    neighbouring branch has the mirror samples on the other side.  Angles reach from 1e-9 to pi - 1e-3, scales from 1/2 to 2."""
    a_thr = np.arccos(1 - EPS)                                        # 4.47e-3
    a_lo, a_hi = np.arccos(1 - EPS*(1 - 1e-3)), np.arccos(1 - EPS*(1 + 1e-3))
    small_s = branch in ("small_sigma", "both"); small_a = branch in ("small_angle", "both")
    if small_s:
        sig = np.concatenate([[EPS*(1 - 1e-3), -EPS*(1 - 1e-3), 1e-9, 0.0], 10.0**rng.uniform(-9, np.log10(EPS*(1 - 1e-3)), n - 4)*rng.choice([-1.0, 1.0], n - 4)])
    else:
        sig = np.concatenate([[EPS*(1 + 1e-3), -EPS*(1 + 1e-3), np.log(2.0), -np.log(2.0)], 10.0**rng.uniform(np.log10(EPS*(1 + 1e-3)), np.log10(np.log(2.0)), n - 4)*rng.choice([-1.0, 1.0], n - 4)])
    if small_a:
        ang = np.concatenate([[a_lo, 1e-9, 1e-6, 1e-3], 10.0**rng.uniform(-9, np.log10(a_lo), n - 4)])
    else:
        ang = np.concatenate([[a_hi, 1e-2, np.pi - 1e-3, np.pi/2], 10.0**rng.uniform(np.log10(a_hi), np.log10(np.pi - 1e-3), n//2 - 2), rng.uniform(a_hi, np.pi - 1e-3, n - n//2 - 2)])
    assert len(sig) == n and len(ang) == n and a_lo < a_thr < a_hi
    return ang, sig


def device_samples(branch, n, rng):
    """(angle, log-scale) for the device tests' connections: the branches and threshold neighbours of branch_samples, restricted to where the
    model itself is well conditioned, because the device test compares a COST to rtol 1e-9 and no evaluation in doubles can promise that
    elsewhere (reasoned from the formulas of logSim3, not from any implementation's output):
      * omega = theta/(2 sqrt(1 - d^2)) deltaR amplifies a rounding of d by 1/(pi - theta)^2 near pi: angles stay <= 3 rad (factor <= 50);
      * in the branch |sigma| >= EPS, d > 1 - EPS the reference's B = (sigma^2/2 - sigma + 1) s / sigma^3 ~ 1/sigma^3 gives W = C I + A Omega
        + B Omega^2 the eigenvalue C - B theta^2 across omega: W is singular at theta^2 ~ |sigma|^3 and has condition number ~ theta^2/|sigma|^3
        beyond; samples keep theta^2 <= |sigma|^3/10.  There omega, of length theta, is the vector part of a product of unit quaternions and
        so carries an ABSOLUTE rounding of about eps = 2.2e-16, which B theta^2 turns into 2 theta eps/|sigma|^3 of upsilon: samples also keep
        theta <= 1e5 |sigma|^3 (4.4e-11 of upsilon).  Next to the |sigma| threshold that means angles below 1e-9."""
    a_lo, a_hi = np.arccos(1 - EPS*(1 - 1e-3)), np.arccos(1 - EPS*(1 + 1e-3))
    small_s = branch in ("small_sigma", "both"); small_a = branch in ("small_angle", "both")
    if small_s:
        sig = np.concatenate([[EPS*(1 - 1e-3), -EPS*(1 - 1e-3), 1e-9, 0.0, -3e-7], 10.0**rng.uniform(-9, np.log10(EPS*(1 - 1e-3)), n - 5)*rng.choice([-1.0, 1.0], n - 5)])
    else:
        sig = np.concatenate([[EPS*(1 + 1e-3), -EPS*(1 + 1e-3), np.log(2.0), -np.log(2.0), 0.05], 10.0**rng.uniform(np.log10(EPS*(1 + 1e-3)), np.log10(np.log(2.0)), n - 5)*rng.choice([-1.0, 1.0], n - 5)])
    if small_a:
        cap = np.full(n, a_lo) if small_s else np.minimum(a_lo, np.minimum(np.sqrt(0.1*np.abs(sig)**3), 1e5*np.abs(sig)**3))
        ang = np.concatenate([cap[:5]*[1.0, 0.5, 1.0, 1.0, 1e-3], 10.0**rng.uniform(np.log10(cap[5:]) - 3, np.log10(cap[5:]))])
    else:
        ang = np.concatenate([[a_hi, 1e-2, 3.0, np.pi/2, a_hi], 10.0**rng.uniform(np.log10(a_hi), np.log10(3.0), n - 5)])
    return ang, sig


def edges_for(ang, sig, rng, k1s=None, k2s=None, t_scale=1.0):
    """Connections whose residual transform meas o S1 o S2^-1 has the given rotation angles and log-scales; the keyframes' Sim3 are random
    (unnormalised quaternions) unless given, and exactly representable in float32."""
    meas, x1, x2, D_ = [], [], [], []
    for i, (a, s) in enumerate(zip(ang, sig)):
        D = np.concatenate([q_axis_angle(rng.normal(size=3), a), rng.uniform(-t_scale, t_scale, 3), [np.exp(s)]])          # the residual transform
        if k1s is None:
            k1 = np.concatenate([q_axis_angle(rng.normal(size=3), rng.uniform(0, 2.5))*rng.uniform(0.5, 1.5), rng.uniform(-3, 3, 3), [rng.uniform(0.7, 1.4)]])
            k2 = np.concatenate([q_axis_angle(rng.normal(size=3), rng.uniform(0, 2.5))*rng.uniform(0.5, 1.5), rng.uniform(-3, 3, 3), [rng.uniform(0.7, 1.4)]])
        else:
            k1, k2 = k1s[i], k2s[i]
        k1, k2 = k1.astype(np.float32).astype(np.float64), k2.astype(np.float32).astype(np.float64)
        meas.append(sim_mul(D, sim_inv(sim_mul(k1, sim_inv(k2)))))                                                       # meas o S1 o S2^-1 = D
        x1.append(k1); x2.append(k2); D_.append(D)
    return np.array(meas), np.array(x1, np.float32), np.array(x2, np.float32), np.array(D_)


def compute_loop(oracle, out):
    rng = np.random.default_rng(20241019)
    for b in LOOP_BRANCHES:
        ang, sig = branch_samples(b, 200, rng)
        out[f"loop/{b}/meas"], out[f"loop/{b}/x1"], out[f"loop/{b}/x2"], D = edges_for(ang, sig, rng)           # x1 / x2 stored as float32: half the bytes
        out[f"logsim3/{b}/q"], out[f"logsim3/{b}/t"], out[f"logsim3/{b}/s"] = D[:, :4].copy(), D[:, 4:7].copy(), D[:, 7].copy()
        out[f"logsim3/{b}/d"] = np.cos(ang)                                     # (what logSim3 compares with 1 - EPS; kept for the tests' branch check)
    # the device tests' connections: fifteen per branch (device_samples)
    for b in LOOP_BRANCHES:
        ang, sig = device_samples(b, 15, rng)
        out[f"loop15/{b}/meas"], out[f"loop15/{b}/x1"], out[f"loop15/{b}/x2"], D = edges_for(ang, sig, rng)
        out[f"loop15/{b}/d"] = np.cos(ang)
    # one 12-keyframe graph: keyframes 0 and 1 constant, a chain with second neighbours and one closing connection; its connections cycle
    # through the four branches (device_samples)
    n_kf = 12
    pose = np.array([np.concatenate([q_axis_angle(rng.normal(size=3), rng.uniform(0, 1.0)), rng.uniform(-2, 2, 3), [rng.uniform(0.8, 1.25)]]) for _ in range(n_kf)])
    pose = pose.astype(np.float32).astype(np.float64)
    ei, ej = [], []
    for k in range(n_kf - 1):
        if k >= 1:                                    # (no connection between the two constant keyframes: Ceres drops such a block, RECALLED C13)
            ei.append(k + 1); ej.append(k)
        if k + 2 < n_kf:
            ei.append(k + 2); ej.append(k)
    ei.append(n_kf - 1); ej.append(2)
    ang, sig = np.zeros(len(ei)), np.zeros(len(ei))
    for e in range(len(ei)):
        a, s = device_samples(LOOP_BRANCHES[e % 4], 8, rng); ang[e], sig[e] = a[5 + e % 3], s[5 + e % 3]
    meas, _, _, _ = edges_for(ang, sig, rng, pose[ei], pose[ej], t_scale=0.3)
    fixed = np.zeros(n_kf, np.uint8); fixed[:2] = 1
    g = dict(pose=pose, fixed=fixed, edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), meas=meas)
    for k, v in g.items():
        out[f"graph12/{k}"] = v


def compute_sim(oracle, out):
    rng = np.random.default_rng(777)
    K4 = np.array([520.0, 521.5, 318.2, 243.7])

    def proj(P):
        return np.stack([K4[0]*P[:, 0]/P[:, 2] + K4[2], K4[1]*P[:, 1]/P[:, 2] + K4[3]], axis=1)
    for name, n in SIM_SETS.items():
        groups = 4 if name == "cpu200" else 1
        per = n//groups
        P1s, P2s, u1s, u2s, xs = [], [], [], [], []
        for gidx in range(groups):
            scale = [0.5, 2.0, 1.07, 0.83][gidx] if groups > 1 else [1.3, 0.6, 1.9][list(SIM_SETS).index(name) - 1]
            true = np.concatenate([q_axis_angle(rng.normal(size=3), rng.uniform(0.05, 0.6)), rng.uniform(-0.5, 0.5, 3), [scale]])
            P2 = np.stack([rng.uniform(-2, 2, per), rng.uniform(-1.5, 1.5, per), rng.uniform(2.5, 8, per)], axis=1)
            P1 = scale*(P2 @ q_R(true[:4]).T) + true[4:7] + rng.normal(0, 0.01, (per, 3))
            if name == "cpu200" and gidx == 0:      # one point that the transform takes to a small positive depth
                P2[0] = q_R(true[:4]).T @ ((np.array([0.01, -0.02, 0.05]) - true[4:7])/scale)
            uv1 = (proj(P1) + rng.normal(0, 2.0, (per, 2))).astype(np.float32); uv2 = (proj(P2) + rng.normal(0, 2.0, (per, 2))).astype(np.float32)
            x = true.copy()
            x[:4] = q_mul(q_axis_angle(rng.normal(size=3), 2e-3), x[:4])*rng.uniform(0.4, 2.5)              # unnormalised, a little off the truth
            x[4:7] += rng.normal(0, 0.004, 3); x[7] *= 1 + rng.normal(0, 0.002)
            P1s.append(P1); P2s.append(P2); u1s.append(uv1); u2s.append(uv2); xs.append(x)
        inl = np.ones(n, np.uint8); inl[rng.choice(n, max(1, n//8), replace=False)] = 0            # some matches arrive flagged out
        # x [groups,8]: group g holds matches [g n/groups, (g+1) n/groups)
        d = dict(P1=np.concatenate(P1s), P2=np.concatenate(P2s), uv1=np.concatenate(u1s), uv2=np.concatenate(u2s), x=np.array(xs), K=K4, inlier=inl)
        for k, v in d.items():
            out[f"sim/{name}/{k}"] = v


def compute_textproj(oracle, out):
    rng = np.random.default_rng(5)
    n = 64
    ray = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), np.ones((n, 1))], axis=1)
    theta = np.stack([rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.5, -0.1, n)], axis=1)
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        T[i, :3, :3] = q_R(q_axis_angle(rng.normal(size=3), rng.uniform(0, 0.4))); T[i, :3, 3] = rng.uniform(-0.3, 0.3, 3)
    K = oracle.K33([384.4, 382.8, 315.6, 249.2])
    out["textproj/ray"], out["textproj/Tcr"], out["textproj/theta"], out["textproj/K"] = ray, T.reshape(n, 16), theta, K


def reference_outputs(oracle, fix):
    """What the compiled functors return on the inputs recorded in `fix` (the loop, Sim3 and TextProj cases: the stored arrays; the BA
    cases: the synthetic problem of that name, whose digest is recorded) -> name -> array, the fixture's output entries."""
    out = {}
    compute_ba(oracle, out)
    f64 = lambda a: np.asarray(a, np.float64)
    for b in LOOP_BRANCHES:
        out[f"loop/{b}/res"] = oracle.ref_loop(fix[f"loop/{b}/meas"], f64(fix[f"loop/{b}/x1"]), f64(fix[f"loop/{b}/x2"]))
        out[f"logsim3/{b}/res"] = oracle.ref_logsim3(fix[f"logsim3/{b}/q"], fix[f"logsim3/{b}/t"], fix[f"logsim3/{b}/s"])
        out[f"loop15/{b}/res"] = oracle.ref_loop(fix[f"loop15/{b}/meas"], f64(fix[f"loop15/{b}/x1"]), f64(fix[f"loop15/{b}/x2"]))
    pose = fix["graph12/pose"]
    out["graph12/res"] = oracle.ref_loop(fix["graph12/meas"], pose[fix["graph12/edge_i"]], pose[fix["graph12/edge_j"]])
    for name, n in SIM_SETS.items():
        g = lambda k: fix[f"sim/{name}/{k}"]
        K = oracle.K33(g("K")); x = g("x"); per = n//len(x); rs, js = [], []
        for i, xi in enumerate(x):
            sl = slice(i*per, (i + 1)*per)
            r1, j1 = oracle.ref_sim(g("P2")[sl], f64(g("uv1")[sl]), K, xi); r2, j2 = oracle.ref_sim(g("P1")[sl], f64(g("uv2")[sl]), K, xi, inv=True)
            rs.append(np.concatenate([r1, r2], axis=1)); js.append(np.concatenate([j1, j2], axis=1))
        out[f"sim/{name}/res"] = np.concatenate(rs)
        if name == "cpu200":                                                 # the Jet Jacobians go with the CPU set only
            out[f"sim/{name}/jac"] = np.concatenate(js)
    out["textproj/p"], out["textproj/uv"] = oracle.ref_textproj(fix["textproj/ray"], fix["textproj/Tcr"], fix["textproj/theta"], fix["textproj/K"])
    return out


def check_cases(fix):
    """What the issue demands of the recorded reference values themselves."""
    for k, v in fix.items():
        if v.dtype.kind == "f":
            assert np.all(np.isfinite(v)), k
    for b in LOOP_BRANCHES:                                                   # the branch the reference took is the one meant, 1e-3 clear of both thresholds
        for fam in ("loop", "logsim3", "loop15"):
            sg = fix[f"{fam}/{b}/res"][:, 6]
            assert np.all((np.abs(sg) < EPS) == (b in ("small_sigma", "both"))), (fam, b)
            assert np.all(np.abs(np.abs(sg) - EPS) >= 0.99e-3*EPS), (fam, b)
        for fam in ("logsim3", "loop15"):
            d = fix[f"{fam}/{b}/d"]
            assert np.all((d > 1 - EPS) == (b in ("small_angle", "both"))) and np.all(np.abs((1 - d) - EPS) >= 0.99e-3*EPS), (fam, b)
    for name in SIM_SETS:                                                     # no |r_k| within 1e-6 of the 4-pixel inlier test
        assert np.all(np.abs(np.abs(fix[f"sim/{name}/res"]) - 4.0) > 1e-6), name


def compute():
    import oracle
    assert oracle.ref_lib() is not None, "oracle/_ref/libtsref.so is missing: build with the reference tree present"
    out = Fixture()
    compute_loop(oracle, out); compute_sim(oracle, out); compute_textproj(oracle, out)       # the inputs
    out.update(reference_outputs(oracle, out))                                                 # the BA cases' inputs and every output
    check_cases(out)
    return out


def save(out, path=OUT):
    """Hundreds of small arrays: one blob per dtype and a JSON index (an npz entry per array would cost more than many of them hold)."""
    import json
    blobs, index = {}, []
    for k, v in out.items():
        v = np.ascontiguousarray(v); dt = v.dtype.str
        b = blobs.setdefault(dt, [])
        index.append([k, dt, sum(len(x) for x in b), list(v.shape)])
        b.append(v.reshape(-1))
    np.savez_compressed(path, index=np.frombuffer(json.dumps(index).encode(), np.uint8), **{"blob" + str(i): np.concatenate(b) for i, (dt, b) in enumerate(sorted(blobs.items()))},
                        dtypes=np.array(sorted(blobs)))


def load(path=OUT):
    import json
    z = np.load(path)
    blobs = {str(dt): z["blob" + str(i)] for i, dt in enumerate(z["dtypes"])}
    fix = Fixture()
    for k, dt, off, shape in json.loads(z["index"].tobytes().decode()):
        n = int(np.prod(shape)) if shape else 1
        fix[k] = blobs[dt][off:off + n].reshape(shape)
    return fix


if __name__ == "__main__":
    out = compute()
    save(out)
    back = load()
    assert list(back) == list(out) and all(np.array_equal(back[k], out[k]) and back[k].dtype == out[k].dtype for k in out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")

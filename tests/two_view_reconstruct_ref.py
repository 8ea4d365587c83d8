"""numpy restatement of the two-view initializer's reconstruction as docs/twoview_reconstruct_recalled.md states it: ReconstructH's 8 / ReconstructF's 4 motion
hypotheses in fp64 from the float model and K (np.linalg.svd, the sign rules, one rounding to float), CheckRT and Triangulate (the 4 x 4 from the reference's float
products, its null vector in fp64, the point rounded once, then float32 operation by operation), the exact order statistic and the keep logic.  What
tsorb_match_two_view_reconstruct (include/tsorb.h, textslam_amd/csrc/tstwoview_rec.h) is compared with, the worlds the tests commit to, and the conditions those
worlds have to meet (sensitivity, decision_margins, conditions_hold)."""
import functools
import itertools
import math
import numpy as np
import two_view_ref as T

F32, F64 = np.float32, np.float64
COS_LOW = 0.99998
RATIO = 1.00001
OUT, NONFINITE, DEPTH1, DEPTH2, ERR1, ERR2, GOOD, TRI = range(8)
EXIT_SV, EXIT_FEW, EXIT_TIE, EXIT_PARALLAX = 1, 2, 4, 8
_ERR = dict(invalid="ignore", divide="ignore", over="ignore")


# ---- the hypotheses (fp64 from the float inputs; rounded once by the caller)
def _kmat(K):
    fx, fy, cx, cy = [float(F32(v)) for v in K]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), np.array([[1/fx, 0, -cx/fx], [0, 1/fy, -cy/fy], [0, 0, 1.0]])


def _noise(A, rng):
    """A's entries moved at the 1e-13 relative level (sensitivity); rng None: A itself."""
    return A if rng is None else A*(1.0 + 1e-13*rng.uniform(-1.0, 1.0, A.shape))


def hypotheses_h(H21, K, rng=None):
    """ReconstructH (:648-752): (R [8, 3, 3], t [8, 3]) in fp64 and whether the singular-value exit (:661) is taken (then both are zero)."""
    Km, iK = _kmat(K)
    A = _noise(iK @ (np.asarray(H21, F32).astype(F64).reshape(3, 3) @ Km), rng)
    _, w, Vt = np.linalg.svd(A); V = Vt.T.copy()
    for j in (0, 2):
        V[:, j] = T.sign_rule(V[:, j])
    with np.errstate(**_ERR):
        U = (A @ V)/w                                                   # u_i = A v_i / d_i
        d1f, d2f, d3f = w.astype(F32)
        if float(d1f/d2f) < RATIO or float(d2f/d3f) < RATIO:             # float divisions against the double constant
            return np.zeros((8, 3, 3)), np.zeros((8, 3)), True
        s = -1.0 if np.linalg.det(U)*np.linalg.det(V) < 0 else 1.0
        d1, d2, d3 = w
        aux1 = math.sqrt((d1*d1 - d2*d2)/(d1*d1 - d3*d3)); aux3 = math.sqrt((d2*d2 - d3*d3)/(d1*d1 - d3*d3))
        x1 = [aux1, aux1, -aux1, -aux1]; x3 = [aux3, -aux3, aux3, -aux3]
        R, t = np.zeros((8, 3, 3)), np.zeros((8, 3))
        aux_st = math.sqrt((d1*d1 - d2*d2)*(d2*d2 - d3*d3))/((d1 + d3)*d2); ct = (d2*d2 + d1*d3)/((d1 + d3)*d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        for i in range(4):
            Rp = np.eye(3); Rp[0, 0] = ct; Rp[0, 2] = -st[i]; Rp[2, 0] = st[i]; Rp[2, 2] = ct
            R[i] = s*(U @ Rp @ V.T)
            tt = U @ (np.array([x1[i], 0.0, -x3[i]])*(d1 - d3)); t[i] = tt/np.linalg.norm(tt)
        aux_sp = math.sqrt((d1*d1 - d2*d2)*(d2*d2 - d3*d3))/((d1 - d3)*d2); cp = (d1*d3 - d2*d2)/((d1 - d3)*d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        for i in range(4):
            Rp = np.eye(3); Rp[0, 0] = cp; Rp[0, 2] = sp[i]; Rp[1, 1] = -1.0; Rp[2, 0] = sp[i]; Rp[2, 2] = -cp
            R[4 + i] = s*(U @ Rp @ V.T)
            tt = U @ (np.array([x1[i], 0.0, x3[i]])*(d1 + d3)); t[4 + i] = tt/np.linalg.norm(tt)
    return R, t, False


def hypotheses_f(F21, K, rng=None):
    """ReconstructF (:540-548) + DecomposeE (:979-999): (R1, t), (R2, t), (R1, -t), (R2, -t) in fp64; rows 4 .. 7 are zero."""
    Km, _ = _kmat(K)
    E = _noise(Km.T @ (np.asarray(F21, F32).astype(F64).reshape(3, 3) @ Km), rng)
    U, w, Vt = np.linalg.svd(E)
    with np.errstate(**_ERR):
        v1, v2 = Vt[0], Vt[1]; u1, u2 = (E @ v1)/w[0], (E @ v2)/w[1]
        u3, v3 = np.cross(u1, u2), np.cross(v1, v2)                      # det U = det V = +1
        Ra = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)      # U W V^T
        Rb = -np.outer(u2, v1) + np.outer(u1, v2) + np.outer(u3, v3)     # U W^T V^T
        R1, R2 = (Ra, Rb) if np.trace(Ra) >= np.trace(Rb) else (Rb, Ra)
        tt = T.sign_rule(u3); tt = tt/np.linalg.norm(tt)
    R, t = np.zeros((8, 3, 3)), np.zeros((8, 3))
    R[0], R[1], R[2], R[3] = R1, R2, R1, R2; t[0], t[1], t[2], t[3] = tt, tt, -tt, -tt
    return R, t, False


def hypotheses(model, M21, K, rng=None):
    return hypotheses_h(M21, K, rng) if model == 0 else hypotheses_f(M21, K, rng)


# ---- CheckRT (:868-977) given a FLOAT R, t, K
def camera(R, t, K):
    """P2 = K [R | t] and O2 = -R^T t: double accumulation, one float rounding per entry (cv::gemm on CV_32F as recalled)."""
    R = np.asarray(R, F32).reshape(3, 3).astype(F64); t = np.asarray(t, F32).reshape(3).astype(F64)
    fx, fy, cx, cy = [F64(F32(v)) for v in K]
    Rt = np.column_stack([R, t])
    with np.errstate(**_ERR):
        P2 = np.stack([fx*Rt[0] + cx*Rt[2], fy*Rt[1] + cy*Rt[2], Rt[2]]).astype(F32)
        O2 = (-((R[0]*t[0] + R[1]*t[1]) + R[2]*t[2])).astype(F32)
    return P2, O2


def system(P2, K, xy1, xy2):
    """Triangulate's 4 x 4 per match [n, 4, 4] in float32: kp.pt.x * P.row(2) - P.row(0), ... as written."""
    fx, fy, cx, cy = [F32(v) for v in K]; z, o = F32(0), F32(1)
    P1 = np.array([[fx, z, cx, z], [z, fy, cy, z], [z, z, o, z]], F32); P2 = np.asarray(P2, F32)
    xy1 = np.ascontiguousarray(xy1, F32).reshape(-1, 2); xy2 = np.ascontiguousarray(xy2, F32).reshape(-1, 2)
    A = np.empty((len(xy1), 4, 4), F32)
    with np.errstate(**_ERR):
        A[:, 0] = xy1[:, 0:1]*P1[2] - P1[0]; A[:, 1] = xy1[:, 1:2]*P1[2] - P1[1]
        A[:, 2] = xy2[:, 0:1]*P2[2] - P2[0]; A[:, 3] = xy2[:, 1:2]*P2[2] - P2[1]
    assert A.dtype == F32
    return A


def triangulate64(A, rng=None):
    """X = v[0 .. 2] / v[3] in fp64, v the right singular vector of the smallest singular value of each 4 x 4 (a NaN system gives a NaN point)."""
    A = _noise(np.asarray(A, F32).astype(F64), rng); X = np.full((len(A), 3), np.nan)
    ok = np.isfinite(A).all(axis=(1, 2))
    if ok.any():
        v = np.linalg.svd(A[ok])[2][:, 3, :]
        with np.errstate(**_ERR):
            X[ok] = v[:, :3]/v[:, 3:4]
    return X


def _to_f32(X):
    with np.errstate(**_ERR):
        return np.asarray(X).astype(F32)


def th2_of(sigma):
    s = F32(sigma)
    return F32(4.0*F64(s*s))


def check(R, t, K, th2, inlier, xy1, xy2, X):
    """CheckRT's loop body after Triangulate on the FLOAT points X [n, 3]: (state [n] uint8, cos [n] float32), the reference's arithmetic operation by operation."""
    R = np.asarray(R, F32).reshape(3, 3); t = np.asarray(t, F32).reshape(3); X = np.ascontiguousarray(X, F32).reshape(-1, 3)
    xy1 = np.ascontiguousarray(xy1, F32).reshape(-1, 2); xy2 = np.ascontiguousarray(xy2, F32).reshape(-1, 2)
    fx, fy, cx, cy = [F32(v) for v in K]; th2 = F32(th2)
    _, O2 = camera(R, t, K)
    with np.errstate(**_ERR):
        finite = np.isfinite(X).all(axis=1)
        a = X - F32(0); b = X - O2                                      # normal1 = p3dC1 - O1, normal2 = p3dC1 - O2
        ad, bd = a.astype(F64), b.astype(F64)
        dist1 = np.sqrt((ad[:, 0]*ad[:, 0] + ad[:, 1]*ad[:, 1]) + ad[:, 2]*ad[:, 2]).astype(F32)          # cv::norm: double accumulation
        dist2 = np.sqrt((bd[:, 0]*bd[:, 0] + bd[:, 1]*bd[:, 1]) + bd[:, 2]*bd[:, 2]).astype(F32)
        dot = (ad[:, 0]*bd[:, 0] + ad[:, 1]*bd[:, 1]) + ad[:, 2]*bd[:, 2]                                  # Mat::dot: double accumulation
        cos = (dot/(dist1*dist2).astype(F64)).astype(F32)
        low = cos.astype(F64) < COS_LOW
        Xd, Rd, td = X.astype(F64), R.astype(F64), t.astype(F64)
        p2 = np.stack([((Rd[i, 0]*Xd[:, 0] + Rd[i, 1]*Xd[:, 1]) + Rd[i, 2]*Xd[:, 2]) + td[i] for i in range(3)], axis=1).astype(F32)
        iz1 = (1.0/Xd[:, 2]).astype(F32)
        u1 = fx*X[:, 0]*iz1 + cx; v1 = fy*X[:, 1]*iz1 + cy
        e1 = (u1 - xy1[:, 0])*(u1 - xy1[:, 0]) + (v1 - xy1[:, 1])*(v1 - xy1[:, 1])
        iz2 = (1.0/p2[:, 2].astype(F64)).astype(F32)
        u2 = fx*p2[:, 0]*iz2 + cx; v2 = fy*p2[:, 1]*iz2 + cy
        e2 = (u2 - xy2[:, 0])*(u2 - xy2[:, 0]) + (v2 - xy2[:, 1])*(v2 - xy2[:, 1])
        assert e1.dtype == F32 and e2.dtype == F32 and cos.dtype == F32
        state = np.select([~np.asarray(inlier, bool), ~finite, np.isnan(cos), (X[:, 2] <= 0) & low, (p2[:, 2] <= 0) & low, e1 > th2, e2 > th2, ~low],
                          [OUT, NONFINITE, NONFINITE, DEPTH1, DEPTH2, ERR1, ERR2, GOOD], TRI).astype(np.uint8)
    parts = dict(z1=X[:, 2], z2=p2[:, 2], e1=e1, e2=e2, cos=cos)
    return state, np.where(state >= DEPTH1, cos, F32(0)).astype(F32), parts


def statistic(state, cos):
    """(nGood, sorted[min(50, nGood - 1)], the parallax in degrees): the exact order statistic; acos of the float, * 180 in float, / CV_PI in double, stored in a float."""
    good = state >= GOOD; n = int(good.sum())
    if n == 0:
        return 0, F32(0), F32(0)
    c = np.sort(cos[good])[min(50, n - 1)]
    with np.errstate(**_ERR):                                           # a cosine one float step above 1 has a NaN parallax, in the reference as well
        return n, F32(c), F32(F64(F32(np.arccos(c))*F32(180))/math.pi)


def keep(model, sv_exit, good, par, N, min_tri, min_par):
    """ReconstructH's (:755-801) / ReconstructF's (:560-633) keep logic, comparison for comparison: [ok, sel, N, best, second best / nsimilar, exit bits]."""
    good = [int(g) for g in good]; par = [F32(p) for p in par]; min_par = F32(min_par)
    if model == 0:
        if sv_exit:
            return [0, -1, N, 0, 0, EXIT_SV]
        best, second, idx, bpar = 0, 0, -1, F32(-1)
        for i in range(8):
            if good[i] > best:
                second, best, idx, bpar = best, good[i], i, par[i]
            elif good[i] > second:
                second = good[i]
        c0, c1, c2, c3 = second < 0.75*best, bool(bpar >= min_par), best > min_tri, best > 0.9*N
        bits = (0 if c0 else EXIT_TIE) | (0 if c1 else EXIT_PARALLAX) | (0 if c2 and c3 else EXIT_FEW)
        return [int(bits == 0), idx if bits == 0 else -1, N, best, second, bits]
    g = good[:4]; mx = max(g); nmin = max(int(0.9*N), min_tri)
    nsim = sum(1 for x in g if x > 0.7*mx)
    bits = (EXIT_FEW if mx < nmin else 0) | (EXIT_TIE if nsim > 1 else 0)
    if bits:
        return [0, -1, N, mx, nsim, bits]
    idx = g.index(mx)
    if par[idx] > min_par:
        return [1, idx, N, mx, nsim, 0]
    return [0, -1, N, mx, nsim, EXIT_PARALLAX]


def derive(w, hyp_pose, hyp_p3d):
    """Everything the call reports that follows from its FLOAT hypotheses [8, 3, 4] and FLOAT points [8, n, 3]: comparison 1 needs no conditions."""
    n = len(w["xy1"]); nh = 8 if w["model"] == 0 else 4
    hyp_pose = np.asarray(hyp_pose, F32).reshape(8, 3, 4); hyp_p3d = np.asarray(hyp_p3d, F32).reshape(8, n, 3)
    sv = w["model"] == 0 and hypotheses_h(w["M21"], w["K"])[2]
    out = dict(hyp_state=np.zeros((8, n), np.uint8), hyp_good=np.zeros(8, np.int32), hyp_cos=np.zeros(8, F32), hyp_parallax=np.zeros(8, F32))
    if not sv:
        for h in range(nh):
            st, cs, _ = check(hyp_pose[h, :, :3], hyp_pose[h, :, 3], w["K"], th2_of(w["sigma"]), w["inlier"], w["xy1"], w["xy2"], hyp_p3d[h])
            out["hyp_state"][h] = st; out["hyp_good"][h], out["hyp_cos"][h], out["hyp_parallax"][h] = statistic(st, cs)
    return out


def decide(w, out, hyp_pose, hyp_p3d, sv, hyp_parallax=None):
    """result, R21, t21, p3d, triangulated from the counts, the parallaxes (the implementation's own where given: its acosf is its own) and the states."""
    n = len(w["xy1"]); hyp_pose = np.asarray(hyp_pose, F32).reshape(8, 3, 4); hyp_p3d = np.asarray(hyp_p3d, F32).reshape(8, n, 3)
    res = keep(w["model"], sv, out["hyp_good"], out["hyp_parallax"] if hyp_parallax is None else hyp_parallax, int(np.asarray(w["inlier"], bool).sum()),
               w["min_triangulated"], w["min_parallax"])
    d = dict(result=np.array(res, np.int32), R21=np.zeros((3, 3), F32), t21=np.zeros(3, F32), p3d=np.zeros((n, 3), F32), triangulated=np.zeros(n, bool))
    if res[0]:
        s = res[1]; st = out["hyp_state"][s]
        d["R21"] = hyp_pose[s, :, :3].copy(); d["t21"] = hyp_pose[s, :, 3].copy()
        d["p3d"][st >= GOOD] = hyp_p3d[s][st >= GOOD]; d["triangulated"] = st == TRI
    return d


def run(w, rng=None):
    """The whole call.  Also pose64 [8, 3, 4] and p3d64 [8, n, 3] (before their roundings) and parts [h] (the compared quantities of every pair)."""
    n = len(w["xy1"]); nh = 8 if w["model"] == 0 else 4
    R, t, sv = hypotheses(w["model"], w["M21"], w["K"], rng)
    pose64 = np.concatenate([R, t[:, :, None]], axis=2); hyp_pose = _to_f32(pose64)
    p3d64 = np.zeros((8, n, 3)); inl = np.asarray(w["inlier"], bool)
    if not sv:
        for h in range(nh):
            P2, _ = camera(hyp_pose[h, :, :3], hyp_pose[h, :, 3], w["K"])
            p3d64[h][inl] = triangulate64(system(P2, w["K"], w["xy1"][inl], w["xy2"][inl]), rng)
    hyp_p3d = _to_f32(p3d64)
    out = derive(w, hyp_pose, hyp_p3d)
    out.update(decide(w, out, hyp_pose, hyp_p3d, sv))
    out.update(hyp_pose=hyp_pose, hyp_p3d=hyp_p3d, pose64=pose64, p3d64=p3d64, sv_exit=sv)
    return out


# ---- the worlds
def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def _finish(w, model, M21, inlier, K, sigma=1.0, min_parallax=1.0, min_triangulated=50, take=None):
    k = len(w["xy1"]) if take is None else take
    return dict(w, model=model, M21=np.asarray(M21, F32).reshape(3, 3), inlier=np.asarray(inlier, bool)[:k].copy(), K=np.asarray(K, F32), sigma=F32(sigma),
                min_parallax=F32(min_parallax), min_triangulated=int(min_triangulated), xy1=w["xy1"][:k].copy(), xy2=w["xy2"][:k].copy(),
                matches=w["matches"][:k].copy(), n=k)


def ransac_world(kind, seed, n, outliers, H, model, take=None, min_triangulated=50, noise=0.5):
    """A world of two_view_ref with the model and the mask its RANSAC restatement keeps (what the initializer hands to ReconstructH / ReconstructF); take: the first
    `take` matches only."""
    w = T.world(kind, seed, n, outliers, H, noise); res = T.run_world(w)
    return _finish(w, model, res["H21" if model == 0 else "F21"], res["inlier_h" if model == 0 else "inlier_f"], w["K"], w["sigma"], 1.0, min_triangulated, take)


def scene_world(kind, seed, n, model, baseline=0.4, noise=0.3, min_triangulated=50, sigma=1.0, K=T.K_DEFAULT, w=160, h=120, drop=0.0):
    """Two views with the model formed from the true motion (rounded to float), for what the RANSAC worlds cannot give: any n from 1, a chosen baseline.  drop: the
    share of matches whose mask is zeroed."""
    g = np.random.default_rng(1000 + seed)
    ax = g.normal(size=3); ax /= np.linalg.norm(ax); ang = g.uniform(0.02, 0.06)
    R = np.eye(3) + math.sin(ang)*_skew(ax) + (1 - math.cos(ang))*(_skew(ax) @ _skew(ax))
    t = np.array([g.choice([-1, 1])*1.0, g.uniform(-0.2, 0.2), g.uniform(-0.2, 0.2)]); t *= baseline/np.linalg.norm(t)
    px = np.column_stack([g.uniform(10, w - 10, n), g.uniform(10, h - 10, n)])
    rays = np.column_stack([(px[:, 0] - K[2])/K[0], (px[:, 1] - K[3])/K[1], np.ones(n)])
    nrm = np.array([0.1, -0.08, 1.0]); nrm /= np.linalg.norm(nrm)
    z = 4.0/(rays @ nrm) if kind == "planar" else g.uniform(2.0, 8.0, n)
    X = rays*z[:, None]; X2 = X @ R.T + t
    px2 = np.column_stack([K[0]*X2[:, 0]/X2[:, 2] + K[2], K[1]*X2[:, 1]/X2[:, 2] + K[3]])
    a = (px + g.normal(0.0, noise, (n, 2))).astype(F32); b = (px2 + g.normal(0.0, noise, (n, 2))).astype(F32)
    Km, iK = _kmat(K)
    M = Km @ (R + np.outer(t, nrm)/4.0) @ iK if model == 0 else iK.T @ _skew(t) @ R @ iK
    M = M/np.abs(M).max()
    k1, k2 = g.permutation(n + 5)[:n], g.permutation(n + 5)[:n]
    keys1 = np.column_stack([g.uniform(0, w, n + 5), g.uniform(0, h, n + 5)]).astype(F32); keys2 = keys1[::-1].copy(); keys1[k1] = a; keys2[k2] = b
    inl = np.ones(n, bool); inl[g.permutation(n)[:int(round(drop*n))]] = False
    wd = dict(kind=kind, seed=seed, R=R, t=t, X=X, truth=np.ones(n, bool), keys1=keys1, keys2=keys2, matches=np.column_stack([k1, k2]).astype(np.int32), xy1=a, xy2=b)
    return _finish(wd, model, M, inl, K, sigma, 1.0, min_triangulated)


def identity_world():
    """H's singular-value exit: a homography that is the identity up to the float rounding of a pure zoom (d1 = d2 = d3)."""
    w = scene_world("planar", 3, 64, 0, min_triangulated=50)
    return dict(w, M21=(np.eye(3)*0.5).astype(F32), kind="identity")


def err2_world():
    """The exit at the second image's error alone needs squareError1 <= th2 < squareError2, and the triangulation splits a displacement almost evenly between the two
    views: match 11's second pixel moved by 4.78 px in y sits in the 0.03 px wide window where it happens (both errors within 1 % of th2 = 4)."""
    w = scene_world("general", 12, 64, 1)
    w["xy2"][11, 1] += F32(4.78); w["keys2"][w["matches"][11, 1]] = w["xy2"][11]
    return dict(w, kind="err2")


def infinity_world():
    """K = (1, 1, 0, 0), F = [t]x exactly for t = (1, 0, 0): R = I and t come out exactly.  Nine matches in normalised coordinates seen by a camera that moved along
    x; match 0 is the principal point in both views: its rays are parallel, the 4 x 4 has a zero column and the point is (0/0, 0/0, 1/0): the isfinite exit."""
    g = np.random.default_rng(7)
    X = np.column_stack([g.uniform(-1, 1, 9), g.uniform(-1, 1, 9), g.uniform(2, 6, 9)]); X2 = X + np.array([1.0, 0, 0])
    a = (X[:, :2]/X[:, 2:]).astype(F32); b = (X2[:, :2]/X2[:, 2:]).astype(F32); a[0] = 0; b[0] = 0
    wd = dict(kind="infinity", seed=7, R=np.eye(3), t=np.array([1.0, 0, 0]), truth=np.ones(9, bool), keys1=a.copy(), keys2=b.copy(),
              matches=np.column_stack([np.arange(9), np.arange(9)]).astype(np.int32), xy1=a, xy2=b)
    return _finish(wd, 1, _skew([1.0, 0, 0]), np.ones(9, bool), (1.0, 1.0, 0.0, 0.0), sigma=0.01, min_triangulated=5)


# name -> (constructor, arguments).  n = 1, 8, 9, 63, 64, 65, 257, 300; both models; every exit; min_triangulated 5 for the small worlds
WORLDS = {
    "h_success_64": (ransac_world, ("planar", 6, 64, 0.0, 200, 0)),                      # success from H: 64 good against a second best of 42
    "f_success_65": (ransac_world, ("general", 1, 65, 0.0, 256, 1)),                     # success from F, more than 51 good
    "h_tie_64": (ransac_world, ("planar", 0, 64, 0.0, 200, 0)),                          # the planar two-fold ambiguity: no clear winner
    "h_tie_257": (ransac_world, ("planar", 0, 257, 0.3, 200, 0)),
    "f_few_300": (ransac_world, ("general", 0, 300, 0.3, 200, 1)),                       # not enough good points against 0.9 N
    "f_63": (ransac_world, ("general", 1, 65, 0.0, 256, 1, 63)),
    "f_51": (scene_world, ("general", 4, 51, 1)),                                        # exactly 51 good: idx = min(50, 50)
    "f_9": (scene_world, ("general", 5, 9, 1, 0.4, 0.3, 5)),
    "h_8": (scene_world, ("planar", 6, 8, 0, 0.4, 0.3, 5)),
    "f_1": (scene_world, ("general", 7, 1, 1, 0.4, 0.3, 0)),
    "f_drop_300": (scene_world, ("general", 8, 300, 1, 0.4, 0.3, 50, 1.0, T.K_DEFAULT, 160, 120, 0.3)),     # 30 % of the mask zero
    "f_parallax_300": (scene_world, ("general", 9, 300, 1, 0.03, 0.1)),                  # a tiny baseline: the parallax exit
    "h_parallax_64": (scene_world, ("planar", 10, 64, 0, 0.04, 0.1)),
    "f_err2_64": (err2_world, ()),
    "identity": (identity_world, ()),
    "infinity": (infinity_world, ()),
}
ALL = list(WORLDS)


@functools.lru_cache(maxsize=None)
def make(name):
    f, a = WORLDS[name]
    return f(*a)


@functools.lru_cache(maxsize=None)
def answer(name):
    return run(make(name))


# ---- sensitivities and conditions
def sensitivity(w, res=None):
    """pose [8]: the largest change of a hypothesis' entries (R | t) relative to its largest entry, and point [8, n]: the largest change of a point's coordinates
    relative to its largest coordinate, when the inputs of the two fp64 stages (A or E; each 4 x 4) move at the 1e-13 relative level in double."""
    res = run(w) if res is None else res
    moved = run(w, np.random.default_rng(12345))
    with np.errstate(**_ERR):
        pose = np.nan_to_num(np.abs(moved["pose64"] - res["pose64"]).max(axis=(1, 2))/np.abs(res["pose64"]).max(axis=(1, 2)))
        # the points from the SAME float hypotheses (a hypothesis whose rounding moved would move every point by far more than the fp64 stage does)
        pt = np.zeros(res["p3d64"].shape[:2]); inl = np.asarray(w["inlier"], bool); rng = np.random.default_rng(54321)
        if not res["sv_exit"]:
            for h in range(8 if w["model"] == 0 else 4):
                P2, _ = camera(res["hyp_pose"][h, :, :3], res["hyp_pose"][h, :, 3], w["K"])
                X = triangulate64(system(P2, w["K"], w["xy1"][inl], w["xy2"][inl]), rng); X0 = res["p3d64"][h][inl]
                pt[h][inl] = np.nan_to_num(np.abs(X - X0).max(axis=1)/np.abs(X0).max(axis=1), posinf=0.0)
    return dict(pose=pose, point=pt)


def tolerance(ref, sens):
    """The larger of 1000 x the sensitivity and one float ulp, of the largest entry (pose [8, 1, 1]) or coordinate (point [8, n, 1])."""
    with np.errstate(**_ERR):
        bp = np.abs(ref["hyp_pose"]).max(axis=(1, 2), keepdims=True); bx = np.abs(ref["hyp_p3d"]).max(axis=2, keepdims=True)
        return dict(pose=np.maximum(1000.0*sens["pose"][:, None, None]*bp, np.spacing(bp).astype(F64)),
                    point=np.maximum(1000.0*sens["point"][:, :, None]*bx, np.spacing(bx).astype(F64)))


def _step(a, up):
    return np.nextafter(np.asarray(a, F32), F32(np.inf if up else -np.inf)).astype(F32)


def decision_margins(w, res=None):
    """Per hypothesis, on the restatement alone: low [8] = the number of evaluated pairs with a margin below 10 tolerances, evaluated [8], and par_margin [8].
    The tolerance of a compared quantity (z in camera 1 and 2 against 0, each squared error against th2, the cosine against 0.99998) is its largest change when every
    coordinate of the float point moves one float step up, or down, or every entry of the float hypothesis does (the point re-triangulated from it and rounded):
    what the single roundings of the two fp64 stages can differ by.  A pair that left CheckRT before a quantity was compared has no margin for it."""
    res = run(w) if res is None else res
    n = len(w["xy1"]); nh = 0 if res["sv_exit"] else (8 if w["model"] == 0 else 4); inl = np.asarray(w["inlier"], bool); th2 = th2_of(w["sigma"])
    low = np.zeros(8, np.int32); ev = np.zeros(8, np.int32); pm = np.full(8, np.inf); worst_cos_tol = np.zeros(8)
    lim = dict(z1=0.0, z2=0.0, e1=float(th2), e2=float(th2), cos=COS_LOW)
    for h in range(nh):
        R, t, X = res["hyp_pose"][h, :, :3], res["hyp_pose"][h, :, 3], res["hyp_p3d"][h]
        st, _, q0 = check(R, t, w["K"], th2, inl, w["xy1"], w["xy2"], X)
        tol = {k: np.zeros(n) for k in lim}
        for up in (True, False):
            alts = [check(R, t, w["K"], th2, inl, w["xy1"], w["xy2"], _step(X, up))[2]]
            pose = _step(res["hyp_pose"][h], up); P2, _ = camera(pose[:, :3], pose[:, 3], w["K"])
            Xm = np.zeros((n, 3), F32); Xm[inl] = _to_f32(triangulate64(system(P2, w["K"], w["xy1"][inl], w["xy2"][inl])))
            alts.append(check(pose[:, :3], pose[:, 3], w["K"], th2, inl, w["xy1"], w["xy2"], Xm)[2])
            for q in alts:
                for k in lim:
                    with np.errstate(**_ERR):
                        tol[k] = np.fmax(tol[k], np.nan_to_num(np.abs(q[k].astype(F64) - q0[k].astype(F64)), nan=np.inf, posinf=np.inf))
        # which quantities a pair's exit compared: depth 1 -> z1, cos; depth 2 -> + z2; error 1 -> + e1; error 2 and the good ones -> + e2
        used = dict(z1=st >= DEPTH1, cos=st >= DEPTH1, z2=st >= DEPTH2, e1=st >= ERR1, e2=st >= ERR2)
        bad = np.zeros(n, bool)
        for k in lim:
            with np.errstate(**_ERR):
                m = np.abs(q0[k].astype(F64) - lim[k])/np.maximum(tol[k], 1e-300)
            bad |= used[k] & ~(m >= 10.0)
        low[h] = int(bad.sum()); ev[h] = int((st >= DEPTH1).sum())
        good = st >= GOOD
        if good.any():                                                  # the parallax: 10 x (the picked cosine's tolerance, in degrees) from min_parallax
            ctol = float(tol["cos"][good].max()); c = float(res["hyp_cos"][h])
            dpar = abs(math.degrees(math.acos(max(-1.0, min(1.0, c - ctol)))) - math.degrees(math.acos(max(-1.0, min(1.0, c + ctol))))) + 4*float(np.spacing(res["hyp_parallax"][h]))
            pm[h] = abs(float(res["hyp_parallax"][h]) - float(w["min_parallax"]))/max(dpar, 1e-300)
    return dict(low=low, evaluated=ev, par_margin=pm)


def keep_is_safe(w, res, mg, most=200000):
    """The keep logic gives the same ok, sel, N, exit bits (and F's nsimilar) for EVERY combination of counts within +- low[h] of the restatement's, and
    the parallax it compares is at least 10 tolerances from min_parallax.  (More combinations than `most`: not safe -- choose another world.)"""
    if res["sv_exit"]:
        return True
    nh = 8 if w["model"] == 0 else 4; g = res["hyp_good"].astype(int); lo = mg["low"].astype(int); N = int(res["result"][2])
    spans = [range(max(0, g[h] - lo[h]), min(N, g[h] + lo[h]) + 1) for h in range(nh)]
    if math.prod(len(r) for r in spans) > most:
        return False
    pick = (lambda r: (r[0], r[1], r[2], r[5])) if w["model"] == 0 else (lambda r: (r[0], r[1], r[2], r[4], r[5]))
    want = pick(res["result"].tolist())
    for combo in itertools.product(*spans):
        if pick(keep(w["model"], False, list(combo) + [0]*(8 - nh), res["hyp_parallax"], N, w["min_triangulated"], w["min_parallax"])) != want:
            return False
    b = int(np.argmax(g[:nh]))                                            # the hypothesis whose parallax the logic compares (the first of the best)
    return bool(g[b] == 0 or mg["par_margin"][b] >= 10.0)


def conditions_hold(w, res=None, mg=None):
    """(holds, margins): a kept hypothesis has no low-margin pair; in every other hypothesis at most 25 % of the evaluated pairs are low-margin; the keep logic is
    safe (keep_is_safe)."""
    res = run(w) if res is None else res; mg = decision_margins(w, res) if mg is None else mg
    if res["sv_exit"]:
        return True, mg
    nh = 8 if w["model"] == 0 else 4
    kept = int(res["result"][1])
    ok = (kept < 0 or mg["low"][kept] == 0) and all(mg["low"][h] <= 0.25*max(mg["evaluated"][h], 1) for h in range(nh) if h != kept)
    return bool(ok and keep_is_safe(w, res, mg)), mg

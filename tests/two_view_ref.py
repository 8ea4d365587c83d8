"""numpy restatement of the two-view initializer's RANSAC as docs/twoview_recalled.md states it: initializer::Normalize, ComputeH21 / ComputeF21 (A from the
reference's float products, then fp64: np.linalg.svd, the sign rule, one rounding to float), CheckHomography / CheckFundamental in float32 with the SEQUENTIAL sum,
the two keep loops.  What tsorb_match_two_view_ransac (include/tsorb.h, textslam_amd/csrc/tstwoview.h) is compared with, the worlds the tests commit to, and the
conditions those worlds have to meet (conditions, model_sensitivity, decision_margins, conditions_hold)."""
import math
import numpy as np

F32 = np.float32
TH_H = F32(5.991)
TH_F, TH_SCORE = F32(3.841), F32(5.991)
DEGENERATE = 1e-12                                                     # eigenvalue ratio of AtA (second smallest over largest) at or below which a subset is degenerate


def _seqsum(x):
    """The float32 sum in index order (np.add.accumulate carries one running value)."""
    x = np.ascontiguousarray(x, F32)
    return F32(np.add.accumulate(x, dtype=F32)[-1]) if x.size else F32(0)


# ---- initializer::Normalize (:819-865)
def normalize(keys):
    """meanX, meanY, sX, sY over ALL keypoints of a frame: sequential float sums, a float division by N, 1.0 / meanDev as a double division rounded to float."""
    keys = np.ascontiguousarray(keys, F32).reshape(-1, 2); N = F32(len(keys))
    mx, my = F32(_seqsum(keys[:, 0])/N), F32(_seqsum(keys[:, 1])/N)
    dx, dy = F32(_seqsum(np.abs(keys[:, 0] - mx))/N), F32(_seqsum(np.abs(keys[:, 1] - my))/N)
    with np.errstate(divide="ignore"):
        return np.array([mx, my, F32(1.0/np.float64(dx)), F32(1.0/np.float64(dy))], F32)


def normalized(xy, norm):
    xy = np.ascontiguousarray(xy, F32); norm = np.asarray(norm, F32)
    return np.stack([(xy[:, 0] - norm[0])*norm[2], (xy[:, 1] - norm[1])*norm[3]], axis=1).astype(F32)


def T_of(norm):
    norm = np.asarray(norm, F32)
    T = np.eye(3, dtype=F32); T[0, 0] = norm[2]; T[1, 1] = norm[3]; T[0, 2] = F32(-norm[0])*norm[2]; T[1, 2] = F32(-norm[1])*norm[3]
    return T


# ---- the fits
def sign_rule(v):
    k = int(np.argmax(np.abs(v)))                                       # the first of equal magnitudes
    return -v if v[k] < 0 else v


def system(model, p1, p2):
    """ComputeH21's 16 x 9 (model 0) or ComputeF21's 8 x 9 (model 1) in float32 from eight normalised float points."""
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]; z, o = np.zeros(8, F32), np.ones(8, F32)
    if model == 0:
        A = np.empty((16, 9), F32)
        A[0::2] = np.stack([z, z, z, -u1, -v1, -o, v2*u1, v2*v1, v2], axis=1)
        A[1::2] = np.stack([u1, v1, o, z, z, z, -u2*u1, -u2*v1, -u2], axis=1)
        return A
    return np.stack([u2*u1, u2*v1, u2, v2*u1, v2*v1, v2, u1, v1, o], axis=1).astype(F32)


def null_vector(A):
    """(unit right singular vector of the smallest singular value with the sign rule, or NaN for a degenerate subset; the eigenvalue ratio)."""
    _, s, Vt = np.linalg.svd(A)
    ev = np.sort(np.concatenate([s*s, np.zeros(9 - len(s))]))
    ratio = float(ev[1]/ev[-1]) if ev[-1] > 0 else 0.0
    if not ratio > DEGENERATE:
        return np.full(9, np.nan), ratio
    return sign_rule(Vt[8]/np.linalg.norm(Vt[8])), ratio


def fit(model, p1, p2, T1, T2, scale=1.0):
    """The fp64 model before its rounding (H21i = T2^-1 Hn T1 or F21i = T2^T Fn T1) and the subset's eigenvalue ratio.  scale multiplies A in double."""
    A = system(model, p1, p2).astype(np.float64)*scale
    v, ratio = null_vector(A)
    T1 = T1.astype(np.float64); T2 = T2.astype(np.float64)
    if model == 0:
        T2inv = np.array([[1.0/T2[0, 0], 0.0, -T2[0, 2]/T2[0, 0]], [0.0, 1.0/T2[1, 1], -T2[1, 2]/T2[1, 1]], [0.0, 0.0, 1.0]])
        return (T2inv @ v.reshape(3, 3)) @ T1, ratio
    if np.isnan(v).any():
        return np.full((3, 3), np.nan), ratio
    U, w, Vt = np.linalg.svd(v.reshape(3, 3)); w[2] = 0.0
    return (T2.T @ (U @ np.diag(w) @ Vt)) @ T1, ratio


def h_inverse(H):
    """H12i from the FLOAT H21i: adjugate over determinant in fp64, rounded to float; zeros for a zero determinant."""
    a, b, c, d, e, f, g, k, l = [np.float64(x) for x in np.asarray(H, F32).reshape(9)]
    with np.errstate(invalid="ignore"):
        adj = np.array([e*l - f*k, c*k - b*l, b*f - c*e, f*g - d*l, a*l - c*g, c*d - a*f, d*k - e*g, b*g - a*k, a*e - b*d])
        det = (a*adj[0] + b*adj[3]) + c*adj[6]
        return (np.zeros(9, F32) if det == 0.0 else (adj/det).astype(F32)).reshape(3, 3)


# ---- the scoring (float32 element by element: numpy rounds every product and sum, nothing is fused)
def _inv(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (1.0/x.astype(np.float64)).astype(F32)


def terms(model, M, xy1, xy2, sigma=1.0):
    """Per match: the two chi squares, the two score terms (0 where the reference adds nothing) and bIn."""
    M = np.asarray(M, F32).reshape(3, 3); xy1 = np.ascontiguousarray(xy1, F32); xy2 = np.ascontiguousarray(xy2, F32)
    u1, v1, u2, v2 = xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]
    sigma = F32(sigma); iss = F32(1.0/np.float64(sigma*sigma))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if model == 0:
            I = h_inverse(M)
            w2 = _inv(I[2, 0]*u2 + I[2, 1]*v2 + I[2, 2])
            a = (I[0, 0]*u2 + I[0, 1]*v2 + I[0, 2])*w2; b = (I[1, 0]*u2 + I[1, 1]*v2 + I[1, 2])*w2
            chi1 = ((u1 - a)*(u1 - a) + (v1 - b)*(v1 - b))*iss
            w1 = _inv(M[2, 0]*u1 + M[2, 1]*v1 + M[2, 2])
            a = (M[0, 0]*u1 + M[0, 1]*v1 + M[0, 2])*w1; b = (M[1, 0]*u1 + M[1, 1]*v1 + M[1, 2])*w1
            chi2 = ((u2 - a)*(u2 - a) + (v2 - b)*(v2 - b))*iss
            th, ths = TH_H, TH_H
        else:
            a2 = M[0, 0]*u1 + M[0, 1]*v1 + M[0, 2]; b2 = M[1, 0]*u1 + M[1, 1]*v1 + M[1, 2]; c2 = M[2, 0]*u1 + M[2, 1]*v1 + M[2, 2]
            num2 = a2*u2 + b2*v2 + c2
            chi1 = (num2*num2/(a2*a2 + b2*b2))*iss
            a1 = M[0, 0]*u2 + M[1, 0]*v2 + M[2, 0]; b1 = M[0, 1]*u2 + M[1, 1]*v2 + M[2, 1]; c1 = M[0, 2]*u2 + M[1, 2]*v2 + M[2, 2]
            num1 = a1*u1 + b1*v1 + c1
            chi2 = (num1*num1/(a1*a1 + b1*b1))*iss
            th, ths = TH_F, TH_SCORE
        assert chi1.dtype == F32 and chi2.dtype == F32
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, F32(0), ths - chi1).astype(F32); t2 = np.where(out2, F32(0), ths - chi2).astype(F32)
    return chi1, chi2, t1, t2, ~(out1 | out2)


def score(model, M, xy1, xy2, sigma=1.0):
    """(the sequential float sum over the matches in index order, first term then second; the mask)."""
    _, _, t1, t2, inl = terms(model, M, xy1, xy2, sigma)
    with np.errstate(invalid="ignore"):
        return _seqsum(np.stack([t1, t2], axis=1).reshape(-1)), inl


def score_scalar(model, M, xy1, xy2, sigma=1.0):
    """The same with np.float32 scalars in a plain loop, a transcription of :366-529 (slow: the tests hold score() equal to it on small inputs)."""
    M = np.asarray(M, F32).reshape(3, 3); s = F32(0); mask = []
    sigma = F32(sigma); iss = F32(1.0/np.float64(sigma*sigma)); I = h_inverse(M)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for (u1, v1), (u2, v2) in zip(np.asarray(xy1, F32), np.asarray(xy2, F32)):
            bIn = True
            if model == 0:
                w = F32(1.0/np.float64(I[2, 0]*u2 + I[2, 1]*v2 + I[2, 2]))
                a = (I[0, 0]*u2 + I[0, 1]*v2 + I[0, 2])*w; b = (I[1, 0]*u2 + I[1, 1]*v2 + I[1, 2])*w
                c1 = ((u1 - a)*(u1 - a) + (v1 - b)*(v1 - b))*iss
                w = F32(1.0/np.float64(M[2, 0]*u1 + M[2, 1]*v1 + M[2, 2]))
                a = (M[0, 0]*u1 + M[0, 1]*v1 + M[0, 2])*w; b = (M[1, 0]*u1 + M[1, 1]*v1 + M[1, 2])*w
                c2 = ((u2 - a)*(u2 - a) + (v2 - b)*(v2 - b))*iss
                th, ths = TH_H, TH_H
            else:
                a2 = M[0, 0]*u1 + M[0, 1]*v1 + M[0, 2]; b2 = M[1, 0]*u1 + M[1, 1]*v1 + M[1, 2]; c2_ = M[2, 0]*u1 + M[2, 1]*v1 + M[2, 2]
                n2 = a2*u2 + b2*v2 + c2_
                c1 = (n2*n2/(a2*a2 + b2*b2))*iss
                a1 = M[0, 0]*u2 + M[1, 0]*v2 + M[2, 0]; b1 = M[0, 1]*u2 + M[1, 1]*v2 + M[2, 1]; c1_ = M[0, 2]*u2 + M[1, 2]*v2 + M[2, 2]
                n1 = a1*u1 + b1*v1 + c1_
                c2 = (n1*n1/(a1*a1 + b1*b1))*iss
                th, ths = TH_F, TH_SCORE
            for c in (c1, c2):
                assert type(c) is F32
                if c > th:
                    bIn = False
                else:
                    s = F32(s + (ths - c))
            mask.append(bIn)
    return s, np.array(mask, bool)


def keep(scores):
    """FindHomography's / FindFundamental's loop: from 0.0, strictly greater (a NaN compares false).  (sel, score); sel = -1: nothing kept."""
    best, sel = F32(0), -1
    for h, s in enumerate(np.asarray(scores, F32)):
        if s > best:
            best, sel = s, h
    return sel, best


def derive(hyp_model, xy1, xy2, sigma=1.0):
    """Everything the call reports, from the FLOAT models [2, H, 3, 3]: hyp_score, sel, score, H21, F21, the masks."""
    hyp_model = np.asarray(hyp_model, F32); H = hyp_model.shape[1]; n = len(xy1)
    hs = np.zeros((2, H), F32)
    for m in range(2):
        for h in range(H):
            hs[m, h] = score(m, hyp_model[m, h], xy1, xy2, sigma)[0]
    out = dict(hyp_score=hs, sel=np.zeros(2, np.int32), score=np.zeros(2, F32))
    for m, (mk, ik) in enumerate((("H21", "inlier_h"), ("F21", "inlier_f"))):
        sel, best = keep(hs[m])
        out["sel"][m] = sel; out["score"][m] = best
        out[mk] = hyp_model[m, sel].copy() if sel >= 0 else np.zeros((3, 3), F32)
        out[ik] = score(m, hyp_model[m, sel], xy1, xy2, sigma)[1] if sel >= 0 else np.zeros(n, bool)
    return out


def RH(res):
    with np.errstate(invalid="ignore", divide="ignore"):
        return F32(res["score"][0]/F32(res["score"][0] + res["score"][1]))


def run(xy1, xy2, norm1, norm2, subsets, sigma=1.0, scale=1.0):
    """The whole call.  Also model64 [2, H, 3, 3] (the models before their rounding) and ratio [2, H] (the subsets' eigenvalue ratios)."""
    xy1 = np.ascontiguousarray(xy1, F32); xy2 = np.ascontiguousarray(xy2, F32)
    p1, p2, T1, T2 = normalized(xy1, norm1), normalized(xy2, norm2), T_of(norm1), T_of(norm2)
    H = len(subsets); m64 = np.zeros((2, H, 3, 3)); ratio = np.zeros((2, H))
    for m in range(2):
        for h, s in enumerate(subsets):
            m64[m, h], ratio[m, h] = fit(m, p1[s], p2[s], T1, T2, scale)
    hm = m64.astype(F32)
    out = derive(hm, xy1, xy2, sigma)
    out.update(hyp_model=hm, model64=m64, ratio=ratio)
    return out


# ---- the worlds
K_DEFAULT = (130.0, 130.0, 80.0, 60.0)
MIN_RATIO = 1e-6                                                       # every non-degenerate subset's eigenvalue ratio: a factor 1e6 above DEGENERATE


def subset_ratio(wd, s):
    """The smaller of the two models' eigenvalue ratios on subset s."""
    p1, p2 = normalized(wd["xy1"][s], wd["norm1"]), normalized(wd["xy2"][s], wd["norm2"])
    return min(null_vector(system(m, p1, p2).astype(np.float64))[1] for m in range(2))


def draw_subsets(g, wd, H, tries=200):
    """H subsets of eight distinct matches.  The caller draws the subsets and MIN_RATIO is a condition on the input: a subset under it is drawn again (the subsets that
    are meant to be degenerate are put in by hand afterwards).  n = 8: the one subset 0 .. 7."""
    n = wd["n"]
    if n == 8:
        return np.tile(np.arange(8, dtype=np.int32), (H, 1))
    out = []
    for _ in range(H):
        for _ in range(tries):
            s = g.choice(n, 8, replace=False)
            if subset_ratio(wd, s) >= MIN_RATIO:
                break
        out.append(s)
    return np.stack(out).astype(np.int32)


def world(kind, seed, n, outliers=0.0, H=200, noise=0.5, extra=23, K=K_DEFAULT, w=160, h=120):
    """Two views of n points in a small (160 x 120) image: kind "planar" (a tilted plane at depth about 4) or "general" (depths 2 - 8).  0.5 px pixel noise in both
    views, a share of matches whose second pixel is uniformly random, `extra` unmatched keypoints per frame (Normalize runs over ALL keypoints), the matches in a
    shuffled keypoint order."""
    g = np.random.default_rng(seed)
    ax = g.normal(size=3); ax /= np.linalg.norm(ax); ang = g.uniform(0.05, 0.15)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + math.sin(ang)*Kx + (1 - math.cos(ang))*(Kx @ Kx)
    t = np.array([g.uniform(0.3, 0.6)*g.choice([-1, 1]), g.uniform(-0.15, 0.15), g.uniform(-0.15, 0.15)])
    px = np.column_stack([g.uniform(10, w - 10, n), g.uniform(10, h - 10, n)])
    rays = np.column_stack([(px[:, 0] - K[2])/K[0], (px[:, 1] - K[3])/K[1], np.ones(n)])
    if kind == "planar":
        nrm = np.array([g.uniform(-0.15, 0.15), g.uniform(-0.15, 0.15), 1.0]); nrm /= np.linalg.norm(nrm)
        z = 4.0/(rays @ nrm)
    else:
        z = g.uniform(2.0, 8.0, n)
    X = rays*z[:, None]
    X2 = X @ R.T + t
    px2 = np.column_stack([K[0]*X2[:, 0]/X2[:, 2] + K[2], K[1]*X2[:, 1]/X2[:, 2] + K[3]])
    a = px + g.normal(0.0, noise, (n, 2)); b = px2 + g.normal(0.0, noise, (n, 2))
    n_out = int(round(outliers*n)); out = g.permutation(n)[:n_out]
    b[out] = np.column_stack([g.uniform(0, w, n_out), g.uniform(0, h, n_out)])
    truth = np.ones(n, bool); truth[out] = False
    return _assemble(g, dict(kind=kind, seed=seed, truth=truth, K=np.array(K), R=R, t=t), a, b, H, extra, w, h)


def _assemble(g, wd, a, b, H, extra, w, h):
    n = len(a)
    k1 = g.permutation(n + extra)[:n]; k2 = g.permutation(n + extra)[:n]
    keys1 = np.column_stack([g.uniform(0, w, n + extra), g.uniform(0, h, n + extra)]).astype(F32); keys2 = keys1[::-1].copy()
    keys1[k1] = a; keys2[k2] = b
    wd.update(n=n, keys1=keys1, keys2=keys2, matches=np.column_stack([k1, k2]).astype(np.int32), xy1=keys1[k1].copy(), xy2=keys2[k2].copy(),
              norm1=normalize(keys1), norm2=normalize(keys2), sigma=1.0)
    wd["subsets"] = draw_subsets(g, wd, H)
    return wd


def twice_world(seed=0, n=64, H=3):
    """A general world in which match n - 1 is a second copy of match 5's pixel pair and subset 0 holds both: F's 8 x 9 system has two equal rows and rank 7
    exactly (degenerate: a NaN F), while H's 16 x 9 keeps rank 9."""
    wd = world("general", seed, n, 0.0, H)
    for key, col in (("keys1", 0), ("keys2", 1)):
        wd[key][wd["matches"][n - 1, col]] = wd[key][wd["matches"][5, col]]
    wd["xy1"] = wd["keys1"][wd["matches"][:, 0]].copy(); wd["xy2"] = wd["keys2"][wd["matches"][:, 1]].copy()
    wd["norm1"], wd["norm2"] = normalize(wd["keys1"]), normalize(wd["keys2"])
    wd["subsets"][0] = [5, n - 1, 0, 1, 2, 3, 4, 6]
    wd["kind"] = "twice"
    return wd


def same_world(seed=0, n=64, H=3):
    """Every match is the same pixel pair (the unmatched keypoints keep Normalize finite): every subset is degenerate for both models, sel = -1, -1."""
    wd = world("general", seed, n, 0.0, H)
    wd["keys1"][wd["matches"][:, 0]] = wd["keys1"][wd["matches"][0, 0]]; wd["keys2"][wd["matches"][:, 1]] = wd["keys2"][wd["matches"][0, 1]]
    wd["xy1"] = wd["keys1"][wd["matches"][:, 0]].copy(); wd["xy2"] = wd["keys2"][wd["matches"][:, 1]].copy()
    wd["norm1"], wd["norm2"] = normalize(wd["keys1"]), normalize(wd["keys2"])
    wd["kind"] = "same"
    return wd


# The worlds the tests commit to: (kind, seed, n, outliers, H).  n = 8 (the one subset 0 .. 7), 9, 64, 65, 257, 300; 1, 3, 200, 256 hypotheses.
PLANAR, GENERAL, OUTLIERS = ("planar", 0, 64, 0.0, 200), ("general", 0, 65, 0.0, 256), ("general", 0, 300, 0.3, 200)
CASES = [("planar", 0, 8, 0.0, 1), ("general", 2, 9, 0.0, 3), PLANAR, GENERAL, ("planar", 0, 257, 0.3, 200), OUTLIERS]
SPECIAL = ["twice", "same"]
ALL = CASES + SPECIAL


def make(case):
    return twice_world() if case == "twice" else same_world() if case == "same" else world(*case)


def run_world(w, scale=1.0):
    return run(w["xy1"], w["xy2"], w["norm1"], w["norm2"], w["subsets"], w["sigma"], scale)


def model_sensitivity(w, res=None):
    """The largest change of any model entry, relative to that matrix's largest entry, when A is scaled by (1 + 1e-13) in double (before the rounding to float):
    1000 x this, or one float ulp of the matrix's largest entry if that is larger, is the device comparison's tolerance on a model."""
    res = run_world(w) if res is None else res
    a, b = res["model64"], run_world(w, 1.0 + 1e-13)["model64"]
    worst = 0.0
    for m in range(2):
        for h in range(a.shape[1]):
            if np.isfinite(a[m, h]).all() and np.isfinite(b[m, h]).all():
                worst = max(worst, float(np.abs(a[m, h] - b[m, h]).max()/np.abs(a[m, h]).max()))
    return worst


def model_tolerance(ref_model, sens):
    """Per hypothesis [2, H, 1, 1]: the larger of 1000 x sens x the matrix's largest entry and one float ulp of that entry."""
    big = np.abs(np.asarray(ref_model, F32)).max(axis=(2, 3), keepdims=True)
    with np.errstate(invalid="ignore"):
        return np.maximum(1000.0*sens*big.astype(np.float64), np.spacing(big).astype(np.float64))


def _moved_scores(w, res, m):
    """Per hypothesis of model m: the largest change of its score when every entry of its float model moves one float step up, or one step down."""
    d = np.zeros(res["hyp_model"].shape[1])
    for step in (np.inf, -np.inf):
        moved = np.nextafter(res["hyp_model"][m], F32(step)).astype(F32)
        for h in range(len(d)):
            if np.isfinite(res["hyp_score"][m, h]):
                d[h] = max(d[h], abs(float(score(m, moved[h], w["xy1"], w["xy2"], w["sigma"])[0]) - float(res["hyp_score"][m, h])))
    return d


def decision_margins(w, res):
    """How far the decisions are from what a model rounded the other way could change, measured on the restatement alone.  The fp64 fits of two SVD routines differ
    by about 1e-10 of an entry (1000 x model_sensitivity) and a float step is 6e-8 of it, so one float step is the most the single rounding can differ by; the
    tolerance of a score or a chi square is its largest change when EVERY entry of its float model moves one step up, or one step down.
    gap: the smallest over the hypotheses h other than the kept one of |kept score - score h| / (tolerance of the kept score + tolerance of score h);
    margin: the smallest over the kept hypotheses' terms of |chi^2 - th| / (that chi square's tolerance).  inf where nothing is compared."""
    gap, margin = math.inf, math.inf
    for m in range(2):
        sel = int(res["sel"][m])
        if sel < 0:
            continue
        d = _moved_scores(w, res, m); s = res["hyp_score"][m].astype(np.float64)
        for h in range(len(s)):
            if h != sel and np.isfinite(s[h]):
                gap = min(gap, abs(s[sel] - s[h])/max(d[sel] + d[h], 1e-30))
        th = float(TH_H if m == 0 else TH_F)
        c0 = terms(m, res["hyp_model"][m, sel], w["xy1"], w["xy2"], w["sigma"])[:2]
        dc = [np.zeros(len(c0[0])), np.zeros(len(c0[0]))]
        for step in (np.inf, -np.inf):
            c1 = terms(m, np.nextafter(res["hyp_model"][m, sel], F32(step)).astype(F32), w["xy1"], w["xy2"], w["sigma"])[:2]
            for k in range(2):
                with np.errstate(invalid="ignore"):
                    dc[k] = np.maximum(dc[k], np.abs(c0[k].astype(np.float64) - c1[k]))
        for k in range(2):
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.abs(c0[k].astype(np.float64) - th)/np.maximum(dc[k], 1e-30)
            r = r[np.isfinite(r)]
            if r.size:
                margin = min(margin, float(r.min()))
    return dict(gap=float(gap), margin=float(margin))


def conditions(w, res=None):
    """gap [2]: the smallest relative gap between the kept score and every other finite score, per model (inf with nothing to compare); margin: the smallest
    |chi^2 - th| over the kept hypotheses' terms; ratio: the smallest eigenvalue ratio over the non-degenerate subsets (inf when all are degenerate)."""
    res = run_world(w) if res is None else res
    gap, margin = [math.inf, math.inf], math.inf
    for m in range(2):
        sel = int(res["sel"][m])
        if sel < 0:
            continue
        s = res["hyp_score"][m].astype(np.float64); kept = s[sel]
        others = np.delete(s, sel); others = others[np.isfinite(others)]
        if others.size:
            gap[m] = float(np.min(np.abs(kept - others))/kept)
        c1, c2 = terms(m, res["hyp_model"][m, sel], w["xy1"], w["xy2"], w["sigma"])[:2]
        c = np.concatenate([c1, c2]).astype(np.float64); c = c[np.isfinite(c)]
        margin = min(margin, float(np.min(np.abs(c - float(TH_H if m == 0 else TH_F)))))
    r = res["ratio"][res["ratio"] > DEGENERATE]
    return dict(gap=gap, margin=margin, ratio=float(r.min()) if r.size else math.inf)


def conditions_hold(w, res, factor=10.0):
    """The device's decisions can be held equal to the restatement's outright: every gap and margin at least `factor` times the comparison's tolerance
    (decision_margins) and every non-degenerate eigenvalue ratio at least MIN_RATIO.  (holds, conditions, margins)"""
    c, t = conditions(w, res), decision_margins(w, res)
    return bool(t["gap"] >= factor and t["margin"] >= factor and c["ratio"] >= MIN_RATIO), c, t

"""Generates tests/golden/loop_edges.npz: single pose-graph connections (x1, x2, m) and what numer_loop_ver2 / logSim3 return on them at 60
digits (mpmath), rounded once to float64.

    python tests/golden/make_loop_edges.py

The residual of a connection is logSim3(m * S1 * S2^-1) (include/numer_loop_ver2.h:28-66, include/ModelTool.hpp:354-432).  restate() is that
function word for word -- the same quaternion algebra (x1, x2 normalised, m not), the same two thresholds (|sigma| < 1e-5, d > 1 - 1e-5), the same
constants in the series branches (A = 1/2, B = 1/6) and the same closed forms in the other three -- evaluated in mpmath; W upsilon = t goes through
mpmath's own lu_solve.  So the fixture says what the reference's function IS on these inputs, free of float64 rounding; it does not say what the true
logarithm is (the small-angle branches are approximations on purpose).

Every connection is built from the relative transform it is to have: E = (rotation by theta about an axis, translation, scale s); m = E * S2 * S1^-1
in mpmath, rounded to float64.  d, sigma and the branch are then taken from the ROUNDED inputs.  Nothing here comes from any implementation under test.

Stored per connection: name, x1, x2, m (float64), res [7], cost = |res|^2 / 2, d, sigma, branch (bit 0: |sigma| < eps, bit 1: d > 1 - eps),
swap [2] (whether a 3x3 elimination with partial pivoting of this W exchanges rows in column 0 / column 1) and near (1: the connection lies within
a differencing step's reach of a threshold; such connections are compared on the residual and the cost only)."""
import os
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loop_edges.npz")
DIGITS = 60
EPS = 0.00001                                # logSim3's eps, the float64 the reference compares with

# name, theta, axis, sigma (None: from s), s (None: from sigma; 1.0 with sigma 0: every scale exactly one), near
CASES = [
    ("both_sigma0",        1e-3, (0.3, -0.5, 0.8),   0.0,   None, 0),
    ("both_sigma5e-6",     1e-3, (0.3, -0.5, 0.8),   5e-6,  None, 0),
    ("small_sigma",        0.5,  (-0.6, 0.2, 0.7),   -5e-6, None, 0),
    ("small_angle",        2e-3, (0.5, 0.5, -0.4),   None,  1.2,  0),
    ("general",            0.5,  (0.1, 0.9, 0.3),    None,  1.2,  0),
    ("general_theta3",     3.0,  (0.4, -0.3, 0.85),  None,  0.8,  0),
    ("swap_col0",          2.9,  (0.05, 0.1, 1.0),   None,  0.8,  0),
    ("swap_col1",          2.9,  (1.0, 0.1, 0.05),   None,  0.8,  0),
    ("near_d_below",       ("d", "-1e-6"), (0.5, 0.5, -0.4), None, 1.2, 1),      # d = 1 - 1.1e-5: the general branch
    ("near_d_above",       ("d", "1e-6"), (0.5, 0.5, -0.4), None, 1.2, 1),      # d = 1 - 0.9e-5: the small-angle branch
    ("near_sigma_inside",  0.3,  (-0.6, 0.2, 0.7),   5e-6,  None, 1),
    ("near_sigma_outside", 0.3,  (-0.6, 0.2, 0.7),   -2e-5, None, 1),
]
T_REL = (0.21, -0.13, 0.34)                   # translation of the relative transform E
X1 = ((0.92, 0.21, -0.17, 0.28), (0.4, -0.2, 1.3))      # the constant keyframe: (q, t), q normalised below
X2 = ((0.85, -0.31, 0.35, 0.22), (-0.7, 0.5, 0.9))


def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


def q_mul(a, b):                              # Eigen quaternion product, (w, x, y, z)
    return [a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3],
            a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
            a[0]*b[2] + a[2]*b[0] + a[3]*b[1] - a[1]*b[3],
            a[0]*b[3] + a[3]*b[0] + a[1]*b[2] - a[2]*b[1]]


def q_rot(q, v):                              # Eigen's q * v: v + w (2 u x v) + u x (2 u x v), no normalisation
    uv = [2*(q[2]*v[2] - q[3]*v[1]), 2*(q[3]*v[0] - q[1]*v[2]), 2*(q[1]*v[1] - q[2]*v[0])]
    return [v[0] + q[0]*uv[0] + (q[2]*uv[2] - q[3]*uv[1]),
            v[1] + q[0]*uv[1] + (q[3]*uv[0] - q[1]*uv[2]),
            v[2] + q[0]*uv[2] + (q[1]*uv[1] - q[2]*uv[0])]


def q_unit(mp, q):
    n = mp.sqrt(sum(c*c for c in q))
    return [c/n for c in q]


def q_to_R(q):                                # Eigen toRotationMatrix (no normalisation)
    w, x, y, z = q
    return [[1 - 2*(y*y + z*z), 2*(x*y - w*z), 2*(x*z + w*y)],
            [2*(x*y + w*z), 1 - 2*(x*x + z*z), 2*(y*z - w*x)],
            [2*(x*z - w*y), 2*(y*z + w*x), 1 - 2*(x*x + y*y)]]


def restate(mp, x1, x2, m):
    """numer_loop_ver2::operator() and logSim3 on exact inputs -> (res [7], d, sigma, branch, W)."""
    x1 = [mp.mpf(float(v)) for v in x1]; x2 = [mp.mpf(float(v)) for v in x2]; m = [mp.mpf(float(v)) for v in m]
    q1 = q_unit(mp, x1[:4]); q2 = q_unit(mp, x2[:4])
    qw2 = [q2[0], -q2[1], -q2[2], -q2[3]]
    tw2 = q_rot(qw2, [(-1/x2[7])*c for c in x2[4:7]])
    sw2 = 1/x2[7]
    q12 = q_mul(q1, qw2)
    rt = q_rot(q1, tw2)
    t12 = [x1[7]*rt[k] + x1[4 + k] for k in range(3)]
    s12 = x1[7]*sw2
    rq = q_mul(m[:4], q12)
    mt = q_rot(m[:4], t12)
    t = [m[7]*mt[k] + m[4 + k] for k in range(3)]
    s = m[7]*s12
    # logSim3
    sigma = mp.log(s)
    R = q_to_R(rq)
    d = (R[0][0] + R[1][1] + R[2][2] - 1)/2
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    eps = mp.mpf(EPS)
    small_sigma, small_angle = abs(sigma) < eps, d > 1 - eps
    if small_sigma:
        Cc = mp.mpf(1)
        if small_angle:
            om = [c/2 for c in dR]; A = mp.mpf(1)/2; B = mp.mpf(1)/6
        else:
            th = mp.acos(d); om = [th/(2*mp.sqrt(1 - d*d))*c for c in dR]
            A = (1 - mp.cos(th))/(th*th); B = (th - mp.sin(th))/(th*th*th)
    else:
        Cc = (s - 1)/sigma
        if small_angle:
            s2 = sigma*sigma; om = [c/2 for c in dR]
            A = ((sigma - 1)*s + 1)/s2; B = ((s2/2 - sigma + 1)*s)/(s2*sigma)
        else:
            th = mp.acos(d); om = [th/(2*mp.sqrt(1 - d*d))*c for c in dR]
            a, b, c = s*mp.sin(th), s*mp.cos(th), th*th + sigma*sigma
            A = (a*sigma + (1 - b)*th)/(th*c); B = (Cc - ((b - 1)*sigma + a*th)/c)/(th*th)
    O = mp.matrix([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    W = A*O + B*O*O + Cc*mp.eye(3)
    ups = mp.lu_solve(W, mp.matrix(t))
    return om + [ups[k] for k in range(3)] + [sigma], d, sigma, int(small_sigma) | (int(small_angle) << 1), W


def pivot_swaps(W):
    """Per column 0, 1 of a 3x3 elimination with partial pivoting: (rows exchanged?, by how much the choice is decided: |chosen pivot| over the
    largest other candidate)."""
    A = [[W[i, j] for j in range(3)] for i in range(3)]
    out = []
    for c in range(2):
        piv = max(range(c, 3), key=lambda r: abs(A[r][c]))
        other = max(abs(A[r][c]) for r in range(c, 3) if r != piv)
        out.append((piv != c, abs(A[piv][c])/other if other else mp_inf()))
        A[c], A[piv] = A[piv], A[c]
        for r in range(c + 1, 3):
            f = A[r][c]/A[c][c]
            A[r] = [A[r][k] - f*A[c][k] for k in range(3)]
    return out


def mp_inf():
    return _mp().inf


def make_connection(mp, theta, axis, sigma, s):
    """(x1, x2, m) as float64 with m = E * S2 * S1^-1 rounded once; E = (theta about axis, T_REL, s)."""
    if isinstance(theta, tuple):                                   # ("d", offset): the angle whose cosine is 1 - eps + offset
        theta = mp.acos(1 - mp.mpf(EPS) + mp.mpf(theta[1]))
    theta = mp.mpf(theta)
    if s is None:
        s = mp.mpf(1) if sigma == 0.0 else mp.exp(mp.mpf(sigma))
        s1 = s2 = mp.mpf(1)                                        # sigma = 0: every scale exactly one, so that s is exactly one in float64 too
    else:
        s = mp.mpf(s); s1, s2 = mp.mpf("1.1"), mp.mpf("0.9")
    ax = [mp.mpf(a) for a in axis]; n = mp.sqrt(sum(a*a for a in ax)); ax = [a/n for a in ax]
    qE = [mp.cos(theta/2)] + [mp.sin(theta/2)*a for a in ax]
    tE = [mp.mpf(v) for v in T_REL]
    x1 = np.array(list(X1[0]) + list(X1[1]) + [float(s1)]); x1[:4] /= np.linalg.norm(x1[:4])
    x2 = np.array(list(X2[0]) + list(X2[1]) + [float(s2)]); x2[:4] /= np.linalg.norm(x2[:4])
    a = [mp.mpf(float(v)) for v in x1]; b = [mp.mpf(float(v)) for v in x2]
    q1 = q_unit(mp, a[:4]); q2 = q_unit(mp, b[:4])

    def mul(A, B):                                                 # (q, t, s) o (q, t, s)
        r = q_rot(A[0], B[1])
        return (q_mul(A[0], B[0]), [A[2]*r[k] + A[1][k] for k in range(3)], A[2]*B[2])

    def inv(A):
        qi = [A[0][0], -A[0][1], -A[0][2], -A[0][3]]
        return (qi, q_rot(qi, [-c/A[2] for c in A[1]]), 1/A[2])
    S1 = (q1, a[4:7], a[7]); S2 = (q2, b[4:7], b[7])
    M = mul(mul((qE, tE, s), S2), inv(S1))
    m = np.array([float(v) for v in M[0]] + [float(v) for v in M[1]] + [float(M[2])])
    return x1, x2, m


def compute():
    mp = _mp()
    out = {k: [] for k in ("name", "x1", "x2", "m", "res", "cost", "d", "sigma", "branch", "swap", "near")}
    for name, theta, axis, sigma, s, near in CASES:
        x1, x2, m = make_connection(mp, theta, axis, sigma, s)
        res, d, sg, branch, W = restate(mp, x1, x2, m)
        sw = pivot_swaps(W)
        out["name"].append(name); out["x1"].append(x1); out["x2"].append(x2); out["m"].append(m)
        out["res"].append([float(v) for v in res]); out["cost"].append(float(sum(v*v for v in res)/2))
        out["d"].append(float(d)); out["sigma"].append(float(sg)); out["branch"].append(branch)
        out["swap"].append([int(sw[0][0]), int(sw[1][0])]); out["near"].append(near)
        # what each connection is there for, from this file's own numbers
        eps = mp.mpf(EPS)
        want = {"both": 3, "smal": None, "gene": 0, "swap": 0, "near": None}[name[:4]]
        if name == "small_sigma": want = 1
        if name == "small_angle": want = 2
        if name == "near_d_below": want = 0; assert abs(d - (1 - eps - mp.mpf("1e-6"))) < mp.mpf("1e-9")
        if name == "near_d_above": want = 2; assert abs(d - (1 - eps + mp.mpf("1e-6"))) < mp.mpf("1e-9")
        if name == "near_sigma_inside": want = 1; assert abs(abs(sg) - mp.mpf("5e-6")) < mp.mpf("1e-12")
        if name == "near_sigma_outside": want = 0; assert abs(abs(sg) - mp.mpf("2e-5")) < mp.mpf("1e-12")
        assert branch == want, (name, branch, want)
        if name == "both_sigma0": assert sg == 0
        if not near:                                               # a differencing step (1e-6 |x|) stays on the same side of both thresholds
            assert abs(abs(sg) - eps) > mp.mpf("4e-6") and abs(d - (1 - eps)) > mp.mpf("4e-6"), (name, sg, d)
        if name == "swap_col0": assert sw[0][0] and sw[0][1] > 2, sw            # every choice decided by more than a factor of two
        if name == "swap_col1": assert not sw[0][0] and sw[0][1] > 2 and sw[1][0] and sw[1][1] > 2, sw
        assert all(np.isfinite(out["res"][-1]))
    F = {"name": np.array(out["name"]), "x1": np.array(out["x1"]), "x2": np.array(out["x2"]), "m": np.array(out["m"]),
         "res": np.array(out["res"]), "cost": np.array(out["cost"]), "d": np.array(out["d"]), "sigma": np.array(out["sigma"]),
         "branch": np.array(out["branch"], np.int32), "swap": np.array(out["swap"], np.int32), "near": np.array(out["near"], np.int32)}
    return F


if __name__ == "__main__":
    F = compute()
    np.savez(OUT, **F)
    for k, name in enumerate(F["name"]):
        print("%-20s branch %d  d = 1 - %.3e  sigma = %+.3e  swap %s  |res| = %.4f" % (name, F["branch"][k], 1 - F["d"][k], F["sigma"][k], F["swap"][k], np.linalg.norm(F["res"][k])))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")

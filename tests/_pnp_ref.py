"""Sequential float64 restatement of ORB_SLAM2::PnPsolver as the project pins
it: SetRansacParameters, iterate / Refine / CheckInliers
and the EPnP core with the pinned one-sided Jacobi SVD and the pinned order of
every reduction over the correspondences (256 strided partial sums, added in
ascending order).

The small-matrix steps are plain Python float arithmetic (IEEE double, one
rounding per + - * / sqrt). The per-correspondence terms are numpy elementwise
expressions written in the kernel's operation order, and they are accumulated
row by row, so no step relies on np.dot / @ / np.linalg.

A run also reports its margins: the smallest relative distance of any error2
to its threshold over every CheckInliers it evaluated, and whether a count
decision was fragile (see Margins)."""
import math

import numpy as np

RAND_MAX = 2147483647
PARTS = 256
MAX_SWEEPS = 30
JACOBI_TOL = 2.0 ** -46
EPS = 2.0 ** -52
INT_MIN = -2 ** 31
NAN = float("nan")
INF = float("inf")


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def _sqrt(x):
    if x < 0.0:
        return NAN
    return math.sqrt(x)


# ---------------------------------------------------------------- SetRansacParameters
def ransac_parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4,
                      epsilon=0.4, th2=5.991, sigma2=None):
    """PnPsolver::SetRansacParameters (:121-157). Returns (min_inliers,
    max_its, epsilon float32, max_error float32[N] or None)."""
    eps = np.float32(epsilon)
    with np.errstate(all="ignore"):
        n_min = int(np.float32(N) * eps)              # int * float -> float product
        if n_min < minInliers:
            n_min = minInliers
        if n_min < minSet:
            n_min = minSet
        ratio = np.float32(n_min) / np.float32(N)     # (float)min / N
        if eps < ratio:
            eps = ratio
        if n_min == N:
            n_it = 1
        else:
            e = float(eps)
            try:
                p3 = math.pow(e, 3)
                v = math.log(1 - probability) / math.log(1 - p3)
                v = math.ceil(v) if math.isfinite(v) else NAN
            except (ValueError, ZeroDivisionError, OverflowError):
                v = NAN
            n_it = int(v) if (v == v and -2147483649.0 < v < 2147483648.0) else INT_MIN
    max_its = max(1, min(n_it, maxIterations))
    max_error = None
    if sigma2 is not None:
        max_error = (np.asarray(sigma2, np.float32) * np.float32(th2)).astype(np.float32)
    return n_min, max_its, np.float32(eps), max_error


def random_int(raw, size):
    """DUtils::Random::RandomInt(0, size - 1) on the raw rand() value"""
    return int((float(raw) / (float(RAND_MAX) + 1.0)) * size)


def sample4(draws, N):
    """the minimal set: swap-with-back removal over mvAllIndices (:188-201)"""
    avail = list(range(N))
    out = []
    for i in range(4):
        r = random_int(draws[i], len(avail))
        r = min(max(r, 0), len(avail) - 1)
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


# ---------------------------------------------------------------- pinned Jacobi SVD
def svd_jacobi(A):
    """One-sided Jacobi SVD of the m x n list-of-rows A. Returns (U, s, V):
    U m x n (column k = A v_k / s_k, zero where s_k == 0), s descending, V n x n
    with the right singular vectors as columns."""
    m, n = len(A), len(A[0])
    a = [[float(A[i][k]) for i in range(m)] for k in range(n)]     # columns
    v = [[1.0 if i == k else 0.0 for i in range(n)] for k in range(n)]
    for _ in range(MAX_SWEEPS):
        rotations = 0
        for p in range(n - 1):
            for q in range(p + 1, n):
                cp, cq = a[p], a[q]
                alpha = beta = gamma = 0.0
                for i in range(m):
                    alpha = alpha + cp[i] * cp[i]
                    beta = beta + cq[i] * cq[i]
                    gamma = gamma + cp[i] * cq[i]
                if not (abs(gamma) > JACOBI_TOL * _sqrt(alpha * beta)):
                    continue
                zeta = _div(beta - alpha, 2.0 * gamma)
                t = _div(1.0, abs(zeta) + _sqrt(1.0 + zeta * zeta))
                if zeta < 0.0:
                    t = -t
                c = _div(1.0, _sqrt(1.0 + t * t))
                sn = c * t
                a[p] = [c * x - sn * y for x, y in zip(cp, cq)]
                a[q] = [sn * x + c * y for x, y in zip(cp, cq)]
                vp, vq = v[p], v[q]
                v[p] = [c * x - sn * y for x, y in zip(vp, vq)]
                v[q] = [sn * x + c * y for x, y in zip(vp, vq)]
                rotations += 1
        if not rotations:
            break
    s = []
    for k in range(n):
        ss = 0.0
        for x in a[k]:
            ss = ss + x * x
        s.append(_sqrt(ss))
    for k in range(n - 1):
        best = k
        for j in range(k + 1, n):
            if s[j] > s[best]:
                best = j
        if best != k:
            s[k], s[best] = s[best], s[k]
            a[k], a[best] = a[best], a[k]
            v[k], v[best] = v[best], v[k]
    U = [[(_div(a[k][i], s[k]) if s[k] > 0.0 else 0.0) for k in range(n)] for i in range(m)]
    V = [[v[k][i] for k in range(n)] for i in range(n)]
    return U, s, V


def svd_in_rank(s, k, m, n):
    return s[k] > s[0] * (float(max(m, n)) * EPS)


def svd_solve(A, b):
    m, n = len(A), len(A[0])
    U, s, V = svd_jacobi(A)
    y = []
    for k in range(n):
        acc = 0.0
        if svd_in_rank(s, k, m, n):
            for i in range(m):
                acc = acc + U[i][k] * b[i]
            acc = _div(acc, s[k])
        y.append(acc)
    x = []
    for j in range(n):
        acc = 0.0
        for k in range(n):
            acc = acc + V[j][k] * y[k]
        x.append(acc)
    return x


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(a, b):
    return ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) +
            (a[2] - b[2]) * (a[2] - b[2]))


def qr_solve_6x4(A, b, x):
    """PnPsolver::qr_solve (:860-950) as written; A, b, x are modified"""
    nr, nc = 6, 4
    A1, A2 = [0.0] * 4, [0.0] * 4
    for k in range(nc):
        eta = abs(A[k][k])
        for i in range(k + 1, nr):
            elt = abs(A[i - 1][k])
            if eta < elt:
                eta = elt
        if eta == 0:
            return
        inv_eta = _div(1.0, eta)
        sm = 0.0
        for i in range(k, nr):
            A[i][k] = A[i][k] * inv_eta
            sm = sm + A[i][k] * A[i][k]
        sigma = _sqrt(sm)
        if A[k][k] < 0:
            sigma = -sigma
        A[k][k] = A[k][k] + sigma
        A1[k] = sigma * A[k][k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            sm = 0.0
            for i in range(k, nr):
                sm = sm + A[i][k] * A[i][j]
            tau = _div(sm, A1[k])
            for i in range(k, nr):
                A[i][j] = A[i][j] - tau * A[i][k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau = tau + A[i][j] * b[i]
        tau = _div(tau, A1[j])
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i][j]
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        sm = 0.0
        for j in range(i + 1, nc):
            sm = sm + A[i][j] * x[j]
        x[i] = _div(b[i] - sm, A2[i])


def gauss_newton(L, rho, betas):
    x = [0.0, 0.0, 0.0, 0.0]
    b0 = betas
    for _ in range(5):
        a, b = [], []
        for i in range(6):
            r = L[i]
            a.append([2 * r[0] * b0[0] + r[1] * b0[1] + r[3] * b0[2] + r[6] * b0[3],
                      r[1] * b0[0] + 2 * r[2] * b0[1] + r[4] * b0[2] + r[7] * b0[3],
                      r[3] * b0[0] + r[4] * b0[1] + 2 * r[5] * b0[2] + r[8] * b0[3],
                      r[6] * b0[0] + r[7] * b0[1] + r[8] * b0[2] + 2 * r[9] * b0[3]])
            b.append(rho[i] - (r[0] * b0[0] * b0[0] + r[1] * b0[0] * b0[1] +
                               r[2] * b0[1] * b0[1] + r[3] * b0[0] * b0[2] +
                               r[4] * b0[1] * b0[2] + r[5] * b0[2] * b0[2] +
                               r[6] * b0[0] * b0[3] + r[7] * b0[1] * b0[3] +
                               r[8] * b0[2] * b0[3] + r[9] * b0[3] * b0[3]))
        qr_solve_6x4(a, b, x)
        for i in range(4):
            b0[i] = b0[i] + x[i]


def find_betas_approx(which, L, rho):
    if which == 1:
        col = (0, 1, 3, 6)
        b = svd_solve([[L[i][c] for c in col] for i in range(6)], rho)
        if b[0] < 0:
            b0 = _sqrt(-b[0])
            return [b0, _div(-b[1], b0), _div(-b[2], b0), _div(-b[3], b0)]
        b0 = _sqrt(b[0])
        return [b0, _div(b[1], b0), _div(b[2], b0), _div(b[3], b0)]
    nc = 3 if which == 2 else 5
    b = svd_solve([[L[i][c] for c in range(nc)] for i in range(6)], rho)
    if b[0] < 0:
        b0 = _sqrt(-b[0])
        b1 = _sqrt(-b[2]) if b[2] < 0 else 0.0
    else:
        b0 = _sqrt(b[0])
        b1 = _sqrt(b[2]) if b[2] > 0 else 0.0
    if b[1] < 0:
        b0 = -b0
    return [b0, b1, 0.0 if which == 2 else _div(b[3], b0), 0.0]


# ---------------------------------------------------------------- pinned reduction
def reduce_points(terms):
    """terms[n, C, T]: point i adds terms[i, c, 0], then terms[i, c, 1], ... to
    accumulator c. Partial j sums the points j, j + 256, ... in ascending
    order; the partials are then added in ascending order. Returns C floats."""
    terms = np.asarray(terms, np.float64)
    n, C, T = terms.shape
    rows = (n + PARTS - 1) // PARTS
    part = np.zeros((PARTS, C))
    with np.errstate(all="ignore"):
        for r in range(rows):
            blk = terms[r * PARTS:(r + 1) * PARTS]
            for t in range(T):
                part[:len(blk)] = part[:len(blk)] + blk[:, :, t]
        tot = np.zeros(C)
        for j in range(min(PARTS, n)):
            tot = tot + part[j]
    return [float(x) for x in tot]


# ---------------------------------------------------------------- EPnP
def compute_pose(cam, pw, uv):
    """PnPsolver::compute_pose (:477-525). cam = (fu, fv, uc, vc); pw[n, 3],
    uv[n, 2] float64. Returns (R as 9 floats row-major, t as 3 floats)."""
    fu, fv, uc, vc = (float(c) for c in cam)
    pw = np.asarray(pw, np.float64).reshape(-1, 3)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    n = len(pw)
    dn = float(n)
    with np.errstate(all="ignore"):
        # choose_control_points
        c0 = [_div(x, dn) for x in reduce_points(pw[:, :, None])]
        d = pw - np.array(c0)
        G = reduce_points((d[:, :, None] * d[:, None, :]).reshape(n, 9, 1))
        _, s3, V3 = svd_jacobi([G[0:3], G[3:6], G[6:9]])
        cws = [c0]
        for i in range(1, 4):
            k = _sqrt(_div(s3[i - 1], dn))
            cws.append([c0[j] + k * V3[j][i - 1] for j in range(3)])
        cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
        U, s3, V3 = svd_jacobi(cc)
        ci = [[0.0] * 3 for _ in range(3)]
        for j in range(3):
            for i in range(3):
                v = 0.0
                for k in range(3):
                    if svd_in_rank(s3, k, 3, 3):
                        v = v + V3[j][k] * _div(U[i][k], s3[k])
                ci[j][i] = v
        # compute_barycentric_coordinates, per point
        al = np.empty((n, 4))
        for j in range(3):
            al[:, 1 + j] = (ci[j][0] * (pw[:, 0] - c0[0]) + ci[j][1] * (pw[:, 1] - c0[1]) +
                            ci[j][2] * (pw[:, 2] - c0[2]))
        al[:, 0] = 1.0 - al[:, 1] - al[:, 2] - al[:, 3]
        # fill_M and MtM, half a row per reduction
        M1 = np.zeros((n, 12))
        M2 = np.zeros((n, 12))
        for j in range(4):
            M1[:, 3 * j] = al[:, j] * fu
            M1[:, 3 * j + 2] = al[:, j] * (uc - uv[:, 0])
            M2[:, 3 * j + 1] = al[:, j] * fv
            M2[:, 3 * j + 2] = al[:, j] * (vc - uv[:, 1])
        mtm = [[0.0] * 12 for _ in range(12)]
        for h in range(24):
            ra, b0 = h >> 1, (h & 1) * 6
            terms = np.stack([M1[:, ra:ra + 1] * M1[:, b0:b0 + 6],
                              M2[:, ra:ra + 1] * M2[:, b0:b0 + 6]], axis=2)
            mtm[ra][b0:b0 + 6] = reduce_points(terms)
        _, _, V = svd_jacobi(mtm)
        # compute_L_6x10 / compute_rho: v[i] = column 11 - i of V
        vv = [[V[r][11 - i] for r in range(12)] for i in range(4)]
        dv = [[None] * 6 for _ in range(4)]
        for i in range(4):
            a, b = 0, 1
            for j in range(6):
                dv[i][j] = [vv[i][3 * a + k] - vv[i][3 * b + k] for k in range(3)]
                b += 1
                if b > 3:
                    a += 1
                    b = a + 1
        L = []
        for i in range(6):
            L.append([dot3(dv[0][i], dv[0][i]), 2.0 * dot3(dv[0][i], dv[1][i]),
                      dot3(dv[1][i], dv[1][i]), 2.0 * dot3(dv[0][i], dv[2][i]),
                      2.0 * dot3(dv[1][i], dv[2][i]), dot3(dv[2][i], dv[2][i]),
                      2.0 * dot3(dv[0][i], dv[3][i]), 2.0 * dot3(dv[1][i], dv[3][i]),
                      2.0 * dot3(dv[2][i], dv[3][i]), dot3(dv[3][i], dv[3][i])])
        rho = [dist2(cws[0], cws[1]), dist2(cws[0], cws[2]), dist2(cws[0], cws[3]),
               dist2(cws[1], cws[2]), dist2(cws[1], cws[3]), dist2(cws[2], cws[3])]
        sols = []
        for sol in range(3):
            betas = find_betas_approx(sol + 1, L, rho)
            gauss_newton(L, rho, betas)
            ccs = [[0.0] * 3 for _ in range(4)]
            for i in range(4):
                for j in range(4):
                    for k in range(3):
                        ccs[j][k] = ccs[j][k] + betas[i] * vv[i][3 * j + k]

            def pcs_of(ccs):
                return np.stack([al[:, 0] * ccs[0][j] + al[:, 1] * ccs[1][j] +
                                 al[:, 2] * ccs[2][j] + al[:, 3] * ccs[3][j] for j in range(3)],
                                axis=1)
            if pcs_of(ccs)[0, 2] < 0.0:
                ccs = [[-x for x in row] for row in ccs]
            pcs = pcs_of(ccs)
            pc0 = [_div(x, dn) for x in reduce_points(pcs[:, :, None])]
            dp = pcs - np.array(pc0)
            abt = reduce_points((dp[:, :, None] * d[:, None, :]).reshape(n, 9, 1))
            U, s3, V3 = svd_jacobi([abt[0:3], abt[3:6], abt[6:9]])
            if not svd_in_rank(s3, 2, 3, 3):
                U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1]
                U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1]
                U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1]
            R = [dot3(U[i], V3[j]) for i in range(3) for j in range(3)]
            det = (R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] -
                   R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7])
            if det < 0:
                R[6], R[7], R[8] = -R[6], -R[7], -R[8]
            t = [pc0[0] - dot3(R[0:3], c0), pc0[1] - dot3(R[3:6], c0),
                 pc0[2] - dot3(R[6:9], c0)]
            # reprojection_error
            Xc = (R[0] * pw[:, 0] + R[1] * pw[:, 1] + R[2] * pw[:, 2]) + t[0]
            Yc = (R[3] * pw[:, 0] + R[4] * pw[:, 1] + R[5] * pw[:, 2]) + t[1]
            inv_Zc = 1.0 / ((R[6] * pw[:, 0] + R[7] * pw[:, 1] + R[8] * pw[:, 2]) + t[2])
            ue = uc + fu * Xc * inv_Zc
            ve = vc + fv * Yc * inv_Zc
            e = np.sqrt((uv[:, 0] - ue) * (uv[:, 0] - ue) + (uv[:, 1] - ve) * (uv[:, 1] - ve))
            err = _div(reduce_points(e.reshape(n, 1, 1))[0], dn)
            sols.append((err, R, t))
    best = 0
    if sols[1][0] < sols[0][0]:
        best = 1
    if sols[2][0] < sols[best][0]:
        best = 2
    return sols[best][1], sols[best][2]


def check_inliers(cam, R, t, p3d, p2d, max_error):
    """PnPsolver::CheckInliers (:308-339) with its mixed precision. Returns
    (mask bool[N], error2 float32[N])."""
    fu, fv, uc, vc = (float(c) for c in cam)
    f32 = np.float32
    p3 = np.asarray(p3d, f32).astype(np.float64)
    p2 = np.asarray(p2d, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        Xc = (R[0] * p3[:, 0] + R[1] * p3[:, 1] + R[2] * p3[:, 2] + t[0]).astype(f32)
        Yc = (R[3] * p3[:, 0] + R[4] * p3[:, 1] + R[5] * p3[:, 2] + t[1]).astype(f32)
        invZc = (1 / (R[6] * p3[:, 0] + R[7] * p3[:, 1] + R[8] * p3[:, 2] + t[2])).astype(f32)
        ue = uc + fu * Xc.astype(np.float64) * invZc.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZc.astype(np.float64)
        dX = (p2[:, 0] - ue).astype(f32)
        dY = (p2[:, 1] - ve).astype(f32)
        e2 = dX * dX + dY * dY
        mask = e2 < np.asarray(max_error, f32)
    return mask, e2


def pose_to_Tcw(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array(R, np.float64).reshape(3, 3).astype(np.float32)
    T[:3, 3] = np.array(t, np.float64).astype(np.float32)
    return T


class Margins:
    """min_rel: the smallest |error2 - max_error| / max_error over every
    CheckInliers evaluated (an error2 that is not a number is an outlier at any
    rounding and does not count). count_fragile: some count decision (>= min, >
    best, Refine's > min) sat next to its boundary - one label would flip it -
    in an evaluation that had a point within NEAR of its threshold. Only such a
    point can change label under rounding-sized differences; a count on its
    boundary whose every point is far from its threshold (the N = 20 /
    10-inlier case has one by construction, and every second pure-inlier
    hypothesis ties the best count) is decided identically by any
    implementation of P28."""
    NEAR = 1e-2

    def __init__(self):
        self.min_rel = INF
        self.count_fragile = False

    def see(self, e2, max_error, decisions):
        """decisions: [(count, bound, strict)]: count > bound or count >= bound"""
        me = np.asarray(max_error, np.float64)
        with np.errstate(all="ignore"):
            rel = np.abs(e2.astype(np.float64) - me) / me
        rel = rel[np.isfinite(rel)]
        m = float(rel.min()) if len(rel) else INF
        self.min_rel = min(self.min_rel, m)
        for count, bound, strict in decisions:
            edge = (count in (bound, bound + 1)) if strict else (count in (bound - 1, bound))
            if edge and m < self.NEAR:
                self.count_fragile = True


class PnPsolver:
    """The whole class over explicit correspondences. State persists across
    iterate() calls as in the reference."""

    def __init__(self, cam, p2d, sigma2, p3d):
        self.cam = tuple(float(np.float32(c)) for c in cam)
        self.p2d = np.asarray(p2d, np.float32).reshape(-1, 2)
        self.p3d = np.asarray(p3d, np.float32).reshape(-1, 3)
        self.sigma2 = np.asarray(sigma2, np.float32).reshape(-1)
        self.N = len(self.p2d)
        self.iterations = 0
        self.best_inliers = 0
        self.best_mask = np.zeros(self.N, bool)
        self.best_Tcw = np.zeros((4, 4), np.float32)
        self.margins = Margins()
        self._refined_for = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4,
                            epsilon=0.4, th2=5.991):
        assert minSet == 4
        self.min_inliers, self.max_its, self.epsilon, self.max_error = ransac_parameters(
            self.N, probability, minInliers, maxIterations, minSet, epsilon, th2, self.sigma2)

    def hypotheses(self, n_iterations):
        if self.N < self.min_inliers:
            return 0
        return max(0, self.max_its - self.iterations, n_iterations)

    def _refine(self):
        idx = np.flatnonzero(self.best_mask)
        R, t = compute_pose(self.cam, self.p3d[idx].astype(np.float64),
                            self.p2d[idx].astype(np.float64))
        mask, e2 = check_inliers(self.cam, R, t, self.p3d, self.p2d, self.max_error)
        n = int(mask.sum())
        self.margins.see(e2, self.max_error, [(n, self.min_inliers, True)])
        return n, mask, pose_to_Tcw(R, t)

    def iterate(self, n_iterations, draws):
        """Returns dict(result, no_more, n_inliers, inliers bool[N], Tcw
        float32[4, 4], draws_consumed)."""
        out = dict(result=0, no_more=False, n_inliers=0, inliers=np.zeros(self.N, bool),
                   Tcw=np.zeros((4, 4), np.float32), draws_consumed=0)
        if self.N < self.min_inliers:
            out["no_more"] = True
            return out
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:
            d = draws[4 * cur:4 * cur + 4]
            assert len(d) == 4, "not enough draws"
            cur += 1
            self.iterations += 1
            out["draws_consumed"] = 4 * cur
            idx = sample4(d, self.N)
            R, t = compute_pose(self.cam, self.p3d[idx].astype(np.float64),
                                self.p2d[idx].astype(np.float64))
            mask, e2 = check_inliers(self.cam, R, t, self.p3d, self.p2d, self.max_error)
            n = int(mask.sum())
            self.margins.see(e2, self.max_error, [(n, self.min_inliers, False),
                                                  (n, self.best_inliers, True)])
            if n >= self.min_inliers:
                if n > self.best_inliers:
                    self.best_mask = mask.copy()
                    self.best_inliers = n
                    self.best_Tcw = pose_to_Tcw(R, t)
                    self._refined_for = None
                # Refine() depends on the best set only: computed when it changed
                if self._refined_for is None:
                    self._refined_for = self._refine()
                rn, rmask, rT = self._refined_for
                if rn > self.min_inliers:
                    out.update(result=1, n_inliers=rn, inliers=rmask.copy(), Tcw=rT.copy())
                    return out
        if self.iterations >= self.max_its:
            out["no_more"] = True
            if self.best_inliers >= self.min_inliers:
                out.update(result=2, n_inliers=self.best_inliers, inliers=self.best_mask.copy(),
                           Tcw=self.best_Tcw.copy())
        return out

    def state(self):
        return dict(iterations=self.iterations, best_inliers=self.best_inliers,
                    best_mask=self.best_mask.copy(), best_Tcw=self.best_Tcw.copy())

"""Sequential restatement of ORB_SLAM2::Sim3Solver as the project pins it
(DESIGN.md P53-P58): the constructor, SetRansacParameters, iterate / find,
ComputeSim3 (Horn's closed form on three correspondences) with the pinned
cyclic Jacobi eigen-decomposition, and CheckInliers / Project.

ComputeSim3 is scalar arithmetic, loop by loop: numpy.float32 scalars where the
reference holds CV_32F (one rounding per + - * /), Python floats (IEEE double)
where the pins say double. CheckInliers is numpy elementwise over the
correspondences in the kernel's operation order. No step relies on np.dot / @
/ np.linalg. sin / cos / atan2 are the platform's double functions rounded once
to float (P55, P56), as tests/_localmap_ref.py does for P12.

A run also reports its margins: the smallest relative distance of any err1 /
err2 to its threshold over every CheckInliers it evaluated, and whether a count
decision was fragile (see Margins)."""
import math

import numpy as np

F = np.float32
RAND_MAX = 2147483647
MAX_SWEEPS = 30
JACOBI_TOL = 2.0 ** -52
DBL_EPS = 2.0 ** -52
INT_MIN = -2 ** 31
INT_MAX = 2 ** 31 - 1
NAN = float("nan")
INF = float("inf")


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def _trig(fn, *x):
    try:
        return fn(*x)
    except ValueError:      # sin / cos of an infinity
        return NAN


# ---------------------------------------------------------------- SetRansacParameters
def ransac_parameters(N, probability=0.99, minInliers=6, maxIterations=300):
    """Sim3Solver::SetRansacParameters (:114-138). Returns mRansacMaxIts."""
    if minInliers == N:
        n_it = 1
    else:
        with np.errstate(all="ignore"):
            eps = float(F(minInliers) / F(N))
        try:
            v = math.log(1 - probability) / math.log(1 - math.pow(eps, 3))
            v = math.ceil(v) if math.isfinite(v) else NAN
        except (ValueError, ZeroDivisionError, OverflowError):
            v = NAN
        n_it = int(v) if (v == v and -2147483649.0 < v < 2147483648.0) else INT_MIN
    return max(1, min(n_it, maxIterations))


# ---------------------------------------------------------------- the constructor
def max_error(sigma2):
    """mvnMaxError's entry: 9.210 * sigma2 in double, truncated toward zero
    (vector<size_t>)"""
    v = 9.210 * float(F(sigma2))
    if not v >= 0.0:
        return 0
    if v >= 2147483647.0:
        return INT_MAX
    return int(v)


def transform(R, t, X):
    """R * X + t as one gemm (P6): products and t added in double, rounded
    once. R: 9 float32, t: 3, X: 3."""
    out = []
    for i in range(3):
        acc = (float(R[3 * i]) * float(X[0]) + float(R[3 * i + 1]) * float(X[1])) \
            + float(R[3 * i + 2]) * float(X[2])
        out.append(F(acc + float(t[i])))
    return out


def to_image(Xc, cam):
    with np.errstate(all="ignore"):
        invz = F(1.0) / Xc[2]
        x = Xc[0] * invz
        y = Xc[1] * invz
        return [F(cam[0]) * x + F(cam[2]), F(cam[1]) * y + F(cam[3])]


def setup(pair, level_sigma2):
    """The constructor (:37-112). pair: dict with matched12 [n1], valid1 [n1],
    xyz1 [n1, 3], octave1 [n1], valid2 [n2], xyz2 [n2, 3], octave2 [n2], Tcw1,
    Tcw2 [4, 4], cam. Returns the compacted arrays."""
    T1 = np.asarray(pair["Tcw1"], F).reshape(4, 4)
    T2 = np.asarray(pair["Tcw2"], F).reshape(4, 4)
    R1, t1 = [T1[i, j] for i in range(3) for j in range(3)], [T1[i, 3] for i in range(3)]
    R2, t2 = [T2[i, j] for i in range(3) for j in range(3)], [T2[i, 3] for i in range(3)]
    cam = [F(c) for c in pair["cam"]]
    n2 = len(pair["valid2"])
    ind, X1, X2, i1, i2, m1, m2 = [], [], [], [], [], [], []
    for i, m in enumerate(pair["matched12"]):
        m = int(m)
        if m == -1:                     # vpMatched12[i1] is NULL
            continue
        if not pair["valid1"][i]:       # no pMP1, or pMP1 is bad
            continue
        if m < 0 or m >= n2:            # indexKF2 < 0
            continue
        if not pair["valid2"][m]:       # pMP2 is bad
            continue
        a = transform(R1, t1, np.asarray(pair["xyz1"][i], F))
        b = transform(R2, t2, np.asarray(pair["xyz2"][m], F))
        ind.append(i)
        X1.append(a)
        X2.append(b)
        i1.append(to_image(a, cam))
        i2.append(to_image(b, cam))
        m1.append(max_error(level_sigma2[int(pair["octave1"][i])]))
        m2.append(max_error(level_sigma2[int(pair["octave2"][m])]))
    n = len(ind)
    return dict(n=n, indices1=np.array(ind, np.int32),
                X3Dc1=np.array(X1, F).reshape(n, 3), X3Dc2=np.array(X2, F).reshape(n, 3),
                P1im1=np.array(i1, F).reshape(n, 2), P2im2=np.array(i2, F).reshape(n, 2),
                max_error1=np.array(m1, np.int32), max_error2=np.array(m2, np.int32))


# ---------------------------------------------------------------- sampling
def random_int(raw, size):
    """DUtils::Random::RandomInt(0, size - 1) on the raw rand() value"""
    return int((float(raw) / (float(RAND_MAX) + 1.0)) * size)


def sample3(draws, N):
    """the minimal set: swap-with-back removal over mvAllIndices (:163-177)"""
    avail = list(range(N))
    out = []
    for i in range(3):
        r = random_int(draws[i], len(avail))
        r = min(max(r, 0), len(avail) - 1)
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


# ---------------------------------------------------------------- pinned cv::eigen (P54)
def eig_jacobi4(a):
    """Cyclic two-sided Jacobi on the symmetric 4 x 4 list-of-rows a (Python
    floats, changed in place). Returns (k, v): the column of the largest
    eigenvalue (first among equals) and the eigenvectors as columns of v; the
    eigenvalues are left on the diagonal of a."""
    ss = 0.0
    for i in range(4):
        for j in range(4):
            ss = ss + a[i][j] * a[i][j]
    v = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    thr = JACOBI_TOL * (math.sqrt(ss) if ss == ss else NAN)
    for _ in range(MAX_SWEEPS):
        rotations = 0
        for p in range(3):
            for q in range(p + 1, 4):
                apq = a[p][q]
                if not abs(apq) > thr:
                    continue
                theta = _div(a[q][q] - a[p][p], 2.0 * apq)
                t = _div(1.0, abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                a[p][p] = a[p][p] - t * apq
                a[q][q] = a[q][q] + t * apq
                a[p][q] = 0.0
                a[q][p] = 0.0
                for r in range(4):
                    if r == p or r == q:
                        continue
                    arp, arq = a[r][p], a[r][q]
                    a[r][p] = c * arp - s * arq
                    a[p][r] = a[r][p]
                    a[r][q] = s * arp + c * arq
                    a[q][r] = a[r][q]
                for r in range(4):
                    vrp, vrq = v[r][p], v[r][q]
                    v[r][p] = c * vrp - s * vrq
                    v[r][q] = s * vrp + c * vrq
                rotations += 1
        if not rotations:
            break
    k = 0
    for j in range(1, 4):
        if a[j][j] > a[k][k]:
            k = j
    return k, v


def _dot3d(a, b):
    return (float(a[0]) * float(b[0]) + float(a[1]) * float(b[1])) + float(a[2]) * float(b[2])


def horn_N(P1, P2):
    """steps 1-3 of ComputeSim3: returns (O1, O2, Pr1, Pr2, N as 4 x 4 float32)"""
    three = F(3.0)
    O1 = [((P1[r][0] + P1[r][1]) + P1[r][2]) / three for r in range(3)]
    O2 = [((P2[r][0] + P2[r][1]) + P2[r][2]) / three for r in range(3)]
    Pr1 = [[P1[r][c] - O1[r] for c in range(3)] for r in range(3)]
    Pr2 = [[P2[r][c] - O2[r] for c in range(3)] for r in range(3)]
    M = [[F(_dot3d(Pr2[i], Pr1[j])) for j in range(3)] for i in range(3)]
    N11 = M[0][0] + M[1][1] + M[2][2]
    N12 = M[1][2] - M[2][1]
    N13 = M[2][0] - M[0][2]
    N14 = M[0][1] - M[1][0]
    N22 = M[0][0] - M[1][1] - M[2][2]
    N23 = M[0][1] + M[1][0]
    N24 = M[2][0] + M[0][2]
    N33 = -M[0][0] + M[1][1] - M[2][2]
    N34 = M[1][2] + M[2][1]
    N44 = -M[0][0] - M[1][1] + M[2][2]
    N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    return O1, O2, Pr1, Pr2, N


def compute_sim3(P1, P2, fix_scale):
    """Sim3Solver::ComputeSim3 (:226-337). P1[r][c], P2[r][c]: coordinate r of
    sampled point c (float32). Returns (R 9 float32, t 3 float32, s float32)."""
    with np.errstate(all="ignore"):
        P1 = [[F(P1[r][c]) for c in range(3)] for r in range(3)]
        P2 = [[F(P2[r][c]) for c in range(3)] for r in range(3)]
        O1, O2, Pr1, Pr2, N = horn_N(P1, P2)
        a = [[float(N[i][j]) for j in range(4)] for i in range(4)]
        k, v = eig_jacobi4(a)
        q = [F(v[i][k]) for i in range(4)]
        # P55
        n2 = (float(q[1]) * float(q[1]) + float(q[2]) * float(q[2])) + float(q[3]) * float(q[3])
        nv = math.sqrt(n2) if n2 == n2 else NAN
        ang = F(math.atan2(nv, float(q[0])))
        kk = _div(2.0 * float(ang), nv)
        rv = [F(kk * float(q[1 + i])) for i in range(3)]
        # P56
        rx, ry, rz = float(rv[0]), float(rv[1]), float(rv[2])
        th2 = (rx * rx + ry * ry) + rz * rz
        theta = math.sqrt(th2) if th2 == th2 else NAN
        if theta < DBL_EPS:
            R = [F(1.0 if i % 4 == 0 else 0.0) for i in range(9)]
        else:
            c = float(F(_trig(math.cos, theta)))
            s = float(F(_trig(math.sin, theta)))
            c1 = 1.0 - c
            it = _div(1.0, theta)
            rx, ry, rz = rx * it, ry * it, rz * it
            rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
            rxm = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
            R = [F((c * (1.0 if i % 4 == 0 else 0.0) + c1 * rrt[i]) + s * rxm[i])
                 for i in range(9)]
        P3 = [[F(_dot3d(R[3 * i:3 * i + 3], [Pr2[0][c], Pr2[1][c], Pr2[2][c]]))
               for c in range(3)] for i in range(3)]
        if not fix_scale:
            nom = den = 0.0
            for i in range(3):
                for c in range(3):
                    nom = nom + float(Pr1[i][c]) * float(P3[i][c])
                    den = den + float(P3[i][c] * P3[i][c])
            s12 = F(_div(nom, den))
        else:
            s12 = F(1.0)
        t = []
        for i in range(3):
            sRO2 = F(_dot3d([s12 * R[3 * i], s12 * R[3 * i + 1], s12 * R[3 * i + 2]], O2))
            t.append(O1[i] - sRO2)
    return R, t, s12


def expand(R, t, s):
    """step 8 (P57): (sR, t, sRinv, tinv) of mT12i and mT21i"""
    with np.errstate(all="ignore"):
        inv = _div(1.0, float(s))
        sR = [s * R[j] for j in range(9)]
        sRi = [F(inv * float(R[3 * j + i])) for i in range(3) for j in range(3)]
        ti = [-F(_dot3d(sRi[3 * i:3 * i + 3], t)) for i in range(3)]
    return sR, list(t), sRi, ti


def to_T12(R, t, s):
    T = np.zeros((4, 4), F)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                T[i, j] = s * R[3 * i + j]
            T[i, 3] = t[i]
    T[3, 3] = 1.0
    return T


def _project(R, t, X, cam):
    """Project (:382-403) over all points: X float32 [n, 3] -> u, v float32 [n]"""
    X = X.astype(np.float64)
    Y = []
    for i in range(3):
        acc = (float(R[3 * i]) * X[:, 0] + float(R[3 * i + 1]) * X[:, 1]) \
            + float(R[3 * i + 2]) * X[:, 2]
        Y.append((acc + float(t[i])).astype(F))
    invz = F(1.0) / Y[2]
    x = Y[0] * invz
    y = Y[1] * invz
    return F(cam[0]) * x + F(cam[2]), F(cam[1]) * y + F(cam[3])


def _err2(dx, dy):
    dx = dx.astype(np.float64)
    dy = dy.astype(np.float64)
    return (dx * dx + dy * dy).astype(F)


def check_inliers(R, t, s, cam, c):
    """CheckInliers (:340-364); c = the compacted correspondences. Returns
    (mask bool[n], err1 float32[n], err2 float32[n])."""
    sR, tt, sRi, ti = expand(R, t, s)
    with np.errstate(all="ignore"):
        u, v = _project(sR, tt, c["X3Dc2"], cam)
        e1 = _err2(c["P1im1"][:, 0] - u, c["P1im1"][:, 1] - v)
        u, v = _project(sRi, ti, c["X3Dc1"], cam)
        e2 = _err2(u - c["P2im2"][:, 0], v - c["P2im2"][:, 1])
        mask = (e1 < c["max_error1"].astype(F)) & (e2 < c["max_error2"].astype(F))
    return mask, e1, e2


class Margins:
    """min_rel: the smallest |err - threshold| / threshold over every err1 and
    err2 of every CheckInliers evaluated (an error that is not a number is an
    outlier at any rounding and does not count). count_fragile: some count
    decision (>= best, > min_inliers) sat next to its boundary - one label
    would flip it - in an evaluation that had a point within NEAR of its
    threshold. Only such a point can change label under rounding-sized
    differences; a count on its boundary whose every point is far from its
    threshold (a tie of two pure-inlier hypotheses) is decided identically by
    any implementation of the pins."""
    NEAR = 1e-2

    def __init__(self):
        self.min_rel = INF
        self.count_fragile = False

    def see(self, errs, thresholds, decisions):
        """decisions: [(count, bound, strict)]: count > bound or count >= bound"""
        m = INF
        for e, th in zip(errs, thresholds):
            th = np.asarray(th, np.float64)
            with np.errstate(all="ignore"):
                rel = np.abs(e.astype(np.float64) - th) / th
            rel = rel[np.isfinite(rel)]
            if len(rel):
                m = min(m, float(rel.min()))
        self.min_rel = min(self.min_rel, m)
        for count, bound, strict in decisions:
            edge = (count in (bound, bound + 1)) if strict else (count in (bound - 1, bound))
            if edge and m < self.NEAR:
                self.count_fragile = True


class Sim3Solver:
    """The class over the compacted correspondences of setup(). State persists
    across iterate() calls as in the reference."""

    def __init__(self, cam, corr, fix_scale, probability=0.99, minInliers=6, maxIterations=300):
        self.cam = [F(c) for c in cam]
        self.c = corr
        self.N = corr["n"]
        self.fix_scale = bool(fix_scale)
        self.best_inliers = 0
        self.best_mask = np.zeros(self.N, bool)
        self.best_T12 = np.zeros((4, 4), F)
        self.best_R = np.zeros(9, F)
        self.best_t = np.zeros(3, F)
        self.best_s = F(0)
        self.margins = Margins()
        self.SetRansacParameters(probability, minInliers, maxIterations)

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.min_inliers = minInliers
        self.max_its = ransac_parameters(self.N, probability, minInliers, maxIterations)
        self.iterations = 0

    def hypotheses(self, n_iterations):
        if self.N < self.min_inliers:
            return 0
        return max(0, min(n_iterations, self.max_its - self.iterations))

    def iterate(self, n_iterations, draws):
        """Returns dict(result, no_more, n_inliers, inliers bool[N] per
        compacted correspondence, T12 float32[4, 4], draws_consumed)."""
        out = dict(result=0, no_more=False, n_inliers=0, inliers=np.zeros(self.N, bool),
                   T12=np.zeros((4, 4), F), draws_consumed=0)
        if self.N < self.min_inliers:
            out["no_more"] = True
            return out
        cur = 0
        X1, X2 = self.c["X3Dc1"], self.c["X3Dc2"]
        while self.iterations < self.max_its and cur < n_iterations:
            d = draws[3 * cur:3 * cur + 3]
            assert len(d) == 3, "not enough draws"
            cur += 1
            self.iterations += 1
            out["draws_consumed"] = 3 * cur
            idx = sample3(d, self.N)
            P1 = [[X1[idx[c]][r] for c in range(3)] for r in range(3)]
            P2 = [[X2[idx[c]][r] for c in range(3)] for r in range(3)]
            R, t, s = compute_sim3(P1, P2, self.fix_scale)
            mask, e1, e2 = check_inliers(R, t, s, self.cam, self.c)
            n = int(mask.sum())
            self.margins.see((e1, e2), (self.c["max_error1"], self.c["max_error2"]),
                             [(n, self.best_inliers, False), (n, self.min_inliers, True)])
            if n >= self.best_inliers:
                self.best_mask = mask.copy()
                self.best_inliers = n
                self.best_T12 = to_T12(R, t, s)
                self.best_R = np.array(R, F)
                self.best_t = np.array(t, F)
                self.best_s = F(s)
                if n > self.min_inliers:
                    out.update(result=1, n_inliers=n, inliers=mask.copy(),
                               T12=self.best_T12.copy())
                    return out
        if self.iterations >= self.max_its:
            out["no_more"] = True
        return out

    def find(self, draws):
        return self.iterate(self.max_its, draws)

    def state(self):
        return dict(iterations=self.iterations, best_inliers=self.best_inliers,
                    best_mask=self.best_mask.copy(), best_T12=self.best_T12.copy(),
                    best_R=self.best_R.copy(), best_t=self.best_t.copy(),
                    best_s=F(self.best_s))


# ---------------------------------------------------------------- ORBmatcher::SearchBySim3
# The keyframe grid, GetFeaturesInArea and PredictScale are the restatements
# the Fuse tests already use (tests/_fuse_ref.py).
TH_HIGH = 100
(SIM3_MATCHED, SIM3_NO_POINT, SIM3_ALREADY, SIM3_BEHIND, SIM3_OUT_OF_IMAGE, SIM3_DISTANCE,
 SIM3_EMPTY_AREA, SIM3_NO_MATCH) = range(8)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class SearchMargins:
    """rel: the relative margins of the float threshold decisions (image
    bounds, distance range, PredictScale's ceil, the window's radius tests).
    hamming_tie: some accepted best distance was reached by two candidates
    (the first in GetFeaturesInArea order wins; the reason codes and vnMatch
    show which). at_th_high: a best distance of exactly TH_HIGH or TH_HIGH + 1
    was decided."""

    def __init__(self):
        self.rel = []
        self.hamming_tie = 0
        self.at_th_high = 0

    def min_rel(self):
        return min(self.rel) if self.rel else INF


def _sbs_direction(cam, src, dst_kf, dst, R, t, already, th, margins):
    """one direction (:1499-1587 / :1592-1669): src's points through x -> R x + t
    into dst's image. Returns (vnMatch, reason)."""
    import _fuse_ref as fr
    n = len(src["valid"])
    vn, why = [-1] * n, [SIM3_MATCHED] * n
    T = np.asarray(src["Tcw"], F).reshape(4, 4)
    Rw, tw = [T[i, j] for i in range(3) for j in range(3)], [T[i, 3] for i in range(3)]
    ddesc = np.asarray(dst["desc"], np.uint8).reshape(-1, 32)
    for i in range(n):
        if not src["valid"][i]:
            why[i] = SIM3_NO_POINT
            continue
        if already[i]:
            why[i] = SIM3_ALREADY
            continue
        with np.errstate(all="ignore"):
            Pa = transform(Rw, tw, np.asarray(src["xyz"][i], F))
            Pb = transform(R, t, Pa)
            if Pb[2] < 0.0:
                why[i] = SIM3_BEHIND
                continue
            invz = F(_div(1.0, float(Pb[2])))
            x, y = Pb[0] * invz, Pb[1] * invz
            u, v = cam.fx * x + cam.cx, cam.fy * y + cam.cy
        if u == u and v == v:
            margins.rel += [fr._rel(u, cam.min_x), fr._rel(u, cam.max_x), fr._rel(v, cam.min_y),
                            fr._rel(v, cam.max_y)]
        if not (u >= cam.min_x and u < cam.max_x and v >= cam.min_y and v < cam.max_y):
            why[i] = SIM3_OUT_OF_IMAGE
            continue
        maxd, mind = F(1.2) * F(src["max_dist"][i]), F(0.8) * F(src["min_dist"][i])
        dist = F(math.sqrt(float(Pb[0]) * float(Pb[0]) + float(Pb[1]) * float(Pb[1])
                           + float(Pb[2]) * float(Pb[2])))
        margins.rel += [fr._rel(dist, mind), fr._rel(dist, maxd)]
        if dist < mind or dist > maxd:
            why[i] = SIM3_DISTANCE
            continue
        level = fr.predict_scale(cam, src["max_dist"][i], dist, margins.rel)
        r = F(th) * cam.scale[level]
        idxs = fr.features_in_area(cam, dst_kf, u, v, r, margins.rel)
        if not idxs:
            why[i] = SIM3_EMPTY_AREA
            continue
        dmp = np.asarray(src["mp_desc"][i], np.uint8)
        best, best_idx, ties = INT_MAX, -1, 0
        for j in idxs:
            if dst_kf.octave[j] < level - 1 or dst_kf.octave[j] > level:
                continue
            d = int(_POP[np.bitwise_xor(dmp, ddesc[j])].sum())
            if d < best:
                best, best_idx, ties = d, j, 0
            elif d == best:
                ties += 1
        if best in (TH_HIGH, TH_HIGH + 1):
            margins.at_th_high += 1
        if best <= TH_HIGH:
            vn[i] = best_idx
            margins.hamming_tie += 1 if ties else 0
        else:
            why[i] = SIM3_NO_MATCH
    return vn, why


def search_by_sim3(cam, kf1, kf2, matched12, s12, R12, t12, th):
    """ORBmatcher::SearchBySim3 (ORBmatcher.cc:1441-1693). cam: a
    _fuse_ref.Camera; kf1 / kf2: dicts of kps_un, desc, valid, xyz, min_dist,
    max_dist, mp_desc, Tcw; matched12 in the encoding of setup(). Returns
    dict(n_found, matched12 (updated copy), vn_match1, vn_match2, reason1,
    reason2, margins)."""
    import _fuse_ref as fr
    n1, n2 = len(kf1["valid"]), len(kf2["valid"])
    K = [fr.KeyFrame(k, k, kf["Tcw"], kf["kps_un"], np.full(len(kf["valid"]), -1, F), kf["desc"],
                     cam) for k, kf in enumerate((kf1, kf2))]
    # sR12, sR21, t21 (P58) are step 8 of ComputeSim3 (P57)
    sR, t, sRi, ti = expand([F(x) for x in np.asarray(R12, F).reshape(9)],
                            [F(x) for x in np.asarray(t12, F).reshape(3)], F(s12))
    m = np.asarray(matched12, np.int32).copy()
    am1 = [int(x) != -1 for x in m]
    am2 = [False] * n2
    for x in m:
        if 0 <= int(x) < n2:
            am2[int(x)] = True
    margins = SearchMargins()
    vn1, r1 = _sbs_direction(cam, kf1, K[1], kf2, sRi, ti, am1, th, margins)
    vn2, r2 = _sbs_direction(cam, kf2, K[0], kf1, sR, t, am2, th, margins)
    found = 0
    for i1 in range(n1):
        idx2 = vn1[i1]
        if idx2 >= 0 and vn2[idx2] == i1:
            m[i1] = idx2
            found += 1
    return dict(n_found=found, matched12=m, vn_match1=np.array(vn1, np.int32).reshape(n1),
                vn_match2=np.array(vn2, np.int32).reshape(n2),
                reason1=np.array(r1, np.int32).reshape(n1),
                reason2=np.array(r2, np.int32).reshape(n2), margins=margins)

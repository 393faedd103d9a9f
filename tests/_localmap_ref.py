"""Sequential numpy restatement of LocalMapping::CreateNewMapPoints and
CreateNewMapLines (LocalMapping.cc:346-665, 668-916), LocalMapping::ComputeF12
(:1106-1127), ORBmatcher::SearchForTriangulation (ORBmatcher.cc:884-1095) with
CheckDistEpipolarLine (:205-232) and LineMatcher::SearchForTriangulation
(LineMatcher.cpp:1174-1204), non-monocular, as the project pins them
(DESIGN.md P33-P39). float32 and float64 stand exactly where the reference has
float and double; cv::Mat products accumulate in double and round once (P6),
cv::norm / Mat::dot are P16, the SVD is _pnp_ref.svd_jacobi (P35). The float
atan2 and cos (P12, P2) are the platform's double functions rounded once to
float, which is what the pins define.

The loops are the reference's, one feature at a time: nothing here is shared
with the kernels, which reach the same result from parallel candidate lists.

A run also counts the branches it takes (`stats`) and records the margins of
its threshold decisions (`margins`), so that tests can demand coverage and pass
over seeds whose decisions hang on the last bit."""
import math
from collections import Counter

import numpy as np

from _pnp_ref import svd_jacobi

F = np.float32
TH_LOW = 50
HISTO_LENGTH = 30


class KeyFrame:
    """What the block reads of a keyframe. kps / kps_un: structured arrays with
    x, y, angle, octave (mvKeys, mvKeysUn)."""

    def __init__(self, kid, Tcw, kps, kps_un, uright, depth, desc, feat_node, has_mp, mp_xyz=None,
                 klines=None, ldesc=None, lcoef=None):
        self.id = int(kid)
        self.Tcw = np.asarray(Tcw, np.float32).reshape(4, 4)
        self.kps, self.kps_un = kps, kps_un
        self.uright = np.asarray(uright, np.float32)
        self.depth = np.asarray(depth, np.float32)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.feat_node = np.asarray(feat_node, np.int32)
        self.has_mp = np.asarray(has_mp, np.uint8)
        self.n = len(self.uright)
        # the world position of each feature's map point (read where has_mp); the raw
        # key lines (startPointX ... endPointY), LBD rows, Vector3d coefficients
        self.mp_xyz = (np.zeros((self.n, 3), np.float32) if mp_xyz is None
                       else np.asarray(mp_xyz, np.float32).reshape(-1, 3))
        self.klines = klines
        self.ldesc = np.zeros((0, 32), np.uint8) if ldesc is None else np.asarray(ldesc, np.uint8).reshape(-1, 32)
        self.lcoef = np.zeros((0, 3)) if lcoef is None else np.asarray(lcoef, np.float64).reshape(-1, 3)
        self.nl = len(self.ldesc)
        T = self.Tcw
        # Ow = -Rwc * tcw: one gemm with alpha = -1
        self.Ow = np.array([F(-1.0 * (float(T[0, r]) * float(T[0, 3]) + float(T[1, r]) * float(T[1, 3])
                                      + float(T[2, r]) * float(T[2, 3]))) for r in range(3)], np.float32)


class Camera:
    def __init__(self, fx, fy, cx, cy, bf, scale, sigma2):
        self.fx, self.fy, self.cx, self.cy, self.bf = F(fx), F(fy), F(cx), F(cy), F(bf)
        self.invfx, self.invfy = F(1.0) / self.fx, F(1.0) / self.fy
        self.mb = self.bf / self.fx
        self.scale = np.asarray(scale, np.float32)
        self.sigma2 = np.asarray(sigma2, np.float32)
        self.nlevels = len(self.scale)
        self.ratio_factor = F(1.5) * self.scale[1]


def _acc(terms):
    """double accumulation of float products, in order"""
    s = float(terms[0][0]) * float(terms[0][1])
    for a, b in terms[1:]:
        s += float(a) * float(b)
    return s


def _mul33(A, B):
    return np.array([[F(_acc([(A[r][k], B[k][c]) for k in range(3)])) for c in range(3)]
                     for r in range(3)], np.float32)


def _inv33(m):
    """P34: OpenCV 3.4's closed form, determinant and cofactors in double"""
    m = [[float(x) for x in row] for row in m]
    d = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1])
         - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
         + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    if d == 0.0:
        return np.zeros((3, 3), np.float32)
    d = 1.0 / d
    o = [(m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d,
         (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d, (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d,
         (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d,
         (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d,
         (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d]
    return np.array(o, np.float64).astype(np.float32).reshape(3, 3)


def compute_f12(cam, kf1, kf2):
    T1, T2 = kf1.Tcw, kf2.Tcw
    R12 = np.array([[F(_acc([(T1[r, k], T2[q, k]) for k in range(3)])) for q in range(3)]
                    for r in range(3)], np.float32)
    t12 = np.array([F(_acc([(-R12[r, k], T2[k, 3]) for k in range(3)]) + float(T1[r, 3]))
                    for r in range(3)], np.float32)
    z = F(0.0)
    tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], np.float32)
    K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]], np.float32)
    return _mul33(_mul33(_mul33(_inv33(K.T), tx), R12), _inv33(K))


def epipole(cam, kf1, kf2):
    T2, C = kf2.Tcw, kf1.Ow
    C2 = [F(_acc([(T2[r, k], C[k]) for k in range(3)]) + float(T2[r, 3])) for r in range(3)]
    with np.errstate(all="ignore"):
        invz = F(1.0) / C2[2]
        return cam.fx * C2[0] * invz + cam.cx, cam.fy * C2[1] * invz + cam.cy


def _rel(a, b):
    """relative distance of a comparison's two sides"""
    a, b = float(a), float(b)
    m = max(abs(a), abs(b))
    return abs(a - b) / m if m > 0 and math.isfinite(m) else 1.0


def check_dist_epipolar_line(cam, x1, y1, x2, y2, oct2, F12, margins):
    a = x1 * F12[0, 0] + y1 * F12[1, 0] + F12[2, 0]
    b = x1 * F12[0, 1] + y1 * F12[1, 1] + F12[2, 1]
    c = x1 * F12[0, 2] + y1 * F12[1, 2] + F12[2, 2]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if den == 0:
        return False
    dsqr = num * num / den
    thr = 3.84 * float(cam.sigma2[oct2])
    margins.append(_rel(dsqr, thr))
    return float(dsqr) < thr


def _hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def three_maxima(sizes):
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    if max2 < F(0.1) * F(max1):
        i2 = i3 = -1
    elif max3 < F(0.1) * F(max1):
        i3 = -1
    return i1, i2, i3


def _feature_vector(nodes):
    fv = {}
    for i, nd in enumerate(nodes):
        if nd >= 0:
            fv.setdefault(int(nd), []).append(i)
    return fv


def search_for_triangulation(cam, kf1, kf2, F12, has_mp1=None, only_stereo=False, check_ori=False,
                             stats=None, margins=None):
    """vMatchedPairs. has_mp1 overrides kf1.has_mp (CreateNewMapPoints' state)."""
    stats = Counter() if stats is None else stats
    margins = [] if margins is None else margins
    has_mp1 = kf1.has_mp if has_mp1 is None else has_mp1
    ex, ey = epipole(cam, kf1, kf2)
    fv1, fv2 = _feature_vector(kf1.feat_node), _feature_vector(kf2.feat_node)
    matched2 = np.zeros(kf2.n, bool)
    m12 = np.full(kf1.n, -1, np.int64)
    rot = [[] for _ in range(HISTO_LENGTH)]
    factor = F(HISTO_LENGTH) / F(360.0)
    u1, u2 = kf1.kps_un, kf2.kps_un
    for node in sorted(fv1):           # the map's order; only common nodes do anything
        if node not in fv2:
            continue
        for idx1 in fv1[node]:
            if has_mp1[idx1]:
                stats["kf1_has_mp"] += 1
                continue
            stereo1 = kf1.uright[idx1] >= 0
            if only_stereo and not stereo1:
                stats["only_stereo_1"] += 1
                continue
            best_dist, best_idx2 = TH_LOW, -1
            for idx2 in fv2[node]:
                if matched2[idx2]:
                    stats["kf2_claimed"] += 1
                    continue
                if kf2.has_mp[idx2]:
                    stats["kf2_has_mp"] += 1
                    continue
                stereo2 = kf2.uright[idx2] >= 0
                if only_stereo and not stereo2:
                    stats["only_stereo_2"] += 1
                    continue
                dist = _hamming(kf1.desc[idx1], kf2.desc[idx2])
                if dist > TH_LOW or dist > best_dist:
                    stats["dist_reject"] += 1
                    continue
                o2 = int(u2["octave"][idx2])
                if not stereo1 and not stereo2:
                    stats["epipole_tested"] += 1
                    dx, dy = ex - u2["x"][idx2], ey - u2["y"][idx2]
                    lhs, rhs = dx * dx + dy * dy, F(100.0) * cam.scale[o2]
                    margins.append(_rel(lhs, rhs))
                    if lhs < rhs:
                        stats["epipole_reject"] += 1
                        continue
                if check_dist_epipolar_line(cam, u1["x"][idx1], u1["y"][idx1], u2["x"][idx2],
                                            u2["y"][idx2], o2, F12, margins):
                    if best_idx2 >= 0 and dist == best_dist:
                        stats["tie_replaced"] += 1
                    best_idx2, best_dist = idx2, dist
                else:
                    stats["epiline_reject"] += 1
            if best_idx2 >= 0:
                m12[idx1] = best_idx2
                matched2[best_idx2] = True
                if check_ori:
                    r = u1["angle"][idx1] - u2["angle"][best_idx2]
                    if r < 0:
                        r = r + F(360.0)
                    rf = float(r * factor)               # round(): half away from zero, rf >= 0
                    b = int(math.floor(rf + 0.5))
                    if b == HISTO_LENGTH:
                        b = 0
                    rot[b].append(idx1)
    if check_ori:
        i1, i2, i3 = three_maxima([len(r) for r in rot])
        for b in range(HISTO_LENGTH):
            if b in (i1, i2, i3):
                continue
            for idx1 in rot[b]:
                m12[idx1] = -1
                stats["ori_removed"] += 1
    return [(i, int(m12[i])) for i in range(kf1.n) if m12[i] >= 0]


def _norm3(v):
    return math.sqrt(float(v[0]) * float(v[0]) + float(v[1]) * float(v[1]) + float(v[2]) * float(v[2]))


def _dot3(a, b):
    return _acc([(a[0], b[0]), (a[1], b[1]), (a[2], b[2])])


def _unproject_stereo(cam, kf, i):
    z = kf.depth[i]
    if not z > 0:
        return None
    u, v = kf.kps["x"][i], kf.kps["y"][i]            # mvKeys, the raw keypoint
    x3 = [(u - cam.cx) * z * cam.invfx, (v - cam.cy) * z * cam.invfy, z]
    T = kf.Tcw
    return np.array([F(_acc([(T[k, r], x3[k]) for k in range(3)]) + float(kf.Ow[r]))
                     for r in range(3)], np.float32)


def _cos_stereo(cam, depth):
    at = F(math.atan2(float(cam.mb / F(2.0)), float(depth)))      # atan2f (P12)
    return F(math.cos(float(F(2.0) * at)))                        # cosf (P2)


def triangulate_pair(cam, kf1, kf2, idx1, idx2, stats, margins):
    """One pair of CreateNewMapPoints: None, or (xyz, normal, min_dist, max_dist)."""
    u1, u2 = kf1.kps_un, kf2.kps_un
    x1, y1, o1 = u1["x"][idx1], u1["y"][idx1], int(u1["octave"][idx1])
    x2, y2, o2 = u2["x"][idx2], u2["y"][idx2], int(u2["octave"][idx2])
    ur1, ur2 = kf1.uright[idx1], kf2.uright[idx2]
    st1, st2 = ur1 >= 0, ur2 >= 0
    T1, T2 = kf1.Tcw, kf2.Tcw
    xn1 = [(x1 - cam.cx) * cam.invfx, (y1 - cam.cy) * cam.invfy, F(1.0)]
    xn2 = [(x2 - cam.cx) * cam.invfx, (y2 - cam.cy) * cam.invfy, F(1.0)]
    ray1 = [F(_acc([(T1[k, r], xn1[k]) for k in range(3)])) for r in range(3)]
    ray2 = [F(_acc([(T2[k, r], xn2[k]) for k in range(3)])) for r in range(3)]
    cos_rays = F(_dot3(ray1, ray2) / (_norm3(ray1) * _norm3(ray2)))
    cs1 = cs2 = cos_rays + F(1.0)
    if st1:
        cs1 = _cos_stereo(cam, kf1.depth[idx1])
    elif st2:
        cs2 = _cos_stereo(cam, kf2.depth[idx2])
    cs = min(cs1, cs2)
    margins.append(_rel(cos_rays, cs))
    if cos_rays < cs and cos_rays > 0 and (st1 or st2 or float(cos_rays) < 0.9998):
        stats["way_triangulate"] += 1
        if not (st1 or st2):
            margins.append(_rel(cos_rays, 0.9998))
        A = []
        rows = [(xn1[0], T1, 0), (xn1[1], T1, 1), (xn2[0], T2, 0), (xn2[1], T2, 1)]
        for s, T, r in rows:      # s * row(2) - row(r): double, one rounding (P36)
            A.append([float(F(float(s) * float(T[2, k]) - float(T[r, k]))) for k in range(4)])
        _, _, V = svd_jacobi(A)
        h = [F(V[i][3]) for i in range(4)]
        if h[3] == 0:
            stats["w_zero"] += 1
            return None
        inv = F(1.0 / float(h[3]))
        X = np.array([h[0] * inv, h[1] * inv, h[2] * inv], np.float32)
    elif st1 and cs1 < cs2:
        stats["way_stereo1"] += 1
        X = _unproject_stereo(cam, kf1, idx1)
        if X is None:
            stats["unproject_empty"] += 1
            return None
    elif st2 and cs2 < cs1:
        stats["way_stereo2"] += 1
        X = _unproject_stereo(cam, kf2, idx2)
        if X is None:
            stats["unproject_empty"] += 1
            return None
    else:
        stats["no_parallax"] += 1
        return None
    z1 = F(_dot3(T1[2, :3], X) + float(T1[2, 3]))
    if z1 <= 0:
        stats["z1_behind"] += 1
        return None
    z2 = F(_dot3(T2[2, :3], X) + float(T2[2, 3]))
    if z2 <= 0:
        stats["z2_behind"] += 1
        return None
    for T, z, x, y, o, ur, st, tag in ((T1, z1, x1, y1, o1, ur1, st1, "1"), (T2, z2, x2, y2, o2, ur2, st2, "2")):
        sig = float(cam.sigma2[o])
        px = F(_dot3(T[0, :3], X) + float(T[0, 3]))
        py = F(_dot3(T[1, :3], X) + float(T[1, 3]))
        invz = F(1.0 / float(z))
        u = cam.fx * px * invz + cam.cx
        v = cam.fy * py * invz + cam.cy
        eX, eY = u - x, v - y
        if not st:
            e2, thr = eX * eX + eY * eY, 5.991 * sig
            margins.append(_rel(e2, thr))
            if float(e2) > thr:
                stats["reproj_mono_" + tag] += 1
                return None
        else:
            u_r = u - cam.bf * invz            # KF1's mbf for both views, as written
            eR = u_r - ur
            e2, thr = eX * eX + eY * eY + eR * eR, 7.8 * sig
            margins.append(_rel(e2, thr))
            if float(e2) > thr:
                stats["reproj_stereo_" + tag] += 1
                return None
    n1, n2 = X - kf1.Ow, X - kf2.Ow
    d1, d2 = F(_norm3(n1)), F(_norm3(n2))
    if d1 == 0 or d2 == 0:
        stats["dist_zero"] += 1
        return None
    ratio_dist = d2 / d1
    ratio_oct = cam.scale[o1] / cam.scale[o2]
    margins.append(_rel(ratio_dist * cam.ratio_factor, ratio_oct))
    margins.append(_rel(ratio_dist, ratio_oct * cam.ratio_factor))
    if ratio_dist * cam.ratio_factor < ratio_oct or ratio_dist > ratio_oct * cam.ratio_factor:
        stats["scale_reject"] += 1
        return None
    # UpdateNormalAndDepth, two observations in keyframe-id order (P24, P25)
    i1, i2 = F(1.0 / _norm3(n1)), F(1.0 / _norm3(n2))
    obs = [(n1, i1), (n2, i2)] if kf1.id < kf2.id else [(n2, i2), (n1, i1)]
    normal = np.zeros(3, np.float32)
    for nv, iv in obs:
        normal = normal + nv * iv
    normal = normal / F(2.0)
    max_dist = d1 * cam.scale[o1]
    min_dist = max_dist / cam.scale[cam.nlevels - 1]
    return X, normal.astype(np.float32), F(min_dist), F(max_dist)


def create_new_map_points(cam, cur, neigh):
    """Returns dict(records, kf1_point_record, pairs, stats, margins, matched).
    A record: (neighbour, idx1, idx2, desc_from, xyz, normal, min_dist, max_dist)."""
    stats, margins = Counter(), []
    has_mp1 = cur.has_mp.copy()
    records = []
    slot = np.full(cur.n, -1, np.int32)
    pairs = [-1] * 10
    matched = {}
    for nb, kf2 in enumerate(neigh):
        base = kf2.Ow - cur.Ow
        baseline = F(_norm3(base))
        margins.append(_rel(baseline, cam.mb))
        if baseline < cam.mb:
            stats["baseline_skip"] += 1
            continue
        F12 = compute_f12(cam, cur, kf2)
        vm = search_for_triangulation(cam, cur, kf2, F12, has_mp1, False, False, stats, margins)
        pairs[nb] = len(vm)
        matched[nb] = vm
        for idx1, idx2 in vm:
            r = triangulate_pair(cam, cur, kf2, idx1, idx2, stats, margins)
            if r is None:
                continue
            X, normal, mn, mx = r
            slot[idx1] = len(records)
            records.append((nb, idx1, idx2, 0 if cur.id < kf2.id else 1, X, normal, mn, mx))
            has_mp1[idx1] = 1
            stats["created"] += 1
    return dict(records=records, kf1_point_record=slot, pairs=pairs, stats=stats, margins=margins,
                matched=matched)


# ---------------------------------------------------------------- CreateNewMapLines
def line_search_for_triangulation(ldesc1, ldesc2, stats=None):
    """LineMatcher::SearchForTriangulation (LineMatcher.cpp:1174-1204) with
    KeyFrame::lineDescriptorMAD (KeyFrame.cc:773-797). Pinned P38: no KF1 line or
    fewer than two KF2 lines give no pairs (the reference indexes past the end)."""
    stats = Counter() if stats is None else stats
    n1, n2 = len(ldesc1), len(ldesc2)
    if n1 == 0 or n2 < 2:
        stats["line_matcher_empty"] += 1
        return []
    knn = []
    for q in range(n1):                       # knnMatch k = 2, ties to the lower train index
        d = [F(_hamming(ldesc1[q], ldesc2[j])) for j in range(n2)]
        order = sorted(range(n2), key=lambda j: (d[j], j))
        knn.append((order[0], d[order[0]], d[order[1]]))
    d12 = [k[2] - k[1] for k in knn]                               # float
    med = float(sorted(d12)[n1 // 2])                              # double nn12_dist_median
    dev = sorted(F(abs(float(x) - med)) for x in d12)              # fabsf
    nn12_mad = 1.4826 * float(dev[n1 // 2])
    th = nn12_mad * 0.1
    out = []
    for q in range(n1):
        if float(d12[q]) > th:
            out.append((q, knn[q][0]))
        else:
            stats["line_nn12_reject"] += 1
    return out


def scene_median_depth(kf, extra=()):
    """KeyFrame::ComputeSceneMedianDepth(2) over the keyframe's map points and
    `extra` (idx2, xyz) points created this call; None when it has none (P39)."""
    T = kf.Tcw
    pts = {i: kf.mp_xyz[i] for i in range(kf.n) if kf.has_mp[i]}
    for i, X in extra:
        pts[i] = X
    z = sorted(float(F(_dot3(T[2, :3], X) + float(T[2, 3]))) for X in pts.values())
    return F(z[(len(z) - 1) // 2]) if z else None


def _projection_matrix(cam, T):
    K = [[cam.fx, F(0), cam.cx], [F(0), cam.fy, cam.cy], [F(0), F(0), F(1)]]
    return [[F(_acc([(K[r][i], T[i, k]) for i in range(3)])) for k in range(4)] for r in range(3)]


def triangulate_line(cam, kf1, kf2, idx1, idx2, median, stats, margins):
    T1, T2 = kf1.Tcw, kf2.Tcw
    M1, M2 = _projection_matrix(cam, T1), _projection_matrix(cam, T2)
    l1 = [F(x) for x in kf1.lcoef[idx1]]
    l2 = [F(x) for x in kf2.lcoef[idx2]]
    row0 = [float(F(_acc([(l1[i], M1[i][k]) for i in range(3)]))) for k in range(4)]
    row1 = [float(F(_acc([(l2[i], M2[i][k]) for i in range(3)]))) for k in range(4)]
    kl = kf1.klines[idx1]
    ends = []
    for u, v in ((kl["startPointX"], kl["startPointY"]), (kl["endPointX"], kl["endPointY"])):
        xn = [(u - cam.cx) * cam.invfx, (v - cam.cy) * cam.invfy]
        A = [row0, row1]
        for r in range(2):
            A.append([float(F(float(xn[r]) * float(T1[2, k]) - float(T1[r, k]))) for k in range(4)])
        _, _, V = svd_jacobi(A)
        h = [F(V[i][3]) for i in range(4)]
        if h[3] == 0:
            stats["line_w_zero"] += 1
            return None
        inv = F(1.0 / float(h[3]))
        ends.append(np.array([h[0] * inv, h[1] * inv, h[2] * inv], np.float32))
    s3, e3 = ends
    with np.errstate(all="ignore"):
        r1 = F(_norm3(s3 - kf1.Ow)) / median
        margins.append(_rel(r1, 0.3))
        if float(r1) < 0.3:
            stats["line_near_1"] += 1
            return None
        r2 = F(_norm3(s3 - kf2.Ow)) / median
        margins.append(_rel(r2, 0.3))
        if float(r2) < 0.3:
            stats["line_near_2"] += 1
            return None
        r3 = F(_norm3(e3 - s3)) / median
        margins.append(_rel(r3, 1.0))
        if r3 > 1:
            stats["line_too_long"] += 1
            return None
    for T, X, tag in ((T1, s3, "s1"), (T2, s3, "s2"), (T1, e3, "e1"), (T2, e3, "e2")):
        if F(_dot3(T[2, :3], X) + float(T[2, 3])) <= 0:
            stats["line_behind_" + tag] += 1
            return None
    return np.concatenate([s3, e3]).astype(np.float32)


def create_new_map_lines(cam, cur, neigh, point_records, stats, margins):
    """CreateNewMapLines after CreateNewMapPoints: records (neighbour, idx1,
    idx2, desc_from, xyz6), KF1's slots (the last record wins), pairs."""
    records = []
    slot = np.full(cur.nl, -1, np.int32)
    pairs = [-1] * 10
    for nb, kf2 in enumerate(neigh):
        if F(_norm3(kf2.Ow - cur.Ow)) < cam.mb:
            continue
        median = scene_median_depth(kf2, [(r[2], r[4]) for r in point_records if r[0] == nb])
        if median is None:
            stats["line_no_median"] += 1
            pairs[nb] = 0
            continue
        vm = line_search_for_triangulation(cur.ldesc, kf2.ldesc, stats)
        pairs[nb] = len(vm)
        for idx1, idx2 in vm:
            x6 = triangulate_line(cam, cur, kf2, idx1, idx2, median, stats, margins)
            if x6 is None:
                continue
            if slot[idx1] >= 0:
                stats["line_created_twice"] += 1
            slot[idx1] = len(records)
            records.append((nb, idx1, idx2, 0 if cur.id < kf2.id else 1, x6))
            stats["line_created"] += 1
    return records, slot, pairs


def create_new_map_features(cam, cur, neigh):
    r = create_new_map_points(cam, cur, neigh)
    lines, lslot, lpairs = create_new_map_lines(cam, cur, neigh, r["records"], r["stats"], r["margins"])
    r.update(lines=lines, kf1_line_record=lslot, line_pairs=lpairs)
    return r

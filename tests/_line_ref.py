"""Sequential restatement of the per-frame line code that
tests/test_gpu_line_cases.py compares the GPU against, written from the
reference's source (src/LineMatcher.cpp, src/Frame.cc) and DESIGN.md's pins:

  liang_barsky         LineMatcher::LiangBarsky            LineMatcher.cpp:1389-1460
  project_map_line     the projection of SearchByProjection :118-193
  update_keyline       UpdateKeyLineData                    :1601-1624
  line_overlap         LineOverLap                          :1508-1559
  reprojection_error   ReprojectionError                    :1579-1596
  line_matching        LineMatching                         :1463-1504
  search_last          SearchByProjection(Frame&, const Frame&)              :72-269
  search_list          SearchByProjection(F, local map lines / RefKF)        :527-952
  search_pairs         the harness overloads, mode 0 :272-487, mode 1 :954-1170
  match_bf_knn         SearchByProjection(Frame&, KeyFrame*, vector<MapLine*>&) :492-525
  line_in_frustum      Frame::IsInFrustum(MapLine*)         Frame.cc:403-430
  line_frame_prepare   UndistortKeyLines + line depths      Frame.cc:769-845, 1090-1116 (P14)
  stereo_line_depths   the defined stereo mode              DESIGN.md P17

Numbers are Python floats (doubles). A C `float` is a Python float that has
been through r32(): a float operation is the double operation rounded once
more, which is exact emulation for + - * / sqrt (53 >= 2 * 24 + 2 bits). A
division is IEEE (x / 0 is an infinity or a NaN) and every comparison is the
one the source writes, so that a NaN falls where it falls there.

`variants` switches on behaviour the reference does NOT have; the tests use
them only to show that the cases tell the difference:
  first_wins     the first passing projected line is kept, not the last
  textbook_clip  a Liang-Barsky that accepts horizontal lines and skips p == 0
  retry_le       `<=` in the last-frame / list retry rule
  wrap_angle     angle differences taken modulo 2 pi
  count_unique   one match counted per current line, not one per passing pair
  nan_rejects    a comparison whose operand is NaN rejects the pair
"""
import math

import numpy as np

KL = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"),
               ("pt_x", "<f4"), ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"),
               ("startPointX", "<f4"), ("startPointY", "<f4"), ("endPointX", "<f4"),
               ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
               ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"),
               ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"),
               ("numOfPixels", "<i4")])

PI = 3.14159265358979323846
NO_VARIANTS = frozenset()
VARIANTS = ("first_wins", "textbook_clip", "retry_le", "wrap_angle", "count_unique", "nan_rejects")

LB_CODES = ("LB_VERTICAL_REJECT", "LB_HORIZONTAL_REJECT", "LB_OUTSIDE", "LB_OK")
BRANCH_CODES = ("INVALID", "BOTH_BEHIND", "START_BEHIND", "END_BEHIND", "NO_BRANCH", "IN_FRONT")
MATCH_REASONS = ("DESC", "ANGLE", "LENGTH", "OVERLAP", "REPROJ", "OK")
OVERLAP_EXITS = ("OV_VERT_Y", "OV_HORZ_X", "OV_X_YOVERLAP", "OV_X_YGAP_SMALL", "OV_Y_AFTER_XGAP",
                 "OV_NONE")
STEREO_REASONS = ("LEFT_FLAT", "DESC", "NOT_BETTER", "ANGLE", "LENGTH", "RIGHT_FLAT", "ROW_OVERLAP",
                  "DISPARITY", "TAKEN")
for _c in LB_CODES + BRANCH_CODES + MATCH_REASONS + OVERLAP_EXITS + STEREO_REASONS:
    globals()[_c] = _c

# codes an entry can never give, with the argument
UNREACHABLE = {
    # The four searches share the projection and LineMatching: every branch, clipping, reason
    # and overlap code can be reached through each of them (a horizontal CURRENT line reaches
    # OV_HORZ_X although a horizontal projected line never leaves LiangBarsky). What cannot
    # happen is a horizontal line that LiangBarsky accepts: it passes its gate only with
    # q[2] < 0 and q[3] < 0, i.e. sy < minY and sy > maxY at once; there is no code for it.
    "last": {}, "list": {}, "pairs0": {}, "pairs1": {},
    # the stereo scan: every reason can be reached
    "stereo": {},
}

_F32 = np.float32


def r32(x):
    """(float)x"""
    with np.errstate(all="ignore"):
        return float(_F32(x))


def ddiv(a, b):
    """IEEE a / b in double"""
    if b != 0 and not (math.isinf(a) and math.isinf(b)):
        return a / b
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def fdiv(a, b):
    """IEEE a / b in float (a, b floats)"""
    return r32(ddiv(a, b))


def cround(x):
    """C round(): halves away from zero"""
    if x != x or math.isinf(x):
        return x
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1.0
    return math.copysign(float(r), x)


def dsqrt(x):
    return math.sqrt(x) if x == x and x >= 0 else float("nan")


# --------------------------------------------------------------------------
# camera: Frame::UndistortPoints' cv::undistortPoints and ComputeImageBounds
# --------------------------------------------------------------------------
def undistort_point(cam, px, py):
    """cv::undistortPoints with P = K (5 fixed iterations, double) on one float point"""
    fx, fy, cx, cy = (r32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k = [r32(cam[c]) for c in ("k1", "k2", "p1", "p2", "k3")]
    x = (px - cx) * (1.0 / fx)
    y = (py - cy) * (1.0 / fy)
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((0.0 * r2 + 0.0) * r2 + 0.0) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + 0.0 * r2 + 0.0 * r2 * r2
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + 0.0 * r2 + 0.0 * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    xx = fx * x + 0.0 * y + cx
    yy = 0.0 * x + fy * y + cy
    ww = 1.0 / (0.0 * x + 0.0 * y + 1.0)
    return r32(xx * ww), r32(yy * ww)


def image_bounds(cam):
    """Frame::ComputeImageBounds (Frame.cc:848-882): (minX, minY, maxX, maxY), the order
    LiangBarsky takes them in. The gate is k1 != 0 alone."""
    W, H = float(cam["width"]), float(cam["height"])
    if r32(cam["k1"]) != 0.0:
        c = [undistort_point(cam, x, y) for x, y in ((0.0, 0.0), (W, 0.0), (0.0, H), (W, H))]
        return (min(c[0][0], c[2][0]), min(c[0][1], c[1][1]), max(c[1][0], c[3][0]),
                max(c[2][1], c[3][1]))
    return (0.0, 0.0, W, H)


# --------------------------------------------------------------------------
# cv::LineIterator(img, Point(pt1), Point(pt2), 8).count
# --------------------------------------------------------------------------
def _clip_line(W, H, x1, y1, x2, y2):
    """cv::clipLine(Size, Point&, Point&) on 64-bit integers"""
    right, bottom = W - 1, H - 1
    if W <= 0 or H <= 0:
        return False, x1, y1, x2, y2
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * (x2 - x1) / (y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * (x2 - x1) / (y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * (y2 - y1) / (x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * (y2 - y1) / (x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def line_iterator_count(W, H, fx1, fy1, fx2, fy2):
    """the end points are cvRound()ed (halves to even) to a cv::Point"""
    x1, y1, x2, y2 = (int(round(v)) for v in (fx1, fy1, fx2, fy2))
    if not (0 <= x1 < W and 0 <= x2 < W and 0 <= y1 < H and 0 <= y2 < H):
        ok, x1, y1, x2, y2 = _clip_line(W, H, x1, y1, x2, y2)
        if not ok:
            return 0
    return max(abs(x2 - x1), abs(y2 - y1)) + 1


# --------------------------------------------------------------------------
# the clipping and the key line rebuilt from it
# --------------------------------------------------------------------------
def liang_barsky(line4, bounds, variants=NO_VARIANTS):
    """LineMatcher.cpp:1389-1460. line4 = (sx, sy, ex, ey) doubles, bounds = (minX, minY,
    maxX, maxY) floats. Returns (ok, new4, code)."""
    sx, sy, ex, ey = line4
    p = [sx - ex, ex - sx, sy - ey, ey - sy]
    q = [sx - bounds[0], bounds[2] - sx, sy - bounds[1], bounds[3] - sy]
    textbook = "textbook_clip" in variants
    if textbook:
        for i in range(4):
            if p[i] == 0 and q[i] < 0:
                return False, None, LB_OUTSIDE
    else:
        if p[0] == 0:
            if q[0] <= 0 or q[2] <= 0:
                return False, None, LB_VERTICAL_REJECT
        if p[2] == 0:
            if q[2] >= 0 or q[3] >= 0:
                return False, None, LB_HORIZONTAL_REJECT
    u = [ddiv(q[i], p[i]) for i in range(4)]
    u_min, u_max = 0.0, 1.0
    for i in range(4):
        if textbook and p[i] == 0:
            continue
        if p[i] < 0:
            if u_min < u[i]:
                u_min = u[i]
        else:
            if u_max > u[i]:
                u_max = u[i]
    if u_max >= u_min:
        return True, (sx + cround(u_min * (ex - sx)), sy + cround(u_min * (ey - sy)),
                      sx + cround(u_max * (ex - sx)), sy + cround(u_max * (ey - sy))), LB_OK
    return False, None, LB_OUTSIDE


def update_keyline(k, W, H):
    """UpdateKeyLineData (LineMatcher.cpp:1601-1624) on the one-element record k whose four
    end-point fields are set: the octave copies and every derived field. The angle is
    float(atan2(double, double)) of the float differences."""
    sx, sy, ex, ey = (float(k[f][0]) for f in ("startPointX", "startPointY", "endPointX",
                                               "endPointY"))
    k["sPointInOctaveX"], k["sPointInOctaveY"] = sx, sy
    k["ePointInOctaveX"], k["ePointInOctaveY"] = ex, ey
    k["pt_x"] = r32(r32(ex + sx) / 2)
    k["pt_y"] = r32(r32(ey + sy) / 2)
    dx, dy = r32(sx - ex), r32(sy - ey)
    length = r32(dsqrt(dx * dx + dy * dy))
    k["lineLength"] = length
    k["numOfPixels"] = line_iterator_count(W, H, sx, sy, ex, ey)
    k["angle"] = r32(math.atan2(r32(ey - sy), r32(ex - sx)))
    k["size"] = r32(r32(ex - sx) * r32(ey - sy))
    k["response"] = fdiv(length, float(max(W, H)))
    return k


def project_map_line(cam, Tcw, X6, base=None, variants=NO_VARIANTS, bounds=None):
    """LineMatcher.cpp:118-193: the map line's end points through Tcw (float entries, a 3x4
    product in double), the crossing with z = 0 when one end is behind the camera (in camera
    coordinates, not pixels, as written), LiangBarsky and UpdateKeyLineData on a copy of
    `base` (a default KeyLine when None). Returns (ok, keyline record or None, code)."""
    fx, fy, cx, cy = (r32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    T = [float(v) for v in np.asarray(Tcw, np.float32).reshape(-1)[:12]]
    X = [float(v) for v in np.asarray(X6, np.float32)]
    cs = [(T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2]) + T[4 * r + 3] for r in range(3)]
    ce = [(T[4 * r] * X[3] + T[4 * r + 1] * X[4] + T[4 * r + 2] * X[5]) + T[4 * r + 3] for r in range(3)]
    if cs[2] < 0 and ce[2] < 0:
        return False, None, BOTH_BEHIND

    def pix(c):
        return r32(ddiv(fx * c[0], c[2]) + cx), r32(ddiv(fy * c[1], c[2]) + cy)

    lp, branch = None, NO_BRANCH
    if cs[2] < 0.0 or ce[2] < 0.0:
        lam = ddiv(-1.0 * cs[2], cs[2] - ce[2])
        xc = cs[0] + lam * (cs[0] - ce[0])
        yc = cs[1] + lam * (cs[1] - ce[1])
        if cs[2] < 0.0:
            lp, branch = (xc, yc) + pix(ce), START_BEHIND
        else:
            lp, branch = pix(cs) + (xc, yc), END_BEHIND
    if cs[2] > 0.0 and ce[2] > 0.0:
        lp, branch = pix(cs) + pix(ce), IN_FRONT
    if lp is None:
        return False, None, NO_BRANCH
    if bounds is None:
        bounds = image_bounds(cam)
    ok, n4, lb = liang_barsky(lp, bounds, variants)
    code = branch + "/" + lb
    if not ok:
        return False, None, code
    k = np.zeros(1, KL) if base is None else np.array([base], KL)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = (r32(v) for v in n4)
    update_keyline(k, int(cam["width"]), int(cam["height"]))
    return True, k[0], code


# --------------------------------------------------------------------------
# LineMatching and what it calls; a key line is g = (sx, sy, ex, ey, angle, length)
# --------------------------------------------------------------------------
def geom(k):
    return tuple(float(k[f]) for f in ("startPointX", "startPointY", "endPointX", "endPointY",
                                       "angle", "lineLength"))


def geoms(kls):
    cols = [np.asarray(kls[f], np.float64).tolist() for f in
            ("startPointX", "startPointY", "endPointX", "endPointY", "angle", "lineLength")]
    return list(zip(*cols))


def line_overlap(k1, k2, th):
    """LineOverLap (LineMatcher.cpp:1508-1559): (bool, which return fired). The extents are
    float abs() of float differences, everything after that is double."""
    d1x, d2x = abs(r32(k1[0] - k1[2])), abs(r32(k2[0] - k2[2]))
    min_x = min(min(k1[0], k1[2]), min(k2[0], k2[2]))
    max_x = max(max(k1[0], k1[2]), max(k2[0], k2[2]))
    d1y, d2y = abs(r32(k1[1] - k1[3])), abs(r32(k2[1] - k2[3]))
    min_y = min(min(k1[1], k1[3]), min(k2[1], k2[3]))
    max_y = max(max(k1[1], k1[3]), max(k2[1], k2[3]))
    qx = ddiv(d1x + d2x - max_x + min_x, min(d1x, d2x))
    qy = ddiv(d1y + d2y - max_y + min_y, min(d1y, d2y))
    if d1x == 0 or d2x == 0:
        if qy >= th:
            return True, OV_VERT_Y
    if d1y == 0 or d2y == 0:
        if qx >= th:
            return True, OV_HORZ_X
    if qx >= th:
        if d1y + d2y + min_y >= max_y:
            return True, OV_X_YOVERLAP
        if max_y - min_y - d1y - d2y < 0.3 * min(d1y, d2y):
            return True, OV_X_YGAP_SMALL
    elif qx < th and (max_x - min_x - d1x - d2x) < 0.3 * min(d1x, d2x):
        if qy >= th:
            return True, OV_Y_AFTER_XGAP
    return False, OV_NONE


def reprojection_error(k1, k2):
    """ReprojectionError (LineMatcher.cpp:1579-1596): the distance of k2's end points to the
    line through k1's, the line normalised by its first two coefficients"""
    s0, s1, e0, e1 = k1[0], k1[1], k1[2], k1[3]
    c0 = s1 * 1.0 - 1.0 * e1
    c1 = 1.0 * e0 - s0 * 1.0
    c2 = s0 * e1 - s1 * e0
    nrm = dsqrt(c0 * c0 + c1 * c1)
    ds = ddiv(k2[0] * c0 + k2[1] * c1 + 1.0 * c2, nrm)
    de = ddiv(k2[2] * c0 + k2[3] * c1 + 1.0 * c2, nrm)
    return dsqrt(ds * ds + de * de)


OFF0 = (0.0, 0.0, 0.0, 0.0, 0.0)
OFF1 = (10.0, -0.1, -0.1, 5.0, 10.0)          # the relaxed pass (LineMatcher.cpp:238)


def line_matching(k1, k2, dist, off, variants=NO_VARIANTS, want_exit=False):
    """LineMatching (LineMatcher.cpp:1463-1504) of the projected line k1 and the current line
    k2 whose descriptors are `dist` apart: (bool, reason)."""
    nanrej = "nan_rejects" in variants
    if dist > 45 + off[3]:
        return False, DESC
    da = abs(r32(k1[4] - k2[4]))
    if "wrap_angle" in variants and da > PI:
        da = 2 * PI - da
    if da > 15.0 * PI / 180.0 + off[0] * PI / 180.0 or (nanrej and da != da):
        return False, ANGLE
    ratio = fdiv(min(k1[5], k2[5]), max(k1[5], k2[5]))
    if ratio < 0.45 + off[1] or (nanrej and ratio != ratio):
        return False, LENGTH
    ov, ex = line_overlap(k1, k2, 0.5 + off[2])
    if nanrej and ov and (0.0 in (abs(r32(k1[0] - k1[2])), abs(r32(k2[0] - k2[2])),
                                  abs(r32(k1[1] - k1[3])), abs(r32(k2[1] - k2[3])))):
        ov = False          # some quotient had a zero divisor: inf or NaN
    if not ov:
        return False, (OVERLAP, ex) if want_exit else OVERLAP
    err = reprojection_error(k1, k2)
    if err > 45 or (nanrej and err != err):
        return False, REPROJ
    return True, (OK, ex) if want_exit else OK


# --------------------------------------------------------------------------
# the searches
# --------------------------------------------------------------------------
def hamming_table(a, b):
    """distances between every row of a (n, 32) and b (m, 32)"""
    a = np.asarray(a, np.uint8).reshape(-1, 32)
    b = np.asarray(b, np.uint8).reshape(-1, 32)
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)), np.int64)
    ab = np.unpackbits(a, axis=1).astype(np.int16)
    bb = np.unpackbits(b, axis=1).astype(np.int16)
    return (ab.sum(1)[:, None] + bb.sum(1)[None, :] - 2 * ab @ bb.T).astype(np.int64)


def project_all(cam, Tcw, valid, base_kl, xyz6, variants=NO_VARIANTS):
    """the projection loop: (projected KeyLines in map-line order, their map-line index,
    the code of every map line)"""
    bounds = image_bounds(cam)
    nk, nidx, codes = [], [], []
    for i in range(len(valid)):
        if not valid[i]:
            codes.append(INVALID)
            continue
        ok, k, code = project_map_line(cam, Tcw, xyz6[i], None if base_kl is None else base_kl[i],
                                       variants, bounds)
        codes.append(code)
        if ok:
            nk.append(k)
            nidx.append(i)
    kl = np.array(nk, KL) if nk else np.zeros(0, KL)
    return kl, nidx, codes


def _verdicts(pg, cg, D, nidx, off, variants):
    """LineMatching of every (projected i, current j): reason[j][i]"""
    return [[line_matching(pg[i], cg[j], int(D[nidx[i], j]), off, variants)[1]
             for i in range(len(pg))] for j in range(len(cg))]


def _search_core(cam, Tcw, cur_kl, cur_desc, cur_nobs, valid, base_kl, xyz6, ml_desc, variants):
    """the body the last-frame, reference-keyframe and local-map overloads share
    (LineMatcher.cpp:72-269, :527-721, :755-952)"""
    ncur = len(cur_kl)
    proj, nidx, codes = project_all(cam, Tcw, valid, base_kl, xyz6, variants)
    pg, cg = geoms(proj), geoms(cur_kl)
    D = hamming_table(ml_desc, cur_desc)
    trace = dict(codes=codes, proj_kl=proj, proj_src=np.array(nidx, np.int32), reasons=[],
                 passing=[], skipped_claimed=[])

    def run(off, skip, npass):
        match = np.full(ncur, -1, np.int32)
        reasons = _verdicts(pg, cg, D, nidx, off, variants)
        passing, cnt = [], 0
        for j in range(ncur):
            ok = [i for i in range(len(pg)) if reasons[j][i] == OK]
            if skip and cur_nobs is not None and cur_nobs[j] > 0:
                trace["skipped_claimed"] += [(npass, i, j) for i in ok]
                ok = []
            passing.append(ok)
            if ok:
                match[j] = nidx[ok[0] if "first_wins" in variants else ok[-1]]
                cnt += 1 if "count_unique" in variants else len(ok)
        trace["reasons"].append(reasons)
        trace["passing"].append(passing)
        return match, cnt

    match, n = run(OFF0, True, 0)
    lhs = ddiv(n * 1.0, float(ncur))
    retry = lhs <= 0.2 if "retry_le" in variants else lhs < 0.2
    trace["retry"] = dict(lhs=lhs, rhs=0.2, op="<", first_pass=n, retried=retry)
    if retry:
        match, n = run(OFF1, False, 1)
    return match, n, retry, trace


def search_last(cam, Tcw, cur_kl, cur_desc, last_kl, has_ml, outlier, xyz6, last_desc,
                variants=NO_VARIANTS):
    """(match, nmatches, trace); match[j] = last-frame line index or -1"""
    valid = [bool(h) and not bool(o) for h, o in zip(has_ml, outlier)]
    match, n, _, trace = _search_core(cam, Tcw, cur_kl, cur_desc, None, valid, last_kl, xyz6,
                                      last_desc, variants)
    return match, n, trace


def search_list(cam, Tcw, cur_kl, cur_desc, cur_nobs, valid, xyz6, ml_desc, variants=NO_VARIANTS):
    """(match, nmatches, wiped, trace). cur_nobs[j] > 0 skips current line j in the first
    pass only; the projected KeyLines start from a default KeyLine."""
    return _search_core(cam, Tcw, cur_kl, cur_desc, cur_nobs, valid, None, xyz6, ml_desc, variants)


def search_pairs(cam, Tcw, mode, cur_kl, cur_desc, cur_nobs, valid, base_kl, xyz6, ml_desc, ml_nobs,
                 pair_cap=None, variants=NO_VARIANTS):
    """The harness overloads. Returns (match, nmatches, wiped, proj_kl, proj_src, pairs,
    npairs, trace): pairs holds min(npairs, pair_cap) rows (i, j)."""
    ncur = len(cur_kl)
    proj, nidx, codes = project_all(cam, Tcw, valid, base_kl if mode == 0 else None, xyz6, variants)
    pg, cg = geoms(proj), geoms(cur_kl)
    D = hamming_table(ml_desc, cur_desc)
    cnobs = [0 if cur_nobs is None else int(c) for c in (cur_nobs if cur_nobs is not None
                                                          else [0] * ncur)]
    trace = dict(codes=codes, reasons=[], passing=[], skipped_claimed=[])

    def run(off, npass):
        match = np.full(ncur, -1, np.int32)
        reasons = _verdicts(pg, cg, D, nidx, off, variants)
        pairs, passing, cnt = [], [], 0
        for j in range(ncur):
            passing.append([])
            if mode == 1 and cnobs[j] > 0:
                trace["skipped_claimed"] += [(npass, i, j) for i in range(len(pg))
                                             if reasons[j][i] == OK]
                continue
            for i in range(len(pg)):
                if mode == 0 and cnobs[j] > 0:
                    if reasons[j][i] == OK:
                        trace["skipped_claimed"].append((npass, i, j))
                    continue
                if reasons[j][i] == OK:
                    passing[j].append(i)
                    if not ("first_wins" in variants and len(passing[j]) > 1):
                        match[j] = nidx[i]
                    cnobs[j] = 0 if ml_nobs is None else int(ml_nobs[nidx[i]])
                    pairs.append((i, j))
                    if not ("count_unique" in variants and len(passing[j]) > 1):
                        cnt += 1
        trace["reasons"].append(reasons)
        trace["passing"].append(passing)
        return match, cnt, pairs

    match, n, pairs = run(OFF0, 0)
    if mode == 0:
        lhs, rhs = ddiv(n * 1.0, float(ncur)), 0.2
        retry, op = lhs < 0.2, "<"
    else:
        lhs, rhs = float(n), 0.2 * ncur
        retry, op = lhs <= rhs, "<="
    trace["retry"] = dict(lhs=lhs, rhs=rhs, op=op, first_pass=n, retried=retry)
    if retry:
        cnobs = [0] * ncur                    # mvpMapLines wiped to NULL
        match, n, pairs = run(OFF1, 1)
    npairs = len(pairs)
    if pair_cap is not None:
        pairs = pairs[:pair_cap]
    return (match, n, retry, proj, np.array(nidx, np.int32),
            np.array(pairs, np.int32).reshape(-1, 2), npairs, trace)


def match_bf_knn(qdesc, tdesc):
    """LineMatcher.cpp:492-525: knnMatch(k = 2) of every query against the train rows (the
    two smallest distances, ties to the lower train index), best / second < 0.75 in float;
    a later query overwrites. A query with fewer than two train rows has no match (pinned).
    Returns (out, nmatches, trace); trace[q] = (best, second, d_best, d_second, ratio, ok)."""
    D = hamming_table(qdesc, tdesc)
    nq, nt = len(np.asarray(qdesc).reshape(-1, 32)), len(np.asarray(tdesc).reshape(-1, 32))
    out = np.full(nt, -1, np.int32)
    n, trace = 0, []
    for q in range(nq):
        b, s, db, ds = -1, -1, 0, 0
        for j in range(nt):
            d = int(D[q, j])
            if b < 0 or d < db:
                s, ds = b, db
                b, db = j, d
            elif s < 0 or d < ds:
                s, ds = j, d
        if s < 0:
            trace.append((b, s, db, ds, None, False))
            continue
        ratio = fdiv(float(db), float(ds))
        ok = ratio < r32(0.75)
        trace.append((b, s, db, ds, ratio, ok))
        if ok:
            out[b] = q
            n += 1
    return out, n, trace


def line_in_frustum(Tcw, xyz6):
    """Frame::IsInFrustum(MapLine*) (Frame.cc:403-430): the third row of Rcw X + tcw as a
    double sum rounded to float, in view unless both are < 0. Returns (in_view, z (n, 2))."""
    T = [float(v) for v in np.asarray(Tcw, np.float32).reshape(-1)]
    X = np.asarray(xyz6, np.float32).reshape(-1, 6)
    view, zs = np.zeros(len(X), np.uint8), np.zeros((len(X), 2), np.float32)
    for i in range(len(X)):
        z = []
        for e in range(2):
            x = [float(v) for v in X[i, 3 * e:3 * e + 3]]
            s = T[8] * x[0]
            s += T[9] * x[1]
            s += T[10] * x[2]
            z.append(r32(s + T[11]))
        zs[i] = z
        view[i] = not (z[0] < 0.0 and z[1] < 0.0)
    return view, zs


def line_frame_prepare(cam, kl, depth=None):
    """Frame::UndistortKeyLines (Frame.cc:769-845; the gate is k1 != 0 alone, :771) and the
    line part of ComputeStereoFromRGBD (:1090-1116): imDepth.at<float>(int(v), int(u)) on the
    DISTORTED end points reads the row-major buffer at int(v) * W + int(u), an index outside
    the buffer is no depth (P14). Returns (kl_un, dstart, dend, ur_start, ur_end)."""
    W, H = int(cam["width"]), int(cam["height"])
    bf = r32(cam["bf"])
    n = len(kl)
    ku = np.array(kl, KL)
    out = [np.full(n, -1.0, np.float32) for _ in range(4)]
    flat = None if depth is None else np.asarray(depth, np.float32).reshape(-1)
    for i in range(n):
        k = ku[i:i + 1]
        if r32(cam["k1"]) != 0.0:
            sx, sy = undistort_point(cam, float(kl["startPointX"][i]), float(kl["startPointY"][i]))
            ex, ey = undistort_point(cam, float(kl["endPointX"][i]), float(kl["endPointY"][i]))
            k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = sx, sy, ex, ey
            update_keyline(k, W, H)
        if flat is None:
            continue
        for e, (fu, fv, fx_un) in enumerate((("startPointX", "startPointY", "startPointX"),
                                             ("endPointX", "endPointY", "endPointX"))):
            idx = int(float(kl[fv][i])) * W + int(float(kl[fu][i]))
            d = float(flat[idx]) if 0 <= idx < W * H else 0.0
            if d > 0:
                out[e][i] = d
                out[2 + e][i] = r32(float(k[fx_un][0]) - fdiv(bf, d))
    return (ku,) + tuple(out)


def stereo_line_depths(cam, kl, desc, kr, desc_r):
    """DESIGN.md P17. Returns (dstart, dend, trace); trace[i] is LEFT_FLAT or the list of the
    reasons of right lines 0 .. nr-1 in scan order."""
    bf, fx = r32(cam["bf"]), r32(cam["fx"])
    max_d = fdiv(bf, fdiv(bf, fx))
    nl, nr = len(kl), len(kr)
    D = hamming_table(desc, desc_r)
    ga, gb = geoms(kl), geoms(kr)
    ds_out, de_out = np.full(nl, -1.0, np.float32), np.full(nl, -1.0, np.float32)
    trace = []
    th45 = r32(0.45)
    for i in range(nl):
        a = ga[i]
        ady = a[3] - a[1]
        if abs(ady) < 0.25 * a[5]:
            trace.append(LEFT_FLAT)
            continue
        ay0, ay1 = min(a[1], a[3]), max(a[1], a[3])
        best, bs, be, why = 46, -1.0, -1.0, []
        for j in range(nr):
            b = gb[j]
            dist = int(D[i, j])
            if dist > 45:
                why.append(DESC)
                continue
            if dist >= best:
                why.append(NOT_BETTER)
                continue
            if abs(a[4] - b[4]) > 10.0 * PI / 180.0:
                why.append(ANGLE)
                continue
            if fdiv(min(a[5], b[5]), max(a[5], b[5])) < th45:
                why.append(LENGTH)
                continue
            bdy = b[3] - b[1]
            if abs(bdy) < 0.25 * b[5]:
                why.append(RIGHT_FLAT)
                continue
            by0, by1 = min(b[1], b[3]), max(b[1], b[3])
            ov = min(ay1, by1) - max(ay0, by0)
            if ov < 0.5 * min(ay1 - ay0, by1 - by0):
                why.append(ROW_OVERLAP)
                continue
            slope = ddiv(b[2] - b[0], bdy)
            xs = b[0] + (a[1] - b[1]) * slope
            xe = b[0] + (a[3] - b[1]) * slope
            ds, de = r32(a[0] - xs), r32(a[2] - xe)
            if not (ds > 0.0 and ds < max_d and de > 0.0 and de < max_d):
                why.append(DISPARITY)
                continue
            why.append(TAKEN)
            best, bs, be = dist, fdiv(bf, ds), fdiv(bf, de)
        trace.append(why)
        if best <= 45:
            ds_out[i], de_out[i] = bs, be
    return ds_out, de_out, trace

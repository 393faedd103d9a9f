"""Sequential numpy restatement of Frame::ComputeStereoMatches
(Frame.cc:888-1062) as the project pins it, written from the
reference's loop, one keypoint at a time. float32 stands where the reference
has `float`, `round` is std::round (half away from zero), `(int)` truncates,
the SAD of the centred integer-valued windows is an integer sum.

Besides (uright, depth) a run returns, per left keypoint, the *reason* it ended
where it did (`reason`: after the median cut; `stage`: before it) and the
intermediate values of the keypoints that reached the SAD search (`trace`), so
that tests can demand that a crafted input takes the branch it was made for.

Nothing here is shared with the kernel, which builds the row bands with a
counting sort and the median with a bitonic sort of packed keys."""
import math
from collections import namedtuple

import numpy as np

F = np.float32
TH_HIGH, TH_LOW = 100, 50
INT_MAX = 2 ** 31 - 1

# reason codes, in the order the reference's loop can leave a keypoint
(ROW_OUTSIDE,       # (int)vL is no row of the image (pinned: skipped)
 EMPTY_BAND,        # vRowIndices[vL] is empty
 MAXU_NEGATIVE,     # maxU < 0
 NO_CANDIDATE,      # bestDist stays >= thOrbDist = 75
 INIU_ENDU,         # iniu < 0 or endu >= cols
 WINDOW_OUTSIDE,    # a window leaves the level (pinned: skipped)
 SAD_MIN_FIRST,     # bestincR == -L
 SAD_MIN_LAST,      # bestincR == +L
 DELTA_RANGE,       # deltaR < -1 or deltaR > 1
 DELTA_NAN,         # deltaR is not a number: fails the disparity test
 DISPARITY_NEGATIVE,
 DISPARITY_MAX,     # disparity >= maxD
 ACCEPTED_CLAMPED,  # disparity 0 replaced by 0.01
 ACCEPTED,
 MEDIAN_CUT) = range(15)

NAMES = ("ROW_OUTSIDE EMPTY_BAND MAXU_NEGATIVE NO_CANDIDATE INIU_ENDU WINDOW_OUTSIDE SAD_MIN_FIRST "
         "SAD_MIN_LAST DELTA_RANGE DELTA_NAN DISPARITY_NEGATIVE DISPARITY_MAX ACCEPTED_CLAMPED "
         "ACCEPTED MEDIAN_CUT").split()

# deltaR = (d1 - d3) / (2 (d1 + d3 - 2 d2)) is taken at the *first* smallest
# SAD of the curve, at an interior position: d1 > d2 (strictly, or d1 would
# have been chosen) and d3 >= d2. With p = d1 - d2 >= 1 and q = d3 - d2 >= 0
# it is (p - q) / (2 (p + q)), in (-1/2, 1/2], and every term is an integer
# below 2^24, exact in float. So these two codes cannot be reached by any
# input; `parabola` keeps the reference's tests all the same.
UNREACHABLE = frozenset((DELTA_RANGE, DELTA_NAN))

Result = namedtuple("Result", "uright depth reason stage trace median th_dist")


def std_round(x):
    """std::round of a float: half away from zero."""
    x = float(x)
    return F(math.copysign(math.floor(abs(x) + 0.5), x))


def as_int(desc):
    """A 32-byte descriptor as one integer (DescriptorDistance counts bits of the xor)."""
    return int.from_bytes(np.asarray(desc, np.uint8).tobytes(), "little")


def parabola(dist1, dist2, dist3):
    """Frame.cc:1020-1027: deltaR, or None where the reference `continue`s."""
    dist1, dist2, dist3 = F(dist1), F(dist2), F(dist3)
    with np.errstate(all="ignore"):
        deltaR = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))
    if deltaR < -1 or deltaR > 1:
        return None
    return deltaR


def row_bands(scale, n_rows, kr):
    """vRowIndices (Frame.cc:898-915); rows outside the image are dropped
    (pinned: the reference would write past the table)."""
    rows = [[] for _ in range(n_rows)]
    for iR in range(len(kr)):
        kpY = F(kr["y"][iR])
        r = F(F(2.0) * F(scale[int(kr["octave"][iR])]))
        maxr = int(math.ceil(F(kpY + r)))
        minr = int(math.floor(F(kpY - r)))
        for yi in range(minr, maxr + 1):
            if 0 <= yi < n_rows:
                rows[yi].append(iR)
    return rows


def compute_stereo_matches(bf, fx, scale, inv_scale, pyr_l, pyr_r, kl, dl, kr, dr):
    """pyr_l / pyr_r: one 2-D uint8 array per level (the level's content, no
    border); kl / kr: structured arrays with x, y, octave; dl / dr: (n, 32)
    uint8. bf, fx: Frame::mbf and the fx of mb = mbf / fx."""
    n = len(kl)
    uright = np.full(n, -1.0, np.float32)
    depth = np.full(n, -1.0, np.float32)
    reason = np.full(n, -1, np.int32)
    trace = {}
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = pyr_l[0].shape[0]
    vRowIndices = row_bands(scale, nRows, kr)
    mbf = F(bf)
    mb = F(mbf / F(fx))
    minZ, minD = mb, F(0)
    maxD = F(mbf / minZ)
    vDistIdx = []
    # plain Python values of the right side (float32 values are exact as Python floats)
    octR_, uR_ = [int(o) for o in kr["octave"]], [float(x) for x in kr["x"]]
    dR_, dL_ = [as_int(d) for d in dr], [as_int(d) for d in dl]
    for iL in range(n):
        levelL = int(kl["octave"][iL])
        vL, uL = F(kl["y"][iL]), F(kl["x"][iL])
        row = int(vL)
        if row < 0 or row >= nRows:
            reason[iL] = ROW_OUTSIDE
            continue
        vCandidates = vRowIndices[row]
        if not vCandidates:
            reason[iL] = EMPTY_BAND
            continue
        minU, maxU = F(uL - maxD), F(uL - minD)
        if maxU < 0:
            reason[iL] = MAXU_NEGATIVE
            continue
        bestDist, bestIdxR = TH_HIGH, 0
        lo, hi = float(minU), float(maxU)
        for iR in vCandidates:
            octR = octR_[iR]
            if octR < levelL - 1 or octR > levelL + 1:
                continue
            uR = uR_[iR]
            if uR >= lo and uR <= hi:
                dist = bin(dL_[iL] ^ dR_[iR]).count("1")
                if dist < bestDist:
                    bestDist, bestIdxR = dist, iR
        if not bestDist < thOrbDist:
            reason[iL] = NO_CANDIDATE
            continue
        uR0 = F(kr["x"][bestIdxR])
        scaleFactor = F(inv_scale[levelL])
        scaleduL = std_round(F(uL * scaleFactor))
        scaledvL = std_round(F(vL * scaleFactor))
        scaleduR0 = std_round(F(uR0 * scaleFactor))
        w = L = 5
        IL, IR = pyr_l[levelL], pyr_r[levelL]
        rows_l, cols_l = IL.shape
        tr = trace[iL] = dict(best_idx=bestIdxR, best_dist=bestDist)
        iniu = F(F(scaleduR0 + F(L)) - F(w))
        endu = F(F(F(scaleduR0 + F(L)) + F(w)) + F(1))
        if iniu < 0 or endu >= IR.shape[1]:
            reason[iL] = INIU_ENDU
            continue
        cuL, cvL, cuR = int(scaleduL), int(scaledvL), int(scaleduR0)
        tr.update(cuL=cuL, cvL=cvL, cuR=cuR)
        # pinned: where rowRange / colRange would leave the level (the reference
        # asserts inside OpenCV) the keypoint stays unmatched
        if cvL - w < 0 or cvL + w >= rows_l or cuL - w < 0 or cuL + w >= cols_l or cuR - L - w < 0:
            reason[iL] = WINDOW_OUTSIDE
            continue
        WL = IL[cvL - w:cvL + w + 1, cuL - w:cuL + w + 1].astype(np.int64)
        WL = WL - WL[w, w]
        bestD, bestincR = INT_MAX, 0
        vDists = [F(0)] * (2 * L + 1)
        for incR in range(-L, L + 1):
            c = cuR + incR
            WR = IR[cvL - w:cvL + w + 1, c - w:c + w + 1].astype(np.int64)
            WR = WR - WR[w, w]
            dist = F(int(np.abs(WL - WR).sum()))
            if dist < bestD:
                bestD, bestincR = int(dist), incR
            vDists[L + incR] = dist
        tr.update(sads=[int(d) for d in vDists], best_sad=bestD, inc=bestincR)
        if bestincR == -L:
            reason[iL] = SAD_MIN_FIRST
            continue
        if bestincR == L:
            reason[iL] = SAD_MIN_LAST
            continue
        deltaR = parabola(vDists[L + bestincR - 1], vDists[L + bestincR], vDists[L + bestincR + 1])
        if deltaR is None:
            reason[iL] = DELTA_RANGE
            continue
        tr.update(delta=deltaR)
        bestuR = F(F(scale[levelL]) * F(F(scaleduR0 + F(bestincR)) + deltaR))
        disparity = F(uL - bestuR)
        tr.update(disparity=disparity)
        if disparity >= minD and disparity < maxD:
            reason[iL] = ACCEPTED
            if disparity <= 0:
                disparity = F(0.01)
                bestuR = F(float(uL) - 0.01)
                reason[iL] = ACCEPTED_CLAMPED
            depth[iL] = F(mbf / disparity)
            uright[iL] = bestuR
            vDistIdx.append((bestD, iL))
        elif disparity != disparity:
            reason[iL] = DELTA_NAN
        elif disparity < minD:
            reason[iL] = DISPARITY_NEGATIVE
        else:
            reason[iL] = DISPARITY_MAX
    stage = reason.copy()
    median = thDist = None
    if vDistIdx:      # the reference indexes an empty vector here; pinned: nothing to cut
        vDistIdx.sort()
        median = F(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F(F(F(1.5) * F(1.4)) * median)
        for d, iL in reversed(vDistIdx):
            if F(d) < thDist:
                break
            uright[iL] = -1
            depth[iL] = -1
            reason[iL] = MEDIAN_CUT
    return Result(uright, depth, reason, stage, trace, median, thDist)

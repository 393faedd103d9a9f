"""Sequential numpy restatement of the two reference functions behind
Tracking::Relocalization that tests/test_gpu_reloc.py compares the GPU against:

  detect_reloc      KeyFrameDatabase::DetectRelocalizationCandidates
                    (src/KeyFrameDatabase.cc:274-412) with L1Scoring::score
                    (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68)
  search_by_projection_kf
                    ORBmatcher::SearchByProjection(Frame&, KeyFrame*,
                    const set<MapPoint*>&, th, ORBdist) (src/ORBmatcher.cc:1891-2024)
                    with Frame::GetFeaturesInArea (src/Frame.cc:432-485)

Written as the C++ reads, one statement after the other: Python float stands
for double, np.float32 for float. It shares nothing with the kernels. Known
answers for it are in tests/test_reloc_ref.py."""
import bisect
import math

import numpy as np

f32 = np.float32


def l1_score(v1w, v1v, v2w, v2v, reverse=False):
    """L1Scoring::score(v1, v2): the double sum over the common words in
    ascending word order (reverse=True: the same terms added last to first,
    for the test that shows the order matters), then -score / 2.0."""
    terms = []
    i, j, n1, n2 = 0, 0, len(v1w), len(v2w)
    while i < n1 and j < n2:
        vi, wi = float(v1v[i]), float(v2v[j])
        if v1w[i] == v2w[j]:
            terms.append(math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi))
            i += 1
            j += 1
        elif v1w[i] < v2w[j]:
            i = bisect.bisect_left(v1w, v2w[j], i)    # v1.lower_bound(v2_it->first)
        else:
            j = bisect.bisect_left(v2w, v1w[i], j)
    score = 0.0
    for t in (reversed(terms) if reverse else terms):
        score += t
    return -score / 2.0


def detect_reloc(kf_bows, covis, reloc_score, q_words, q_vals, reverse_sum=False):
    """kf_bows[k] = (words, values) of database keyframe k in add() order;
    covis[k] = GetBestCovisibilityKeyFrames(10) as database indices (-1: not
    in the database); reloc_score[k] = mRelocScore on entry. Returns (cand,
    common_words, reloc_score after, info)."""
    nkf = len(kf_bows)
    q_words = [int(w) for w in q_words]
    bows = [([int(w) for w in ws], vs) for ws, vs in kf_bows]
    # KeyFrameDatabase::add: mvInvertedFile[word].push_back(pKF)
    inverted = {}
    for k, (ws, _) in enumerate(bows):
        for w in ws:
            inverted.setdefault(w, []).append(k)
    score = [f32(s) for s in reloc_score]
    reloc_query = [False] * nkf
    reloc_words = [0] * nkf
    sharing = []
    for w in q_words:                           # F->mBowVec, a std::map: ascending
        for k in inverted.get(w, []):
            if not reloc_query[k]:
                reloc_words[k] = 0
                reloc_query[k] = True
                sharing.append(k)
            reloc_words[k] += 1
    info = dict(sharing=list(sharing), dedup_removed=0, scored=[])
    if not sharing:
        return [], reloc_words, np.array(score, f32), info
    max_common = 0
    for k in sharing:
        if reloc_words[k] > max_common:
            max_common = reloc_words[k]
    min_common = int(f32(max_common) * f32(0.8))
    score_and_match = []
    for k in sharing:
        if reloc_words[k] > min_common:
            si = f32(l1_score(q_words, q_vals, bows[k][0], bows[k][1], reverse_sum))
            score[k] = si
            score_and_match.append((si, k))
    info["scored"] = [k for _, k in score_and_match]
    if not score_and_match:
        return [], reloc_words, np.array(score, f32), info
    acc_and_match = []
    best_acc = f32(0)
    for si, k in score_and_match:
        best_score = si
        acc = best_score
        best_kf = k
        for k2 in list(covis[k])[:10]:
            if k2 < 0:
                continue
            if not reloc_query[k2]:
                continue
            acc = f32(acc + score[k2])
            if score[k2] > best_score:
                best_kf = k2
                best_score = score[k2]
        acc_and_match.append((acc, best_kf))
        if acc > best_acc:
            best_acc = acc
    min_retain = f32(f32(0.75) * best_acc)
    added, cand = set(), []
    for acc, k in acc_and_match:
        if acc > min_retain:
            if k not in added:
                cand.append(k)
                added.add(k)
            else:
                info["dedup_removed"] += 1
    return cand, reloc_words, np.array(score, f32), info


# --------------------------------------------------------------------------
def _gemm3(R, x, t=None):
    """cv::Mat float product (+ vector): exact products summed in double, one
    rounding."""
    out = []
    for r in range(3):
        s = float(R[r][0]) * float(x[0])
        s += float(R[r][1]) * float(x[1])
        s += float(R[r][2]) * float(x[2])
        if t is not None:
            s = s + float(t[r])
        out.append(f32(s))
    return out


def _hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class RefFrame:
    """The Frame members the matcher reads: camera, bounds, scale factors,
    mvKeysUn, mDescriptors and the grid (AssignFeaturesToGrid, Frame.cc:265-287,
    PosInGrid :527-538)."""

    def __init__(self, cam, bounds, scale_factors, Tcw, kps_un, desc):
        self.fx, self.fy, self.cx, self.cy = (f32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
        self.minX, self.maxX, self.minY, self.maxY = (f32(b) for b in bounds)
        self.scale = [f32(s) for s in scale_factors]
        self.nlevels = len(self.scale)
        # mfLogScaleFactor = log(mfScaleFactor) (P15: double log of the float)
        self.log_scale = f32(math.log(float(self.scale[1]))) if self.nlevels > 1 else f32(1)
        self.Tcw = np.asarray(Tcw, f32).reshape(4, 4)
        self.kps, self.desc = kps_un, desc
        self.inv_w = f32(f32(64) / f32(self.maxX - self.minX))
        self.inv_h = f32(f32(48) / f32(self.maxY - self.minY))
        self.grid = [[[] for _ in range(48)] for _ in range(64)]
        for i in range(len(kps_un)):
            # C round(): halves away from zero
            px = self._cround(f32(f32(kps_un["x"][i] - self.minX) * self.inv_w))
            py = self._cround(f32(f32(kps_un["y"][i] - self.minY) * self.inv_h))
            if 0 <= px < 64 and 0 <= py < 48:
                self.grid[px][py].append(i)

    @staticmethod
    def _cround(x):
        x = float(x)
        return int(math.floor(x + 0.5)) if x >= 0 else int(math.ceil(x - 0.5))

    def features_in_area(self, x, y, r, min_level, max_level):
        out = []
        c0 = max(0, int(math.floor(f32(f32(f32(x - self.minX) - r) * self.inv_w))))
        if c0 >= 64:
            return out
        c1 = min(63, int(math.ceil(f32(f32(f32(x - self.minX) + r) * self.inv_w))))
        if c1 < 0:
            return out
        r0 = max(0, int(math.floor(f32(f32(f32(y - self.minY) - r) * self.inv_h))))
        if r0 >= 48:
            return out
        r1 = min(47, int(math.ceil(f32(f32(f32(y - self.minY) + r) * self.inv_h))))
        if r1 < 0:
            return out
        check_levels = (min_level > 0) or (max_level >= 0)
        for ix in range(c0, c1 + 1):
            for iy in range(r0, r1 + 1):
                for j in self.grid[ix][iy]:
                    octave = int(self.kps["octave"][j])
                    if check_levels:
                        if octave < min_level:
                            continue
                        if max_level >= 0 and octave > max_level:
                            continue
                    dx = f32(self.kps["x"][j] - x)
                    dy = f32(self.kps["y"][j] - y)
                    if abs(dx) < r and abs(dy) < r:
                        out.append(j)
        return out


def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2035-2077)"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, h in enumerate(hist):
        s = len(h)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif max3 < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search_by_projection_kf(frame, cur_has_mp, kf_angle, kf_valid, kf_found, mp_xyz, mp_min_dist,
                            mp_max_dist, mp_desc, th, orb_dist, check_ori, trace=None):
    """Returns (match, nmatches): match[i] = keyframe feature whose map point
    the call put into CurrentFrame.mvpMapPoints[i], else -1. trace (a dict, for
    the tests' non-vacuity checks) receives points[i] = (ncand, skipped, taken):
    the keypoints of the window not held on entry with distance <= orb_dist, how
    many of them a point of this call held when point i chose, the keypoint it
    took or -1; and, with check_ori, hist (bin sizes) and keep (the kept bins)."""
    F = frame
    n = len(F.kps)
    holds = [bool(h) for h in cur_has_mp]      # CurrentFrame.mvpMapPoints[i] != NULL
    match = [-1] * n
    nmatches = 0
    R = F.Tcw[:3, :3]
    t = F.Tcw[:3, 3]
    Rt = [[R[c][r] for c in range(3)] for r in range(3)]
    Ow = [f32(-float(v)) for v in _gemm3(Rt, t)]          # -Rcw.t() * tcw
    hist = [[] for _ in range(30)]
    factor = f32(f32(30) / f32(360.0))
    th = f32(th)
    for i in range(len(kf_angle)):
        if not kf_valid[i] or kf_found[i]:
            continue
        X = [f32(v) for v in mp_xyz[i]]
        xc, yc, zc = _gemm3(R, X, t)
        if zc == 0:
            continue                                      # not a number: rejected (pinned)
        invzc = f32(1.0 / float(zc))
        u = f32(f32(f32(F.fx * xc) * invzc) + F.cx)
        v = f32(f32(f32(F.fy * yc) * invzc) + F.cy)
        if u < F.minX or u > F.maxX:
            continue
        if v < F.minY or v > F.maxY:
            continue
        PO = [f32(X[k] - Ow[k]) for k in range(3)]
        # cv::norm (P16): double squares, one sqrt, one rounding
        dist3d = f32(math.sqrt(float(PO[0]) * float(PO[0]) + float(PO[1]) * float(PO[1]) +
                               float(PO[2]) * float(PO[2])))
        max_d = f32(f32(1.2) * f32(mp_max_dist[i]))
        min_d = f32(f32(0.8) * f32(mp_min_dist[i]))
        if dist3d < min_d or dist3d > max_d:
            continue
        level = 0
        if F.nlevels > 1:                                 # MapPoint::PredictScale
            ratio = f32(f32(mp_max_dist[i]) / dist3d)
            level = int(math.ceil(f32(f32(math.log(float(ratio))) / F.log_scale)))
            if level < 0:
                level = 0
            elif level >= F.nlevels:
                level = F.nlevels - 1
        radius = f32(th * F.scale[level])
        idx = F.features_in_area(u, v, radius, level - 1, level + 1)
        if not idx:
            continue
        best_dist, best_idx = 256, -1
        ncand = skipped = 0
        for i2 in idx:
            if trace is not None and not cur_has_mp[i2] and \
                    _hamming(mp_desc[i], F.desc[i2]) <= orb_dist:
                ncand += 1
                skipped += holds[i2]
            if holds[i2]:
                continue
            d = _hamming(mp_desc[i], F.desc[i2])
            if d < best_dist:
                best_dist, best_idx = d, i2
        if trace is not None:
            taken = best_idx if best_dist <= orb_dist else -1
            trace.setdefault("points", {})[i] = (ncand, skipped, taken)
        if best_dist <= orb_dist and best_idx >= 0:
            holds[best_idx] = True
            match[best_idx] = i
            nmatches += 1
            if check_ori:
                rot = f32(f32(kf_angle[i]) - f32(F.kps["angle"][best_idx]))
                if rot < 0.0:
                    rot = f32(rot + f32(360.0))
                b = RefFrame._cround(f32(rot * factor))
                if b == 30:
                    b = 0
                hist[b].append(best_idx)
    if check_ori:
        i1, i2, i3 = three_maxima(hist)
        if trace is not None:
            trace.update(hist=[len(h) for h in hist], keep=(i1, i2, i3))
        for b in range(30):
            if b != i1 and b != i2 and b != i3:
                for j in hist[b]:
                    match[j] = -1
                    nmatches -= 1
    return np.array(match, np.int32), nmatches

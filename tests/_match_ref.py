"""Sequential numpy restatement of the three per-frame point matchers that
tests/test_gpu_match_cases.py compares the GPU against:

  search_last    ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)
                 (src/ORBmatcher.cc:1710-1879)
  search_local   ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
                 (src/ORBmatcher.cc:72-183) with RadiusByViewingCos (:186-192)
  search_bow     ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
                 (src/ORBmatcher.cc:247-410)

with Frame::GetFeaturesInArea, PosInGrid (RefFrame) and ComputeThreeMaxima
from tests/_reloc_ref.py. Python float stands for double, np.float32 for
float; a cv::Mat product is the pinned one of DESIGN.md P6 (_gemm3).

Each function returns (match, nmatches, rec, info). rec[i] describes map point
i: `reason` (one of REASONS), `kp` (the keypoint it took, -1 none), `best`,
`second`, `best_level`, `second_level`, `bin` (rotation bin, -1 none),
`ncand` (candidates that pass every gate with distance <= the threshold),
`skipped` (how many of those were claimed when the point chose) and
`overwrote` (the keypoint was held by a point that does not claim).

Every function runs its points twice over the same gated candidate lists:
scheme "loop" is the reference's running best / second with its strict
comparisons; scheme "topk" is replay_topk, the kernels' scheme: the first four
of (distance, scan position) order, the first unclaimed entries of those, and
an exact re-scan when the four run out while more candidates exist (scheme
"topk_without_rescan" leaves that out: the tests use it to show that the cases
would catch a kernel that forgot it). Known answers are in
tests/test_match_ref.py."""
import numpy as np

from _reloc_ref import RefFrame, _gemm3, _hamming, f32, three_maxima

TH_HIGH, TH_LOW, HISTO_LENGTH, TOPK = 100, 50, 30, 4

REASONS = ("NO_MP", "OUTLIER", "BEHIND", "OUT_OF_IMAGE", "NOT_IN_VIEW", "NO_NODE", "NODE_UNSHARED",
           "NO_WINDOW", "NO_CANDIDATE", "ALL_CLAIMED", "OVER_TH", "RATIO_REJECT", "ACCEPTED",
           "ACCEPTED_OVERWRITES", "ROT_CUT")
for _r in REASONS:
    globals()[_r] = _r

# reason codes a matcher can never give, with the argument
UNREACHABLE = {
    "last": {
        "NOT_IN_VIEW": "isInFrustum is not part of this function",
        "NO_NODE": "no vocabulary", "NODE_UNSHARED": "no vocabulary",
        "RATIO_REJECT": "no ratio test (ORBmatcher.cc:1832 tests the distance alone)"},
    "local": {
        "NO_MP": "every entry of vpMapPoints is a map point", "OUTLIER": "no outlier flags here",
        "BEHIND": "isInFrustum ran before: in_view 0", "OUT_OF_IMAGE": "isInFrustum ran before",
        "NO_NODE": "no vocabulary", "NODE_UNSHARED": "no vocabulary",
        "ROT_CUT": "no rotation histogram in this function"},
    "bow": {
        "OUTLIER": "no outlier flags here", "BEHIND": "no projection", "OUT_OF_IMAGE": "no projection",
        "NOT_IN_VIEW": "no projection", "NO_WINDOW": "a shared node holds a frame feature",
        "ACCEPTED_OVERWRITES": "vpMapPointMatches[j] != NULL skips j whatever its point "
                               "(ORBmatcher.cc:314): every match claims"},
}


def rot_bin(a_from, a_to):
    """ORBmatcher.cc:1840-1845 / :354-359"""
    factor = f32(f32(HISTO_LENGTH) / f32(360.0))
    rot = f32(f32(a_from) - f32(a_to))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = RefFrame._cround(f32(rot * factor))
    return 0 if b == HISTO_LENGTH else b


def _pick_loop(cands, claimed, octave):
    """the candidate loops of ORBmatcher.cc:123-164, :308-334, :1802-1829:
    (bestDist, bestIdx, bestLevel, bestDist2, bestLevel2)"""
    bd, bj, bl, sd, sl = 256, -1, -1, 256, -1
    for d, _, j in cands:
        if claimed[j]:
            continue
        if d < bd:
            sd, sl = bd, bl
            bd, bl, bj = d, octave(j), j
        elif d < sd:
            sd, sl = d, octave(j)
    return bd, bj, bl, sd, sl


def _pick_topk(cands, claimed, octave, need, cap, stats, rescan=True):
    """The kernels' scheme. cands is in scan order; the order of the list is
    (distance, scan position). `cap`: distances above it never enter the list
    (256 can set neither slot; the last-frame matcher needs the best alone and
    drops what is over its threshold)."""
    order = sorted(c for c in cands if c[0] <= cap)
    free = [c for c in order[:TOPK] if not claimed[c[2]]][:need]
    if len(free) < need and len(order) > TOPK:
        stats["rescans"] += 1
        if rescan:      # rescan=False: the scheme gone wrong, for the tests' own non-vacuity check
            free = [c for c in order if not claimed[c[2]]][:need]
    bd, bj, bl, sd, sl = 256, -1, -1, 256, -1
    if free:
        bd, bj, bl = free[0][0], free[0][2], octave(free[0][2])
    if len(free) > 1:
        sd, sl = free[1][0], octave(free[1][2])
    return bd, bj, bl, sd, sl


def _greedy(n, tasks, rec, claimed, octave, th, judge, need, cap, scheme, stats):
    """Runs the tasks (i, candidates, claims) in order against the claims.
    judge(bd, bl, sd, sl) -> None (accept) or a reason. Returns (holder,
    accepted): holder[j] = last writer of keypoint j, accepted = [(i, j)]."""
    holder = [-1] * n
    accepted = []
    for i, cands, claims in tasks:
        r = rec[i]
        under = [c for c in cands if c[0] <= th]
        r["ncand"] = len(under)
        r["skipped"] = sum(1 for c in under if claimed[c[2]])
        if scheme == "loop":
            bd, bj, bl, sd, sl = _pick_loop(cands, claimed, octave)
        else:
            bd, bj, bl, sd, sl = _pick_topk(cands, claimed, octave, need, cap, stats,
                                            scheme != "topk_without_rescan")
        r.update(best=bd, second=sd, best_level=bl, second_level=sl)
        if bj < 0:
            r["reason"] = NO_CANDIDATE if any(not claimed[c[2]] for c in cands) or not cands \
                else ALL_CLAIMED
            continue
        why = OVER_TH if bd > th else judge(bd, bl, sd, sl)
        if why is not None:
            r["reason"] = why
            continue
        r["overwrote"] = holder[bj] >= 0
        r["reason"] = ACCEPTED_OVERWRITES if holder[bj] >= 0 else ACCEPTED
        r["kp"] = bj
        holder[bj] = i
        claimed[bj] = bool(claims)
        accepted.append((i, bj))
    return holder, accepted


def _rotation(holder, accepted, rec, angle_from, angle_to, check_ori, info):
    """The histogram and its cut (ORBmatcher.cc:1856-1876, :384-407): an entry
    is a keypoint index, so a keypoint written twice is cleared, and counted,
    once per entry whose bin is cut, whoever wrote it last."""
    nmatches = len(accepted)
    hist = [[] for _ in range(HISTO_LENGTH)]
    if check_ori:
        for i, j in accepted:
            b = rot_bin(angle_from[i], angle_to[j])
            rec[i]["bin"] = b
            hist[b].append((i, j))
        keep = three_maxima(hist)
        info["hist"] = [len(h) for h in hist]
        info["keep"] = keep
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for i, j in hist[b]:
                    holder[j] = -1
                    nmatches -= 1
                    rec[i]["reason"] = ROT_CUT
    return np.array(holder, np.int32), nmatches


def _new_rec(n):
    return [dict(reason=None, kp=-1, best=256, second=256, best_level=-1, second_level=-1, bin=-1,
                 ncand=0, skipped=0, overwrote=False) for _ in range(n)]


def search_last(F, bf, uright, last, th, mono=False, check_ori=True, scheme="loop"):
    """F: RefFrame of the current frame (pose included); last: dict Tcw,
    kps_un, has_mp, outlier, mp_xyz, mp_desc, mp_nobs. match[j] = last-frame
    index whose map point ends in CurrentFrame.mvpMapPoints[j]."""
    n, nl = len(F.kps), len(last["kps_un"])
    rec, info = _new_rec(nl), dict(rescans=0)
    bf = f32(bf)
    mb = f32(bf / F.fx)
    R, t = F.Tcw[:3, :3], F.Tcw[:3, 3]
    Rt = [[R[c][r] for c in range(3)] for r in range(3)]
    twc = [f32(-float(v)) for v in _gemm3(Rt, t)]
    Tl = np.asarray(last["Tcw"], f32).reshape(4, 4)
    tlc = _gemm3(Tl[:3, :3], twc, Tl[:3, 3])
    forward = bool(tlc[2] > mb) and not mono
    backward = bool(f32(-tlc[2]) > mb) and not mono
    info.update(forward=forward, backward=backward, tlc_z=tlc[2])
    th = f32(th)
    tasks = []
    for i in range(nl):
        r = rec[i]
        if not last["has_mp"][i]:
            r["reason"] = NO_MP
            continue
        if last["outlier"][i]:
            r["reason"] = OUTLIER
            continue
        xc, yc, zc = _gemm3(R, [f32(v) for v in last["mp_xyz"][i]], t)
        invzc = f32(1.0 / float(zc))
        if invzc < 0:
            r["reason"] = BEHIND
            continue
        u = f32(f32(f32(F.fx * xc) * invzc) + F.cx)
        v = f32(f32(f32(F.fy * yc) * invzc) + F.cy)
        r["u"], r["v"] = u, v
        if u < F.minX or u > F.maxX or v < F.minY or v > F.maxY:
            r["reason"] = OUT_OF_IMAGE
            continue
        octv = int(last["kps_un"]["octave"][i])
        radius = f32(th * F.scale[octv])
        if forward:
            lo, hi = octv, -1
        elif backward:
            lo, hi = 0, octv
        else:
            lo, hi = octv - 1, octv + 1
        idx = F.features_in_area(u, v, radius, lo, hi)
        r["window"] = list(idx)
        if not idx:
            r["reason"] = NO_WINDOW
            continue
        cands = []
        for pos, j in enumerate(idx):
            if uright[j] > 0:
                ur = f32(u - f32(bf * invzc))
                er = abs(f32(ur - f32(uright[j])))
                if er > radius:
                    continue
            cands.append((_hamming(last["mp_desc"][i], F.desc[j]), pos, j))
        tasks.append((i, cands, last["mp_nobs"][i] > 0))
    holder, accepted = _greedy(n, tasks, rec, [False] * n, lambda j: int(F.kps["octave"][j]),
                               TH_HIGH, lambda *a: None, 1, TH_HIGH, scheme, info)
    match, nm = _rotation(holder, accepted, rec, last["kps_un"]["angle"], F.kps["angle"],
                          check_ori, info)
    return match, nm, rec, info


def search_local(F, uright, track, mp_desc, mp_nobs, cur_nobs, th, nnratio, scheme="loop"):
    """track: dict in_view, proj_x, proj_y, proj_xr, level, view_cos (what
    Frame::isInFrustum left in the map points); cur_nobs[j]: Observations() of
    the map point keypoint j holds on entry (None: no keypoint holds one)."""
    n, nmp = len(F.kps), len(track["in_view"])
    rec, info = _new_rec(nmp), dict(rescans=0)
    th, nnratio = f32(th), f32(nnratio)
    factor = float(th) != 1.0
    tasks = []
    for i in range(nmp):
        r = rec[i]
        if not track["in_view"][i]:
            r["reason"] = NOT_IN_VIEW
            continue
        level = int(track["level"][i])
        rad = f32(2.5) if float(f32(track["view_cos"][i])) > 0.998 else f32(4.0)
        if factor:
            rad = f32(rad * th)
        r["r"] = rad
        rad = f32(rad * F.scale[level])
        x, y = f32(track["proj_x"][i]), f32(track["proj_y"][i])
        idx = F.features_in_area(x, y, rad, level - 1, level)
        r["window"] = list(idx)
        if not idx:
            r["reason"] = NO_WINDOW
            continue
        cands = []
        for pos, j in enumerate(idx):
            if uright[j] > 0:
                er = abs(f32(f32(track["proj_xr"][i]) - f32(uright[j])))
                if er > rad:
                    continue
            cands.append((_hamming(mp_desc[i], F.desc[j]), pos, j))
        tasks.append((i, cands, mp_nobs[i] > 0))

    def judge(bd, bl, sd, sl):
        if bl == sl and f32(bd) > f32(nnratio * f32(sd)):
            return RATIO_REJECT
        return None

    claimed = [False] * n if cur_nobs is None else [bool(c > 0) for c in cur_nobs]
    holder, accepted = _greedy(n, tasks, rec, claimed, lambda j: int(F.kps["octave"][j]), TH_HIGH,
                               judge, 2, 255, scheme, info)
    return np.array(holder, np.int32), len(accepted), rec, info


def search_bow(kf_node, kf_valid, kf_desc, kf_angle, f_node, f_desc, f_angle, nnratio=0.7,
               check_ori=True, scheme="loop"):
    """The FeatureVectors are given as one node id per feature (-1: none); DBoW2
    adds a feature to its node in index order. match[j] = keyframe feature
    whose map point ends in vpMapPointMatches[j]."""
    nkf, nf = len(kf_node), len(f_node)
    rec, info = _new_rec(nkf), dict(rescans=0)
    nnratio = f32(nnratio)
    fv_kf, fv_f = {}, {}
    for i in range(nkf):
        if kf_node[i] >= 0:
            fv_kf.setdefault(int(kf_node[i]), []).append(i)
        else:
            rec[i]["reason"] = NO_NODE
    for j in range(nf):
        if f_node[j] >= 0:
            fv_f.setdefault(int(f_node[j]), []).append(j)
    tasks = []
    # the two-iterator walk with lower_bound visits the common nodes in ascending order
    for node in sorted(fv_kf):
        for i in fv_kf[node]:
            if node not in fv_f:
                rec[i]["reason"] = NODE_UNSHARED
            elif not kf_valid[i]:
                rec[i]["reason"] = NO_MP
            else:
                cands = [(_hamming(kf_desc[i], f_desc[j]), pos, j)
                         for pos, j in enumerate(fv_f[node])]
                tasks.append((i, cands, True))

    def judge(bd, bl, sd, sl):
        return None if f32(bd) < f32(nnratio * f32(sd)) else RATIO_REJECT

    holder, accepted = _greedy(nf, tasks, rec, [False] * nf, lambda j: 0, TH_LOW, judge, 2, 255,
                               scheme, info)
    match, nm = _rotation(holder, accepted, rec, kf_angle, f_angle, check_ori, info)
    return match, nm, rec, info


def replay_topk(fn, *args, **kw):
    """fn (search_last / search_local / search_bow) under the kernels' scheme.
    Returns (match, nmatches, rescans)."""
    match, nm, _, info = fn(*args, scheme="topk", **kw)
    return match, nm, info["rescans"]

"""Sequential restatement of LocalMapping::KeyFrameCulling (LocalMapping.cc:
1224-1319, non-monocular) with KeyFrame::SetBadFlag / EraseConnection /
UpdateBestCovisibles (KeyFrame.cc:139-158, 526-650), MapPoint::EraseObservation
/ SetBadFlag (MapPoint.cc:111-168), and of LocalMapping::MapPointCulling /
MapLineCulling (LocalMapping.cc:246-340), with plain Python objects, as the
project pins them.

The loops are the reference's: one list entry, one slot, one observer at a
time, with the break at three observers. Nothing here is shared with the
kernel, which counts all slots of a keyframe at once and commits with one slot
per thread: the agreement of the two checks that split.

A run counts every branch it takes (`stats`); BRANCHES / RECENT_BRANCHES name
them all."""
from collections import Counter

import numpy as np

from _localmap_ref import F

ACTIONS = ("kept", "culled", "first", "deferred")
REASONS = ("was_bad", "found_ratio", "few_observations", "aged_out", "stays")
BRANCHES = (
    "entry_first", "entry_kept", "entry_culled", "entry_deferred", "entry_no_points", "entry_bad_keyframe",
    "slot_null", "slot_bad_point", "slot_depth_far", "slot_depth_negative", "slot_depth_nan", "slot_counted",
    "obs_at_most_3", "obs_above_3", "observer_self", "observer_scale_pass", "observer_scale_fail",
    "observer_break_at_3", "slot_redundant", "slot_not_redundant",
    "connection_erased", "connection_not_listed", "erase_obs_not_observing", "erase_obs_stereo",
    "erase_obs_mono", "ref_handed_over", "ref_none_left", "point_goes_bad", "point_survives",
    "bad_point_slot_cleared",
    "tree_no_children", "tree_child_attached", "tree_child_bad_skipped", "tree_child_leftover",
    "tree_weight_tie", "tree_weight_absent", "tree_no_parent")
RECENT_BRANCHES = tuple("point_" + r for r in REASONS) + tuple("line_" + r for r in REASONS) + (
    "ratio_visible_zero_found_zero", "ratio_visible_zero_found_nonzero", "point_slot_cleared",
    "line_slot_cleared")


class KeyFrame:
    def __init__(self, index, k, depth):
        self.index, self.id = index, int(k["id"])
        self.Tcw = np.asarray(k["Tcw"], np.float32).reshape(4, 4)
        self.octave = [int(o) for o in k["kps_un"]["octave"]]
        self.uright = [float(u) for u in np.asarray(k["uright"], np.float32)]
        self.depth = None if depth is None else [float(d) for d in np.asarray(depth, np.float32)]
        self.mp = [None] * len(self.uright)     # mvpMapPoints
        self.weights = {}                       # mConnectedKeyFrameWeights: keyframe id -> (KeyFrame, w)
        self.ordered = []                       # mvpOrderedConnectedKeyFrames
        self.parent = None
        self.not_erase = self.bad = self.to_be_erased = False
        self.Tcp = None

    def weight(self, other):
        return self.weights[other.id][1] if other.id in self.weights else 0

    def pose_inverse(self):
        """Twc as KeyFrame::SetPose builds it (P6)"""
        T = self.Tcw
        Twc = np.eye(4, dtype=np.float32)
        for r in range(3):
            for c in range(3):
                Twc[r, c] = T[c, r]
            s = float(T[0, r]) * float(T[0, 3])
            s += float(T[1, r]) * float(T[1, 3])
            s += float(T[2, r]) * float(T[2, 3])
            Twc[r, 3] = F(s * -1.0)
        return Twc


class MapPoint:
    def __init__(self, index, bad, n_visible, n_found, ref):
        self.index, self.bad = index, bool(bad)
        self.n_visible, self.n_found = int(n_visible), int(n_found)
        self.obs = {}                           # keyframe id -> (KeyFrame, feature): iterated by id (P24)
        self.n_obs = 0
        self.ref_index = int(ref)
        self.ref_kf = None

    def observations(self):
        return [self.obs[k] for k in sorted(self.obs)]


class Map:
    """the dict form the package takes; a bad keyframe keeps its slots, but its
    points do not observe it"""

    def __init__(self, m, kf_bad=None, depth=None):
        K = len(m["kfs"])
        self.kfs = [KeyFrame(i, k, None if depth is None else depth[i]) for i, k in enumerate(m["kfs"])]
        self.points = [MapPoint(i, m["bad"][i], m["n_visible"][i], m["n_found"][i], m["ref_kf"][i])
                       for i in range(len(m["bad"]))]
        for kf, k in zip(self.kfs, m["kfs"]):
            kf.bad = bool(kf_bad[kf.index]) if kf_bad is not None else False
            for i, p in enumerate(k["mp"]):
                if p < 0:
                    continue
                pt = self.points[int(p)]
                kf.mp[i] = pt
                if not kf.bad:
                    pt.obs[kf.id] = (kf, i)
                    pt.n_obs += 2 if kf.uright[i] >= 0 else 1
        for p in self.points:
            p.ref_kf = self.kfs[p.ref_index] if 0 <= p.ref_index < K else None

    def state(self):
        P = self.points
        obs = np.full((len(P), 64), -1, np.int16)
        for p in P:
            for kf, i in p.obs.values():
                obs[p.index, kf.index] = i
        return dict(mp=[np.array([-1 if p is None else p.index for p in kf.mp], np.int32) for kf in self.kfs],
                    ref_kf=np.array([-1 if p.ref_kf is None else p.ref_kf.index for p in P], np.int32),
                    bad=np.array([p.bad for p in P], np.uint8), n_obs=np.array([p.n_obs for p in P], np.int32),
                    obs=obs)


def point_set_bad_flag(p, stats, what="bad_point_slot_cleared"):
    """MapPoint::SetBadFlag"""
    obs = p.observations()
    p.bad = True
    p.obs = {}
    for kf, idx in obs:
        kf.mp[idx] = None
        stats[what] += 1


def erase_observation(p, kf, stats):
    """MapPoint::EraseObservation(kf): True if the point went from good to bad"""
    if kf.id not in p.obs:
        stats["erase_obs_not_observing"] += 1
        return False
    idx = p.obs[kf.id][1]
    if kf.uright[idx] >= 0:
        p.n_obs -= 2
        stats["erase_obs_stereo"] += 1
    else:
        p.n_obs -= 1
        stats["erase_obs_mono"] += 1
    del p.obs[kf.id]
    if p.ref_kf is kf:
        left = p.observations()
        # begin() of an empty map: pinned to "no reference"
        p.ref_kf = left[0][0] if left else None
        stats["ref_handed_over" if left else "ref_none_left"] += 1
    if p.n_obs <= 2:
        was_good = not p.bad
        point_set_bad_flag(p, stats)
        stats["point_goes_bad"] += 1
        return was_good
    stats["point_survives"] += 1
    return False


def update_best_covisibles(kf):
    pairs = sorted((w, kid) for kid, (_, w) in kf.weights.items())
    kf.ordered = [kf.weights[kid][0] for _, kid in reversed(pairs)]


def set_bad_flag(kfs, kf, stats):
    """KeyFrame::SetBadFlag past its two early returns: the number of points set bad"""
    for kid in sorted(kf.weights):
        other = kf.weights[kid][0]
        if kf.id in other.weights:              # KeyFrame::EraseConnection
            del other.weights[kf.id]
            update_best_covisibles(other)
            stats["connection_erased"] += 1
        else:
            stats["connection_not_listed"] += 1
    n_bad = 0
    for p in kf.mp:
        if p is not None:
            n_bad += erase_observation(p, kf, stats)
    kf.weights = {}
    kf.ordered = []
    parent = kf.parent
    cands = [] if parent is None else [parent]
    children = sorted((c for c in kfs if c.parent is kf), key=lambda c: c.id)
    if not children:
        stats["tree_no_children"] += 1
    while children:
        go, mx, pc, pp = False, -1, None, None
        for c in children:
            if c.bad:
                stats["tree_child_bad_skipped"] += 1
                continue
            for conn in c.ordered:
                for cand in cands:
                    if conn.id == cand.id:
                        if conn.id not in c.weights:
                            stats["tree_weight_absent"] += 1
                        w = c.weight(conn)
                        if w > mx:
                            pc, pp, mx, go = c, conn, w, True
                        elif w == mx:
                            stats["tree_weight_tie"] += 1
        if not go:
            break
        pc.parent = pp
        cands.append(pc)
        children.remove(pc)
        stats["tree_child_attached"] += 1
    for c in children:
        c.parent = parent
        stats["tree_child_leftover"] += 1
    if parent is None:
        stats["tree_no_parent"] += 1            # the reference dereferences a null mpParent: pinned to "no mTcp"
    else:
        A, B = kf.Tcw, parent.pose_inverse()
        Tcp = np.zeros((4, 4), np.float32)
        for r in range(4):
            for c in range(4):
                s = float(A[r, 0]) * float(B[0, c])
                s += float(A[r, 1]) * float(B[1, c])
                s += float(A[r, 2]) * float(B[2, c])
                s += float(A[r, 3]) * float(B[3, c])
                Tcp[r, c] = F(s)
        kf.Tcp = Tcp
    kf.bad = True
    return n_bad


def keyframe_culling(prob, th_depth):
    """the whole call on a problem dict: (result dict, stats)"""
    stats = Counter()
    m = prob["map"]
    K = len(m["kfs"])
    mp_ = Map(m, prob["kf_bad"], prob["depth"])
    kfs = mp_.kfs
    W = np.asarray(prob["conn_w"]).reshape(K, K)
    for k, kf in enumerate(kfs):
        kf.weights = {kfs[j].id: (kfs[j], int(W[k, j])) for j in range(K) if W[k, j] > 0}
        kf.ordered = [kfs[int(j)] for j in prob["ordered"][k]]
        kf.parent = kfs[int(prob["parent"][k])] if prob["parent"][k] >= 0 else None
        kf.not_erase = bool(prob["not_erase"][k])
    th = F(th_depth)
    local = list(kfs[prob["cur"]].ordered)
    n_mps, n_red, action, n_bad = [], [], [], 0
    for kf in local:
        if kf.id == 0:
            stats["entry_first"] += 1
            n_mps.append(0)
            n_red.append(0)
            action.append(ACTIONS.index("first"))
            continue
        if kf.bad:
            stats["entry_bad_keyframe"] += 1    # no isBad() test: processed as written
        nmps = nred = 0
        for i, p in enumerate(kf.mp):
            if p is None:
                stats["slot_null"] += 1
                continue
            if p.bad:
                stats["slot_bad_point"] += 1
                continue
            d = F(kf.depth[i])
            if d > th or d < 0:
                stats["slot_depth_far" if d > th else "slot_depth_negative"] += 1
                continue
            if d != d:
                stats["slot_depth_nan"] += 1
            nmps += 1
            stats["slot_counted"] += 1
            if p.n_obs > 3:
                stats["obs_above_3"] += 1
                level = kf.octave[i]
                nobs = 0
                for okf, oi in p.observations():
                    if okf is kf:
                        stats["observer_self"] += 1
                        continue
                    if okf.octave[oi] <= level + 1:
                        stats["observer_scale_pass"] += 1
                        nobs += 1
                        if nobs >= 3:
                            stats["observer_break_at_3"] += 1
                            break
                    else:
                        stats["observer_scale_fail"] += 1
                if nobs >= 3:
                    nred += 1
                    stats["slot_redundant"] += 1
                else:
                    stats["slot_not_redundant"] += 1
            else:
                stats["obs_at_most_3"] += 1
        n_mps.append(nmps)
        n_red.append(nred)
        if nmps == 0:
            stats["entry_no_points"] += 1
        if float(nred) > 0.9 * float(nmps):
            if kf.not_erase:
                kf.to_be_erased = True
                stats["entry_deferred"] += 1
                action.append(ACTIONS.index("deferred"))
            else:
                n_bad += set_bad_flag(kfs, kf, stats)
                stats["entry_culled"] += 1
                action.append(ACTIONS.index("culled"))
        else:
            stats["entry_kept"] += 1
            action.append(ACTIONS.index("kept"))
    res = mp_.state()
    conn_w = np.zeros((K, K), np.int32)
    ordered = np.full((K, 64), -1, np.int32)
    Tcp = (np.array(prob["Tcp"], np.float32).reshape(K, 16).copy() if "Tcp" in prob
           else np.zeros((K, 16), np.float32))
    for k, kf in enumerate(kfs):
        for other, w in kf.weights.values():
            conn_w[k, other.index] = w
        ordered[k, :len(kf.ordered)] = [o.index for o in kf.ordered]
        if kf.Tcp is not None:
            Tcp[k] = kf.Tcp.reshape(16)
    res.update(conn_w=conn_w, ordered=ordered,
               parent=np.array([-1 if kf.parent is None else kf.parent.index for kf in kfs], np.int32),
               kf_bad=np.array([kf.bad for kf in kfs], np.uint8),
               to_be_erased=np.array([kf.to_be_erased for kf in kfs], np.uint8), Tcp=Tcp,
               list=np.array([kf.index for kf in local], np.int32), n_mps=np.array(n_mps, np.int32),
               n_redundant=np.array(n_red, np.int32), action=np.array(action, np.int32), n_points_bad=n_bad)
    return res, stats


class MapLine:
    def __init__(self, index, bad, n_visible, n_found, first_kf, n_obs):
        self.index, self.bad = index, bool(bad)
        self.n_visible, self.n_found = int(n_visible), int(n_found)
        self.first_kf, self.n_obs = int(first_kf), int(n_obs)
        self.slots = []                         # mObservations: (slot list of the keyframe, index)


def _cull_list(items, cur_id, set_bad, stats, what):
    """the loop of MapPointCulling / MapLineCulling: (what remains, reason per entry)"""
    remain, reasons = [], []
    for it in items:
        age = int(cur_id) - it.first_kf
        if not it.bad:
            with np.errstate(all="ignore"):
                ratio = F(it.n_found) / F(it.n_visible)
            if it.n_visible == 0:
                stats["ratio_visible_zero_found_zero" if it.n_found == 0
                      else "ratio_visible_zero_found_nonzero"] += 1
        if it.bad:
            r = "was_bad"
        elif ratio < F(0.25):
            set_bad(it)
            r = "found_ratio"
        elif age >= 2 and it.n_obs <= 3:
            set_bad(it)
            r = "few_observations"
        elif age >= 3:
            r = "aged_out"
        else:
            remain.append(it)
            r = "stays"
        stats[what + "_" + r] += 1
        reasons.append(REASONS.index(r))
    return remain, reasons


def cull_recent(prob):
    """MapPointCulling then MapLineCulling on a problem dict: (result dict, stats)"""
    stats = Counter()
    m, ln = prob["map"], prob["lines"]
    mp_ = Map(m, prob.get("kf_bad"))
    for p, f in zip(mp_.points, prob["first_kf"]):
        p.first_kf = int(f)
    lines = [MapLine(i, ln["bad"][i], ln["n_visible"][i], ln["n_found"][i], ln["first_kf"][i], ln["n_obs"][i])
             for i in range(len(ln["bad"]))]
    ml = [[None if x < 0 else lines[int(x)] for x in row] for row in ln["ml"]]
    for row in ml:
        for j, l in enumerate(row):
            if l is not None:
                l.slots.append((row, j))

    def line_set_bad(l):
        l.bad = True
        for row, j in l.slots:
            row[j] = None
            stats["line_slot_cleared"] += 1
        l.slots = []

    remain, reason = _cull_list([mp_.points[int(i)] for i in prob["recent"]], prob["cur_id"],
                                lambda p: point_set_bad_flag(p, stats, "point_slot_cleared"), stats, "point")
    lremain, lreason = _cull_list([lines[int(i)] for i in prob["recent_lines"]], prob["cur_id"],
                                  line_set_bad, stats, "line")
    res = mp_.state()
    del res["ref_kf"]
    res.update(recent=np.array([p.index for p in remain], np.int32), reason=np.array(reason, np.int32),
               ml=[np.array([-1 if l is None else l.index for l in row], np.int32) for row in ml],
               line_bad=np.array([l.bad for l in lines], np.uint8),
               recent_lines=np.array([l.index for l in lremain], np.int32),
               line_reason=np.array(lreason, np.int32))
    return res, stats

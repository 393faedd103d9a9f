"""Sequential restatement of LocalMapping::SearchInNeighbors (LocalMapping.cc:
922-1103, the point half, non-monocular), ORBmatcher::Fuse (ORBmatcher.cc:
1107-1277), MapPoint::Replace / ComputeDistinctiveDescriptors /
UpdateNormalAndDepth / PredictScale (MapPoint.cc) and KeyFrame::
GetFeaturesInArea / IsInImage / UpdateConnections (KeyFrame.cc) with plain
Python objects, as the project pins them. float32 and
float64 stand exactly where the reference has float and double (P6, P15, P16,
P24, P25).

The loops are the reference's, one map point and one candidate at a time; only
the Hamming popcount over a window's candidates is one numpy call. Nothing here
is shared with the kernel, which searches all points of a Fuse call at once and
commits in order: the agreement of the two checks that split.

A run counts the branches it takes (`stats`) and records the relative margin of
every threshold decision (`margins`)."""
import math
from collections import Counter

import numpy as np

from _localmap_ref import F, _acc, _rel

TH_LOW = 50
GRID_COLS, GRID_ROWS = 64, 48
REASONS = ("null", "bad", "in_kf", "behind", "out_of_image", "distance", "view", "empty_window",
           "no_match", "added", "replaced", "replaces", "bad_slot")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class Camera:
    """pinhole without distortion: the undistorted bounds are the image's"""

    def __init__(self, fx, fy, cx, cy, bf, width, height, scale, sigma2):
        self.fx, self.fy, self.cx, self.cy, self.bf = F(fx), F(fy), F(cx), F(cy), F(bf)
        self.min_x, self.max_x, self.min_y, self.max_y = F(0), F(width), F(0), F(height)
        self.grid_inv_w = F(GRID_COLS) / F(self.max_x - self.min_x)
        self.grid_inv_h = F(GRID_ROWS) / F(self.max_y - self.min_y)
        self.scale = np.asarray(scale, np.float32)
        self.inv_sigma2 = (F(1.0) / np.asarray(sigma2, np.float32)).astype(np.float32)
        self.nlevels = len(self.scale)
        # mfLogScaleFactor = log(mfScaleFactor) (P15)
        self.log_scale = F(math.log(float(self.scale[1]))) if self.nlevels > 1 else F(1)


class KeyFrame:
    def __init__(self, index, kid, Tcw, kps_un, uright, desc, cam):
        self.index, self.id = index, int(kid)
        self.Tcw = np.asarray(Tcw, np.float32).reshape(4, 4)
        self.kps_un = kps_un
        self.x = np.asarray(kps_un["x"], np.float32)
        self.y = np.asarray(kps_un["y"], np.float32)
        self.octave = [int(o) for o in kps_un["octave"]]
        self.uright = np.asarray(uright, np.float32)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.n = len(self.uright)
        self.mp = [None] * self.n          # mvpMapPoints
        self.ordered = []                  # mvpOrderedConnectedKeyFrames
        T = self.Tcw
        self.Ow = np.array([F(-1.0 * (float(T[0, r]) * float(T[0, 3]) + float(T[1, r]) * float(T[1, 3])
                                      + float(T[2, r]) * float(T[2, 3]))) for r in range(3)], np.float32)
        # Frame::AssignFeaturesToGrid with PosInGrid (Frame.cc:265-287, 527-538)
        self.grid = {}
        for i in range(self.n):
            # round(): halves away from zero
            px = int(math.floor(float(F(F(self.x[i] - cam.min_x) * cam.grid_inv_w)) + 0.5))
            py = int(math.floor(float(F(F(self.y[i] - cam.min_y) * cam.grid_inv_h)) + 0.5))
            if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
                self.grid.setdefault((px, py), []).append(i)


class MapPoint:
    def __init__(self, index, xyz, normal, min_dist, max_dist, desc, bad, n_visible, n_found):
        self.index = index
        self.xyz = np.asarray(xyz, np.float32).copy()
        self.normal = np.asarray(normal, np.float32).copy()
        self.min_dist, self.max_dist = F(min_dist), F(max_dist)
        self.desc = np.asarray(desc, np.uint8).copy()
        self.bad = bool(bad)
        self.n_visible, self.n_found = int(n_visible), int(n_found)
        self.obs = {}                      # keyframe id -> (KeyFrame, feature); iterated by id (P24)
        self.n_obs = 0
        self.ref_kf = None
        self.replaced = None
        self.desc_src = (-1, -1)

    def observations(self):
        return [self.obs[k] for k in sorted(self.obs)]

    def is_in_keyframe(self, kf):
        return kf.id in self.obs

    def add_observation(self, kf, idx):
        if kf.id in self.obs:
            return
        self.obs[kf.id] = (kf, idx)
        self.n_obs += 2 if kf.uright[idx] >= 0 else 1

    def compute_distinctive_descriptors(self):
        ob = self.observations()
        if self.bad or not ob:
            return
        n = len(ob)
        d = np.stack([kf.desc[i] for kf, i in ob])
        best_median, best = 2 ** 31 - 1, 0
        for i in range(n):
            row = sorted(int(_POP[np.bitwise_xor(d[i], d[j])].sum()) for j in range(n))
            median = row[int(0.5 * (n - 1))]
            if median < best_median:
                best_median, best = median, i
        kf, i = ob[best]
        self.desc = kf.desc[i].copy()
        self.desc_src = (kf.index, i)

    def update_normal_and_depth(self, cam):
        ob = self.observations()
        if self.bad or not ob:
            return
        normal = np.zeros(3, np.float32)
        for kf, _ in ob:
            d = self.xyz - kf.Ow
            inv = F(1.0 / math.sqrt(float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) + float(d[2]) * float(d[2])))
            normal = normal + d * inv
        ref = self.ref_kf
        pc = self.xyz - ref.Ow
        dist = F(math.sqrt(float(pc[0]) * float(pc[0]) + float(pc[1]) * float(pc[1]) + float(pc[2]) * float(pc[2])))
        level = ref.octave[self.obs[ref.id][1]]
        self.max_dist = dist * cam.scale[level]
        self.min_dist = self.max_dist / cam.scale[cam.nlevels - 1]
        self.normal = normal / F(len(ob))

    def replace(self, other, stats):
        """this->Replace(other): other survives"""
        if other is self:
            return
        obs = self.observations()
        self.obs = {}
        self.n_obs = 0
        self.bad = True
        self.replaced = other
        for kf, idx in obs:
            if not other.is_in_keyframe(kf):
                kf.mp[idx] = other
                other.add_observation(kf, idx)
                stats["replace_handover"] += 1
            else:
                kf.mp[idx] = None
                stats["replace_conflict"] += 1
        other.n_found += self.n_found
        other.n_visible += self.n_visible
        other.compute_distinctive_descriptors()


class Map:
    """keyframes (the table), points, and the index of the current keyframe's
    problem-independent parts; built from the dict form the package takes"""

    def __init__(self, cam, m):
        self.cam = cam
        self.kfs = [KeyFrame(i, k["id"], k["Tcw"], k["kps_un"], k["uright"], k["desc"], cam)
                    for i, k in enumerate(m["kfs"])]
        M = len(m["bad"])
        self.points = [MapPoint(i, m["xyz"][i], m["normal"][i], m["min_dist"][i], m["max_dist"][i],
                                m["desc"][i], m["bad"][i], m["n_visible"][i], m["n_found"][i])
                       for i in range(M)]
        for kf, k in zip(self.kfs, m["kfs"]):
            kf.ordered = [self.kfs[int(j)] for j in k.get("ordered", ())]
            for i, p in enumerate(k["mp"]):
                if p >= 0:
                    kf.mp[i] = self.points[int(p)]
                    self.points[int(p)].add_observation(kf, i)
        for p, r in zip(self.points, m["ref_kf"]):
            p.ref_kf = self.kfs[int(r)]

    def state(self):
        """the arrays of the package's result"""
        P, K = self.points, len(self.kfs)
        obs = np.full((len(P), 64), -1, np.int16)
        for p in P:
            for kf, i in p.obs.values():
                obs[p.index, kf.index] = i
        f = lambda attr, dt: np.array([getattr(p, attr) for p in P], dt)
        return dict(
            mp=[np.array([-1 if p is None else p.index for p in kf.mp], np.int32) for kf in self.kfs],
            xyz=np.array([p.xyz for p in P], np.float32).reshape(-1, 3),
            normal=np.array([p.normal for p in P], np.float32).reshape(-1, 3),
            min_dist=f("min_dist", np.float32), max_dist=f("max_dist", np.float32),
            desc=np.array([p.desc for p in P], np.uint8).reshape(-1, 32),
            ref_kf=np.array([p.ref_kf.index for p in P], np.int32), bad=f("bad", np.uint8),
            n_visible=f("n_visible", np.int32), n_found=f("n_found", np.int32),
            replaced_by=np.array([-1 if p.replaced is None else p.replaced.index for p in P], np.int32),
            n_obs=f("n_obs", np.int32), obs=obs,
            desc_src=np.array([p.desc_src for p in P], np.int32).reshape(-1, 2))


def _norm3(v):
    return F(math.sqrt(float(v[0]) * float(v[0]) + float(v[1]) * float(v[1]) + float(v[2]) * float(v[2])))


def predict_scale(cam, max_dist, dist, margins):
    if cam.nlevels <= 1:
        return 0
    ratio = F(max_dist) / F(dist)
    x = F(F(math.log(float(ratio))) / cam.log_scale)
    margins.append(abs(float(x) - round(float(x))) / max(1.0, abs(float(x))))
    return min(max(int(math.ceil(x)), 0), cam.nlevels - 1)


def features_in_area(cam, kf, x, y, r, margins):
    """KeyFrame::GetFeaturesInArea (KeyFrame.cc:642-681)"""
    out = []
    c0 = max(0, int(math.floor(F(F(x - cam.min_x - r) * cam.grid_inv_w))))
    if c0 >= GRID_COLS:
        return out
    c1 = min(GRID_COLS - 1, int(math.ceil(F(F(x - cam.min_x + r) * cam.grid_inv_w))))
    if c1 < 0:
        return out
    r0 = max(0, int(math.floor(F(F(y - cam.min_y - r) * cam.grid_inv_h))))
    if r0 >= GRID_ROWS:
        return out
    r1 = min(GRID_ROWS - 1, int(math.ceil(F(F(y - cam.min_y + r) * cam.grid_inv_h))))
    if r1 < 0:
        return out
    for ix in range(c0, c1 + 1):
        for iy in range(r0, r1 + 1):
            for j in kf.grid.get((ix, iy), ()):
                dx, dy = abs(kf.x[j] - x), abs(kf.y[j] - y)
                margins.append(_rel(dx, r))
                if dx < r:
                    margins.append(_rel(dy, r))
                if dx < r and dy < r:
                    out.append(j)
    return out


def fuse(cam, kf, points, th=3.0, stats=None, margins=None, trace=None):
    """ORBmatcher::Fuse(pKF, vpMapPoints, th): nFused. trace, if a list, gets
    (reason, best_idx, best_dist) per list entry."""
    stats = Counter() if stats is None else stats
    margins = [] if margins is None else margins
    T, Ow, th = kf.Tcw, kf.Ow, F(th)
    n_fused = 0

    def end(reason, bi=-1, bd=256):
        stats[reason] += 1
        if trace is not None:
            trace.append((REASONS.index(reason), bi, bd))

    for mp in points:
        if mp is None:
            end("null")
            continue
        if mp.bad:
            end("bad")
            continue
        if mp.is_in_keyframe(kf):
            end("in_kf")
            continue
        P = mp.xyz
        Pc = [F(_acc([(T[r, 0], P[0]), (T[r, 1], P[1]), (T[r, 2], P[2])]) + float(T[r, 3])) for r in range(3)]
        if Pc[2] < F(0):
            end("behind")
            continue
        with np.errstate(all="ignore"):
            invz = F(1) / Pc[2]
            x, y = Pc[0] * invz, Pc[1] * invz
            u, v = cam.fx * x + cam.cx, cam.fy * y + cam.cy
            ur = u - cam.bf * invz
        margins.extend((_rel(u, cam.min_x), _rel(u, cam.max_x), _rel(v, cam.min_y), _rel(v, cam.max_y)))
        if not (u >= cam.min_x and u < cam.max_x and v >= cam.min_y and v < cam.max_y):
            end("out_of_image")
            continue
        max_d, min_d = F(1.2) * mp.max_dist, F(0.8) * mp.min_dist
        PO = P - Ow
        dist = _norm3(PO)
        margins.extend((_rel(dist, min_d), _rel(dist, max_d)))
        if dist < min_d or dist > max_d:
            end("distance")
            continue
        dot = float(F(PO[0] * mp.normal[0])) + float(F(PO[1] * mp.normal[1])) + float(F(PO[2] * mp.normal[2]))
        margins.append(_rel(dot, 0.5 * float(dist)))
        if dot < 0.5 * float(dist):
            end("view")
            continue
        level = predict_scale(cam, mp.max_dist, dist, margins)
        radius = th * cam.scale[level]
        idxs = features_in_area(cam, kf, u, v, radius, margins)
        if not idxs:
            end("empty_window")
            continue
        dists = _POP[np.bitwise_xor(kf.desc[idxs], mp.desc[None, :])].sum(axis=1)
        best_dist, best_idx = 256, -1
        for idx, d in zip(idxs, dists):
            lv = kf.octave[idx]
            if lv < level - 1 or lv > level:
                stats["gate_level"] += 1
                continue
            ex, ey = u - kf.x[idx], v - kf.y[idx]
            if kf.uright[idx] >= 0:
                er = ur - kf.uright[idx]
                chi = float(F(F(ex * ex + ey * ey) + er * er) * cam.inv_sigma2[lv])
                margins.append(_rel(chi, 7.8))
                if chi > 7.8:
                    stats["gate_chi_stereo"] += 1
                    continue
            else:
                chi = float(F(ex * ex + ey * ey) * cam.inv_sigma2[lv])
                margins.append(_rel(chi, 5.99))
                if chi > 5.99:
                    stats["gate_chi_mono"] += 1
                    continue
            if d < best_dist:
                best_dist, best_idx = int(d), idx
            elif d == best_dist:
                stats["tie_first_wins"] += 1
        if best_dist > TH_LOW:
            stats["no_match_none_passed" if best_idx < 0 else "no_match_over_th_low"] += 1
            end("no_match", best_idx, best_dist)
            continue
        in_kf = kf.mp[best_idx]
        if in_kf is not None:
            if not in_kf.bad:
                if in_kf.n_obs > mp.n_obs:
                    mp.replace(in_kf, stats)
                    end("replaced", best_idx, best_dist)
                else:
                    if in_kf.n_obs == mp.n_obs:
                        stats["replace_equal_counts"] += 1
                    in_kf.replace(mp, stats)
                    end("replaces", best_idx, best_dist)
            else:
                end("bad_slot", best_idx, best_dist)
        else:
            mp.add_observation(kf, best_idx)
            kf.mp[best_idx] = mp
            end("added", best_idx, best_dist)
        n_fused += 1
    return n_fused


def update_connections(kf, stats):
    """KeyFrame::UpdateConnections (KeyFrame.cc:363-452) of kf: (conn_w by table
    index, ordered table indices, weights, {table index: AddConnection weight});
    ordered is None when KFcounter is empty"""
    counter = {}
    for mp in kf.mp:
        if mp is None or mp.bad:
            continue
        for okf, _ in mp.observations():
            if okf.id == kf.id:
                continue
            counter[okf.id] = (okf, counter.get(okf.id, (okf, 0))[1] + 1)
    conn_w = np.zeros(64, np.int32)
    if not counter:
        stats["connections_empty"] += 1
        return conn_w, None, None, {}
    nmax, kmax, pairs, added = 0, None, [], {}
    for kid in sorted(counter):
        okf, w = counter[kid]
        conn_w[okf.index] = w
        if w > nmax:
            nmax, kmax = w, okf
        if w >= 15:
            pairs.append((w, okf.id, okf))
            added[okf.index] = w
    if not pairs:
        stats["connections_below_threshold"] += 1
        pairs.append((nmax, kmax.id, kmax))
        added[kmax.index] = nmax
    pairs.sort(key=lambda t: (t[0], t[1]))
    pairs.reverse()
    return conn_w, [p[2].index for p in pairs], [p[0] for p in pairs], added


def search_in_neighbors(cam, m, cur_index):
    """the whole call on a map dict: (Map after the call, result dict, stats, margins)"""
    stats, margins = Counter(), []
    mp_ = Map(cam, m)
    cur = mp_.kfs[cur_index]
    targets, fuse_target = [], set()
    for kf1 in cur.ordered[:10]:
        if kf1.id in fuse_target:
            continue
        targets.append(kf1)
        fuse_target.add(kf1.id)
        for kf2 in kf1.ordered[:5]:
            if kf2.id in fuse_target or kf2.id == cur.id:
                stats["second_neighbour_skipped"] += 1
                continue
            targets.append(kf2)
    if len(set(t.id for t in targets)) < len(targets):
        stats["duplicate_target"] += 1
    matches = list(cur.mp)
    n_fused = [fuse(cam, t, matches, 3.0, stats, margins) for t in targets]
    cands, seen = [], set()
    for t in targets:
        for p in t.mp:
            if p is None:
                continue
            if p.bad or p.index in seen:
                stats["candidate_bad" if p.bad else "candidate_dedup"] += 1
                continue
            seen.add(p.index)
            cands.append(p)
    n_fused.append(fuse(cam, cur, cands, 3.0, stats, margins))
    for p in cur.mp:
        if p is not None and not p.bad:
            p.compute_distinctive_descriptors()
            p.update_normal_and_depth(cam)
    conn_w, ordered, ordered_w, added = update_connections(cur, stats)
    add_conn = np.zeros(64, np.int32)
    for k, w in added.items():
        add_conn[k] = w
    res = mp_.state()
    res.update(targets=np.array([t.index for t in targets], np.int32), n_fused=np.array(n_fused, np.int32),
               n_candidates=len(cands), conn_w=conn_w, n_ordered=-1 if ordered is None else len(ordered),
               ordered=np.array(ordered or [], np.int32), ordered_w=np.array(ordered_w or [], np.int32),
               add_conn=add_conn)
    return mp_, res, stats, margins

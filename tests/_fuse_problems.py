"""Seeded SearchInNeighbors / Fuse problems (no images): scene corners seen by K
keyframes on a short trajectory, projected in double and stored as float with
controlled pixel noise. The maps are built as triangulation leaves them: a
corner is owned by several two-observation points that different keyframe
pairs created, by older points with three and more observations, and some of
its keypoints hold no point. The set holds the smallest shapes at which the
kernel can still go wrong (see NAMES)."""
import functools
import math

import numpy as np

import _fuse_ref as ref

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
W, H = 640, 480
CAM = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, bf=40.0)
NLEVELS = 8
SCALE = np.cumprod(np.concatenate([[1.0], np.full(NLEVELS - 1, 1.2)]).astype(np.float32)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)


def camera():
    return ref.Camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["bf"], W, H, SCALE, SIGMA2)


def _pose(R, centre):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ centre
    return T.astype(np.float32)


def _rot(rng, max_angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _project(T, X):
    Xc = T[:3, :3].astype(np.float64) @ X + T[:3, 3].astype(np.float64)
    z = Xc[2]
    return CAM["fx"] * Xc[0] / z + CAM["cx"], CAM["fy"] * Xc[1] / z + CAM["cy"], z


def _flip(rng, desc, nbits):
    d = desc.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _finish(kfs, pts, cur, corner=None):
    """the dict form from keyframe dicts (with mp filled) and point dicts (xyz,
    ref_kf, n_visible, n_found): descriptor, normal and distances are the
    restatement's ComputeDistinctiveDescriptors / UpdateNormalAndDepth of the map
    as built"""
    M = len(pts)
    m = dict(kfs=kfs, xyz=np.array([p["xyz"] for p in pts], np.float32).reshape(M, 3),
             normal=np.zeros((M, 3), np.float32), min_dist=np.zeros(M, np.float32),
             max_dist=np.zeros(M, np.float32), desc=np.zeros((M, 32), np.uint8),
             ref_kf=np.array([p["ref_kf"] for p in pts], np.int32).reshape(M),
             bad=np.zeros(M, np.uint8),
             n_visible=np.array([p.get("n_visible", 3) for p in pts], np.int32).reshape(M),
             n_found=np.array([p.get("n_found", 2) for p in pts], np.int32).reshape(M))
    cam = camera()
    built = ref.Map(cam, m)
    for p in built.points:
        p.compute_distinctive_descriptors()
        p.update_normal_and_depth(cam)
        m["desc"][p.index], m["normal"][p.index] = p.desc, p.normal
        m["min_dist"][p.index], m["max_dist"][p.index] = p.min_dist, p.max_dist
    for p, over in zip(range(M), pts):       # a hand-built problem's own attributes
        for k in ("normal", "min_dist", "max_dist", "desc"):
            if k in over:
                m[k][p] = over[k]
    return dict(map=m, cur=cur, corner=np.array([-1] * M if corner is None else corner, np.int64))


def scene(seed, K, N, n_first=10, noise=0.5, mono=None, cur_points=True, empty_target=False,
          clutter=0.25, corners_per=1.3, spread=0.5):
    """K keyframes of N keypoints each; the current keyframe is the newest.
    mono: per-keyframe share of keypoints without a right coordinate (default:
    keyframe 1 all, keyframe 2 half, the rest a twentieth)."""
    rng = np.random.default_rng(seed)
    C = max(1, int(N * corners_per))
    u, v = rng.uniform(15, W - 15, C), rng.uniform(15, H - 15, C)
    z = rng.uniform(2.0, 8.0, C)
    X = np.stack([(u - CAM["cx"]) * z / CAM["fx"], (v - CAM["cy"]) * z / CAM["fy"], z], 1)
    dmax = z * 1.2 ** rng.uniform(0.0, 6.5, C)       # the distance at which a corner is at level 0
    base = rng.integers(0, 256, (C, 32), dtype=np.uint8)
    ids = rng.permutation(K) * 3 + 7                 # table order is not id order
    cur = int(np.argmax(ids))
    kfs, seen = [], [dict() for _ in range(C)]       # seen[c]: table index -> feature
    for k in range(K):
        centre = rng.normal(size=3) * np.array([spread, 0.3 * spread, 0.6 * spread])
        T = _pose(_rot(rng, 0.04), centre if k != cur else np.zeros(3))
        share = (1.0 if k == 1 else 0.5 if k == 2 else 0.05) if mono is None else mono[k]
        vis = []
        for c in rng.permutation(C):
            pu, pv, pz = _project(T, X[c])
            if pz > 0.5 and 12 < pu < W - 12 and 12 < pv < H - 12:
                vis.append((int(c), pu, pv, pz))
        n_real = min(len(vis), int(round(N * (1 - clutter))))
        kp = np.zeros(N, KP_DTYPE)
        ur = np.full(N, -1, np.float32)
        desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        order = rng.permutation(N)
        for j, (c, pu, pv, pz) in enumerate(vis[:n_real]):
            i = int(order[j])
            dist = float(np.linalg.norm(X[c] - centre if k != cur else X[c]))
            lv = int(np.clip(round(math.log(dmax[c] / dist) / math.log(1.2)), 0, NLEVELS - 1))
            s = noise * float(SCALE[lv])
            kp["x"][i], kp["y"][i] = pu + rng.normal() * s, pv + rng.normal() * s
            kp["octave"][i] = lv
            if rng.random() >= share:
                ur[i] = kp["x"][i] - CAM["bf"] / pz + rng.normal() * s
            desc[i] = _flip(rng, base[c], int(rng.integers(0, 14)) if rng.random() > 0.08 else 70)
            seen[c][k] = i
        real = [int(order[j]) for j in range(n_real)]
        for j in range(n_real, N):                   # clutter, a third of it beside a real keypoint
            i = int(order[j])
            kp["octave"][i] = rng.integers(0, NLEVELS)
            kp["x"][i], kp["y"][i] = rng.uniform(5, W - 5), rng.uniform(5, H - 5)
            if real and rng.random() < 0.35:
                r = real[int(rng.integers(len(real)))]
                off = rng.uniform(2.0, 7.0) * float(SCALE[kp["octave"][r]])
                ang = rng.uniform(0, 2 * math.pi)
                kp["x"][i] = np.clip(kp["x"][r] + off * math.cos(ang), 1, W - 2)
                kp["y"][i] = np.clip(kp["y"][r] + off * math.sin(ang), 1, H - 2)
                kp["octave"][i] = max(0, int(kp["octave"][r]) - int(rng.integers(0, 3)))
                desc[i] = _flip(rng, desc[r], int(rng.integers(0, 30)))
                if rng.random() < 0.5:
                    ur[i] = ur[r]
            elif rng.random() >= share:
                ur[i] = kp["x"][i] - rng.uniform(5, 20)
        kp["angle"] = rng.uniform(0, 360, N)
        kfs.append(dict(id=int(ids[k]), Tcw=T, kps_un=kp, uright=ur, desc=desc,
                        mp=np.full(N, -1, np.int32), ordered=[]))
    # the map points: per corner an older point (three or more observers) with
    # some probability, two-observation points from the remaining observers
    skip = set() if cur_points else {cur}
    blank = None
    if empty_target and K > 2:
        blank = [k for k in range(K) if k != cur][-1]
        skip.add(blank)
    pts, corner = [], []
    for c in range(C):
        obs = [(k, i) for k, i in seen[c].items() if k not in skip]
        rng.shuffle(obs)
        groups = []
        if len(obs) >= 3 and rng.random() < 0.35:
            g = int(rng.integers(3, len(obs) + 1))
            groups.append(obs[:g])
            obs = obs[g:]
        while len(obs) >= 2:
            if rng.random() < 0.75:
                groups.append(obs[:2])
            obs = obs[2:]
        for g in groups:
            p = len(pts)
            jitter = rng.normal(size=3) * (0.002 * X[c][2] if noise else 0.0)
            pts.append(dict(xyz=X[c] + jitter, ref_kf=g[0][0], n_visible=int(rng.integers(1, 30)),
                            n_found=int(rng.integers(1, 20))))
            corner.append(c)
            for k, i in g:
                kfs[k]["mp"][i] = p
    # covisibility: shared points, weight descending, id descending (P24)
    w = np.zeros((K, K), np.int64)
    owner = {}
    for k in range(K):
        for p in kfs[k]["mp"]:
            if p >= 0:
                owner.setdefault(int(p), []).append(k)
    for ks in owner.values():
        for a in ks:
            for b in ks:
                if a != b:
                    w[a, b] += 1
    for k in range(K):
        nb = [j for j in range(K) if j != k and w[k, j] > 0]
        nb.sort(key=lambda j: (-w[k, j], -ids[j]))
        kfs[k]["ordered"] = nb
    first = [j for j in kfs[cur]["ordered"]]
    if not cur_points:                               # no shared point: the nearest ids stand in
        first = sorted((j for j in range(K) if j != cur and j != blank), key=lambda j: -ids[j])
    if blank is not None:
        first.insert(1, blank)
    kfs[cur]["ordered"] = first[:n_first]
    return _finish(kfs, pts, cur, corner)


def _hand_kf(kid, centre, feats):
    """a keyframe looking along +z at `centre`; feats: (x, y, octave, uright, desc)"""
    n = len(feats)
    kp = np.zeros(n, KP_DTYPE)
    for i, f in enumerate(feats):
        kp["x"][i], kp["y"][i], kp["octave"][i] = f[0], f[1], f[2]
    return dict(id=kid, Tcw=_pose(np.eye(3), np.asarray(centre, float)), kps_un=kp,
                uright=np.array([f[3] for f in feats], np.float32).reshape(n),
                desc=np.array([f[4] for f in feats], np.uint8).reshape(n, 32),
                mp=np.full(n, -1, np.int32), ordered=[])


def _px(centre, X):
    return _project(_pose(np.eye(3), np.asarray(centre, float)), np.asarray(X, float))


def hand_tie():
    """two candidates of one window tie on distance in different cell columns:
    the lower column wins although its keypoint has the higher index"""
    rng = np.random.default_rng(5)
    X, d = np.array([0.03986, 0.02, 4.0]), rng.integers(0, 256, 32, dtype=np.uint8)
    cu, cv, cz = _px([0, 0, 0], X)
    tu, tv, tz = _px([0.3, 0, 0], X)
    dr = CAM["bf"] / tz
    # cells are 10 px wide and tu is 285.0: 1.9 px either side straddle a column border
    # and stay under the stereo chi-square gate (2 * 1.9^2 < 7.8)
    da, db = _flip(rng, d, 6), _flip(rng, d, 6)
    t = _hand_kf(4, [0.3, 0, 0], [(tu + 1.9, tv, 0, tu + 1.9 - dr, da), (tu - 1.9, tv, 0, tu - 1.9 - dr, db),
                                  (50.0, 60.0, 0, -1.0, _flip(rng, d, 120))])
    c = _hand_kf(9, [0, 0, 0], [(cu, cv, 0, cu - CAM["bf"] / cz, d)])
    c["mp"][0] = 0
    c["ordered"] = [0]
    return _finish([t, c], [dict(xyz=X, ref_kf=1)], 1, [0])


def hand_conflict():
    """Replace conflict: A (in the current keyframe) and B (in the target) are both
    seen by a third keyframe that is no target; a second point of the current
    keyframe has an observer outside the target list too"""
    rng = np.random.default_rng(6)
    X, X2 = np.array([-0.1, 0.05, 3.5]), np.array([0.6, -0.3, 5.0])
    d, d2 = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)

    def feat(centre, P, desc, dx=0.0):
        pu, pv, pz = _px(centre, P)
        return (pu + dx, pv, 0, pu + dx - CAM["bf"] / pz, desc)

    cc, ct, c3, c4 = [0, 0, 0], [0.25, 0, 0], [-0.2, 0.1, 0], [0.1, -0.15, 0.05]
    cur = _hand_kf(20, cc, [feat(cc, X, d), feat(cc, X2, d2)])
    tgt = _hand_kf(11, ct, [feat(ct, X, _flip(rng, d, 4))])
    third = _hand_kf(3, c3, [feat(c3, X, _flip(rng, d, 3)), feat(c3, X, _flip(rng, d, 5), 1.5),
                             feat(c3, X2, _flip(rng, d2, 2))])
    fourth = _hand_kf(15, c4, [feat(c4, X, _flip(rng, d, 2))])
    # A = point 0: cur[0], third[0]; B = point 1: tgt[0], third[1], fourth[0]; point 2: cur[1], third[2]
    cur["mp"][:] = [0, 2]
    tgt["mp"][:] = [1]
    third["mp"][:] = [0, 1, 2]
    fourth["mp"][:] = [1]
    cur["ordered"] = [1]
    return _finish([cur, tgt, third, fourth],
                   [dict(xyz=X, ref_kf=0), dict(xyz=X, ref_kf=1), dict(xyz=X2, ref_kf=0)], 0, [0, 0, 1])


def hand_gates():
    """points of the current keyframe that each target rejects: behind it,
    outside its image, too near, too far, seen from behind; two targets ahead
    of the current keyframe"""
    rng = np.random.default_rng(7)
    cc, t1, t2 = [0, 0, 0], [0.1, 0, 3.0], [-0.1, 0.05, 3.2]
    Xs = [np.array([0.2, 0.1, 2.0]),        # in front of the current keyframe, behind the targets
          np.array([3.4, 0.5, 6.0]),        # outside the targets' images
          np.array([0.1, 0.1, 7.0]), np.array([-0.2, 0.1, 7.5]), np.array([0.3, -0.2, 8.0]),
          np.array([0.0, 0.2, 6.5])]        # passes the gates: an empty window
    ds = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in Xs]
    feats = []
    for X, d in zip(Xs, ds):
        pu, pv, pz = _px(cc, X)
        feats.append((pu, pv, 1, pu - CAM["bf"] / pz, d))
    cur = _hand_kf(30, cc, feats)
    cur["mp"][:] = range(len(Xs))
    tg = [_hand_kf(10 + i, t, [(100.0 + i, 100.0, 0, 90.0, rng.integers(0, 256, 32, dtype=np.uint8))])
          for i, t in enumerate((t1, t2))]
    cur["ordered"] = [1, 2]
    pts = [dict(xyz=X, ref_kf=0) for X in Xs]
    pts[2].update(min_dist=np.float32(20.0), max_dist=np.float32(80.0))      # too near
    pts[3].update(min_dist=np.float32(0.1), max_dist=np.float32(1.0))        # too far
    pts[4].update(normal=np.array([0, 0, -1], np.float32))                   # seen from behind
    return _finish([cur] + tg, pts, 0, list(range(len(Xs))))


# name -> builder; seeds chosen so that no decision hangs on the last bits
# (test_fuse_ref.py checks it on the restatement alone)
_BUILDERS = {
    "n0": lambda: scene(11, 3, 0),
    "n1": lambda: scene(12, 3, 1, clutter=0.0),
    "n65": lambda: scene(13, 5, 65, n_first=3),
    "n300": lambda: scene(14, 8, 300),
    "n300_clean": lambda: scene(15, 8, 300, noise=0.0),
    "n300_first1": lambda: scene(16, 6, 300, n_first=1),
    "n300_first0": lambda: scene(17, 4, 300, n_first=0),
    "n2048": lambda: scene(18, 12, 2048, n_first=4, corners_per=1.1),
    "kf64": lambda: scene(19, 64, 120, corners_per=2.0, spread=0.35),
    "cur_empty": lambda: scene(20, 5, 80, cur_points=False),
    "target_empty": lambda: scene(21, 6, 80, empty_target=True),
    "mono_mixed": lambda: scene(22, 5, 120, mono=[1.0, 0.5, 0.0, 0.5, 0.2]),
    "hand_tie": hand_tie,
    "hand_conflict": hand_conflict,
    "hand_gates": hand_gates,
}
NAMES = tuple(_BUILDERS)
SMALL = ("n0", "n1", "n65", "cur_empty", "target_empty", "hand_tie", "hand_conflict", "hand_gates",
         "mono_mixed")


@functools.lru_cache(maxsize=None)
def problem(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def ref_run(name):
    """(Map after the call, result, stats, margins) of the restatement, computed once"""
    p = problem(name)
    return ref.search_in_neighbors(camera(), p["map"], p["cur"])

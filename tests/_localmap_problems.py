"""Seeded CreateNewMapPoints / CreateNewMapLines problems (no images): world
points and 3D segments in front of a
current keyframe and up to ten neighbours on a trajectory whose steps straddle
the stereo baseline mb, projected in double and stored as float with pixel
noise of 0-2 sigma of the level. The set holds the smallest shapes at which the
kernels can still go wrong (see problems())."""
import functools

import numpy as np

import _localmap_ref as ref

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
KL_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"),
                     ("pt_y", "<f4"), ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"),
                     ("startPointY", "<f4"), ("endPointX", "<f4"), ("endPointY", "<f4"),
                     ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"),
                     ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"),
                     ("numOfPixels", "<i4")])
W, H = 640, 480
CAM = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, bf=40.0)
NLEVELS = 8
SCALE = np.cumprod(np.concatenate([[1.0], np.full(NLEVELS - 1, 1.2)]).astype(np.float32)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)


def camera():
    return ref.Camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], CAM["bf"], SCALE, SIGMA2)


def _rot(rng, max_angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _pose(rng, centre, max_angle=0.03):
    R = _rot(rng, max_angle)          # Rcw
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ centre
    return T.astype(np.float32)


class Scene:
    """n_cur features in the current keyframe; neighbour k has n_neigh[k]."""

    def __init__(self, seed, n_cur, n_neigh, steps=None, nodes_per=8, big_node=0, forward=False,
                 noise=True, mp_share=None, neigh_mp_share=None, clones=0, nl_cur=0, nl_neigh=None):
        rng = self.rng = np.random.default_rng(seed)
        self.seed, self.noise, self.clones = seed, noise, clones
        cam = self.cam = camera()
        mb = float(cam.mb)
        self.M = M = max([n_cur] + list(n_neigh) + [1])
        # world points from pixels of the current view (identity-like pose at the origin)
        self.Tc = _pose(rng, np.zeros(3), 0.0)
        u = rng.uniform(20, W - 20, M)
        v = rng.uniform(20, H - 20, M)
        z = rng.uniform(0.8, 6.0, M)
        far = rng.random(M) < 0.06
        z[far] = rng.uniform(30.0, 80.0, far.sum())
        if forward:                     # a cluster near the principal point (the epipole)
            c = rng.random(M) < 0.25
            u[c] = CAM["cx"] + rng.uniform(-14, 14, c.sum())
            v[c] = CAM["cy"] + rng.uniform(-14, 14, c.sum())
        self.Xw = np.stack([(u - CAM["cx"]) * z / CAM["fx"], (v - CAM["cy"]) * z / CAM["fy"], z], 1)
        self.level = rng.integers(0, NLEVELS, M)
        self.base_desc = rng.integers(0, 256, (M, 32), dtype=np.uint8)
        n_nodes = max(1, M // nodes_per)
        self.node = rng.integers(0, n_nodes, M).astype(np.int32) * 7 + 3
        if big_node:
            self.node[rng.permutation(M)[:big_node]] = 5
        self.angle = rng.uniform(0, 360, M).astype(np.float32)
        self.mp_share = rng.uniform(0.3, 0.7) if mp_share is None else mp_share
        self.neigh_mp_share = neigh_mp_share
        self.nodepth_share = rng.uniform(0.05, 0.30)
        # 3D segments: most of moderate length at the scene's depth, some longer than
        # the median depth, some closer than 0.3 of it
        nl_neigh = [nl_cur] * len(n_neigh) if nl_neigh is None else nl_neigh
        self.L = L = max([nl_cur] + list(nl_neigh) + [1])
        su, sv = rng.uniform(40, W - 40, L), rng.uniform(40, H - 40, L)
        sz = rng.uniform(1.0, 6.0, L)
        near = rng.random(L) < 0.10
        sz[near] = rng.uniform(0.25, 0.6, near.sum())
        self.seg_s = np.stack([(su - CAM["cx"]) * sz / CAM["fx"], (sv - CAM["cy"]) * sz / CAM["fy"], sz], 1)
        d = rng.normal(size=(L, 3))
        d[:, 2] *= 0.3
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        length = rng.uniform(0.1, 1.2, L)
        long_ = rng.random(L) < 0.12
        length[long_] = rng.uniform(4.0, 9.0, long_.sum())
        length[near] = rng.uniform(0.05, 0.2, near.sum())
        self.seg_e = self.seg_s + d * length[:, None]
        self.seg_e[:, 2] = np.maximum(self.seg_e[:, 2], 0.15)
        self.seg_desc = rng.integers(0, 256, (L, 32), dtype=np.uint8)
        self.nl_cur = nl_cur
        self.cur = self._keyframe(100, self.Tc, n_cur, first=True, nl=nl_cur)
        # the trajectory: steps as multiples of mb, at least one under 1
        if steps is None:
            steps = [0.5, 1.6, 3.0, 0.9, 6.0, 2.2, 12.0, 1.2, 4.0, 8.0]
        self.neigh = []
        for k, n in enumerate(n_neigh):
            d = rng.normal(size=3)
            d[2] *= 0.2
            if forward and k % 2 == 0:
                d = np.array([0.02, -0.01, 1.0]) * (1 if k % 4 == 0 else -1)
            d = d / np.linalg.norm(d) * steps[k % len(steps)] * mb
            # ids on both sides of the current keyframe's (observation order, P24)
            self.neigh.append(self._keyframe(100 - 7 * (k + 1) if k % 3 else 100 + 5 * (k + 1),
                                             _pose(rng, d), n, first=False, nl=nl_neigh[k]))

    def _lines(self, T, nl, first):
        """nl key lines: the segments' projections (raw pixels, double then float),
        the line through both end points as three doubles, LBD rows with 0-80 bits
        flipped between views"""
        rng = self.rng
        kl = np.zeros(nl, KL_DTYPE)
        ld = np.zeros((nl, 32), np.uint8)
        lc = np.zeros((nl, 3))
        lsrc = np.full(nl, -1, np.int64)
        order = rng.permutation(self.L)[:nl]
        for i, m in enumerate(order):
            ends = []
            for X in (self.seg_s[m], self.seg_e[m]):
                Xc = T[:3, :3] @ X + T[:3, 3]
                zc = Xc[2] if abs(Xc[2]) > 1e-3 else 1e-3
                u, v = CAM["fx"] * Xc[0] / zc + CAM["cx"], CAM["fy"] * Xc[1] / zc + CAM["cy"]
                if self.noise:
                    u, v = u + rng.normal() * 0.5, v + rng.normal() * 0.5
                ends.append((np.float32(u), np.float32(v)))
            (kl["startPointX"][i], kl["startPointY"][i]), (kl["endPointX"][i], kl["endPointY"][i]) = ends
            kl["lineLength"][i] = np.hypot(ends[1][0] - ends[0][0], ends[1][1] - ends[0][1])
            a = np.array([float(ends[0][0]), float(ends[0][1]), 1.0])
            b = np.array([float(ends[1][0]), float(ends[1][1]), 1.0])
            l = np.cross(a, b)
            lc[i] = l / max(np.hypot(l[0], l[1]), 1e-12)
            d = self.seg_desc[m].copy()
            if not first:
                flips = int(80 * rng.random() ** 2) if self.noise else 0
                bits = rng.permutation(256)[:flips]
                np.bitwise_xor.at(d, bits // 8, (1 << (bits % 8)).astype(np.uint8))
            ld[i] = d
            lsrc[i] = m
        return kl, ld, lc, lsrc

    def _keyframe(self, kid, Tcw, n, first, nl=0):
        rng, cam = self.rng, self.cam
        M = self.M
        T = Tcw.astype(np.float64)
        Xc = self.Xw @ T[:3, :3].T + T[:3, 3]
        kps = np.zeros(n, KP_DTYPE)
        kun = np.zeros(n, KP_DTYPE)
        ur = np.full(n, -1.0, np.float32)
        dep = np.full(n, -1.0, np.float32)
        desc = np.zeros((n, 32), np.uint8)
        node = np.full(n, -1, np.int32)
        src = np.full(n, -1, np.int64)     # the world point a feature shows, -1 clutter / decoy
        mpx = np.zeros((n, 3), np.float32) # where the feature's map point is (read where has_mp)
        Rwc, tcw = T[:3, :3].T, T[:3, 3]
        order = rng.permutation(M)[:n]
        for i, m in enumerate(order):
            zc = Xc[m, 2]
            lvl = int(self.level[m])
            if not first and rng.random() < 0.12:       # inconsistent octave
                lvl = int(rng.integers(0, NLEVELS))
            ok = zc > 0.05
            if ok:
                uu = CAM["fx"] * Xc[m, 0] / zc + CAM["cx"]
                vv = CAM["fy"] * Xc[m, 1] / zc + CAM["cy"]
                ok = -50 < uu < W + 50 and -50 < vv < H + 50
            if not ok:                                  # clutter in its place
                uu, vv, zc = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.5, 8.0)
            else:
                src[i] = m
            if self.noise:
                amp = rng.uniform(0, 2.0) * float(SCALE[lvl])
                th = rng.uniform(0, 2 * np.pi)
                uu, vv = uu + amp * np.cos(th), vv + amp * np.sin(th)
            if not first and self.noise and rng.random() < 0.10:
                # a decoy: moved along the ray's image (the epipolar line), so it still
                # passes the matcher and triangulates somewhere else
                zz = Xc[m, 2] * rng.choice([0.05, 0.3, 3.0, -0.5])
                Xd = self.Xw[m] * (zz / max(self.Xw[m, 2], 1e-6))
                Xd = Xd @ T[:3, :3].T + T[:3, 3]
                src[i] = -1
                if abs(Xd[2]) > 1e-3:
                    uu = CAM["fx"] * Xd[0] / Xd[2] + CAM["cx"]
                    vv = CAM["fy"] * Xd[1] / Xd[2] + CAM["cy"]
            kun["x"][i], kun["y"][i] = uu, vv
            kun["octave"][i] = lvl
            kun["angle"][i] = self.angle[m] + (0 if first else rng.choice([0, 0, 0, 0, 0, 3.0, 40.0, 95.0, 200.0, 310.0]))
            kun["angle"][i] = np.float32(kun["angle"][i] % 360.0)
            kun["size"][i] = 31.0 * SCALE[lvl]
            kps[i] = kun[i]
            if self.noise:
                kps["x"][i] = kun["x"][i] + np.float32(0.37)     # mvKeys differs from mvKeysUn
                kps["y"][i] = kun["y"][i] - np.float32(0.21)
            if rng.random() >= self.nodepth_share and zc < 40.0:
                dz = zc * (1 + (rng.normal() * 0.01 if self.noise else 0.0))
                dep[i] = dz
                ur[i] = kun["x"][i] - np.float32(CAM["bf"]) / dep[i]
            d = self.base_desc[m].copy()
            if not first:
                flips = int(80 * rng.random() ** 2) if self.noise else 0
                bits = rng.permutation(256)[:flips]
                np.bitwise_xor.at(d, bits // 8, (1 << (bits % 8)).astype(np.uint8))
            desc[i] = d
            zz = zc * (1 + (rng.normal() * 0.02 if self.noise else 0.0))
            mpx[i] = Rwc @ (np.array([(uu - CAM["cx"]) * zz / CAM["fx"], (vv - CAM["cy"]) * zz / CAM["fy"], zz]) - tcw)
            node[i] = self.node[m]
            if not first and rng.random() < 0.10:
                node[i] = self.node[rng.integers(0, M)]      # the word changed between views
            if rng.random() < 0.02:
                node[i] = -1
        # twins: the same feature twice (equal distances: the later one replaces; two
        # KF1 features after one KF2 feature: the second finds it claimed)
        for i in range(1, n):
            if rng.random() < 0.06:
                j = int(rng.integers(0, i))
                kun[i], kps[i], ur[i], dep[i], desc[i], node[i], src[i], mpx[i] = (
                    kun[j], kps[j], ur[j], dep[j], desc[j], node[j], src[j], mpx[j])
        share = self.mp_share if first or self.neigh_mp_share is None else self.neigh_mp_share
        has_mp = (rng.random(n) < share).astype(np.uint8)
        if self.clones:
            # one clean feature `clones` times over, all free, in every keyframe: KF1's
            # fifth clone finds the four best candidates of its list claimed
            i0 = int(np.flatnonzero(order == 0)[0])
            node[i0] = self.node[0]
            has_mp[i0] = 0
            for i in range(n - self.clones + 1, n):
                if i != i0:
                    kun[i], kps[i], ur[i], dep[i], desc[i], node[i], src[i] = (
                        kun[i0], kps[i0], ur[i0], dep[i0], desc[i0], node[i0], src[i0])
                    has_mp[i] = 0
        kl, ld, lc, lsrc = self._lines(T, nl, first)
        kf = ref.KeyFrame(kid, Tcw, kps, kun, ur, dep, desc, node, has_mp, mpx, kl, ld, lc)
        kf.src, kf.lsrc = src, lsrc
        return kf


class Problem:
    def __init__(self, name, scene, reverse=False):
        self.name, self.cam = name, scene.cam
        self.cur = scene.cur
        self.neigh = list(reversed(scene.neigh)) if reverse else list(scene.neigh)
        self.scene = scene


@functools.lru_cache(maxsize=None)
def problems():
    """name -> Problem. N = 0, 1, 65 (one over a wave), 300, 2048; a node with
    more than 64 features; 0, 1, 3 and 10 neighbours; one neighbour list in both
    orders; neighbours smaller than the current keyframe; forward motion (the
    epipole inside the image). Lines: NL = 0, 1, 2, 80 and 256, neighbours with
    fewer than two lines, a neighbour without a map point ("mixed", neighbour 2)."""
    s300 = Scene(11, 300, [300] * 10, nl_cur=80)
    out = [
        Problem("n0", Scene(1, 0, [0])),
        Problem("n1", Scene(2, 1, [1], steps=[2.0], mp_share=0.0, neigh_mp_share=0.0, nl_cur=1, nl_neigh=[2])),
        Problem("no_neigh", Scene(3, 65, [])),
        Problem("n65", Scene(4, 65, [65, 65, 65], steps=[1.5, 0.6, 4.0], nl_cur=2, nl_neigh=[2, 80, 1])),
        Problem("n300", s300),
        Problem("n300_rev", s300, reverse=True),
        Problem("bignode", Scene(5, 300, [300], steps=[3.0], big_node=120, mp_share=0.2, neigh_mp_share=0.2)),
        Problem("forward", Scene(6, 300, [300, 300, 300], steps=[4.0, 3.0, 9.0], forward=True, mp_share=0.3, nl_cur=256, nl_neigh=[256, 80, 200])),
        Problem("mixed", Scene(7, 300, [200, 65, 0, 1], steps=[2.0, 3.0, 2.0, 5.0], nl_cur=80, nl_neigh=[80, 0, 80, 40])),
        Problem("clones", Scene(9, 65, [65, 65], steps=[3.0, 5.0], noise=False, clones=7)),
        Problem("n2048", Scene(8, 2048, [2048, 2048], steps=[0.7, 3.0], nodes_per=16, nl_cur=80)),
    ]
    out.append(planted())
    return {p.name: p for p in out}


def _project(T, X):
    """pixel of world point X by pose T, also for a point behind the camera"""
    Xc = T[:3, :3].astype(np.float64) @ X + T[:3, 3].astype(np.float64)
    return CAM["fx"] * Xc[0] / Xc[2] + CAM["cx"], CAM["fy"] * Xc[1] / Xc[2] + CAM["cy"]


def _planted_keyframe(kid, T, feats, segs, mp=()):
    """feats: (u, v, node, descriptor byte) mono features without map points; mp:
    world points held by extra features; segs: (S, E, descriptor byte)"""
    n = len(feats) + len(mp)
    kun = np.zeros(n, KP_DTYPE)
    node = np.full(n, -1, np.int32)
    desc = np.zeros((n, 32), np.uint8)
    has_mp = np.zeros(n, np.uint8)
    mpx = np.zeros((n, 3), np.float32)
    for i, (u, v, nd, b) in enumerate(feats):
        kun["x"][i], kun["y"][i], node[i], desc[i] = u, v, nd, b
    for j, X in enumerate(mp):
        i = len(feats) + j
        kun["x"][i], kun["y"][i] = _project(T, np.asarray(X, np.float64))
        has_mp[i], mpx[i] = 1, X
    kl = np.zeros(len(segs), KL_DTYPE)
    ld = np.zeros((len(segs), 32), np.uint8)
    lc = np.zeros((len(segs), 3))
    for i, (S, E, b) in enumerate(segs):
        a = np.float32(_project(T, np.asarray(S, np.float64)))
        e = np.float32(_project(T, np.asarray(E, np.float64)))
        kl["startPointX"][i], kl["startPointY"][i], kl["endPointX"][i], kl["endPointY"][i] = *a, *e
        l = np.cross([float(a[0]), float(a[1]), 1.0], [float(e[0]), float(e[1]), 1.0])
        lc[i] = l / np.hypot(l[0], l[1])
        ld[i] = b
    full = np.full(n, -1.0, np.float32)
    return ref.KeyFrame(kid, T, kun.copy(), kun, full, full.copy(), desc, node, has_mp, mpx, kl, ld, lc)


@functools.lru_cache(maxsize=None)
def planted():
    """The branches a random scene does not reach, built by hand (exact
    geometry, no noise). Neighbour 0 is 0.3 m ahead: a KF2 feature three pixels
    from the epipole (the epipole test rejects it), and a point 0.15 m in front
    of KF1, which is behind KF2 (z2 <= 0). Neighbour 1 looks along the world's x
    axis from (0, 0, 3): one segment crosses its image plane (the end point is
    behind it), one lies wholly behind it (the start point is), one is in front
    of both; its one map point gives the median depth 3."""
    T1 = np.eye(4, dtype=np.float32)
    T2 = np.eye(4, dtype=np.float32)
    T2[:3, 3] = [0.0, 0.0, -0.3]                       # centre (0, 0, 0.3)
    T3 = np.zeros((4, 4), np.float32)
    T3[:3, :3] = [[0, 0, -1], [0, 1, 0], [1, 0, 0]]    # z axis = world x
    T3[:3, 3] = -T3[:3, :3] @ np.array([0.0, 0.0, 3.0], np.float32)
    T3[3, 3] = 1
    ex, ey = _project(T2, np.zeros(3))
    near = np.array([0.05, 0.03, 0.15])
    segs = [([0.5, 0.2, 4.0], [-0.5, 0.3, 4.0], 0x11),        # ends behind neighbour 1
            ([-0.5, 0.2, 4.2], [-0.9, 0.1, 4.4], 0x2e),       # starts behind it
            ([0.9, -0.2, 4.0], [0.6, -0.3, 4.3], 0xc7)]       # in front of both
    cur = _planted_keyframe(50, T1, [(400.0, 300.0, 11, 0x5a), (*_project(T1, near), 12, 0xa5)], segs)
    n0 = _planted_keyframe(40, T2, [(ex + 3.0, ey + 2.0, 11, 0x5a), (*_project(T2, near), 12, 0xa5)], [])
    n1 = _planted_keyframe(60, T3, [], segs, mp=[[3.0, 0.1, 3.0]])
    p = Problem.__new__(Problem)
    p.name, p.cam, p.cur, p.neigh, p.scene = "planted", camera(), cur, [n0, n1], None
    return p


def as_dict(kf):
    """a restatement keyframe as the Python mirror takes it"""
    return dict(id=kf.id, Tcw=kf.Tcw, kps=kf.kps, kps_un=kf.kps_un, uright=kf.uright,
                depth=kf.depth, desc=kf.desc, feat_node=kf.feat_node, has_mp=kf.has_mp,
                mp_xyz=kf.mp_xyz, klines=kf.klines, ldesc=kf.ldesc, lcoef=kf.lcoef)


def kernel_problem(p):
    return dict(cur=as_dict(p.cur), neigh=[as_dict(k) for k in p.neigh])


@functools.lru_cache(maxsize=None)
def noise_free():
    """exact projections, equal descriptors, baselines from just over mb: what the
    restatement creates is measured against the scene's own points"""
    return Problem("noise_free", Scene(21, 300, [300] * 4, steps=[1.05, 2.0, 4.0, 8.0], noise=False,
                                       mp_share=0.2, neigh_mp_share=0.2, nl_cur=80))


@functools.lru_cache(maxsize=None)
def ref_run(name):
    p = problems()[name]
    return ref.create_new_map_features(p.cam, p.cur, p.neigh)

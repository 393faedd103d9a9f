"""Seeded synthetic inputs for the Tracking::Relocalization tests, in the style
of _pnp_problems.make_problem: world points in front of the lost frame's true
pose, keyframe features and frame keypoints as their projections, descriptors
a few bits apart, vocabulary node ids as the BoW test's stand-in. The branches
of the function are planted by construction (three come from bounded seed
searches over a generator built for them: ROUND2_SEED, MANY_ROUNDS_SEED,
SECOND_SEED), out of these kinds of feature:

  bow       a feature with the same node id on both sides: SearchByBoW finds it
  proj      a feature with different node ids on the two sides: only
            SearchByProjection can find it
  decoy     a keyframe point whose own keypoint is missing, with a keypoint of
            its descriptor 6 px from its projection: inside the 10 px window,
            outside the chi2 radius
  garbage   a BoW match whose map point lies somewhere else
  hidden    a bow feature whose keypoint octave is far from the level the map
            point predicts, so that no projection search can re-find it

Inputs and planted answers only: the expected results come from
tests/_relocalize_ref.py."""
import functools

import numpy as np

from _reloc_problems import KP

CFG = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0,
           bf=40.0, thdepth=40.0, width=640, height=480)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SCALE = (1.2 ** np.arange(8)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)
RAND_MAX = 2147483647
Q_WORDS = np.arange(10, 30, dtype=np.uint32)          # the lost frame's BowVector
OTHER_WORDS = np.arange(100, 120, dtype=np.uint32)    # a place the frame does not see


def _unit(words):
    return np.array(words, np.uint32), np.full(len(words), 1.0 / len(words))


class Builder:
    def __init__(self, seed, draw_pitch=1280):
        self.rng = rng = np.random.default_rng(seed)
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = rng.uniform(-0.4, 0.4)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        self.R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        self.t = rng.uniform(-1.0, 1.0, 3)
        self.kps, self.desc, self.node, self.uright = [], [], [], []
        self.kfs, self.bows = [], []
        self.next_node = 1000
        self.draw_pitch = draw_pitch
        self.used = []                                     # keypoint positions taken
        self.spacing = 14.0                                # px between any two of them

    # -- helpers --
    def _pixel(self, region):
        x0, x1, y0, y1 = region
        for _ in range(1000):
            u, v = self.rng.uniform(x0, x1), self.rng.uniform(y0, y1)
            if all(abs(u - a) > self.spacing or abs(v - b) > self.spacing for a, b in self.used):
                self.used.append((u, v))
                return u, v
        raise RuntimeError("region too crowded")

    def _world(self, u, v):
        z = self.rng.uniform(1.0, 4.0)
        Xc = np.array([(u - CFG["cx"]) / CFG["fx"] * z, (v - CFG["cy"]) / CFG["fy"] * z, z])
        return (Xc - self.t) @ self.R, float(np.linalg.norm(Xc))

    def _node(self):
        self.next_node += 1
        return self.next_node

    def _near(self, d, bits):
        d = d.copy()
        for b in self.rng.choice(256, bits, replace=False):
            d[b // 8] ^= 1 << (b % 8)
        return d

    def _keypoint(self, u, v, octave, angle, desc, node, uright=-1.0):
        self.kps.append((u, v, 31.0, angle % 360.0, 1.0, octave, -1))
        self.desc.append(desc)
        self.node.append(node)
        self.uright.append(uright)

    # -- one database keyframe --
    def keyframe(self, bow=0, proj=0, decoy=0, garbage=0, hidden=0, noise=0.0, bad_uright=0,
                 region=(30, 610, 30, 450), proj_region=None, octaves=(0, 1, 2), proj_octaves=None,
                 candidate=True):
        rng = self.rng
        f = dict(angle=[], feat_node=[], desc=[], valid=[], mp_xyz=[], mp_min_dist=[],
                 mp_max_dist=[], mp_desc=[])
        rot = rng.uniform(0, 360)

        def feature(Xw, dist, level, angle, desc, node):
            f["angle"].append(angle)
            f["feat_node"].append(node)
            f["desc"].append(desc)
            f["valid"].append(1)
            f["mp_xyz"].append(Xw)
            mx = dist * float(SCALE[level])
            f["mp_max_dist"].append(mx)
            f["mp_min_dist"].append(mx / float(SCALE[-1]))
            f["mp_desc"].append(desc)

        kinds = (["bow"] * bow + ["hidden"] * hidden + ["garbage"] * garbage + ["proj"] * proj +
                 ["decoy"] * decoy)
        n_bad = 0
        for kind in kinds:
            reg = proj_region if (kind in ("proj", "decoy") and proj_region) else region
            u, v = self._pixel(reg)
            Xw, dist = self._world(u, v)
            o = int(rng.choice(proj_octaves if (kind in ("proj", "decoy") and proj_octaves)
                               else octaves))
            a = float(rng.uniform(0, 360))
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            n1 = self._node()
            if kind == "garbage":
                Xw, dist = self._world(rng.uniform(30, 610), rng.uniform(30, 450))
            if kind == "hidden":
                feature(Xw, dist, 0, a, d, n1)
                o = 5
            else:
                feature(Xw, dist, o, a, d, n1)
            if kind == "decoy":
                th = rng.uniform(0, 2 * np.pi)
                u, v = u + 6.0 * np.cos(th), v + 6.0 * np.sin(th)
            if noise and kind in ("bow", "hidden"):
                th, r = rng.uniform(0, 2 * np.pi), rng.uniform(0, noise) * float(SCALE[o])
                u, v = u + r * np.cos(th), v + r * np.sin(th)
            ur = -1.0
            if kind == "bow" and n_bad < bad_uright:
                n_bad += 1
                ur = float(u - rng.uniform(25, 60))
            fnode = n1 if kind in ("bow", "hidden", "garbage") else self._node()
            self._keypoint(u, v, 0 if kind == "decoy" else o, a + rot, self._near(d, 3), fnode, ur)
            if kind == "decoy":        # its map point predicts level 0
                f["mp_max_dist"][-1] = dist
                f["mp_min_dist"][-1] = dist / float(SCALE[-1])
        kf = dict(angle=np.array(f["angle"], np.float32), feat_node=np.array(f["feat_node"], np.int32),
                  desc=np.array(f["desc"], np.uint8).reshape(-1, 32),
                  valid=np.array(f["valid"], np.uint8),
                  mp_xyz=np.array(f["mp_xyz"], np.float32).reshape(-1, 3),
                  mp_min_dist=np.array(f["mp_min_dist"], np.float32),
                  mp_max_dist=np.array(f["mp_max_dist"], np.float32),
                  mp_desc=np.array(f["mp_desc"], np.uint8).reshape(-1, 32))
        self.kfs.append(kf)
        self.bows.append(_unit(Q_WORDS if candidate else OTHER_WORDS))
        return kf

    def clutter(self, n):
        """keypoints that belong to no keyframe (no node id), first in the frame"""
        rng = self.rng
        pad = [(rng.uniform(0, 640), rng.uniform(0, 480), 31.0, rng.uniform(0, 360), 1.0,
                int(rng.integers(0, 8)), -1) for _ in range(n)]
        self.kps = pad + self.kps
        self.desc = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(n)] + self.desc
        self.node = [-1] * n + self.node
        self.uright = [-1.0] * n + self.uright

    def problem(self, name, streams=None, **expect):
        nkf = len(self.kfs)
        ns = nkf if streams is None else streams
        frame = dict(kps_un=np.array(self.kps, KP), uright=np.array(self.uright, np.float32),
                     desc=np.array(self.desc, np.uint8).reshape(-1, 32),
                     feat_node=np.array(self.node, np.int32), bow_words=_unit(Q_WORDS)[0],
                     bow_vals=_unit(Q_WORDS)[1])
        draws = self.rng.integers(0, RAND_MAX + 1, (ns, self.draw_pitch),
                                  dtype=np.int64).astype(np.int32)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = self.R, self.t
        return dict(name=name, kf_bows=self.bows, covis=[[] for _ in range(nkf)],
                    reloc_score=np.zeros(nkf, np.float32), kfs=self.kfs, frame=frame, draws=draws,
                    draw_pitch=self.draw_pitch, kp_pitch=1024 if len(self.kps) <= 1024 else 2048,
                    cfg=CFG, bounds=BOUNDS, Tcw_true=T, expect=expect)


# seeds are constants; tests/test_relocalize_ref.py checks each problem against
# its planted branches and for clean _pnp_ref.Margins
def _no_candidates():
    b = Builder(101)
    b.keyframe(bow=40, candidate=False)
    b.keyframe(bow=40, candidate=False)
    return b.problem("no_candidates", ok=False, branches=("no_candidates",))


def _under_15():
    b = Builder(102)
    b.keyframe(bow=10)
    b.keyframe(bow=14)
    return b.problem("under_15", ok=False, branches=("all_under_15",))


def _direct():
    b = Builder(103)
    b.keyframe(bow=80)
    return b.problem("direct", ok=True, winner=0, n_good=80, branches=("direct",))


def _first_search():
    b = Builder(104)
    b.keyframe(bow=30, proj=40)
    return b.problem("first_search", ok=True, winner=0, n_good=70,
                     branches=("first_search_success",))


def _second_entry():
    """35 BoW inliers and 20 decoys: the first search takes the decoys (55 >=
    50), the second pose throws them out (30 < 35 < 50), the second search
    finds nothing, and the solver, never out of inliers, is never discarded:
    the call ends when its 160 draws run out (P31)"""
    b = Builder(105, draw_pitch=160)
    b.keyframe(bow=35, decoy=20, octaves=(0,))
    return b.problem("second_entry", ok=False, branches=("second_search_entry", "draw_exhausted"))


def _fail_then_win():
    b = Builder(106)
    b.keyframe(garbage=24)
    b.keyframe(bow=60)
    return b.problem("fail_then_win", ok=True, winner=1, n_good=60,
                     branches=("fail_then_later_wins", "exhaust_without_pose"))


def _two_win():
    b = Builder(107)
    b.keyframe(bow=60)
    b.keyframe(bow=55)
    return b.problem("two_win", ok=True, winner=0, n_good=60, branches=("direct",))


def _exhaust():
    """every candidate runs out of iterations: one without a pose (garbage
    only), one with mBestTcw (10 consistent of 20: Refine's strict > never
    passes)"""
    b = Builder(108)
    b.keyframe(garbage=20)
    b.keyframe(bow=10, garbage=10)
    return b.problem("exhaust", ok=False,
                     branches=("exhaust_without_pose", "exhaust_with_pose", "failed"))


def _ngood_lt10():
    """16 BoW inliers of which 11 carry a stereo coordinate 25-60 px off: the
    solver keeps all 16, the optimiser's stereo edges throw them out; the
    second keyframe wins in the same round"""
    b = Builder(109)
    b.keyframe(bow=16, bad_uright=11)
    b.keyframe(bow=60)
    return b.problem("ngood_lt10", ok=True, winner=1, n_good=60,
                     branches=("ngood_lt10", "fail_then_later_wins"))


# Found by a bounded search over seeds 0..39 of this generator (the only
# branches that are not planted by construction): seed 26 fails in rounds 1-3
# and wins in round 4 with 51 inliers, seed 12 keeps a pose for 10 rounds and
# is then discarded. Seeds whose Margins report a fragile count were passed over.
ROUND2_SEED = 26
MANY_ROUNDS_SEED = 12


def _noisy(name, seed, **expect):
    """56 BoW matches up to 2.7 sigma off that no projection search can
    re-find, and 10 garbage ones: a win needs 50 optimiser inliers, which the
    first refined hypothesis does not give and a later, larger consensus set
    may"""
    b = Builder(200 + seed)
    b.keyframe(hidden=56, garbage=10, noise=2.7)
    return b.problem(name, **expect)


def _round2():
    return _noisy("round2", ROUND2_SEED, ok=True, winner=0, branches=("win_round_ge2",))


def _many_rounds():
    return _noisy("many_rounds", MANY_ROUNDS_SEED, ok=False,
                  branches=("exhaust_with_pose", "failed"))


SECOND_SEED = 16    # of seeds 0..59: 6 win through the second search, this one with the widest margins


def _second_success():
    """the second projection search saves the day: 20 coarse-octave BoW
    matches up to 2.2 sigma off, clustered in one image corner, so the first
    pose is many pixels off on the far side; 36 level-0 points there that
    only projection finds, and 8 decoys. The 10 px search reaches some of the
    far points and the decoys (>= 50 together), the second pose drops the
    decoys (30 < nGood < 50) and is good enough for the 3 px search to find
    the rest"""
    b = Builder(300 + SECOND_SEED)
    b.spacing = 6.0
    b.keyframe(bow=20, proj=36, decoy=8, noise=2.2, octaves=(7,), proj_octaves=(0,),
               region=(30, 130, 30, 110), proj_region=(150, 610, 30, 450))
    return b.problem("second_success", ok=True, winner=0,
                     branches=("second_search_entry", "second_search_success"))


def _four():
    """four candidates: garbage (out of iterations without a pose), 10
    consistent of 20 (out of iterations with mBestTcw), the winner, and one
    that would win too; a fifth keyframe of the database sees another place"""
    b = Builder(112)
    b.spacing = 9.0
    b.keyframe(garbage=24)
    b.keyframe(bow=10, garbage=10)
    b.keyframe(bow=30, proj=40)
    b.keyframe(bow=55)
    b.keyframe(bow=40, candidate=False)
    return b.problem("four", ok=True, winner=2, n_good=70,
                     branches=("exhaust_without_pose", "exhaust_with_pose",
                               "first_search_success", "fail_then_later_wins"))


def _wide():
    """the first-search problem behind 1020 clutter keypoints: 1090 keypoints,
    the 2048 build of every kernel"""
    b = Builder(110)
    b.keyframe(bow=30, proj=40)
    b.clutter(1020)
    return b.problem("wide", ok=True, winner=0, n_good=70, branches=("first_search_success",))


def _no_stream():
    """two candidates, one draw stream: the second is out of draws at once"""
    b = Builder(111)
    b.keyframe(garbage=24)
    b.keyframe(bow=60)
    return b.problem("no_stream", streams=1, ok=False, branches=("draw_exhausted",))


IMAGE_LEVELSUP = 4


def image_vocabulary():
    """the seeded synthetic vocabulary tests/test_gpu_bow.py uses (path; cached per process)"""
    from _vocab import vocabulary
    return vocabulary(k=10, L=5, seed=3, n_frames=8)[0]


def _image():
    """image-derived: frames 0 and 1 of a rendered TUM1 sequence (distorted
    camera, depth) are the database's keyframes, with map points from their
    depth; frame 2 is the lost frame. Descriptors, node ids and BowVectors
    come from the extractor and the synthetic vocabulary; keyframe 1 is
    listed as keyframe 0's covisible."""
    from _pkg import load_oracle
    from _reloc_problems import _kf_from_frame
    from _scenes import frame_data, sequence
    O = load_oracle()
    cfg, traj, frames = sequence(3, 11)
    cam = O.camera(cfg)
    sc = np.asarray(O.level_sizes(O.params(), 640, 480)[3], np.float32)
    voc = O.Vocabulary(image_vocabulary())
    rng = np.random.default_rng(77)
    fds = [frame_data(O, cam, cfg, *f) for f in frames]
    kfs, bows = [], []
    for k in (0, 1):
        Tcw = np.linalg.inv(traj[k]).astype(np.float32)
        kf = _kf_from_frame(cfg, sc, fds[k], Tcw, traj[k], rng, 0.0)
        w, v, node = voc.transform(fds[k]["desc"], IMAGE_LEVELSUP)[:3]
        kf.update(feat_node=node, desc=fds[k]["desc"].copy())
        del kf["found"]
        kfs.append(kf)
        bows.append((w, v))
    w, v, node = voc.transform(fds[2]["desc"], IMAGE_LEVELSUP)[:3]
    frame = dict(kps_un=fds[2]["kps_un"], uright=fds[2]["uright"], desc=fds[2]["desc"],
                 feat_node=node, bow_words=w, bow_vals=v)
    draws = rng.integers(0, RAND_MAX + 1, (2, 1280), dtype=np.int64).astype(np.int32)
    return dict(name="image", kf_bows=bows, covis=[[1], [0]], reloc_score=np.zeros(2, np.float32),
                kfs=kfs, frame=frame, draws=draws, draw_pitch=1280, kp_pitch=1024, cfg=cfg,
                bounds=tuple(float(b) for b in fds[2]["bounds"]),
                Tcw_true=np.linalg.inv(traj[2]), expect=dict(ok=True, winner=0, branches=()))


@functools.lru_cache(maxsize=1)
def problems():
    ps = [_no_candidates(), _under_15(), _direct(), _first_search(), _second_entry(),
          _fail_then_win(), _two_win(), _exhaust(), _ngood_lt10(), _round2(), _many_rounds(), _wide(),
          _no_stream(), _second_success(), _four(), _image()]
    return {p["name"]: p for p in ps}


REQUIRED_BRANCHES = ("no_candidates", "all_under_15", "direct", "first_search_success",
                     "second_search_entry", "second_search_success", "fail_then_later_wins", "exhaust_with_pose",
                     "exhaust_without_pose", "failed", "win_round_ge2", "ngood_lt10",
                     "draw_exhausted")

_REF = {}


def ref_run(name):
    """the restatement's result for a problem, computed once and shared"""
    if name not in _REF:
        import _relocalize_ref as R
        P = problems()[name]
        _REF[name] = R.relocalize(P, P["cfg"], P["bounds"], SCALE, SIGMA2)
    return _REF[name]

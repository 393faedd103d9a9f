"""Seeded inputs for the relocalisation tests (keyframe databases, queries and
projection-matcher problems). Inputs only: the expected results come from
tests/_reloc_ref.py."""
import functools

import numpy as np

from _pkg import load_oracle
from _scenes import frame_data, perturb, sequence, unproject

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
               ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def unit_bow(words, rng=None):
    """a BowVector over `words` (ascending) with L1 norm 1"""
    w = np.array(sorted(words), np.uint32)
    v = np.ones(len(w)) if rng is None else rng.random(len(w)) + 0.05
    return w, v / v.sum()


@functools.lru_cache(maxsize=1)
def random_db_batch(seed=3, nq=200):
    """200 (database, query) problems: 1..64 keyframes, words from 0..999, 20 to
    600 entries per vector. A problem's keyframes are views of a few places (a
    place = a word set), the query is a view of one of them, so that several
    keyframes pass the common-word threshold and covisible groups overlap."""
    rng = np.random.default_rng(seed)
    problems = []
    for _ in range(nq):
        nkf = int(rng.integers(1, 65))
        size = int(rng.integers(20, 601))
        nplaces = int(rng.integers(1, 5))
        places = [rng.choice(1000, size, replace=False) for _ in range(nplaces)]

        def view(place):
            keep = int(rng.integers(max(20, int(0.85 * size)), size + 1))
            w = rng.choice(places[place], keep, replace=False)
            extra = min(600 - keep, int(rng.integers(0, 1 + size // 10)))
            w = np.union1d(w, rng.choice(1000, extra, replace=False))[:600]
            return unit_bow(w, rng)

        place_of = rng.integers(0, nplaces, nkf)
        kf_bows = [view(p) for p in place_of]
        covis = []
        for k in range(nkf):
            same = [j for j in range(nkf) if j != k and place_of[j] == place_of[k]]
            rng.shuffle(same)
            c = same[:int(rng.integers(0, 11))]
            if c and rng.random() < 0.3:
                c[int(rng.integers(0, len(c)))] = -1      # a neighbour not in the database
            if rng.random() < 0.3 and nkf > 1:
                c = (c + [int(rng.integers(0, nkf))])[:10]
            covis.append(c)
        q = view(int(rng.integers(0, nplaces))) if rng.random() < 0.9 else \
            unit_bow(rng.choice(1000, 20, replace=False), rng)
        score = (rng.random(nkf) * 0.05).astype(np.float32)    # kept from earlier queries
        problems.append(dict(kf_bows=kf_bows, covis=covis, reloc_score=score, q_words=q[0],
                             q_vals=q[1]))
    return problems


def _kf_from_frame(cfg, sc, fd, Tcw, Twc, rng, found_frac):
    """map points of a keyframe from its depth: world position, the distances
    MapPoint::UpdateNormalAndDepth sets from the observation level, the
    keypoint's descriptor"""
    ok = fd["depth"] > 0
    xyz = unproject(cfg, fd["kps_un"], np.where(ok, fd["depth"], 1.0), Tcw)
    d = np.linalg.norm(xyz.astype(np.float64) - Twc[:3, 3], axis=1)
    mx = (d * sc[fd["kps_un"]["octave"]]).astype(np.float32)
    return dict(angle=fd["kps_un"]["angle"].copy(), valid=ok.astype(np.uint8),
                found=(rng.random(len(ok)) < found_frac).astype(np.uint8), mp_xyz=xyz,
                mp_min_dist=(mx / sc[-1]).astype(np.float32), mp_max_dist=mx,
                mp_desc=fd["desc"].copy())


@functools.lru_cache(maxsize=1)
def sequence_problem(seed=0):
    """keyframe = frame 0 of a seeded 640x480 sequence with map points from its
    depth; current frame = frame 2, its true pose moved by a few centimetres;
    some keypoints hold a map point on entry, some keyframe points are found"""
    O = load_oracle()
    cfg, traj, frames = sequence(3, seed)
    cam = O.camera(cfg)
    sc = O.level_sizes(O.params(), 640, 480)[3]
    f0 = frame_data(O, cam, cfg, *frames[0])
    f2 = frame_data(O, cam, cfg, *frames[2])
    rng = np.random.default_rng(seed + 21)
    T0 = np.linalg.inv(traj[0]).astype(np.float32)
    T2 = np.linalg.inv(traj[2]).astype(np.float32)
    kf = _kf_from_frame(cfg, sc, f0, T0, traj[0], rng, 0.1)
    cur = dict(Tcw=perturb(T2, 0.02, 0.005, seed=seed), kps_un=f2["kps_un"], desc=f2["desc"])
    has = (rng.random(len(f2["kps_un"])) < 0.15).astype(np.uint8)
    return dict(cam_cfg=cfg, bounds=f2["bounds"], scale=sc, cur=cur, cur_has_mp=has, kf=kf)


_CFG = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0,
            bf=40.0, thdepth=40.0, width=640, height=480)
_SCALE = (1.2 ** np.arange(8)).astype(np.float32)


@functools.lru_cache(maxsize=1)
def conflict_problem():
    """128 keyframe points at one world position with one descriptor; 40
    keypoints inside the window (and 20 outside), with few distinct
    distances so that ties are broken by scan order: every point wants the
    same keypoint as the one before it"""
    rng = np.random.default_rng(17)
    n = 60
    kps = np.zeros(n, KP)
    kps["x"][:40] = 320 + rng.uniform(-9, 9, 40)
    kps["y"][:40] = 240 + rng.uniform(-9, 9, 40)
    kps["x"][40:] = rng.uniform(20, 200, 20)
    kps["y"][40:] = rng.uniform(20, 200, 20)
    kps["angle"] = rng.uniform(0, 360, n)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.tile(base, (n, 1))
    for i in range(n):                    # 0..5 bits away from the points' descriptor
        for b in rng.choice(256, int(rng.integers(0, 6)), replace=False):
            desc[i, b // 8] ^= 1 << (b % 8)
    nk = 128
    kf = dict(angle=rng.uniform(0, 360, nk).astype(np.float32), valid=np.ones(nk, np.uint8),
              found=np.zeros(nk, np.uint8),
              mp_xyz=np.tile(np.array([0, 0, 2], np.float32), (nk, 1)),
              mp_min_dist=np.full(nk, 1.0, np.float32), mp_max_dist=np.full(nk, 2.0, np.float32),
              mp_desc=np.tile(base, (nk, 1)))
    cur = dict(Tcw=np.eye(4, dtype=np.float32), kps_un=kps, desc=desc)
    return dict(cam_cfg=_CFG, bounds=(0, 640, 0, 480), scale=_SCALE, cur=cur,
                cur_has_mp=np.zeros(n, np.uint8), kf=kf, expect_claims=40)


@functools.lru_cache(maxsize=1)
def wide_pitch_problem(seed=31):
    """conflict_problem() behind 1030 padding keypoints (1090 keypoints, 128
    keyframe points): more than 1024 keypoints, so the 2048-keypoint build of
    the matcher runs and every match lies at an index >= 1030. The padding is
    spread over the image but kept out of the +-40 px box around the points'
    projection (320, 240), with random octaves, angles and descriptors"""
    P = conflict_problem()
    rng = np.random.default_rng(seed)
    npad = 1030
    pad = np.zeros(npad, KP)
    pad["x"] = rng.uniform(0, 640, npad)
    pad["y"] = rng.uniform(0, 480, npad)
    box = (np.abs(pad["x"] - 320) < 40) & (np.abs(pad["y"] - 240) < 40)
    pad["x"][box] += np.where(pad["x"][box] < 320, -80, 80)
    pad["angle"] = rng.uniform(0, 360, npad)
    pad["octave"] = rng.integers(0, 8, npad)
    pdesc = rng.integers(0, 256, (npad, 32), dtype=np.uint8)
    cur = dict(Tcw=P["cur"]["Tcw"], kps_un=np.concatenate([pad, P["cur"]["kps_un"]]),
               desc=np.concatenate([pdesc, P["cur"]["desc"]]))
    return dict(P, cur=cur, cur_has_mp=np.zeros(len(cur["kps_un"]), np.uint8), npad=npad)


@functools.lru_cache(maxsize=1)
def level_edge_problem():
    """points whose predicted level is 0 (mfMaxDistance below the distance) and
    nlevels - 1 (far above it), each with keypoints of every octave around its
    projection: only octaves {0, 1} / {6, 7} may be taken"""
    rng = np.random.default_rng(23)
    pts, mx = [], []
    for k in range(12):
        x, y, z = rng.uniform(-1, 1), rng.uniform(-0.7, 0.7), rng.uniform(2, 4)
        pts.append((x, y, z))
        d = np.sqrt(x * x + y * y + z * z)
        mx.append(d * (0.9 if k % 2 == 0 else 50.0))
    pts = np.array(pts, np.float32)
    nk = len(pts)
    mpd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    kps, desc = [], []
    for k, (x, y, z) in enumerate(pts):
        u, v = 500 * x / z + 320, 500 * y / z + 240
        for octave in range(8):
            kps.append((u + rng.uniform(-2, 2), v + rng.uniform(-2, 2), 31.0, rng.uniform(0, 360),
                        1.0, octave, -1))
            d = mpd[k].copy()
            d[octave] ^= 0xFF >> (octave % 4)       # octave-dependent distance
            desc.append(d)
    kps = np.array(kps, KP)
    kf = dict(angle=rng.uniform(0, 360, nk).astype(np.float32), valid=np.ones(nk, np.uint8),
              found=np.zeros(nk, np.uint8), mp_xyz=pts,
              mp_min_dist=np.full(nk, 0.1, np.float32), mp_max_dist=np.array(mx, np.float32),
              mp_desc=mpd)
    cur = dict(Tcw=np.eye(4, dtype=np.float32), kps_un=kps, desc=np.array(desc, np.uint8))
    return dict(cam_cfg=_CFG, bounds=(0, 640, 0, 480), scale=_SCALE, cur=cur,
                cur_has_mp=np.zeros(len(kps), np.uint8), kf=kf)

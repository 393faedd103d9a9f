"""Seeded synthetic keyframe pairs for the Sim3Solver tests: TUM1 intrinsics,
points 2-8 m in front of keyframe 1, a ground-truth Sim3 (s12, R12, t12) with
X1 = s12 R12 X2 + t12 that keeps them in front of keyframe 2, inlier noise of
at most `noise` pixels on keyframe 2's side (the solver projects the 3-D
points themselves, so the noise is applied to the point), outliers replaced by
unrelated points, octaves from the 8-level 1.2 pyramid. Keyframe 2 lives in a
map of its own (its world differs from keyframe 1's by the Sim3, as after
drift). Every problem is a dict(pair, fix_scale, min_inliers, s12, R12, t12,
draws, name); draws are raw rand() values in [0, RAND_MAX]."""
import numpy as np

RAND_MAX = 2147483647
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float32)
N_DRAWS = 3 * 320
F = np.float32


def _rot(rng, amax):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(-amax, amax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _pose(rng):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rot(rng, 0.6), rng.uniform(-1.0, 1.0, 3)
    return T


def default_min_inliers(N):
    """ComputeSim3 uses 20; small problems use half their points, at least 3"""
    return 20 if N > 40 else max(3, N // 2)


def make_problem(N, outlier_share=0.0, fix_scale=False, noise=0.5, seed=0, n_outliers=None,
                 extras=True, min_inliers=None, name=None):
    """N accepted correspondences; with extras, keyframe 1 also has features of
    every skipped kind and keyframe 2 some unmatched ones"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = TUM1
    s12 = 1.0 if fix_scale else rng.uniform(0.8, 1.25)
    R12, t12 = _rot(rng, 0.25), rng.uniform(-0.3, 0.3, 3)
    u = rng.uniform(60, 580, N)
    v = rng.uniform(60, 420, N)
    z = rng.uniform(2.0, 8.0, N)
    Xc1 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    Xc2 = (Xc1 - t12) @ R12 / s12                     # R12^T (X1 - t12) / s12
    ang = rng.uniform(0, 2 * np.pi, N)
    rad = rng.uniform(0, noise, N)
    Xc2[:, 0] += rad * np.cos(ang) / fx * Xc2[:, 2]
    Xc2[:, 1] += rad * np.sin(ang) / fy * Xc2[:, 2]
    n_out = int(round(outlier_share * N)) if n_outliers is None else n_outliers
    out = rng.permutation(N)[:n_out]
    zo = rng.uniform(2.0, 8.0, n_out)
    Xc2[out] = np.stack([(rng.uniform(60, 580, n_out) - cx) / fx * zo,
                         (rng.uniform(60, 420, n_out) - cy) / fy * zo, zo], axis=1)
    T1, T2 = _pose(rng), _pose(rng)
    Xw1 = (Xc1 - T1[:3, 3]) @ T1[:3, :3]
    Xw2 = (Xc2 - T2[:3, 3]) @ T2[:3, :3]
    # keyframe 2: the matched points in a shuffled order, then unmatched ones
    n2 = N + (5 if extras else 0)
    perm = rng.permutation(N)
    xyz2 = np.zeros((n2, 3))
    xyz2[perm] = Xw2
    xyz2[N:] = rng.uniform(-3, 3, (n2 - N, 3))
    valid2 = np.ones(n2, np.uint8)
    # keyframe 1: the accepted features with the skipped kinds spread among them
    kinds = ["ok"] * N
    if extras:
        for kind in ("nomatch", "nomatch", "bad1", "bad2", "minus2", "nomatch"):
            kinds.insert(int(rng.integers(0, len(kinds) + 1)), kind)
        valid2[N] = 0                                  # the bad point of keyframe 2
    n1 = len(kinds)
    matched12 = np.full(n1, -1, np.int32)
    valid1 = np.ones(n1, np.uint8)
    xyz1 = rng.uniform(-3, 3, (n1, 3))
    k = 0
    for i, kind in enumerate(kinds):
        if kind == "ok":
            matched12[i] = perm[k]
            xyz1[i] = Xw1[k]
            k += 1
        elif kind == "bad1":
            matched12[i], valid1[i] = N + 1, 0
        elif kind == "bad2":
            matched12[i] = N
        elif kind == "minus2":
            matched12[i] = -2
    is_out = np.zeros(N, bool)
    is_out[out] = True
    pair = dict(matched12=matched12, valid1=valid1, xyz1=xyz1.astype(F),
                octave1=rng.integers(0, 8, n1).astype(np.int32), valid2=valid2,
                xyz2=xyz2.astype(F), octave2=rng.integers(0, 8, n2).astype(np.int32),
                Tcw1=T1.astype(F), Tcw2=T2.astype(F), cam=TUM1)
    return dict(pair=pair, fix_scale=bool(fix_scale), N=N, outlier=is_out,
                min_inliers=default_min_inliers(N) if min_inliers is None else min_inliers,
                s12=s12, R12=R12, t12=t12,
                draws=rng.integers(0, RAND_MAX + 1, N_DRAWS, dtype=np.int64).astype(np.int32),
                name=name or f"N{N}_o{n_out}_{'fix' if fix_scale else 'free'}_s{seed}")


def direct_problem(X1, X2, octaves1=None, octaves2=None, fix_scale=False, min_inliers=3,
                   seed=0, draws=None, name="direct"):
    """a pair whose compacted correspondences are exactly X1 / X2 (camera
    coordinates): identity poses, feature i matched to point i"""
    X1 = np.asarray(X1, F).reshape(-1, 3)
    X2 = np.asarray(X2, F).reshape(-1, 3)
    n = len(X1)
    rng = np.random.default_rng(seed)
    o1 = np.zeros(n, np.int32) if octaves1 is None else np.asarray(octaves1, np.int32)
    o2 = np.zeros(n, np.int32) if octaves2 is None else np.asarray(octaves2, np.int32)
    pair = dict(matched12=np.arange(n, dtype=np.int32), valid1=np.ones(n, np.uint8), xyz1=X1,
                octave1=o1, valid2=np.ones(n, np.uint8), xyz2=X2, octave2=o2,
                Tcw1=np.eye(4, dtype=F), Tcw2=np.eye(4, dtype=F), cam=TUM1)
    if draws is None:
        draws = rng.integers(0, RAND_MAX + 1, N_DRAWS, dtype=np.int64).astype(np.int32)
    return dict(pair=pair, fix_scale=fix_scale, N=n, min_inliers=min_inliers,
                draws=np.asarray(draws, np.int32), name=name)


def _grid_points(n, seed):
    """camera points whose coordinates are multiples of 3/8: the sum of any
    three is a multiple of 3/8 and the centroid (sum / 3) is exact"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-4, 5, n), rng.integers(-3, 4, n), rng.integers(8, 17, n)],
                    axis=1) * 0.375


def _rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def pure_translation(n=12, seed=3):
    """X1 = X2 + t in exact floats with exact centroids: Pr1 == Pr2, M is
    exactly symmetric, the quaternion is (1, 0, 0, 0) and norm(vec) == 0 makes
    T12 not a number"""
    X2 = _grid_points(n, seed)
    return direct_problem(X2 + np.array([0.25, -0.125, 0.5]), X2, min_inliers=3, seed=seed,
                          name="pure_translation")


def identical_points(n=10, seed=4):
    X = np.tile(np.array([[0.25, -0.5, 4.0]]), (n, 1))
    return direct_problem(X, X, min_inliers=3, seed=seed, name="identical_points")


def collinear_points(n=10, seed=5):
    """all points on one line: every sample is collinear, the rotation about
    the line is undetermined"""
    k = np.arange(n)[:, None]
    X2 = np.array([[-1.0, 0.5, 3.0]]) + k * np.array([[0.25, 0.125, 0.25]])
    X1 = X2 @ _rot_z(0.15).T + np.array([0.125, 0.0, 0.25])
    return direct_problem(X1, X2, min_inliers=3, seed=seed, name="collinear_points")


def exactly_min_inliers(seed=13, min_inliers=6):
    """2 x min_inliers points with exactly min_inliers noise-free inliers: the
    strict > never passes"""
    return make_problem(2 * min_inliers, noise=0.0, seed=seed, n_outliers=min_inliers,
                        min_inliers=min_inliers, extras=False, name="exactly_min_inliers")


TRUNCATED_POINT = 3


def truncated_threshold():
    """X1 = Rz X2 + t (a rotation about the optical axis, a translation across
    it, scale 1: both images see the same displacement), all keypoints at
    level 1: 9.21 sigma2 = 13.26 and the stored threshold is 13. Point 3 of
    camera 1 is moved by 3.6235 px (13.13 px^2): inside 9.21 sigma2, outside
    the truncated threshold, so it is an outlier. The draws (all zero) sample
    points 0, 8 and 7."""
    fx = TUM1[0]
    rng = np.random.default_rng(21)
    X2 = np.stack([rng.uniform(-1.5, 1.5, 9), rng.uniform(-1.0, 1.0, 9), rng.uniform(3, 6, 9)],
                  axis=1)
    X1 = X2 @ _rot_z(0.2).T + np.array([0.25, -0.125, 0.0])
    X1[TRUNCATED_POINT, 0] += 3.6235 / fx * X1[TRUNCATED_POINT, 2]
    return direct_problem(X1, X2, octaves1=np.ones(9), octaves2=np.ones(9), min_inliers=3,
                          draws=np.zeros(N_DRAWS, np.int32), seed=21, name="truncated_threshold")


def problems():
    """the driven problems of the GPU comparison (name -> problem)"""
    ps = []
    seed = 100
    for N in (3, 4, 8, 25, 64, 65, 100, 257):
        for share in (0.0, 0.3, 0.6):
            seed += 1
            ps.append(make_problem(N, share, fix_scale=(seed % 2 == 0), seed=seed))
    ps.append(make_problem(100, 0.3, fix_scale=True, seed=131))
    ps.append(make_problem(100, 0.3, fix_scale=False, seed=132))
    ps += [exactly_min_inliers(), pure_translation(), identical_points(), collinear_points(),
           truncated_threshold()]
    return {p["name"]: p for p in ps}


def big_problems():
    """at the 2048 cap, no skipped features"""
    return [make_problem(2048, share, fix_scale=fs, seed=140 + k, extras=False)
            for k, (share, fs) in enumerate(((0.0, False), (0.3, True), (0.6, False)))]


_RUNS = {}


def ref_solver(p):
    import _sim3_ref as ref
    corr = ref.setup(p["pair"], SIGMA2)
    return ref.Sim3Solver(p["pair"]["cam"], corr, p["fix_scale"], 0.99, p["min_inliers"], 300)


def ref_run(p, n_iterations=5, max_calls=80):
    """The restatement driven like LoopClosing::ComputeSim3 drives the solver:
    SetRansacParameters(0.99, min_inliers, 300), then iterate(n_iterations)
    until a Sim3 or bNoMore. Returns dict(solver, calls=[(draw offset, output,
    state after)]); computed once per problem and shared by the tests."""
    key = (p["name"], n_iterations)
    if key in _RUNS:
        return _RUNS[key]
    s = ref_solver(p)
    calls, off = [], 0
    for _ in range(max_calls):
        o = s.iterate(n_iterations, p["draws"][off:])
        calls.append((off, o, s.state()))
        off += o["draws_consumed"]
        if o["result"] or o["no_more"]:
            break
    _RUNS[key] = dict(solver=s, calls=calls)
    return _RUNS[key]


# ---------------------------------------------------------------- SearchBySim3
MATCH_CAM = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0,
                 bf=40.0, th_depth=40.0, width=640, height=480)
SCALE = np.array([1.2 ** l for l in range(8)], np.float32)
TH = 7.5                       # ComputeSim3's SearchBySim3(..., 7.5)
# the hand-made pairs' Sim3: X1 = 2 X2 + (0.5, 0, 0), exact in floats
HAND_S, HAND_R, HAND_T = 2.0, np.eye(3, dtype=F), np.array([0.5, 0.0, 0.0], F)


def ref_camera():
    import _fuse_ref as fr
    c = MATCH_CAM
    return fr.Camera(c["fx"], c["fy"], c["cx"], c["cy"], c["bf"], c["width"], c["height"], SCALE,
                     SCALE * SCALE)


def kernel_camera(orbpl):
    c = MATCH_CAM
    return orbpl.Camera(c["fx"], c["fy"], c["cx"], c["cy"], c["k1"], c["k2"], c["p1"], c["p2"],
                        c["k3"], c["bf"], c["th_depth"], c["width"], c["height"])


def bits(k):
    """a descriptor with its first k bits set: k from the zero descriptor"""
    d = np.zeros(32, np.uint8)
    d[:k // 8] = 255
    if k % 8:
        d[k // 8] = (1 << (k % 8)) - 1
    return d


def keyframe(features):
    """features: dicts with x, y, octave, desc and, for a feature with a point,
    xyz, min_dist, max_dist, mp_desc (valid defaults to having xyz)"""
    from _pkg import load_pkg
    n = len(features)
    kps = np.zeros(n, load_pkg().KP_DTYPE)
    kf = dict(kps_un=kps, desc=np.zeros((n, 32), np.uint8), valid=np.zeros(n, np.uint8),
              xyz=np.zeros((n, 3), F), min_dist=np.zeros(n, F), max_dist=np.zeros(n, F),
              mp_desc=np.zeros((n, 32), np.uint8), Tcw=np.eye(4, dtype=F))
    for i, f in enumerate(features):
        kps["x"][i], kps["y"][i], kps["octave"][i] = f.get("x", 100.0), f.get("y", 100.0), f.get("octave", 0)
        kf["desc"][i] = f.get("desc", bits(0))
        if "xyz" in f:
            kf["valid"][i] = f.get("valid", 1)
            kf["xyz"][i] = f["xyz"]
            kf["min_dist"][i], kf["max_dist"][i] = f.get("min_dist", 0.01), f.get("max_dist", 100.0)
            kf["mp_desc"][i] = f.get("mp_desc", bits(0))
    return kf


def probe_point(direction, u, v, z, level=None, **kw):
    """a feature whose point lands at pixel (u, v), depth z in the OTHER
    camera (identity poses, the hand-made Sim3); level: the level PredictScale
    shall give there (max_dist is set half a level inside it)"""
    c = MATCH_CAM
    P = np.array([(u - c["cx"]) / c["fx"] * z, (v - c["cy"]) / c["fy"] * z, z], np.float64)
    X = HAND_S * P + HAND_T if direction == 1 else (P - HAND_T) / HAND_S
    f = dict(xyz=X.astype(F), **kw)
    if level is not None:
        f["max_dist"] = float(np.linalg.norm(P)) * 1.2 ** (level - 0.5)
    return f


def hand_pair(direction, probe, targets, others=(), matched12=None):
    """direction 1: the probe is feature 0 of keyframe 1 and the targets are
    keyframe 2's features; direction 2: the other way round. others: further
    features on the probe's side."""
    a, b = keyframe([probe] + list(others)), keyframe(list(targets))
    kf1, kf2 = (a, b) if direction == 1 else (b, a)
    n1 = len(kf1["valid"])
    m = np.full(n1, -1, np.int32) if matched12 is None else np.asarray(matched12, np.int32)
    return dict(kf1=kf1, kf2=kf2, matched12=m, s12=HAND_S, R12=HAND_R, t12=HAND_T)


def scene(n, seed, n2=None):
    """A seeded pair of about n features per keyframe: common points seen by
    both (keypoints at their projections plus up to 2 px, octaves that the
    other side's PredictScale meets or misses by one), features without
    points, earlier matches of every kind, descriptors 0..130 bits apart."""
    from _pkg import load_pkg
    rng = np.random.default_rng(seed)
    c = MATCH_CAM
    n2 = n if n2 is None else n2
    s12 = rng.uniform(0.8, 1.25)
    R12, t12 = _rot(rng, 0.15), rng.uniform(-0.2, 0.2, 3)
    T1, T2 = _pose(rng), _pose(rng)
    ncom = int(0.7 * min(n, n2))
    kfs = []
    X1 = np.stack([(rng.uniform(-40, 680, ncom) - c["cx"]) / c["fx"],
                   (rng.uniform(-40, 520, ncom) - c["cy"]) / c["fy"], np.ones(ncom)], axis=1) \
        * rng.uniform(1.5, 9.0, ncom)[:, None]
    X2 = (X1 - t12) @ R12 / s12
    Xc = (X1, X2)
    order = (rng.permutation(n)[:ncom], rng.permutation(n2)[:ncom])
    base_desc = rng.integers(0, 256, (ncom, 32), dtype=np.uint8)
    octs = (rng.integers(0, 8, ncom), rng.integers(0, 8, ncom))
    for side, (cnt, T) in enumerate(((n, T1), (n2, T2))):
        kps = np.zeros(cnt, load_pkg().KP_DTYPE)
        kps["x"], kps["y"] = rng.uniform(0, 640, cnt), rng.uniform(0, 480, cnt)
        kps["octave"] = rng.integers(0, 8, cnt)
        kf = dict(kps_un=kps, desc=rng.integers(0, 256, (cnt, 32), dtype=np.uint8),
                  valid=(rng.uniform(size=cnt) < 0.3).astype(np.uint8),
                  xyz=rng.uniform(-4, 4, (cnt, 3)).astype(F), min_dist=np.full(cnt, 0.5, F),
                  max_dist=np.full(cnt, 20.0, F),
                  mp_desc=rng.integers(0, 256, (cnt, 32), dtype=np.uint8), Tcw=T.astype(F))
        X, Xo = Xc[side], Xc[1 - side]
        idx = order[side]
        kps["x"][idx] = c["fx"] * X[:, 0] / X[:, 2] + c["cx"] + rng.uniform(-2, 2, ncom)
        kps["y"][idx] = c["fy"] * X[:, 1] / X[:, 2] + c["cy"] + rng.uniform(-2, 2, ncom)
        kps["octave"][idx] = octs[side]
        kf["valid"][idx] = rng.uniform(size=ncom) < 0.9
        kf["xyz"][idx] = ((X - T[:3, 3]) @ T[:3, :3]).astype(F)
        # the other side's octave, met or missed by one level
        dist_o = np.linalg.norm(Xo, axis=1)
        kf["max_dist"][idx] = dist_o * 1.2 ** (octs[1 - side] + rng.choice([-1.4, -0.4, 0.6], ncom,
                                                                              p=[0.1, 0.7, 0.2]))
        kf["min_dist"][idx] = kf["max_dist"][idx] / rng.choice([30.0, 1.3], ncom, p=[0.9, 0.1])
        flips = rng.choice([0, 10, 60, 99, 130], ncom, p=[0.2, 0.4, 0.2, 0.1, 0.1])
        for d, k in ((kf["desc"], flips), (kf["mp_desc"], flips // 2)):
            dd = base_desc.copy()
            for j in range(ncom):
                pos = rng.permutation(256)[:k[j]]
                np.bitwise_xor.at(dd[j], pos // 8, (1 << (pos % 8)).astype(np.uint8))
            d[idx] = dd
        kfs.append(kf)
    m = np.full(n, -1, np.int32)
    pick = rng.permutation(n)[:n // 5]
    m[pick] = rng.choice(np.concatenate([np.arange(n2), [-2, -2, n2, n2 + 7]]), len(pick))
    return dict(kf1=kfs[0], kf2=kfs[1], matched12=m, s12=F(s12), R12=R12.astype(F),
                t12=t12.astype(F), name=f"scene_{n}_{n2}_s{seed}")


def hand_cases():
    """The branch-by-branch pairs: name -> (pair, direction, expected reason of
    the probe, expected vnMatch of the probe, expected nFound). Direction d's
    probe is feature 0 of keyframe d; the targets are the other keyframe's."""
    import _sim3_ref as ref
    cases = {}
    near = dict(x=300.0, y=200.0, octave=3, desc=bits(20))       # a target at the probe's pixel
    for d in (1, 2):
        def add(name, probe, targets, reason, vn=-1, found=0, others=(), matched12=None):
            cases[f"{name}_dir{d}"] = (hand_pair(d, probe, targets, others, matched12), d, reason,
                                       vn, found)
        P = lambda u=300.0, v=200.0, z=4.0, level=3, **kw: probe_point(d, u, v, z, level, **kw)
        add("matched_one_sided", P(), [near], ref.SIM3_MATCHED, 0)
        add("no_point", dict(), [near], ref.SIM3_NO_POINT)
        add("bad_point", P(valid=0), [near], ref.SIM3_NO_POINT)
        # the probe already matched: on side 1 its own entry, on side 2 an entry naming it
        if d == 1:
            add("already", P(), [near], ref.SIM3_ALREADY, matched12=[0])
            add("already_minus2", P(), [near], ref.SIM3_ALREADY, matched12=[-2])
            add("already_out_of_range", P(), [near], ref.SIM3_ALREADY, matched12=[5])
        else:
            add("already", P(), [near], ref.SIM3_ALREADY, matched12=[0])
            add("minus2_marks_nothing", P(), [near], ref.SIM3_MATCHED, 0, matched12=[-2])
            add("out_of_range_marks_nothing", P(), [near], ref.SIM3_MATCHED, 0, matched12=[1])
        add("behind", P(z=-4.0), [near], ref.SIM3_BEHIND)
        zero = P()
        zero["xyz"] = np.array([0.5, 0.0, 0.0], F) if d == 1 else np.array([-0.25, 0.0, 0.0], F)
        add("depth_zero", zero, [near], ref.SIM3_OUT_OF_IMAGE)
        nan = P()
        nan["xyz"] = np.array([np.nan, 0.0, 4.0], F)
        add("depth_nan", dict(nan, xyz=np.array([0.0, 0.0, np.nan], F)), [near],
            ref.SIM3_OUT_OF_IMAGE)
        add("x_nan", nan, [near], ref.SIM3_OUT_OF_IMAGE)
        for name, u, v, inside in (("left_in", 0.02, 200.0, True), ("left_out", -0.02, 200.0, False),
                                   ("right_in", 639.98, 200.0, True), ("right_out", 640.02, 200.0, False),
                                   ("top_in", 300.0, 0.02, True), ("top_out", 300.0, -0.02, False),
                                   ("bottom_in", 300.0, 479.98, True),
                                   ("bottom_out", 300.0, 480.02, False)):
            add("bound_" + name, P(u=u, v=v), [], ref.SIM3_EMPTY_AREA if inside else ref.SIM3_OUT_OF_IMAGE)
        # the distance range: dist = 4 on the optical axis
        ax = dict(u=320.0, v=240.0, z=4.0, level=None)
        on_axis = dict(x=320.0, y=240.0, octave=0, desc=bits(5))
        add("distance_below_min", P(**ax, min_dist=4.0 / 0.8 * 1.001, max_dist=100.0), [on_axis],
            ref.SIM3_DISTANCE)
        add("distance_at_min", P(**ax, min_dist=4.0 / 0.8 * 0.999, max_dist=4.2), [on_axis],
            ref.SIM3_MATCHED, 0)
        add("distance_above_max", P(**ax, min_dist=0.1, max_dist=4.0 / 1.2 * 0.999), [on_axis],
            ref.SIM3_DISTANCE)
        add("distance_at_max", P(**ax, min_dist=0.1, max_dist=4.0 / 1.2 * 1.001), [on_axis],
            ref.SIM3_MATCHED, 0)
        # PredictScale clamps: ratio far below 1 -> level 0, far above -> nlevels - 1
        add("level_clamped_to_0", P(**ax, min_dist=0.1, max_dist=3.5),
            [dict(on_axis, octave=1), dict(on_axis, octave=0, desc=bits(9))], ref.SIM3_MATCHED, 1)
        add("level_clamped_to_top", P(**ax, min_dist=0.1, max_dist=90.0),
            [dict(on_axis, octave=5), dict(on_axis, octave=7, desc=bits(9)),
             dict(on_axis, octave=6, desc=bits(7))], ref.SIM3_MATCHED, 2)
        add("empty_area", P(), [dict(near, x=400.0)], ref.SIM3_EMPTY_AREA)
        add("octave_gate_level_minus_1", P(), [dict(near, octave=2)], ref.SIM3_MATCHED, 0)
        add("octave_gate_level", P(), [dict(near, octave=3)], ref.SIM3_MATCHED, 0)
        add("octave_gate_level_plus_1", P(), [dict(near, octave=4)], ref.SIM3_NO_MATCH)
        add("all_gated_out", P(), [dict(near, octave=4), dict(near, octave=1), dict(near, octave=7)],
            ref.SIM3_NO_MATCH)
        add("distance_th_high", P(), [dict(near, desc=bits(100))], ref.SIM3_MATCHED, 0)
        add("distance_th_high_plus_1", P(), [dict(near, desc=bits(101))], ref.SIM3_NO_MATCH)
        # ties: GetFeaturesInArea walks the cells column by column, a cell in index order
        add("tie_across_cells", P(), [dict(near, x=306.0), dict(near, x=294.0)], ref.SIM3_MATCHED, 1)
        add("tie_in_one_cell", P(), [dict(near), dict(near, y=200.5), dict(near, desc=bits(21))],
            ref.SIM3_MATCHED, 0)
        add("first_minimum_later_smaller", P(),
            [dict(near, x=294.0), dict(near, x=306.0, desc=bits(19))], ref.SIM3_MATCHED, 1)
        # mutual: the target holds the same point, seen from its own camera, and
        # the probe's keypoint lies at that point's pixel in the probe's image
        c = MATCH_CAM
        Pd = np.array([(300.0 - c["cx"]) / c["fx"] * 4.0, (200.0 - c["cy"]) / c["fy"] * 4.0, 4.0])
        Ps = HAND_S * Pd + HAND_T if d == 1 else (Pd - HAND_T) / HAND_S     # in the probe's camera
        pu, pv = c["fx"] * Ps[0] / Ps[2] + c["cx"], c["fy"] * Ps[1] / Ps[2] + c["cy"]
        back = dict(near, xyz=Pd.astype(F), max_dist=float(np.linalg.norm(Ps)) * 1.2 ** 1.5,
                    mp_desc=bits(3))
        add("mutual", P(x=pu, y=pv, octave=2, desc=bits(8)), [back], ref.SIM3_MATCHED, 0, found=1)
        add("mutual_refused_by_octave", P(x=pu, y=pv, octave=5, desc=bits(8)), [back],
            ref.SIM3_MATCHED, 0)
        add("mutual_points_elsewhere", P(x=pu + 80.0, y=pv, octave=2, desc=bits(8)), [back],
            ref.SIM3_MATCHED, 0)
    return cases

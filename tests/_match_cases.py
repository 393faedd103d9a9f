"""Hand-built frames for the three per-frame point matchers, each case aimed at
one branch of the reference loop (tests/_match_ref.py names them), and seeded
crowds that force the parallel kernels' claim replay. Inputs and the values
worked out by hand only: the expected matches come from tests/_match_ref.py.

The camera has no distortion (bounds exactly 0 / 640 / 0 / 480, grid cells of
10 px), fx = fy = 512 and bf = 64, and every map point lies at camera depth 2,
so a projection is 256 * X + 320 and uR is u - 32, exact in float32. Descriptors
are Hadamard codewords (any two 128 bits apart) with `flip` for an exact
distance. A case names the reason code (and traced values) it was made for in
Problem.expect; test_match_ref.py checks that the restatement reaches it.
No case has camera-space z == 0."""
import functools

import numpy as np

import _match_ref as M
import _reloc_ref as RR
from _stereo_cases import code, flip

f32 = np.float32
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
               ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CFG = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0,
           bf=64.0, thdepth=40.0, width=640, height=480)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SCALE = np.ones(8, f32)
for _i in range(1, 8):
    SCALE[_i] = f32(SCALE[_i - 1] * f32(1.2))      # mvScaleFactors, as ORBextractor builds them
UP = f32(np.inf)


def above(x):
    return np.nextafter(f32(x), UP)


def below(x):
    return np.nextafter(f32(x), -UP)


class Problem:
    """kind: last / local / bow / kf; args: the matcher's inputs; expect: map
    point -> dict(reason=..., traced record fields...)"""

    def __init__(self, kind, name, args, expect=None):
        self.kind, self.name, self.args, self.expect = kind, name, args, expect or {}

    def __repr__(self):
        return f"{self.kind}:{self.name}"


def _frame(P):
    a = P.args
    cur = a["cur"]
    return RR.RefFrame(CFG, BOUNDS, SCALE, cur.get("Tcw", np.eye(4)), cur["kps_un"], cur["desc"])


def _ref_call(P):
    a = P.args
    if P.kind == "last":
        return M.search_last, (_frame(P), CFG["bf"], a["cur"]["uright"], a["last"], a["th"],
                               a["mono"], a["check_ori"])
    if P.kind == "local":
        return M.search_local, (_frame(P), a["cur"]["uright"], a["track"], a["mp_desc"],
                                a["mp_nobs"], a["cur_nobs"], a["th"], a["nnratio"])
    assert P.kind == "bow"
    return M.search_bow, (a["kf_node"], a["kf_valid"], a["kf_desc"], a["kf_angle"], a["f_node"],
                          a["f_desc"], a["f_angle"], a["nnratio"], a["check_ori"])


def run_topk(P):
    """(match, nmatches, rescans) of the kernels' scheme on the CPU"""
    fn, args = _ref_call(P)
    return M.replay_topk(fn, *args)


def run_ref(P, scheme="loop"):
    """(match, nmatches, rec, info) of the restatement (kf: rec None, info the
    trace of _reloc_ref.search_by_projection_kf)"""
    a = P.args
    if P.kind != "kf":
        fn, args = _ref_call(P)
        return fn(*args, scheme=scheme)
    kf = a["kf"]
    trace = {}
    m, n = RR.search_by_projection_kf(_frame(P), a["cur_has_mp"], kf["angle"], kf["valid"],
                                      kf["found"], kf["mp_xyz"], kf["mp_min_dist"],
                                      kf["mp_max_dist"], kf["mp_desc"], a["th"], a["orb_dist"],
                                      a["check_ori"], trace=trace)
    return m, n, None, trace


def run_oracle(O, P):
    a = P.args
    cam = O.camera(CFG)
    if P.kind == "last":
        return O.search_by_projection_last(cam, SCALE, a["cur"], a["last"], a["th"], a["mono"],
                                           a["check_ori"])
    if P.kind == "local":
        return O.search_by_projection_local(cam, SCALE, a["cur"], a["track"], a["mp_desc"],
                                            a["mp_nobs"], a["cur_nobs"], a["th"], a["nnratio"])
    assert P.kind == "bow"
    return O.search_by_bow(a["kf_node"], a["kf_valid"], a["kf_desc"], a["kf_angle"], a["f_node"],
                           a["f_desc"], a["f_angle"], a["nnratio"], a["check_ori"])


def run_gpu(orbpl, P):
    a = P.args
    cam = orbpl.make_camera(CFG)
    if P.kind == "last":
        m = orbpl.ORBmatcher(0.9, a["check_ori"])
        return m.SearchByProjectionLastFrame(cam, SCALE, a["cur"], a["last"], a["th"], a["mono"])
    if P.kind == "local":
        m = orbpl.ORBmatcher(a["nnratio"], True)
        return m.SearchByProjectionLocalMap(cam, SCALE, a["cur"], a["track"], a["mp_desc"],
                                            a["mp_nobs"], a["cur_nobs"], a["th"])
    if P.kind == "bow":
        m = orbpl.ORBmatcher(a["nnratio"], a["check_ori"])
        return m.SearchByBoW(a["kf_node"], a["kf_valid"], a["kf_desc"], a["kf_angle"],
                             a["f_node"], a["f_desc"], a["f_angle"])
    m = orbpl.ORBmatcher(0.9, a["check_ori"])
    return m.SearchByProjectionKeyFrame(cam, SCALE, a["cur"], a["cur_has_mp"], a["kf"], a["th"],
                                        a["orb_dist"])


def _sites(step, x0=60, y0=60, x1=580, y1=400):
    for y in range(y0, y1 + 1, step):
        for x in range(x0, x1 + 1, step):
            yield float(x), float(y)


def _kps(rows):
    k = np.zeros(len(rows), KP)
    for i, (x, y, o, ang) in enumerate(rows):
        k["x"][i], k["y"][i], k["octave"][i], k["angle"][i] = x, y, o, ang
    k["size"], k["response"], k["class_id"] = 31.0, 20.0, -1
    return k


def _desc(rows):
    return np.ascontiguousarray(np.stack(rows) if rows else np.zeros((0, 32)), np.uint8)


class _Codes:
    def __init__(self):
        self._code = 0

    def new_code(self):
        self._code += 1
        return code(self._code)


# ==========================================================================
# SearchByProjection(CurrentFrame, LastFrame)
# ==========================================================================
class LastBuilder(_Codes):
    """Current pose = translation (0, 0, tz), last pose = identity, so
    tlc.z = -tz against mb = 64 / 512 = 0.125; a map point meant for pixel
    (u, v) lies at camera depth zc (world z = zc - tz)."""

    def __init__(self, name, tz=0.0, th=7.0, mono=False, check_ori=True, step=40):
        super().__init__()
        self.name, self.tz, self.th, self.mono, self.check_ori = name, tz, th, mono, check_ori
        self.k, self.kd, self.kur = [], [], []
        self.p, self.expect = [], {}
        self.sites = _sites(step)

    def site(self):
        return next(self.sites)

    def kp(self, x, y, octave=0, desc=None, angle=0.0, uright=-1.0):
        self.k.append((x, y, octave, angle))
        self.kd.append(self.new_code() if desc is None else desc)
        self.kur.append(uright)
        return len(self.k) - 1

    def mp(self, pu, pv, desc, octave=0, nobs=1, angle=0.0, has_mp=1, outlier=0, zc=2.0, X=None,
           Y=None, expect=None, **trace):
        X = (pu - 320.0) * zc / 512.0 if X is None else X
        Y = (pv - 240.0) * zc / 512.0 if Y is None else Y
        self.p.append(dict(xyz=(X, Y, zc - self.tz), desc=desc, octave=octave, nobs=nobs,
                           angle=angle, has_mp=has_mp, outlier=outlier))
        i = len(self.p) - 1
        if expect is not None:
            self.expect[i] = dict(reason=expect, **trace)
        return i

    def fill(self, upto):
        """last-frame keypoints without a map point, so that the next point has index upto"""
        c = code(255)
        while len(self.p) < upto:
            self.p.append(dict(xyz=(0.0, 0.0, 2.0), desc=c, octave=0, nobs=1, angle=0.0, has_mp=0,
                               outlier=0))

    def pair(self, rot=0.0, d=0, nobs=1, expect=M.ACCEPTED, **trace):
        """an isolated point with one keypoint at distance d and rotation rot"""
        u, v = self.site()
        c = self.new_code()
        j = self.kp(u + 1.0, v, 0, flip(c, d), angle=0.0 if rot >= 0 else -rot)
        i = self.mp(u, v, c, angle=max(rot, 0.0), nobs=nobs, expect=expect,
                    kp=j if expect in (M.ACCEPTED, M.ROT_CUT) else -1, **trace)
        return i, j

    def done(self):
        Tc = np.eye(4, dtype=f32)
        Tc[2, 3] = self.tz
        cur = dict(Tcw=Tc, kps_un=_kps(self.k), desc=_desc(self.kd),
                   uright=np.array(self.kur, f32))
        p = self.p
        last = dict(Tcw=np.eye(4, dtype=f32),
                    kps_un=_kps([(0.0, 0.0, q["octave"], q["angle"]) for q in p]),
                    has_mp=np.array([q["has_mp"] for q in p], np.uint8),
                    outlier=np.array([q["outlier"] for q in p], np.uint8),
                    mp_xyz=np.array([q["xyz"] for q in p], f32).reshape(-1, 3),
                    mp_desc=_desc([q["desc"] for q in p]),
                    mp_nobs=np.array([q["nobs"] for q in p], np.int32))
        return Problem("last", self.name, dict(cur=cur, last=last, th=self.th, mono=self.mono,
                                               check_ori=self.check_ori), self.expect)


def last_gates():
    b = LastBuilder("gates")
    c = b.new_code()
    u, v = b.site()
    b.kp(u, v, 0, c)
    b.mp(u, v, c, has_mp=0, expect=M.NO_MP)
    u, v = b.site()
    b.kp(u, v, 0, c)
    b.mp(u, v, c, outlier=1, expect=M.OUTLIER)
    u, v = b.site()
    b.kp(u, v, 0, c)
    b.mp(u, v, c, zc=-2.0, expect=M.BEHIND)
    # on the bound: kept; one step of the point's coordinate outside: dropped.
    # The dropped point comes first: were it kept, it would take the keypoint
    for (u, v, kx, ky, X, Y, uo, vo) in (
            (0.0, 100.0, 2.0, 100.0, below(-1.25), None, -2.0 ** -15, 100.0),
            (640.0, 140.0, 634.0, 140.0, f32(1.25 + 2.0 ** -22), None, above(640.0), 140.0),
            (100.0, 0.0, 100.0, 2.0, None, below(-0.9375), 100.0, -2.0 ** -16),
            (140.0, 480.0, 140.0, 474.0, None, f32(0.9375 + 2.0 ** -23), 140.0, above(480.0))):
        c = b.new_code()
        j = b.kp(kx, ky, 0, c)
        b.mp(u, v, c, X=X, Y=Y, expect=M.OUT_OF_IMAGE, u=f32(uo), v=f32(vo))
        b.mp(u, v, c, expect=M.ACCEPTED, kp=j, u=f32(u), v=f32(v))
    return b.done()


def _level_window(octave, tz, mono):
    if -tz > 0.125 and not mono:
        return octave, 7
    if tz > 0.125 and not mono:
        return 0, octave
    return max(octave - 1, 0), min(octave + 1, 7)


def last_levels(tz, mono=False):
    """tlc.z = -tz above / on / below +-mb (and bMono overriding): for
    nLastOctave 0, 3 and 7, two sites with a keypoint of every octave, the
    distance falling with the octave at one and rising at the other, so that
    the accepted keypoint is the top / bottom of the level window"""
    b = LastBuilder(f"levels_tz{tz}_{'mono' if mono else 'rgbd'}", tz=tz, mono=mono, step=80)
    for octave in (0, 3, 7):
        lo, hi = _level_window(octave, tz, mono)
        for rising in (False, True):
            u, v = b.site()
            c = b.new_code()
            js = [b.kp(u + 0.25 * o, v + 1.0, o, flip(c, 10 + (o if rising else 7 - o)))
                  for o in range(8)]
            b.mp(u, v, c, octave=octave, expect=M.ACCEPTED, kp=js[lo if rising else hi],
                 ncand=hi - lo + 1)
    return b.done()


def last_radius_grid():
    b = LastBuilder("radius_grid")
    # |dx| == radius is out; the keypoint coordinate one float step nearer is in
    for dx, dy, inside in ((7.0, 0.0, False), (7.0, 0.0, True), (-7.0, 0.0, False),
                           (-7.0, 0.0, True), (0.0, 7.0, False), (0.0, 7.0, True),
                           (0.0, -7.0, False), (0.0, -7.0, True)):
        u, v = b.site()
        c = b.new_code()
        x, y = f32(u + dx), f32(v + dy)
        if inside:
            x = np.nextafter(x, f32(u)) if dx else x
            y = np.nextafter(y, f32(v)) if dy else y
        j = b.kp(x, y, 0, c)
        b.mp(u, v, c, expect=M.ACCEPTED if inside else M.NO_WINDOW, kp=j if inside else -1)
    # PosInGrid rounds 636 * 0.1f to column 64: the keypoint is in no cell
    c = b.new_code()
    b.kp(636.0, 300.0, 0, c)
    b.mp(632.0, 300.0, c, expect=M.NO_WINDOW)
    # windows clipped at columns 0 / 63 and rows 0 / 47
    for u, v, kx, ky in ((3.0, 3.0, 1.0, 1.0), (630.0, 3.0, 632.0, 1.0), (3.0, 470.0, 1.0, 472.0),
                         (630.0, 470.0, 632.0, 472.0)):
        c = b.new_code()
        j = b.kp(kx, ky, 0, c)
        b.mp(u, v, c, expect=M.ACCEPTED, kp=j)
    return b.done()


def last_uright():
    """u = site, uR = u - 32, radius 7"""
    b = LastBuilder("uright")
    for off, exp in ((7.0, M.ACCEPTED), (None, M.NO_CANDIDATE), (-7.0, M.ACCEPTED),
                     (100.0, M.NO_CANDIDATE), ("zero", M.ACCEPTED), ("minus", M.ACCEPTED)):
        u, v = b.site()
        c = b.new_code()
        ur = {None: above(u - 32.0 + 7.0), "zero": 0.0, "minus": -1.0}.get(off)
        if ur is None:
            ur = u - 32.0 + off
        j = b.kp(u + 1.0, v, 0, c, uright=ur)
        b.mp(u, v, c, expect=exp, kp=j if exp == M.ACCEPTED else -1)
    return b.done()


def last_threshold():
    b = LastBuilder("threshold")
    for d, exp in ((100, M.ACCEPTED), (101, M.OVER_TH)):
        b.pair(d=d, expect=exp, best=d)
    # the best unclaimed candidate at 101 while a claimed one sits at 40
    u, v = b.site()
    c = b.new_code()
    j = b.kp(u + 1.0, v, 0, flip(c, 40))
    b.kp(u - 1.0, v, 0, flip(c, 101))
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j, best=40)
    b.mp(u, v, c, expect=M.OVER_TH, best=101, ncand=1, skipped=1)
    # the complementary descriptor as the only candidate
    u, v = b.site()
    c = b.new_code()
    b.kp(u, v, 0, flip(c, 256))
    b.mp(u, v, c, expect=M.NO_CANDIDATE, best=256)
    return b.done()


def last_ties_claims():
    b = LastBuilder("ties_claims")
    # equal distances: the scan (grid column, then row, then index) decides, not the index
    for first, second in (((5.0, 0.0), (-5.0, 0.0)), ((0.0, 5.0), (0.0, -5.0))):
        u, v = b.site()
        c = b.new_code()
        b.kp(u + first[0], v + first[1], 0, flip(c, 10, 0))       # lower index, later cell
        j = b.kp(u + second[0], v + second[1], 0, flip(c, 10, 50))
        b.mp(u, v, c, expect=M.ACCEPTED, kp=j, best=10)
    u, v = b.site()        # one cell: the lower index
    c = b.new_code()
    j = b.kp(u + 1.0, v + 1.0, 0, flip(c, 10, 0))
    b.kp(u + 0.5, v + 0.5, 0, flip(c, 10, 50))
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j)
    # a claimer and a non-claimer on one keypoint, in both orders, and two non-claimers
    for n1, n2, e2 in ((1, 0, M.ALL_CLAIMED), (0, 1, M.ACCEPTED_OVERWRITES),
                       (0, 0, M.ACCEPTED_OVERWRITES)):
        u, v = b.site()
        c = b.new_code()
        j = b.kp(u, v, 0, c)
        b.mp(u, v, c, nobs=n1, expect=M.ACCEPTED, kp=j)
        b.mp(u, v, c, nobs=n2, expect=e2, kp=-1 if e2 == M.ALL_CLAIMED else j)
    return b.done()


def _claimed_site(b, dists, nclaim, keypoints_first=True):
    """one site with keypoints at the given (distinct where it matters)
    distances from code c and nclaim points that take the nclaim best, one each"""
    u, v = b.site()
    c = b.new_code()
    js = []
    for q, d in enumerate(dists):
        # a 27 x 27 lattice of half pixels inside the 7 px window
        js.append(b.kp(u - 6.5 + 0.5 * (q // 27), v - 6.5 + 0.5 * (q % 27), 0, flip(c, d)))
    order = sorted(range(len(dists)), key=lambda q: (dists[q], q))
    for q in order[:nclaim]:
        b.mp(u, v, c, expect=M.ACCEPTED, kp=js[q])
    return u, v, c, js, order


def last_exhaustion():
    b = LastBuilder("exhaustion")
    u, v, c, js, _ = _claimed_site(b, [0, 1, 2, 3], 4)
    b.mp(u, v, c, expect=M.ALL_CLAIMED, ncand=4, skipped=4)
    u, v, c, js, _ = _claimed_site(b, [3, 100, 2, 1, 0], 4)
    b.mp(u, v, c, expect=M.ACCEPTED, kp=js[1], best=100, ncand=5, skipped=4)
    u, v, c, js, _ = _claimed_site(b, [3, 101, 2, 1, 0], 4)
    b.mp(u, v, c, expect=M.OVER_TH, best=101, ncand=4, skipped=4)
    # the count of candidates <= 100 saturates at 255, the four best claimed. An 8-bit count
    # that wrapped instead would read 0 at 256 candidates (no candidate at all: not even the
    # four claimers match), 2 at 258 (a list of two, both claimed, and no re-scan) and 44 at
    # 300 (harmless: still above four)
    for count in (256, 258, 300):
        d = [min(5 + q % 90, 100) for q in range(count)]
        d[17], d[250], d[40], d[3] = 0, 1, 2, 3
        d[count - 1] = 4
        u, v, c, js, _ = _claimed_site(b, d, 4)
        b.mp(u, v, c, expect=M.ACCEPTED, kp=js[count - 1], best=4, ncand=count, skipped=4)
    return b.done()


def _domino_geometry(nchain):
    """points 3 px apart on one row with radius 3: point i sees exactly the
    keypoints i and i + 1 (half a pixel left of point i / 2.5 px right)"""
    assert nchain <= 190
    return [(20.0 + 3.0 * i, 100.0) for i in range(nchain + 1)]


def last_domino(nchain=134):
    """An extra first point takes k0; chain point i prefers k_i (distance i / 2)
    over k_(i+1), finds it claimed by the point before and takes k_(i+1):
    every lane collides with the lane before it, across 63 | 64 and 127 | 128"""
    b = LastBuilder("domino", th=3.0)
    c = b.new_code()
    pos = _domino_geometry(nchain)
    js = [b.kp(x - 0.5, y, 0, flip(c, i // 2)) for i, (x, y) in enumerate(pos)]
    b.mp(pos[0][0] - 3.0, pos[0][1], c, expect=M.ACCEPTED, kp=js[0])
    for i in range(nchain):
        b.mp(pos[i][0], pos[i][1], c, expect=M.ACCEPTED, kp=js[i + 1], skipped=1)
    return b.done()


def _rot_problem(name, groups, check_ori=True, extra=None):
    """groups: [(rot, count, cut, bin)]: count isolated pairs with rotation
    rot, which falls into histogram bin `bin`; cut = the caller's hand-worked
    verdict that this bin is outside the three kept ones"""
    b = LastBuilder(name, check_ori=check_ori)
    for rot, count, cut, bin_ in groups:
        for _ in range(count):
            b.pair(rot=rot, expect=M.ROT_CUT if (cut and check_ori) else M.ACCEPTED,
                   bin=bin_ if check_ori else -1)
    if extra:
        extra(b)
    return b.done()


def last_rotation():
    out = []
    # bins: rot / 12 rounded half away from zero, 30 -> 0. -10 -> 350 -> 29; 6 -> 0.5 -> 1
    # (rint would say 0); 18 -> 1.5 -> 2; 359 -> 29.9 -> 30 -> 0; 0 -> 0.
    # sizes: bin 29: 1, bin 1: 2, bin 2: 2, bin 0: 3 -> kept 0, 1, 2 (first of equals), cut 29
    out.append(_rot_problem("rot_bins", [(-10.0, 1, True, 29), (6.0, 2, False, 1),
                                         (18.0, 2, False, 2), (359.0, 2, False, 0),
                                         (0.0, 1, False, 0)]))
    # four equal bins: the first three in bin order stay
    out.append(_rot_problem("rot_equal", [(120.0, 2, False, 10), (24.0, 2, False, 2),
                                          (240.0, 2, True, 20), (60.0, 2, False, 5)]))
    # max2 = max3 = 1 = 0.1f * 10 in float32: kept
    out.append(_rot_problem("rot_tenth_on", [(0.0, 10, False, 0), (48.0, 1, False, 4),
                                             (96.0, 1, False, 8)]))
    # one more in the first bin: 1 < 0.1f * 11, both cut
    out.append(_rot_problem("rot_tenth_below", [(0.0, 11, False, 0), (48.0, 1, True, 4),
                                                (96.0, 1, True, 8)]))
    # max2 = 2 on 0.1f * 20, max3 = 1 below it
    out.append(_rot_problem("rot_tenth_third", [(0.0, 20, False, 0), (48.0, 2, False, 4),
                                                (96.0, 1, True, 8)]))
    # no match at all: an empty histogram cuts nothing
    b = LastBuilder("rot_empty")
    b.pair(d=101, expect=M.OVER_TH)
    out.append(b.done())

    # two non-claimers on one keypoint: the entry of the first writer is cut
    # with its bin although the second writer's stays (the keypoint is cleared
    # and counted once), and both cut (counted twice)
    def twice(rots_cut):
        def add(b):
            u, v = b.site()
            c = b.new_code()
            j = b.kp(u, v, 0, c, angle=0.0)
            for q, (rot, cut) in enumerate(rots_cut):
                exp = M.ROT_CUT if cut and b.check_ori else \
                    (M.ACCEPTED_OVERWRITES if q else M.ACCEPTED)
                b.mp(u, v, c, nobs=0, angle=rot, expect=exp, kp=j)
        return add
    main = [(0.0, 6, False, 0), (48.0, 5, False, 4), (96.0, 4, False, 8)]
    out.append(_rot_problem("rot_first_writer_cut", main, extra=twice([(180.0, True),
                                                                        (0.0, False)])))
    out.append(_rot_problem("rot_both_writers_cut", main, extra=twice([(180.0, True),
                                                                        (200.0, True)])))
    out.append(_rot_problem("rot_off", main, check_ori=False,
                            extra=twice([(180.0, True), (0.0, False)])))
    return out


def last_many_points():
    """2048 last-frame keypoints against three current ones: the 2048 build by
    the last frame's size alone, claims across 1023 | 1024 and at index 2047"""
    b = LastBuilder("nl2048", check_ori=False)
    u, v = b.site()
    c = b.new_code()
    js = [b.kp(u + q, v, 0, flip(c, 10 * q)) for q in range(3)]
    b.fill(1023)
    b.mp(u, v, c, expect=M.ACCEPTED, kp=js[0])
    b.mp(u, v, c, nobs=0, expect=M.ACCEPTED, kp=js[1], skipped=1)
    b.fill(2047)
    b.mp(u, v, c, expect=M.ACCEPTED_OVERWRITES, kp=js[1], skipped=1)
    assert len(b.p) == 2048
    return b.done()


def last_sizes():
    b = LastBuilder("no_keypoints")
    b.mp(100.0, 100.0, b.new_code(), expect=M.NO_WINDOW)
    b2 = LastBuilder("no_points")
    b2.kp(100.0, 100.0)
    return [b.done(), b2.done()]


def pad_keypoints(P, total, seed=5):
    """P with padding keypoints in front (rows 452 .. 478, far from every site
    of P, whose windows end above row 446), total keypoints in all: the real
    keypoints move to the highest indices, the last one to total - 1"""
    a = dict(P.args)
    cur = dict(a["cur"])
    npad = total - len(cur["kps_un"])
    assert npad > 0
    rng = np.random.default_rng(seed)
    pad = np.zeros(npad, KP)
    pad["x"] = rng.uniform(1, 630, npad).astype(f32)
    pad["y"] = rng.uniform(452, 478, npad).astype(f32)
    pad["octave"] = rng.integers(0, 8, npad)
    pad["angle"] = rng.uniform(0, 360, npad)
    pad["size"], pad["response"], pad["class_id"] = 31.0, 20.0, -1
    cur["kps_un"] = np.concatenate([pad, cur["kps_un"]])
    cur["desc"] = np.concatenate([rng.integers(0, 256, (npad, 32), dtype=np.uint8), cur["desc"]])
    cur["uright"] = np.concatenate([np.full(npad, -1, f32), cur["uright"]])
    a["cur"] = cur
    if a.get("cur_nobs") is not None:
        a["cur_nobs"] = np.concatenate([np.zeros(npad, np.int32), a["cur_nobs"]])
    expect = {i: dict(e, kp=e["kp"] + npad) if e.get("kp", -1) >= 0 else e
              for i, e in P.expect.items()}
    Q = Problem(P.kind, f"{P.name}_{total}kp", a, expect)
    Q.npad = npad
    return Q


@functools.lru_cache(maxsize=1)
def last_cases():
    out = [last_gates()]
    for tz in (-0.25, -0.125, -0.0625, 0.0, 0.0625, 0.125, 0.25):
        out.append(last_levels(tz))
    out += [last_levels(-0.25, mono=True), last_levels(0.25, mono=True)]
    out += [last_radius_grid(), last_uright(), last_threshold(), last_ties_claims(),
            last_exhaustion(), last_domino()]
    rot = last_rotation()
    out += rot + last_sizes() + [last_many_points()]
    small = [last_ties_claims(), last_exhaustion(), rot[6]]
    out += [pad_keypoints(p, 1025) for p in small] + [pad_keypoints(p, 2048) for p in small]
    return out


# ==========================================================================
# SearchByProjection(Frame, vpLocalMapPoints)
# ==========================================================================
LOW_COS = 0.5                      # radius factor 4.0


class LocalBuilder(_Codes):
    def __init__(self, name, th=1.0, nnratio=0.8, step=40, cur_nobs=True):
        super().__init__()
        self.name, self.th, self.nnratio, self.with_nobs = name, th, nnratio, cur_nobs
        self.k, self.kd, self.kur, self.kobs = [], [], [], []
        self.p, self.expect = [], {}
        self.sites = _sites(step)

    def site(self):
        return next(self.sites)

    def kp(self, x, y, octave=0, desc=None, uright=-1.0, nobs=0):
        self.k.append((x, y, octave, 0.0))
        self.kd.append(self.new_code() if desc is None else desc)
        self.kur.append(uright)
        self.kobs.append(nobs)
        return len(self.k) - 1

    def mp(self, x, y, desc, level=0, nobs=1, view_cos=LOW_COS, in_view=1, xr=0.0, expect=None,
           **trace):
        self.p.append(dict(x=x, y=y, desc=desc, level=level, nobs=nobs, view_cos=view_cos,
                           in_view=in_view, xr=xr))
        i = len(self.p) - 1
        if expect is not None:
            self.expect[i] = dict(reason=expect, **trace)
        return i

    def fill(self, upto):
        """fillers that are not in view, so that the next point has index upto"""
        c = code(255)
        while len(self.p) < upto:
            self.p.append(dict(x=0.0, y=0.0, desc=c, level=0, nobs=1, view_cos=0.0, in_view=0,
                               xr=0.0))

    def done(self):
        p = self.p
        cur = dict(kps_un=_kps(self.k), desc=_desc(self.kd), uright=np.array(self.kur, f32))
        track = dict(in_view=np.array([q["in_view"] for q in p], np.uint8),
                     proj_x=np.array([q["x"] for q in p], f32),
                     proj_y=np.array([q["y"] for q in p], f32),
                     proj_xr=np.array([q["xr"] for q in p], f32),
                     level=np.array([q["level"] for q in p], np.int32),
                     view_cos=np.array([q["view_cos"] for q in p], f32))
        args = dict(cur=cur, track=track, mp_desc=_desc([q["desc"] for q in p]),
                    mp_nobs=np.array([q["nobs"] for q in p], np.int32),
                    cur_nobs=np.array(self.kobs, np.int32) if self.with_nobs else None,
                    th=self.th, nnratio=self.nnratio)
        return Problem("local", self.name, args, self.expect)


def local_visibility(th=1.0):
    """radius = (2.5 | 4.0) [* th] at level 0"""
    b = LocalBuilder(f"visibility_th{th}", th=th)
    c = b.new_code()
    u, v = b.site()
    b.kp(u, v, 0, c)
    b.mp(u, v, c, in_view=0, expect=M.NOT_IN_VIEW)
    k = f32(th)
    for cos, r in ((f32(0.998), 2.5), (below(f32(0.998)), 4.0), (1.0, 2.5), (0.0, 4.0)):
        for inside in (False, True):
            u, v = b.site()
            c = b.new_code()
            x = f32(u + float(f32(r) * k))             # |dx| == radius: out
            j = b.kp(below(x) if inside else x, v, 0, c)
            b.mp(u, v, c, view_cos=cos, expect=M.ACCEPTED if inside else M.NO_WINDOW,
                 kp=j if inside else -1, r=f32(f32(r) * k) if th != 1.0 else f32(r))
    return b.done()


def local_levels_gates():
    b = LocalBuilder("levels_gates", th=1.0, step=80)
    # level 0: octave 0 alone
    u, v = b.site()
    c = b.new_code()
    j = b.kp(u + 1.0, v, 0, flip(c, 30))
    b.kp(u - 1.0, v, 1, flip(c, 5))
    b.mp(u, v, c, level=0, expect=M.ACCEPTED, kp=j, best=30, second=256)
    # level 3: octaves 2 and 3 (1 and 4 lie closer)
    u, v = b.site()
    c = b.new_code()
    b.kp(u - 2.0, v, 1, flip(c, 5))
    j = b.kp(u - 1.0, v, 2, flip(c, 30))
    b.kp(u + 1.0, v, 3, flip(c, 60, 100))
    b.kp(u + 2.0, v, 4, flip(c, 6))
    b.mp(u, v, c, level=3, expect=M.ACCEPTED, kp=j, best=30, second=60, best_level=2,
         second_level=3)
    # level 7, the top
    u, v = b.site()
    c = b.new_code()
    j = b.kp(u + 1.0, v, 7, flip(c, 9))
    b.kp(u - 1.0, v, 5, flip(c, 1))
    b.mp(u, v, c, level=7, expect=M.ACCEPTED, kp=j, best=9)
    # a keypoint holding a point with observations is skipped, one holding a point without is not
    u, v = b.site()
    c = b.new_code()
    b.kp(u - 1.0, v, 0, flip(c, 5), nobs=2)
    j = b.kp(u + 1.0, v, 0, flip(c, 20, 100))
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j, best=20, second=256, skipped=1)
    u, v = b.site()
    c = b.new_code()
    j = b.kp(u - 1.0, v, 0, flip(c, 5), nobs=0)
    b.kp(u + 1.0, v, 0, flip(c, 20, 100))
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j, best=5, second=20)
    # the proj_xr gate: radius 4 at level 0
    for xr, exp in ((54.0, M.ACCEPTED), (above(54.0), M.NO_CANDIDATE), (46.0, M.ACCEPTED),
                    (below(46.0), M.NO_CANDIDATE)):
        u, v = b.site()
        c = b.new_code()
        j = b.kp(u + 1.0, v, 0, c, uright=50.0)
        b.mp(u, v, c, xr=xr, expect=exp, kp=j if exp == M.ACCEPTED else -1)
    u, v = b.site()       # uright <= 0: no gate
    c = b.new_code()
    j = b.kp(u + 1.0, v, 0, c, uright=0.0)
    b.mp(u, v, c, xr=500.0, expect=M.ACCEPTED, kp=j)
    # the complementary descriptor as the only candidate; 100 and 101
    u, v = b.site()
    c = b.new_code()
    b.kp(u, v, 0, flip(c, 256))
    b.mp(u, v, c, expect=M.NO_CANDIDATE, best=256)
    for d, exp in ((100, M.ACCEPTED), (101, M.OVER_TH)):
        u, v = b.site()
        c = b.new_code()
        j = b.kp(u, v, 0, flip(c, d))
        b.mp(u, v, c, expect=exp, kp=j if exp == M.ACCEPTED else -1, best=d)
    # cell (63, 47)
    c = b.new_code()
    j = b.kp(632.0, 472.0, 0, c)
    b.mp(631.0, 471.0, c, expect=M.ACCEPTED, kp=j)
    return b.done()


def local_no_cur_nobs():
    """the layout of the held keypoint above with cur_nobs = NULL: nothing is held"""
    b = LocalBuilder("cur_nobs_none", cur_nobs=False)
    u, v = b.site()
    c = b.new_code()
    j = b.kp(u - 1.0, v, 0, flip(c, 5), nobs=2)
    b.kp(u + 1.0, v, 0, flip(c, 20, 100))
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j, best=5, second=20)
    return b.done()


def local_best_second():
    """th 3: radius 12 at level 1 is 14.4; the keypoints lie 10 px apart along
    x, so the scan meets them left to right. (distance, octave) per keypoint."""
    b = LocalBuilder("best_second", th=3.0, step=80)
    for seq, best_q, tr in (
            ([(50, 1), (30, 1)], 1, dict(best=30, second=50, best_level=1, second_level=1)),
            ([(30, 1), (50, 0), (40, 1)], 0, dict(best=30, second=40, best_level=1,
                                                   second_level=1)),
            # the second is the first 45 (octave 0): were it the other, 40 > 0.8 * 45 rejects
            ([(45, 0), (45, 1), (40, 1)], 2, dict(best=40, second=45, best_level=1,
                                                   second_level=0)),
            ([(45, 1), (45, 0), (40, 0)], 2, dict(best=40, second=45, best_level=0,
                                                   second_level=1)),
            ([(30, 1), (30, 0)], 0, dict(best=30, second=30, best_level=1, second_level=0)),
            ([(30, 0), (30, 1)], 0, dict(best=30, second=30, best_level=0, second_level=1))):
        u, v = b.site()
        c = b.new_code()
        js = [b.kp(u - 10.0 + 10.0 * q, v, o, flip(c, d, 60 * q)) for q, (d, o) in enumerate(seq)]
        b.mp(u, v, c, level=1, expect=M.ACCEPTED, kp=js[best_q], **tr)
    return b.done()


def local_ratio():
    """0.8f * 50 = 40.0f: 40 passes (not greater), 41 does not"""
    b = LocalBuilder("ratio")
    for bd, o2, exp in ((40, 0, M.ACCEPTED), (41, 0, M.RATIO_REJECT), (39, 0, M.ACCEPTED),
                        (45, 1, M.ACCEPTED)):      # o2 = 1: the second lies on another level
        u, v = b.site()
        c = b.new_code()
        j = b.kp(u - 1.0, v, 0, flip(c, bd))
        b.kp(u + 1.0, v, o2, flip(c, 50, 100))
        b.mp(u, v, c, level=o2, expect=exp, kp=j if exp == M.ACCEPTED else -1, best=bd, second=50,
             best_level=0, second_level=o2)
    u, v = b.site()      # a single candidate: the second stays 256 at level -1
    c = b.new_code()
    j = b.kp(u, v, 0, flip(c, 99))
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j, best=99, second=256, second_level=-1)
    return b.done()


def local_claims():
    b = LocalBuilder("claims")
    # B's candidates: k1 at 30, k2 at 32 (same level: 30 > 0.8 * 32 rejects)
    def site(dists):
        u, v = b.site()
        c = b.new_code()
        ks = [flip(c, d, 70 * q) for q, d in enumerate(dists)]
        js = [b.kp(u - 1.0 + q, v, 0, k) for q, k in enumerate(ks)]
        return u, v, c, ks, js
    # control: nobody claims, B is rejected and claims nothing; F then takes k1
    u, v, c, ks, js = site([30, 32])
    b.mp(u, v, c, expect=M.RATIO_REJECT, best=30, second=32)
    b.mp(u, v, flip(c, 25), expect=M.ACCEPTED, kp=js[0], best=5, second=57)
    # A (k2's descriptor) claims B's second: the reject becomes an accept
    u, v, c, ks, js = site([30, 32])
    b.mp(u, v, ks[1], expect=M.ACCEPTED, kp=js[1], best=0, second=62)
    b.mp(u, v, c, expect=M.ACCEPTED, kp=js[0], best=30, second=256, skipped=1)
    # A claims B's best: B takes its second
    u, v, c, ks, js = site([10, 60])
    b.mp(u, v, ks[0], expect=M.ACCEPTED, kp=js[0])
    b.mp(u, v, c, expect=M.ACCEPTED, kp=js[1], best=60, second=256)
    # A claims B's third: nothing changes
    u, v, c, ks, js = site([10, 40, 50])
    b.mp(u, v, ks[2], expect=M.ACCEPTED, kp=js[2], best=0, second=60)
    b.mp(u, v, c, expect=M.ACCEPTED, kp=js[0], best=10, second=40, skipped=1)
    # points without observations do not claim: the next point overwrites
    u, v, c, ks, js = site([10])
    b.mp(u, v, c, nobs=0, expect=M.ACCEPTED, kp=js[0])
    b.mp(u, v, c, nobs=0, expect=M.ACCEPTED_OVERWRITES, kp=js[0])
    b.mp(u, v, c, nobs=3, expect=M.ACCEPTED_OVERWRITES, kp=js[0])
    b.mp(u, v, c, nobs=1, expect=M.ALL_CLAIMED)
    # order: the level-1 point has the lower index and goes first
    u, v = b.site()
    c = b.new_code()
    j = b.kp(u, v, 0, c)
    b.mp(u, v, c, level=1, expect=M.ACCEPTED, kp=j)
    b.mp(u, v, c, level=0, expect=M.ALL_CLAIMED)
    return b.done()


def local_exhaustion():
    b = LocalBuilder("exhaustion")
    for dists, exp, tr in (
            ([10, 20, 30, 40], M.ACCEPTED, dict(best=40, second=256, ncand=4, skipped=3)),
            # a fifth at 45 is the second after a re-scan: 40 > 0.8 * 45
            ([10, 20, 30, 40, 45], M.RATIO_REJECT, dict(best=40, second=45, ncand=5, skipped=3)),
            ([10, 20, 30, 40, 90, 70, 55], M.ACCEPTED, dict(best=40, second=55, ncand=7,
                                                            skipped=3))):
        u, v = b.site()
        c = b.new_code()
        ks = [flip(c, d) for d in dists]       # nested flips: k_q and k_r are |d_q - d_r| apart
        js = [b.kp(u - 3.0 + q, v, 0, k) for q, k in enumerate(ks)]
        for q in range(3):
            b.mp(u, v, ks[q], expect=M.ACCEPTED, kp=js[q], best=0)
        b.mp(u, v, c, expect=exp, kp=js[3] if exp == M.ACCEPTED else -1, **tr)
    return b.done()


def local_domino(nchain=134):
    """last_domino for the local matcher: radius 4.0 * 0.75 = 3 at level 0"""
    b = LocalBuilder("domino", th=0.75)
    c = b.new_code()
    pos = _domino_geometry(nchain)
    js = [b.kp(x - 0.5, y, 0, flip(c, i // 2)) for i, (x, y) in enumerate(pos)]
    b.mp(pos[0][0] - 3.0, pos[0][1], c, expect=M.ACCEPTED, kp=js[0])
    for i in range(nchain):
        b.mp(pos[i][0], pos[i][1], c, expect=M.ACCEPTED, kp=js[i + 1], skipped=1)
    return b.done()


def local_window(edge):
    """two points at map indices edge - 1 | edge that want one keypoint (the
    kernel lists the in-view points 4 * 1024 or 4 * 2048 at a time)"""
    b = LocalBuilder(f"window_{edge}")
    u, v = b.site()
    c = b.new_code()
    j = b.kp(u, v, 0, c)
    j2 = b.kp(u + 1.0, v, 0, flip(c, 50))
    b.fill(edge - 1)
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j, best=0, second=50)
    b.mp(u, v, c, expect=M.ACCEPTED, kp=j2, best=50, second=256)
    b.fill(edge + 3)
    b.mp(u, v, c, expect=M.ALL_CLAIMED)
    return b.done()


def local_sizes():
    b = LocalBuilder("no_keypoints")
    b.mp(100.0, 100.0, b.new_code(), expect=M.NO_WINDOW)
    b2 = LocalBuilder("no_points")
    b2.kp(100.0, 100.0)
    return [b.done(), b2.done()]


@functools.lru_cache(maxsize=1)
def local_cases():
    out = [local_visibility(1.0), local_visibility(3.0), local_levels_gates(), local_no_cur_nobs(),
           local_best_second(), local_ratio(), local_claims(), local_exhaustion(), local_domino(),
           local_window(4096), pad_keypoints(local_window(8192), 1025)]
    out += local_sizes()
    out += [pad_keypoints(local_claims(), 2048), pad_keypoints(local_domino(), 1025)]
    return out


# ==========================================================================
# SearchByBoW(KeyFrame, Frame)
# ==========================================================================
class BowBuilder(_Codes):
    def __init__(self, name, nnratio=0.7, check_ori=True):
        super().__init__()
        self.name, self.nnratio, self.check_ori = name, nnratio, check_ori
        self.kf, self.f, self.expect = [], [], {}
        self._node = 10

    def node(self):
        self._node += 3
        return self._node

    def F(self, node, desc, angle=0.0):
        self.f.append((node, desc, angle))
        return len(self.f) - 1

    def K(self, node, desc, angle=0.0, valid=1, expect=None, **trace):
        self.kf.append((node, desc, angle, valid))
        i = len(self.kf) - 1
        if expect is not None:
            self.expect[i] = dict(reason=expect, **trace)
        return i

    def pair(self, rot=0.0, cut=False, bin_=None):
        n = self.node()
        c = self.new_code()
        j = self.F(n, c, angle=0.0 if rot >= 0 else -rot)
        tr = {} if bin_ is None else dict(bin=bin_ if self.check_ori else -1)
        self.K(n, c, angle=max(rot, 0.0),
               expect=M.ROT_CUT if cut and self.check_ori else M.ACCEPTED, kp=j, **tr)

    def done(self):
        def cols(rows, k, dt):
            return np.array([r[k] for r in rows], dt)
        args = dict(kf_node=cols(self.kf, 0, np.int32), kf_valid=cols(self.kf, 3, np.uint8),
                    kf_desc=_desc([r[1] for r in self.kf]), kf_angle=cols(self.kf, 2, f32),
                    f_node=cols(self.f, 0, np.int32), f_desc=_desc([r[1] for r in self.f]),
                    f_angle=cols(self.f, 2, f32), nnratio=self.nnratio, check_ori=self.check_ori)
        return Problem("bow", self.name, args, self.expect)


def bow_membership(check_ori=False):
    b = BowBuilder("membership", check_ori=check_ori)
    c = b.new_code()
    b.F(-1, c)
    b.K(-1, c, expect=M.NO_NODE)
    b.K(b.node(), c, expect=M.NODE_UNSHARED)       # a node of the keyframe alone
    b.F(b.node(), c)                               # a node of the frame alone
    n = b.node()
    j = b.F(n, c)
    b.K(n, c, valid=0, expect=M.NO_MP)
    b.K(n, c, expect=M.ACCEPTED, kp=j)
    # node ids 0 and 2^21 - 2
    for n in (0, (1 << 21) - 2):
        c = b.new_code()
        j = b.F(n, c)
        b.K(n, c, expect=M.ACCEPTED, kp=j)
    # 50 and 51; a single frame feature in the node
    for d, exp in ((50, M.ACCEPTED), (51, M.OVER_TH)):
        n = b.node()
        c = b.new_code()
        j = b.F(n, flip(c, d))
        b.K(n, c, expect=exp, kp=j if exp == M.ACCEPTED else -1, best=d, second=256)
    # the strict ratio: 0.7f * 50 = 35.0f, 35 is not below it
    for bd, exp in ((35, M.RATIO_REJECT), (34, M.ACCEPTED), (36, M.RATIO_REJECT)):
        n = b.node()
        c = b.new_code()
        j = b.F(n, flip(c, bd))
        b.F(n, flip(c, 50, 100))
        b.K(n, c, expect=exp, kp=j if exp == M.ACCEPTED else -1, best=bd, second=50)
    # ties by index: the lower frame index is the best, the other the second (10 < 0.7 * 10 fails)
    n = b.node()
    c = b.new_code()
    b.F(n, flip(c, 10))
    b.F(n, flip(c, 10, 100))
    b.K(n, c, expect=M.RATIO_REJECT, best=10, second=10)
    # distance 256: sets neither slot
    n = b.node()
    c = b.new_code()
    b.F(n, flip(c, 256))
    b.K(n, c, expect=M.NO_CANDIDATE, best=256)
    n = b.node()
    c = b.new_code()
    b.F(n, flip(c, 256))
    j = b.F(n, flip(c, 20))
    b.K(n, c, expect=M.ACCEPTED, kp=j, best=20, second=256)
    return b.done()


def bow_runs():
    """runs of 4, 5 and 6 frame features (one of the 6 at 256) with two and
    three of the four best claimed by earlier keyframe features of the node"""
    b = BowBuilder("runs", check_ori=False)
    for dists, nclaim, exp, tr in (
            ([5, 6, 20, 40], 2, M.ACCEPTED, dict(best=20, second=40, skipped=2)),
            ([5, 6, 7, 40], 3, M.ACCEPTED, dict(best=40, second=256, skipped=3)),
            ([5, 6, 20, 40, 41], 2, M.ACCEPTED, dict(best=20, second=40, skipped=2)),
            # three claimed: the fifth (41) is the second after the re-scan, 40 < 0.7 * 41 fails
            ([5, 6, 7, 40, 41], 3, M.RATIO_REJECT, dict(best=40, second=41, skipped=3)),
            ([5, 6, 20, 40, 41, 45], 2, M.ACCEPTED, dict(best=20, second=40, skipped=2)),
            ([5, 6, 7, 25, 256, 41], 3, M.ACCEPTED, dict(best=25, second=41, skipped=3)),
            ([41, 256, 7, 6, 5, 25], 3, M.ACCEPTED, dict(best=25, second=41, skipped=3)),
            ([5, 6, 7, 8], 4, M.ALL_CLAIMED, dict(skipped=4))):
        n = b.node()
        c = b.new_code()
        ks = [flip(c, d) for d in dists]       # nested flips: k_q and k_r are |d_q - d_r| apart
        js = [b.F(n, k) for k in ks]
        order = sorted(range(len(dists)), key=lambda q: (dists[q], q))
        for q in order[:nclaim]:
            b.K(n, ks[q], expect=M.ACCEPTED, kp=js[q], best=0)
        b.K(n, c, expect=exp, kp=js[order[nclaim]] if exp == M.ACCEPTED else -1, **tr)
    return b.done()


def bow_large_node(nk=300, nf=300, seed=9):
    """one node holding 300 x 300 features: descriptors from four codes with
    0..3 flipped bits, so most keyframe features find their best ones taken"""
    rng = np.random.default_rng(seed)
    b = BowBuilder("large_node", check_ori=True)
    pool = [b.new_code() for _ in range(4)]

    def draw():
        d = pool[int(rng.integers(0, 4))].copy()
        for bit in rng.choice(256, int(rng.integers(0, 4)), replace=False):
            d[bit // 8] ^= 1 << (bit % 8)
        return d
    for _ in range(nf):
        b.F(7, draw(), angle=float(rng.integers(0, 4)) * 45.0)
    for _ in range(nk):
        b.K(7, draw(), angle=float(rng.integers(0, 6)) * 45.0)
    return b.done()


def bow_sizes(nkf):
    """nkf keyframe features (the sort sizes 64 / 128 / 2048) in nodes of four,
    frame features in reverse node order; the last index is matched"""
    b = BowBuilder(f"nkf{nkf}", check_ori=False)
    codes = [code(1 + q % 255) for q in range(nkf)]
    for i in range(nkf):
        b.K(100 + i // 4, flip(codes[i], i % 3), expect=M.ACCEPTED, kp=nkf - 1 - i)
    for i in reversed(range(nkf)):
        b.F(100 + i // 4, codes[i])
    return b.done()


def bow_wide_frame(nf=2048):
    """2048 frame features in nodes of four against three keyframe features:
    the sort size by the frame's count alone, frame indices 0, 1024 and 2047"""
    b = BowBuilder(f"nf{nf}", check_ori=False)
    codes = [code(1 + q % 255) for q in range(nf)]
    for j in range(nf):
        b.F(200 + j // 4, codes[j])
    for j in (nf - 1, 1024, 0):
        b.K(200 + j // 4, flip(codes[j], 3), expect=M.ACCEPTED, kp=j, best=3)
    return b.done()


def bow_rotation():
    out = []
    for name, groups in (
            ("rot_bins", [(-10.0, 1, True, 29), (6.0, 2, False, 1), (18.0, 2, False, 2),
                          (359.0, 2, False, 0), (0.0, 1, False, 0)]),
            ("rot_equal", [(120.0, 2, False, 10), (24.0, 2, False, 2), (240.0, 2, True, 20),
                           (60.0, 2, False, 5)]),
            ("rot_tenth_on", [(0.0, 10, False, 0), (48.0, 1, False, 4), (96.0, 1, False, 8)]),
            ("rot_tenth_below", [(0.0, 11, False, 0), (48.0, 1, True, 4), (96.0, 1, True, 8)]),
            ("rot_tenth_third", [(0.0, 20, False, 0), (48.0, 2, False, 4), (96.0, 1, True, 8)])):
        for check in (True, False) if name == "rot_bins" else (True,):
            b = BowBuilder(name + ("" if check else "_off"), check_ori=check)
            for rot, count, cut, bin_ in groups:
                for _ in range(count):
                    b.pair(rot, cut, bin_)
            out.append(b.done())
    b = BowBuilder("rot_empty")
    n = b.node()
    c = b.new_code()
    b.F(n, flip(c, 51))
    b.K(n, c, expect=M.OVER_TH)
    out.append(b.done())
    return out


def bow_empty():
    b = BowBuilder("no_frame_features")
    b.K(3, b.new_code(), expect=M.NODE_UNSHARED)
    b2 = BowBuilder("no_keyframe_features")
    b2.F(3, b2.new_code())
    return [b.done(), b2.done()]


@functools.lru_cache(maxsize=1)
def bow_cases():
    return [bow_membership(False), bow_runs(), bow_large_node(), bow_sizes(1), bow_sizes(64),
            bow_sizes(65), bow_sizes(2048), bow_wide_frame()] + bow_rotation() + bow_empty()


# ==========================================================================
# crowds: seeded contention
# ==========================================================================
def _pool_desc(rng, pool):
    d = pool[int(rng.integers(0, len(pool)))].copy()
    for bit in rng.choice(256, int(rng.integers(0, 4)), replace=False):
        d[bit // 8] ^= 1 << (bit % 8)
    return d


def _crowd_keypoints(rng, nk, pool, cx, cy, octaves):
    k = np.zeros(nk, KP)
    k["x"] = (cx + rng.uniform(-15, 15, nk)).astype(f32)
    k["y"] = (cy + rng.uniform(-15, 15, nk)).astype(f32)
    k["octave"] = rng.choice(octaves, nk)
    k["angle"] = rng.integers(0, 5, nk) * 40.0
    k["size"], k["response"], k["class_id"] = 31.0, 20.0, -1
    return k, _desc([_pool_desc(rng, pool) for _ in range(nk)])


def crowd_last(seed):
    """48-96 keypoints in a 30 px patch, 150-300 points projecting into it,
    descriptors from six codes with 0-3 flipped bits, mixed observations"""
    rng = np.random.default_rng(seed)
    nk, npt = int(rng.integers(48, 97)), int(rng.integers(150, 301))
    pool = [code(q) for q in range(1, 7)]
    kps, desc = _crowd_keypoints(rng, nk, pool, 320.0, 240.0, [0, 1])
    ur = np.where(rng.random(nk) < 0.3, kps["x"] - 32.0 + rng.uniform(-9, 9, nk), -1.0)
    u = 320.0 + rng.integers(-40, 41, npt) * 0.25
    v = 240.0 + rng.integers(-40, 41, npt) * 0.25
    xyz = np.stack([(u - 320.0) / 256.0, (v - 240.0) / 256.0, np.full(npt, 2.0)], 1)
    lk = np.zeros(npt, KP)
    lk["octave"] = rng.integers(0, 2, npt)
    lk["angle"] = rng.integers(0, 5, npt) * 40.0
    last = dict(Tcw=np.eye(4, dtype=f32), kps_un=lk,
                has_mp=(rng.random(npt) < 0.95).astype(np.uint8),
                outlier=(rng.random(npt) < 0.05).astype(np.uint8), mp_xyz=xyz.astype(f32),
                mp_desc=_desc([_pool_desc(rng, pool) for _ in range(npt)]),
                mp_nobs=rng.integers(0, 3, npt).astype(np.int32))
    cur = dict(Tcw=np.eye(4, dtype=f32), kps_un=kps, desc=desc, uright=ur.astype(f32))
    return Problem("last", f"crowd{seed}", dict(cur=cur, last=last, th=7.0, mono=False,
                                                 check_ori=True))


def crowd_local(seed):
    rng = np.random.default_rng(seed)
    nk, npt = int(rng.integers(48, 97)), int(rng.integers(150, 301))
    pool = [code(q) for q in range(1, 7)]
    kps, desc = _crowd_keypoints(rng, nk, pool, 320.0, 240.0, [0, 1, 2])
    ur = np.where(rng.random(nk) < 0.3, kps["x"] - 32.0, -1.0)
    x = 320.0 + rng.integers(-40, 41, npt) * 0.25
    track = dict(in_view=(rng.random(npt) < 0.95).astype(np.uint8), proj_x=x.astype(f32),
                 proj_y=(240.0 + rng.integers(-40, 41, npt) * 0.25).astype(f32),
                 proj_xr=(x - 32.0 + rng.uniform(-14, 14, npt)).astype(f32),
                 level=rng.integers(0, 3, npt).astype(np.int32),
                 view_cos=rng.choice([0.5, 0.999], npt).astype(f32))
    cur = dict(kps_un=kps, desc=desc, uright=ur.astype(f32))
    return Problem("local", f"crowd{seed}", dict(
        cur=cur, track=track, mp_desc=_desc([_pool_desc(rng, pool) for _ in range(npt)]),
        mp_nobs=rng.integers(0, 3, npt).astype(np.int32),
        cur_nobs=(rng.random(nk) < 0.05).astype(np.int32), th=3.0, nnratio=0.8))


def crowd_bow(seed):
    rng = np.random.default_rng(seed)
    nf, nk = int(rng.integers(48, 97)), int(rng.integers(150, 301))
    pool = [code(q) for q in range(1, 7)]
    f_desc = _desc([_pool_desc(rng, pool) for _ in range(nf)])
    # most keyframe features repeat a frame feature's draw: the first of them
    # passes the ratio test and claims it, the later ones find their best ones taken
    kf_desc = _desc([f_desc[int(rng.integers(0, nf))] if rng.random() < 0.7
                     else _pool_desc(rng, pool) for _ in range(nk)])
    args = dict(kf_node=rng.choice([5, 5, 5, 9], nk).astype(np.int32),
                kf_valid=(rng.random(nk) < 0.95).astype(np.uint8), kf_desc=kf_desc,
                kf_angle=(rng.integers(0, 5, nk) * 40.0).astype(f32),
                f_node=rng.choice([5, 5, 5, 9], nf).astype(np.int32),
                f_desc=f_desc,
                f_angle=(rng.integers(0, 5, nf) * 40.0).astype(f32), nnratio=0.9, check_ori=True)
    return Problem("bow", f"crowd{seed}", args)


def crowd_kf(seed):
    rng = np.random.default_rng(seed)
    nk, npt = int(rng.integers(48, 97)), int(rng.integers(150, 301))
    pool = [code(q) for q in range(1, 7)]
    kps, desc = _crowd_keypoints(rng, nk, pool, 320.0, 240.0, [0, 1])
    u = 320.0 + rng.integers(-40, 41, npt) * 0.25
    v = 240.0 + rng.integers(-40, 41, npt) * 0.25
    xyz = np.stack([(u - 320.0) / 256.0, (v - 240.0) / 256.0, np.full(npt, 2.0)], 1).astype(f32)
    kf = dict(angle=(rng.integers(0, 5, npt) * 40.0).astype(f32),
              valid=(rng.random(npt) < 0.95).astype(np.uint8),
              found=(rng.random(npt) < 0.05).astype(np.uint8), mp_xyz=xyz,
              mp_min_dist=np.full(npt, 1.0, f32), mp_max_dist=np.full(npt, 2.2, f32),
              mp_desc=_desc([_pool_desc(rng, pool) for _ in range(npt)]))
    cur = dict(Tcw=np.eye(4, dtype=f32), kps_un=kps, desc=desc)
    return Problem("kf", f"crowd{seed}", dict(cur=cur, cur_has_mp=(rng.random(nk) < 0.05)
                                               .astype(np.uint8), kf=kf, th=10.0, orb_dist=100,
                                               check_ori=True))


CROWD_SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=1)
def crowds():
    return {"last": [crowd_last(s) for s in CROWD_SEEDS],
            "local": [crowd_local(s) for s in CROWD_SEEDS],
            "bow": [crowd_bow(s) for s in CROWD_SEEDS],
            "kf": [crowd_kf(s) for s in CROWD_SEEDS]}


def all_problems(kind):
    cases = {"last": last_cases, "local": local_cases, "bow": bow_cases, "kf": lambda: []}[kind]()
    return list(cases) + crowds()[kind]

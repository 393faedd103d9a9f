"""Hand-built key lines for tests/test_line_ref.py (CPU) and
tests/test_gpu_line_cases.py (GPU): one case per branch of the line code that
tests/_line_ref.py restates, and seeded crowds.

The camera is distortion-free 640x480 with fx = fy = 512 and integer cx, cy;
a map line is given by the pixels it shall project to and a depth that is a
power of two, its world coordinates are (u - cx) * z / fx, so the float
products of the projection are exact and a line meant for x = 100 is at 100.
Every case still asserts its own projected end points (expect["proj"]).
Descriptors are Hadamard codewords (128 bits apart) with bits flipped to an
exact Hamming distance.

A search problem is run through the last-frame, list and both harness entries
alike (ENTRIES); `expect` holds what the case was built for:
  codes   {map line: projection code}
  proj    {map line: (sx, sy, ex, ey) of its projected KeyLine}
  reasons {(pass, map line, current line): LineMatching reason or (reason, overlap exit)}
  match   {entry: [match per current line]}     nm {entry: count}
  retry   {entry: bool}
"""
import ctypes as C
import functools
import math

import numpy as np

import _line_ref as R
from _stereo_cases import code, flip

f32 = np.float32
KL = R.KL
CAM = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0,
           bf=40.0, thdepth=40.0, width=640, height=480)
TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989,
            k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628, k3=1.163314,
            width=640, height=480, bf=40.0, thdepth=40.0)
NEG_K1 = dict(TUM1, k1=-0.2, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
K2_ONLY = dict(TUM1, k1=0.0)            # k1 == 0 with k2 != 0: no undistortion (Frame.cc:771)
EYE = np.eye(4, dtype=f32)
ENTRIES = ("last", "list", "pairs0", "pairs1")
FILL_ML, FILL_CUR = code(254), code(253)
S = -7                                   # the sentinel around capacity-bound outputs
UP = f32(np.inf)


def above(x):
    return float(np.nextafter(f32(x), UP))


def below(x):
    return float(np.nextafter(f32(x), -UP))


def keyline(sx, sy, ex, ey, W=640, H=480, **over):
    """a KeyLine with these end points, its derived fields as UpdateKeyLineData
    sets them, then `over`"""
    k = np.zeros(1, KL)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = sx, sy, ex, ey
    R.update_keyline(k, W, H)
    for f, v in over.items():
        k[f] = v
    return k[0]


def unproject(u, v, z, cam=CAM):
    return [f32(f32(u - cam["cx"]) * f32(z) / f32(cam["fx"])),
            f32(f32(v - cam["cy"]) * f32(z) / f32(cam["fy"])), f32(z)]


class Search:
    """inputs of the four searches; build with ml() / ml_px() / cur(), then done()"""
    kind = "search"

    def __init__(self, name, cam=CAM, Tcw=EYE, entries=ENTRIES, pair_cap=None):
        self.name, self.cam, self.Tcw, self.entries, self.pair_cap = name, cam, Tcw, entries, pair_cap
        self._ml, self._cur, self._ncode = [], [], 0
        self.expect = dict(codes={}, proj={}, reasons={}, match={}, nm={}, retry={})

    def __repr__(self):
        return f"search:{self.name}"

    def new_code(self):
        self._ncode += 1
        assert self._ncode <= 252
        return code(self._ncode)

    def ml(self, X6, desc=FILL_ML, has=1, outlier=0, nobs=0):
        i = len(self._ml)
        base = keyline(1.0, 2.0, 3.0, 5.0, class_id=100 + i, octave=1)
        self._ml.append((np.array(X6, f32), desc, has, outlier, nobs, base))
        return i

    def ml_px(self, u0, v0, u1, v1, desc=FILL_ML, z0=2.0, z1=2.0, **kw):
        return self.ml(unproject(u0, v0, z0, self.cam) + unproject(u1, v1, z1, self.cam), desc, **kw)

    def cur(self, seg, desc=FILL_CUR, nobs=0, **over):
        self._cur.append((keyline(*seg, **over), desc, nobs))
        return len(self._cur) - 1

    def proj(self, i):
        """the projected KeyLine of map line i, by the restatement"""
        ok, k, _ = R.project_map_line(self.cam, self.Tcw, self._ml[i][0])
        assert ok, (self.name, i)
        return k

    def site(self, seg, cur_seg=None, dist=0, z=2.0, nobs=0, ml_nobs=0, **over):
        """a map line projecting to seg and a current line on cur_seg (seg when None) whose
        descriptors are `dist` apart: (map line, current line)"""
        c = self.new_code()
        i = self.ml_px(*seg, desc=c, z0=z, z1=z, nobs=ml_nobs)
        j = self.cur(cur_seg or seg, flip(c, dist), nobs=nobs, **over)
        return i, j

    def set_pose(self, Tcw):
        """the map lines given so far were placed in the camera frame: move them to the
        world of this pose (rounded to float, so the projections are no longer exact)"""
        T = np.asarray(Tcw, np.float64)
        Rm, t = T[:3, :3], T[:3, 3]
        for q, x in enumerate(self._ml):
            X = np.concatenate([Rm.T @ (x[0][:3].astype(np.float64) - t),
                                Rm.T @ (x[0][3:].astype(np.float64) - t)]).astype(f32)
            self._ml[q] = (X,) + x[1:]
        self.Tcw = np.asarray(Tcw, f32)

    def done(self):
        n, m = len(self._cur), len(self._ml)
        self.cur_kl = np.array([c[0] for c in self._cur], KL) if n else np.zeros(0, KL)
        self.cur_desc = np.array([c[1] for c in self._cur], np.uint8).reshape(n, 32)
        self.cur_nobs = np.array([c[2] for c in self._cur], np.int32)
        self.xyz6 = np.array([x[0] for x in self._ml], f32).reshape(m, 6)
        self.ml_desc = np.array([x[1] for x in self._ml], np.uint8).reshape(m, 32)
        self.has_ml = np.array([x[2] for x in self._ml], np.uint8)
        self.outlier = np.array([x[3] for x in self._ml], np.uint8)
        self.ml_nobs = np.array([x[4] for x in self._ml], np.int32)
        self.base_kl = np.array([x[5] for x in self._ml], KL) if m else np.zeros(0, KL)
        self.valid = (self.has_ml.astype(bool) & ~self.outlier.astype(bool)).astype(np.uint8)
        if m > 80:
            self.entries = tuple(e for e in self.entries if e != "last")
        return self


class Problem:
    def __init__(self, kind, name, expect=None, **args):
        self.kind, self.name, self.expect = kind, name, expect or {}
        self.__dict__.update(args)

    def __repr__(self):
        return f"{self.kind}:{self.name}"


# --------------------------------------------------------------------------
# running a problem: every runner returns a dict of the entry's outputs
# --------------------------------------------------------------------------
def _search_out(match, nm, wiped=None, proj_kl=None, proj_src=None, pairs=None, npairs=None):
    out = dict(match=np.asarray(match, np.int32), nm=int(nm))
    if wiped is not None:
        out["wiped"] = bool(wiped)
    if proj_kl is not None:
        out.update(proj_kl=np.asarray(proj_kl, KL).tobytes(), proj_src=np.asarray(proj_src, np.int32),
                   pairs=np.asarray(pairs, np.int32).reshape(-1, 2), npairs=int(npairs))
    return out


def run_ref(P, entry=None, variants=R.NO_VARIANTS):
    """(outputs, trace) of the restatement"""
    if P.kind == "search":
        if entry == "last":
            m, n, tr = R.search_last(P.cam, P.Tcw, P.cur_kl, P.cur_desc, P.base_kl, P.has_ml,
                                     P.outlier, P.xyz6, P.ml_desc, variants)
            return _search_out(m, n), tr
        if entry == "list":
            m, n, w, tr = R.search_list(P.cam, P.Tcw, P.cur_kl, P.cur_desc, P.cur_nobs, P.valid,
                                        P.xyz6, P.ml_desc, variants)
            return _search_out(m, n, w), tr
        mode = int(entry[-1])
        m, n, w, pk, ps, pr, npr, tr = R.search_pairs(
            P.cam, P.Tcw, mode, P.cur_kl, P.cur_desc, P.cur_nobs, P.valid, P.base_kl, P.xyz6,
            P.ml_desc, P.ml_nobs, _pair_cap(P), variants)
        return _search_out(m, n, w, pk, ps, pr, npr), tr
    if P.kind == "bf":
        out, n, tr = R.match_bf_knn(P.q, P.t)
        return dict(out=out, nm=n), tr
    if P.kind == "frustum":
        v, z = R.line_in_frustum(P.Tcw, P.xyz6)
        return dict(in_view=v), z
    if P.kind == "prepare":
        ku, ds, de, us, ue = R.line_frame_prepare(P.cam, P.kl, P.depth)
        return dict(kl_un=ku.tobytes(), dstart=ds, dend=de, ur_start=us, ur_end=ue), None
    assert P.kind == "stereo"
    ds, de, tr = R.stereo_line_depths(P.cam, P.kl, P.desc, P.kr, P.desc_r)
    return dict(dstart=ds, dend=de), tr


def _pair_cap(P):
    return P.pair_cap if P.pair_cap is not None else max(1, len(P.cur_kl) * len(P.valid))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _call_pairs(fn, cam, P, mode):
    """the C entry (the oracle's or the library's: one signature) with sentinels around
    every capacity-bound output; asserts that they survive"""
    ncur, nml, cap = len(P.cur_kl), len(P.valid), _pair_cap(P)
    match = np.full(ncur + 2, S, np.int32)
    pk = np.zeros(nml + 2, KL)
    pk["class_id"] = S
    ps = np.full(nml + 2, S, np.int32)
    pairs = np.full((cap + 2, 2), S, np.int32)
    nm, wiped, npj, npr = C.c_int(S), C.c_int(S), C.c_int(S), C.c_int(S)
    keep = [np.ascontiguousarray(a) for a in (P.Tcw, P.cur_kl, P.cur_desc, P.cur_nobs, P.valid,
                                              P.base_kl, P.xyz6, P.ml_desc, P.ml_nobs)]
    rc = fn(C.byref(cam), _p(keep[0]), mode, ncur, _p(keep[1]), _p(keep[2]), _p(keep[3]), nml,
            _p(keep[4]), _p(keep[5]), _p(keep[6]), _p(keep[7]), _p(keep[8]), _p(pk), _p(ps),
            C.byref(npj), _p(pairs), cap, C.byref(npr), _p(match), C.byref(nm), C.byref(wiped))
    assert rc == 0, rc
    k = min(npr.value, cap)
    assert np.all(match[ncur:] == S) and np.all(ps[npj.value:] == S), "sentinel overwritten"
    assert np.all(pk["class_id"][npj.value:] == S) and np.all(pairs[k:] == S), "sentinel overwritten"
    return _search_out(match[:ncur], nm.value, wiped.value, pk[:npj.value], ps[:npj.value], pairs[:k],
                       npr.value)


def run_oracle(O, P, entry=None):
    if P.kind == "search":
        cam = O.camera(P.cam)
        if entry == "last":
            return _search_out(*O.line_search_by_projection_last(
                cam, P.Tcw, P.cur_kl, P.cur_desc, P.base_kl, P.has_ml, P.outlier, P.xyz6, P.ml_desc))
        if entry == "list":
            return _search_out(*O.line_search_by_projection_list(
                cam, P.Tcw, P.cur_kl, P.cur_desc, P.cur_nobs, P.valid, P.xyz6, P.ml_desc))
        return _call_pairs(O.lib().oracle_line_search_pairs, cam, P, int(entry[-1]))
    if P.kind == "bf":
        out, n = O.line_match_bf_knn(P.q, P.t)
        return dict(out=out, nm=n)
    if P.kind == "frustum":
        return dict(in_view=O.line_is_in_frustum(P.Tcw, P.xyz6))
    if P.kind == "prepare":
        ku, ds, de, us, ue = O.line_frame_prepare(O.camera(P.cam), P.kl, P.depth)
        return dict(kl_un=ku.tobytes(), dstart=ds, dend=de, ur_start=us, ur_end=ue)
    ds, de = O.stereo_line_depths(O.camera(P.cam), P.kl, P.desc, P.kr, P.desc_r)
    return dict(dstart=ds, dend=de)


def run_gpu(orbpl, P, entry=None):
    if P.kind == "search":
        cam = orbpl.make_camera(P.cam)
        LM = orbpl.LineMatcher
        if entry == "last":
            return _search_out(*LM.SearchByProjectionLastFrame(
                cam, P.Tcw, P.cur_kl, P.cur_desc, P.base_kl, P.has_ml, P.outlier, P.xyz6, P.ml_desc))
        if entry == "list":
            return _search_out(*LM.SearchByProjectionLocalMap(
                cam, P.Tcw, P.cur_kl, P.cur_desc, P.cur_nobs, P.valid, P.xyz6, P.ml_desc))
        return _call_pairs(orbpl.lib().orbl_search_by_projection_pairs, cam, P, int(entry[-1]))
    if P.kind == "bf":
        out, n = orbpl.LineMatcher.MatchBFKnn(P.q, P.t)
        return dict(out=out, nm=n)
    if P.kind == "frustum":
        return dict(in_view=orbpl.line_is_in_frustum(P.Tcw, P.xyz6))
    if P.kind == "prepare":
        ku, ds, de, us, ue = orbpl.line_frame_prepare(orbpl.make_camera(P.cam), P.kl, P.depth)
        return dict(kl_un=ku.tobytes(), dstart=ds, dend=de, ur_start=us, ur_end=ue)
    ds, de = orbpl.stereo_line_depths(orbpl.make_camera(P.cam), P.kl, P.desc, P.kr, P.desc_r)
    return dict(dstart=ds, dend=de)


def differences(a, b):
    """names of the outputs that differ bit for bit (floats by their bit patterns)"""
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            if x.shape != y.shape or x.tobytes() != np.asarray(y, x.dtype).tobytes():
                bad.append(k)
        elif x != y:
            bad.append(k)
    return bad


# --------------------------------------------------------------------------
# projection and clipping
# --------------------------------------------------------------------------
def _fill(b, n_ok=0):
    """`n_ok` sites that match exactly, far from everything else (to steer the retry rule)"""
    for q in range(n_ok):
        b.site((400.0 + 10 * q, 300.0, 430.0 + 10 * q, 420.0))


def projection_cases():
    b = Search("projection")
    e = b.expect
    rows = [  # name, pixels of the map line, code, projected KeyLine
        ("inside", (100, 100, 200, 180), "IN_FRONT/LB_OK", (100, 100, 200, 180)),
        ("left", (-50, 100, 50, 200), "IN_FRONT/LB_OK", (0, 150, 50, 200)),
        ("right", (600, 100, 700, 200), "IN_FRONT/LB_OK", (600, 100, 640, 140)),
        ("top", (100, -50, 200, 50), "IN_FRONT/LB_OK", (150, 0, 200, 50)),
        ("bottom", (100, 440, 180, 520), "IN_FRONT/LB_OK", (100, 440, 140, 480)),
        ("corner_cut", (-20, 30, 40, -30), "IN_FRONT/LB_OK", (0, 10, 10, 0)),
        ("outside", (-100, -100, -50, -20), "IN_FRONT/LB_OUTSIDE", None),
        ("outside_past_corner", (-30, 10, 10, -40), "IN_FRONT/LB_OUTSIDE", None),
        ("vertical", (100, 100, 100, 200), "IN_FRONT/LB_OK", (100, 100, 100, 200)),
        ("vertical_up", (120, 200, 120, 0), "IN_FRONT/LB_OK", (120, 200, 120, 0)),
        ("vertical_through_bottom", (140, 400, 140, 500), "IN_FRONT/LB_OK", (140, 400, 140, 480)),
        ("vertical_at_minX", (0, 100, 0, 200), "IN_FRONT/LB_VERTICAL_REJECT", None),
        ("vertical_start_at_minY", (160, 0, 160, 200), "IN_FRONT/LB_VERTICAL_REJECT", None),
        ("vertical_start_above", (180, -10, 180, 50), "IN_FRONT/LB_VERTICAL_REJECT", None),
        ("vertical_right_of_maxX", (650, 100, 650, 200), "IN_FRONT/LB_OUTSIDE", None),
        ("horizontal", (100, 220, 300, 220), "IN_FRONT/LB_HORIZONTAL_REJECT", None),
        ("horizontal_outside", (100, -20, 300, -20), "IN_FRONT/LB_HORIZONTAL_REJECT", None),
        ("half_up", (-5, 100, 5, 103), "IN_FRONT/LB_OK", (0, 102, 5, 103)),
        ("half_down", (-5, 103, 5, 100), "IN_FRONT/LB_OK", (0, 101, 5, 100)),
        ("half_end_up", (635, 300, 645, 303), "IN_FRONT/LB_OK", (635, 300, 640, 302)),
        ("half_end_down", (635, 303, 645, 300), "IN_FRONT/LB_OK", (635, 303, 640, 301)),
    ]
    b.names = {}
    for name, px, cd, seg in rows:
        c = b.new_code()
        i = b.ml_px(*[float(v) for v in px], desc=c)
        b.names[name] = i
        if name in ("horizontal", "vertical_start_at_minY"):
            # a current line where a clipping that kept the line would put it
            b.cur(tuple(float(v) for v in px), c)
        e["codes"][i] = cd
        if seg is not None:
            seg = tuple(float(v) for v in seg)
            e["proj"][i] = seg
            j = b.cur(seg, c)
            e["reasons"][(0, i, j)] = R.OK
    # depth: behind the camera, on its plane
    c = b.new_code()
    xe = unproject(200.0, 180.0, 2.0)
    i = b.ml([0.5, 0.25, -2.0] + xe, c)
    b.names["start_behind"] = i
    e["codes"][i] = "START_BEHIND/LB_OK"
    # lambda = -0.5: the crossing point is the mid point, in camera coordinates (metres)
    # LiangBarsky adds the ROUNDED extent to the start, so the end moves by the start's fraction
    xc, yc = (0.5 + float(xe[0])) / 2, (0.25 + float(xe[1])) / 2
    e["proj"][i] = (xc, yc, xc + 200.0, yc + 180.0)
    j = b.cur(e["proj"][i], c)
    e["reasons"][(0, i, j)] = R.OK
    c = b.new_code()
    xs = unproject(300.0, 100.0, 4.0)
    i = b.ml(xs + [1.0, 0.5, -4.0], c)
    b.names["end_behind"] = i
    e["codes"][i] = "END_BEHIND/LB_OK"
    # the crossing (0.421875, -0.296875) lies above the image: p[2] = 100.296875, q[2] = 100,
    # u_max = 0.99704: end = (300 + round(-298.69), 100 + round(-100.0))
    assert ((float(xs[0]) + 1.0) / 2, (float(xs[1]) + 0.5) / 2) == (0.421875, -0.296875)
    e["proj"][i] = (300.0, 100.0, 1.0, 0.0)
    j = b.cur(e["proj"][i], c)
    e["reasons"][(0, i, j)] = R.OK
    for name, zs, ze, cd in (("both_behind", -2.0, -1.0, "BOTH_BEHIND"),
                             ("z0_start", 0.0, 2.0, "NO_BRANCH"), ("z0_end", 2.0, 0.0, "NO_BRANCH"),
                             ("z0_both", 0.0, 0.0, "NO_BRANCH")):
        i = b.ml([0.1, 0.1, zs, 0.3, 0.2, ze], b.new_code())
        b.names[name] = i
        e["codes"][i] = cd
    # flags
    for name, kw in (("no_map_line", dict(has=0)), ("outlier", dict(outlier=1))):
        c = b.new_code()
        i = b.ml_px(300.0, 300.0, 380.0, 400.0, desc=c, **kw)
        b.names[name] = i
        e["codes"][i] = "INVALID"
    b.cur((300.0, 300.0, 380.0, 400.0), c)        # would match the outlier
    return b.done()


def corner_touch():
    """a line through the corner (0, 0) from outside to outside: u_max == u_min, a
    zero-length KeyLine (length 0, angle atan2(0, 0) = 0). Against a current line: the length
    ratio is 0 (LENGTH), or 0 / 0 = NaN with a current lineLength of 0, which is not < 0.45,
    so the pair goes on to LineOverLap, whose quotients are then 0 / 0 or -x / 0: OVERLAP."""
    b = Search("corner_touch")
    c = b.new_code()
    i = b.ml_px(-10.0, 10.0, 10.0, -10.0, desc=c)
    b.expect["codes"][i] = "IN_FRONT/LB_OK"
    b.expect["proj"][i] = (0.0, 0.0, 0.0, 0.0)
    j0 = b.cur((0.0, 0.0, 10.0, 1.0), c)
    j1 = b.cur((0.0, 0.0, 10.0, 1.0), c, lineLength=0.0)
    j2 = b.cur((0.0, 0.0, 0.0, 0.0), c)
    b.expect["reasons"].update({(0, i, j0): R.LENGTH, (0, i, j1): (R.OVERLAP, R.OV_NONE),
                                (0, i, j2): (R.OVERLAP, R.OV_NONE),
                                (1, i, j0): R.LENGTH, (1, i, j1): (R.OVERLAP, R.OV_NONE)})
    return b.done()


def distorted_camera(name, cam):
    """the image bounds are the undistorted corners. TUM1's coefficients pull them INTO the
    image (about 10.8, 14.7, 626.0, 473.3: non-integer, positive); NEG_K1 pushes them out, to
    non-integer negative minX and minY. The map lines cross each bound."""
    b = Search("distorted_" + name, cam=cam)
    bd = R.image_bounds(cam)
    assert all(v != round(v) for v in bd)
    assert (bd[0] < 0 and bd[1] < 0 and bd[2] > 640 and bd[3] > 480) == (cam is NEG_K1)
    for px in ((-80, 100, 60, 220), (100, -70, 200, 60), (600, 300, 720, 420), (300, 440, 380, 560),
               (-40, -20, 30, 40), (200, 200, 300, 320), (-30.0, 100, -30.0, 300)):
        c = b.new_code()
        i = b.ml_px(*[float(v) for v in px], desc=c)
        ok, k, cd = R.project_map_line(cam, EYE, b._ml[i][0])
        if ok:
            b.expect["codes"][i] = "IN_FRONT/LB_OK"
            b.cur(tuple(float(k[f]) for f in ("startPointX", "startPointY", "endPointX", "endPointY")), c)
    assert len(b._cur) >= 5
    return b.done()


# --------------------------------------------------------------------------
# LineMatching thresholds
# --------------------------------------------------------------------------
def _angle_with_diff(a1, d):
    """a float a2 with |float(a1 - a2)| == d exactly"""
    for start in (R.r32(a1 - d), R.r32(a1 + d)):
        x = start
        for _ in range(4):
            x = below(x)
        for _ in range(9):
            if abs(R.r32(a1 - x)) == d:
                return x
            x = above(x)
    raise AssertionError((a1, d))


def _length_pair(L1, th, proj_shorter):
    """two adjacent floats for the current lineLength: (passes, fails) ratio >= th"""
    L = R.r32(L1 / th) if proj_shorter else R.r32(L1 * th)

    def ratio(x):
        return R.fdiv(min(L1, x), max(L1, x))
    step_fail = above if proj_shorter else below
    step_pass = below if proj_shorter else above
    while ratio(L) < th:
        L = step_pass(L)
    while ratio(step_fail(L)) >= th:
        L = step_fail(L)
    return L, step_fail(L)


def threshold_cases(relaxed):
    """a site on either side of every threshold of LineMatching. strict: the sides of the
    first pass's thresholds, enough sites pass for no retry. relaxed: the sides of the
    retry's thresholds, every site but two fails the first pass, so the retry runs."""
    npass = 1 if relaxed else 0
    b = Search("thresholds_relaxed" if relaxed else "thresholds_strict")
    e = b.expect
    off = R.OFF1 if relaxed else R.OFF0

    def want(ij, reason):
        e["reasons"][(npass,) + ij] = reason

    seg = (100.0, 100.0, 200.0, 180.0)
    # Hamming: 45 / 46, relaxed 50 / 51
    hd = 50 if relaxed else 45
    want(b.site(seg, dist=hd), R.OK)
    want(b.site(seg, dist=hd + 1), R.DESC)
    # angle: the float difference one float below / above 15 (25) degrees, compared in double
    T = 15.0 * R.PI / 180.0 + off[0] * R.PI / 180.0
    lo = R.r32(T) if R.r32(T) <= T else below(R.r32(T))
    i = b.ml_px(*seg, desc=b.new_code())
    a1 = float(b.proj(i)["angle"])
    for d, reason in ((lo, R.OK), (above(lo), R.ANGLE)):
        c = b.new_code()
        i = b.ml_px(*seg, desc=c)
        j = b.cur(seg, c, angle=_angle_with_diff(a1, d))
        want((i, j), reason)
    assert lo <= T < above(lo)
    # length ratio: the projected line the shorter and the longer one
    L1 = float(b.proj(i)["lineLength"])
    th = 0.45 + off[1]
    for shorter in (True, False):
        ok_len, bad_len = _length_pair(L1, th, shorter)
        for L2, reason in ((ok_len, R.OK), (bad_len, R.LENGTH)):
            want(b.site(seg, lineLength=L2), reason)
    # LineOverLap, th = 0.5 (0.4): s is the shift that puts the x (y) quotient at th
    s = 60.0 if relaxed else 50.0
    v = (100.0, 100.0, 100.0, 200.0)                       # vertical projected line
    want(b.site(v, (102.0, 100.0 + s, 102.0, 200.0 + s)), (R.OK, R.OV_VERT_Y))
    want(b.site(v, (102.0, 101.0 + s, 102.0, 201.0 + s)), (R.OVERLAP, R.OV_NONE))
    # the same x: the x quotient of the general branch is 0 / 0
    want(b.site(v, (100.0, 101.0 + s, 100.0, 201.0 + s)), (R.OVERLAP, R.OV_NONE))
    h = (100.0, 300.0, 200.0, 310.0)                       # against a horizontal current line
    want(b.site(h, (100.0 + s, 305.0, 200.0 + s, 305.0)), (R.OK, R.OV_HORZ_X))
    want(b.site(h, (101.0 + s, 305.0, 201.0 + s, 305.0)), (R.OVERLAP, R.OV_NONE))
    g = (300.0, 100.0, 400.0, 150.0)                       # the general branch
    want(b.site(g, (300.0 + s, 125.0, 400.0 + s, 175.0)), (R.OK, R.OV_X_YOVERLAP))
    want(b.site(g, (301.0 + s, 100.0 + s / 2, 401.0 + s, 150.0 + s / 2)), (R.OK, R.OV_Y_AFTER_XGAP))
    want(b.site(g, (301.0 + s, 101.0 + s / 2, 401.0 + s, 151.0 + s / 2)), (R.OVERLAP, R.OV_NONE))
    f = (300.0, 300.0, 400.0, 310.0)                       # disjoint rows, a gap of 2 and of 3
    want(b.site(f, (300.0, 312.0, 400.0, 322.0)), (R.OK, R.OV_X_YGAP_SMALL))
    want(b.site(f, (300.0, 313.0, 400.0, 323.0)), (R.OVERLAP, R.OV_NONE))
    # reprojection error: end-point distances 27 and 36 give exactly 45
    r = (500.0, 100.0, 500.0, 300.0)
    want(b.site(r, (527.0, 100.0, 536.0, 300.0)), (R.OK, R.OV_VERT_Y))
    want(b.site(r, (527.0, 100.0, above(536.0), 300.0)), R.REPROJ)
    # angles -pi + eps and pi - eps of one and the same line
    want(b.site((600.0, 400.0, 400.0, 399.0), (600.0, 399.0, 400.0, 400.0)), R.ANGLE)
    e["retry"] = {en: relaxed for en in ENTRIES}
    return b.done()


def nan_fields():
    """a current line whose angle field is NaN: |a1 - NaN| > 15 deg is false, the pair passes
    the angle gate and matches. A NaN lineLength: std::min / std::max keep their first
    argument, the ratio is L1 / L1."""
    b = Search("nan_fields")
    seg = (100.0, 100.0, 200.0, 180.0)
    nan = float("nan")
    ij = b.site(seg, angle=nan)
    b.expect["reasons"][(0,) + ij] = R.OK
    ij = b.site((300.0, 100.0, 400.0, 180.0), lineLength=nan)
    b.expect["reasons"][(0,) + ij] = R.OK
    b.expect["match"] = {en: [0, 1] for en in ENTRIES}
    return b.done()


# --------------------------------------------------------------------------
# assignment and counting
# --------------------------------------------------------------------------
def _slot(q):
    """a place of its own for group q: an oblique segment"""
    x, y = 20.0 + 60.0 * (q % 10), 20.0 + 90.0 * (q // 10)
    return (x, y, x + 40.0, y + 60.0)


def several_pass():
    """three map lines pass for current line 0 (the last wins, all count); map line 3 passes
    for current lines 1, 2 and 3"""
    b = Search("several_pass")
    c = b.new_code()
    for q in range(3):
        b.ml_px(*_slot(0), desc=flip(c, q))
    b.cur(_slot(0), c)
    c = b.new_code()
    b.ml_px(*_slot(1), desc=c)
    for q in range(3):
        b.cur(_slot(1), flip(c, 2 * q))
    b.expect["match"] = {en: [2, 3, 3, 3] for en in ENTRIES}
    b.expect["nm"] = {en: 6 for en in ENTRIES}
    return b.done()


def projected_count(n, ncur_fill=0):
    """n projected lines; current line w has a passing projected line in every bit word up
    to w (31 | 32, 63 | 64), its winner being the highest index of word w (or n - 1)"""
    b = Search(f"projected_{n}" + (f"_ncur80" if ncur_fill else ""))
    words = [[3, 31], [5, 32, 63], [7, 40, 64, 79]]
    groups = [sorted({min(i, n - 1) for i in w}) for w in words]
    codes = [b.new_code() for _ in groups]
    owner = {}
    for q, g in enumerate(groups):
        for i in g:
            owner.setdefault(i, q)
    for i in range(n):
        if i in owner:
            b.ml_px(*_slot(owner[i]), desc=codes[owner[i]])
        else:
            b.ml_px(*_slot(10 + i % 30), desc=FILL_ML)
    for q in range(ncur_fill):
        b.cur(_slot(10 + q % 30))
    want = [-1] * ncur_fill
    for q, g in enumerate(groups):
        b.cur(_slot(q), codes[q])
        mine = [i for i in g if owner[i] == q]
        want.append(mine[-1])
    b.expect["match"] = {en: want for en in ENTRIES}
    return b.done()


def many_map_lines(nml):
    """list and harness entries: invalid and unprojectable map lines spread so that the
    compacted position of a line depends on every chunk before it; current line 0 passes for
    the lines on either side of the first 256-line seam, current line 1 for the last line
    (for nml = 513 at a compacted position >= 256)"""
    b = Search(f"map_lines_{nml}", entries=("list", "pairs0", "pairs1"))
    c0, c1 = b.new_code(), b.new_code()
    seam = [i for i in (250, 254, 255, 256, 257) if i < nml - 1]
    for i in range(nml):
        if i in seam:
            b.ml_px(*_slot(0), desc=c0)
        elif i == nml - 1:
            b.ml_px(*_slot(1), desc=c1)
        elif i % 7 == 3:
            b.ml_px(*_slot(10 + i % 30), has=0)
        elif i % 11 == 5:
            b.ml([0.1, 0.1, -2.0, 0.3, 0.2, -1.0])                    # both behind
        elif i % 13 == 6:
            b.ml_px(100.0, 220.0, 300.0, 220.0)                        # horizontal
        else:
            b.ml_px(*_slot(10 + i % 30))
    b.cur(_slot(0), c0)
    b.cur(_slot(1), c1)
    for q in range(4):
        b.cur(_slot(10 + q))
    b.expect["match"] = {en: [seam[-1], nml - 1, -1, -1, -1, -1] for en in b.entries}
    b.expect["nm"] = {en: len(seam) + 1 for en in b.entries}
    return b.done()


def pair_cap_case():
    """five passing pairs against a pair capacity of 3"""
    b = Search("pair_cap_3", pair_cap=3)
    c = b.new_code()
    for q in range(5):
        b.ml_px(*_slot(0), desc=flip(c, q))
    b.cur(_slot(0), c)
    b.expect["nm"] = {en: 5 for en in ENTRIES}
    return b.done()


# --------------------------------------------------------------------------
# the retry rule
# --------------------------------------------------------------------------
def retry_case(nl, k):
    """nl current lines, k of them match in the first pass; one more would in the retry"""
    b = Search(f"retry_{nl}_{k}")
    for q in range(k):
        b.site(_slot(q))
    if nl > k:
        b.site(_slot(k), dist=48)
    for q in range(k + 1, nl):
        b.cur(_slot(q))
    frac_retry = k * 1.0 / nl < 0.2
    le_retry = k <= 0.2 * nl
    b.expect["retry"] = {"last": frac_retry, "list": frac_retry, "pairs0": frac_retry,
                         "pairs1": le_retry}
    return b.done()


def retry_empty():
    """NL = 0: 0 / 0 < 0.2 is false, 0 <= 0 is true"""
    b = Search("retry_nl0")
    b.ml_px(*_slot(0))
    b.expect["retry"] = {"last": False, "list": False, "pairs0": False, "pairs1": True}
    return b.done()


def retry_replaces():
    """ten current lines, one first-pass match by map line 0; the retry also admits map
    line 1 (Hamming 48) for the same current line: its assignment moves to map line 1 and
    the count is the retry's. (For the last-frame, list and mode 1 overloads the retry's
    gates contain the first pass's, so their retry never counts fewer pairs than the pass
    before it; mode 0's can: retry_fewer.)"""
    b = Search("retry_replaces")
    c = b.new_code()
    b.ml_px(*_slot(0), desc=c)
    b.ml_px(*_slot(0), desc=flip(c, 48))
    b.cur(_slot(0), c)
    for q in range(1, 10):
        b.cur(_slot(q))
    b.expect["match"] = {en: [1] + [-1] * 9 for en in ENTRIES}
    b.expect["nm"] = {en: 2 for en in ENTRIES}
    b.expect["retry"] = {en: True for en in ENTRIES}
    return b.done()


def retry_fewer():
    """Mode 0's retry finds fewer pairs than its first pass. 16 current lines; current line
    0 has four map lines on it: map line 0 at Hamming 48 with ml_nobs 3, map lines 1 - 3 at
    Hamming 1 - 3 with ml_nobs 0. First pass, every overload: 1, 2 and 3 pass, 3 / 16 < 0.2
    (and 3 <= 3.2), so all retry. Mode 0's retry tests Observations() per pair too
    (LineMatcher.cpp:454-459): map line 0 now passes, has observations, and stops current
    line 0 before 1 - 3 are counted: 1 pair, match 0, the first pass's assignment to 3 gone.
    The other overloads count all four and end on map line 3."""
    b = Search("retry_fewer")
    c = b.new_code()
    b.ml_px(*_slot(0), desc=flip(c, 48), nobs=3)
    for q in (1, 2, 3):
        b.ml_px(*_slot(0), desc=flip(c, q), nobs=0)
    b.cur(_slot(0), c)
    for q in range(1, 16):
        b.cur(_slot(q))
    b.expect["match"] = {en: [0 if en == "pairs0" else 3] + [-1] * 15 for en in ENTRIES}
    b.expect["nm"] = {en: 1 if en == "pairs0" else 4 for en in ENTRIES}
    b.expect["retry"] = {en: True for en in ENTRIES}
    return b.done()


def claims_no_retry():
    """Ten current lines; 0 holds a map line with observations and would match map line 0,
    1 - 3 match theirs: three first-pass matches, no overload retries (3 > 0.2 * 10). Mode 1
    skips current line 0 as a whole, the list overload skips it in its only pass, mode 0
    skips each of its pairs: it stays at -1. The last-frame overload knows no claims."""
    b = Search("claims_no_retry")
    b.site(_slot(0), nobs=1)
    for q in (1, 2, 3):
        b.site(_slot(q))
    for q in range(4, 10):
        b.cur(_slot(q))
    tail = [1, 2, 3] + [-1] * 6
    b.expect["match"] = {"last": [0] + tail, "list": [-1] + tail, "pairs0": [-1] + tail,
                         "pairs1": [-1] + tail}
    b.expect["nm"] = {"last": 4, "list": 3, "pairs0": 3, "pairs1": 3}
    b.expect["retry"] = {en: False for en in ENTRIES}
    return b.done()


def claims():
    """cur_nobs > 0. Ten current lines; 0 and 1 hold a map line with observations.
    list: both are skipped in the first pass (0 of 10 match), the retry matches them.
    mode 1: skipped per line, then the retry (claims wiped). mode 0: tested per pair."""
    b = Search("claims")
    b.site(_slot(0), nobs=2)
    b.site(_slot(1), nobs=1)
    for q in range(2, 10):
        b.cur(_slot(q))
    b.expect["match"] = {"last": [0, 1] + [-1] * 8, "list": [0, 1] + [-1] * 8,
                         "pairs0": [0, 1] + [-1] * 8, "pairs1": [0, 1] + [-1] * 8}
    b.expect["retry"] = {"last": False, "list": True, "pairs0": True, "pairs1": True}
    return b.done()


def mode0_observations():
    """mode 0 tests Observations() per pair on the map line held at that moment. Current line
    0: passers 0, 1, 2 with ml_nobs 0, 3, 0: it takes 0, goes on to 1 and stops there. Current
    line 1: passers 3, 4 with ml_nobs 0, 0: it goes on to the last. Current line 2: passers
    5, 6 with ml_nobs 2, 0: it keeps its first. Lists and mode 1 take the last of each."""
    b = Search("mode0_observations")
    for q, nobs in enumerate(((0, 3, 0), (0, 0), (2, 0))):
        c = b.new_code()
        for k, n in enumerate(nobs):
            b.ml_px(*_slot(q), desc=flip(c, k), nobs=n)
        b.cur(_slot(q), c)
    b.expect["match"] = {"last": [2, 4, 6], "list": [2, 4, 6], "pairs1": [2, 4, 6],
                         "pairs0": [1, 4, 5]}
    b.expect["nm"] = {"last": 7, "list": 7, "pairs1": 7, "pairs0": 5}
    return b.done()


def search_cases():
    out = [projection_cases(), corner_touch(), distorted_camera("tum1", TUM1),
           distorted_camera("negative_bounds", NEG_K1), threshold_cases(False),
           threshold_cases(True), nan_fields(), several_pass(), pair_cap_case()]
    out += [projected_count(n) for n in (31, 32, 33, 64, 65, 80)]
    out.append(projected_count(80, ncur_fill=77))
    out += [many_map_lines(n) for n in (255, 256, 257, 513)]
    out += [posed(5, 64, 2), posed(6, 40, 8, entries=("list", "pairs0", "pairs1"))]
    out += [retry_case(10, 1), retry_case(10, 2), retry_case(10, 3), retry_case(5, 1),
            retry_case(15, 3), retry_empty(), retry_replaces(), retry_fewer(), claims(),
            claims_no_retry(), mode0_observations()]
    return out


# --------------------------------------------------------------------------
# match_bf_knn
# --------------------------------------------------------------------------
def bf_cases():
    c = [code(i) for i in range(1, 9)]
    z = np.zeros((0, 32), np.uint8)
    A = np.array
    out = [
        Problem("bf", "nt0", q=A([c[0]]), t=z, expect=dict(out=[], nm=0)),
        Problem("bf", "nq0", q=z, t=A([c[0], c[1]]), expect=dict(out=[-1, -1], nm=0)),
        Problem("bf", "nt1", q=A([c[0]]), t=A([c[0]]), expect=dict(out=[-1], nm=0)),
        Problem("bf", "nt2", q=A([c[0]]), t=A([c[1], c[0]]), expect=dict(out=[-1, 0], nm=1)),
        # 30 / 40 is not < 0.75f, 29 / 40 is
        Problem("bf", "ratio_30_40", q=A([c[0]]), t=A([flip(c[0], 40), flip(c[0], 30)]),
                expect=dict(out=[-1, -1], nm=0)),
        Problem("bf", "ratio_29_40", q=A([c[0]]), t=A([flip(c[0], 40), flip(c[0], 29)]),
                expect=dict(out=[-1, 0], nm=1)),
        # 0 / 0 is NaN: not < 0.75f
        Problem("bf", "best0_second0", q=A([c[0]]), t=A([c[0], c[0]]), expect=dict(out=[-1, -1], nm=0)),
        Problem("bf", "best0_second1", q=A([c[0]]), t=A([flip(c[0], 1), c[0]]),
                expect=dict(out=[-1, 0], nm=1)),
        Problem("bf", "equal_best_second", q=A([c[0]]), t=A([flip(c[0], 9), flip(c[0], 9, 100)]),
                expect=dict(out=[-1, -1], nm=0)),
        # two train rows at the best distance 5 after one at 60: the lower index is the best
        # match, the other the second (5 / 5 fails); with the second at 60 the best passes
        Problem("bf", "tie_lower_index", q=A([c[0], c[1]]),
                t=A([flip(c[0], 60), flip(c[0], 5), flip(c[0], 5, 50), flip(c[1], 7), flip(c[1], 7, 90),
                     flip(c[1], 100)]),
                expect=dict(out=[-1] * 6, nm=0)),
        Problem("bf", "tie_first_of_three", q=A([c[0]]),
                t=A([flip(c[0], 90), flip(c[0], 90, 100), flip(c[0], 90, 20)]),
                expect=dict(out=[-1, -1, -1], nm=0)),
        # queries 0 and 2 both take train row 1: the later one stays, both count
        Problem("bf", "later_overwrites", q=A([flip(c[0], 3), c[1], flip(c[0], 2)]),
                t=A([c[1], c[0], c[2]]), expect=dict(out=[1, 2, -1], nm=3)),
    ]
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)

    def mutate(rows, lo, hi):
        return np.array([flip(r, int(rng.integers(lo, hi)), int(rng.integers(0, 150))) for r in rows])
    q = mutate(base[rng.integers(0, 40, 256)], 0, 30)
    t = mutate(base[rng.integers(0, 40, 300)], 0, 60)
    out.append(Problem("bf", "nq256_nt300", q=q, t=t))
    out.append(Problem("bf", "nq255_nt257", q=q[:255], t=t[:257]))
    return out


# --------------------------------------------------------------------------
# line_in_frustum
# --------------------------------------------------------------------------
def frustum_cases():
    T = np.eye(4, dtype=f32)
    rows = [  # xyz6, in view
        ([0, 0, 0, 0, 0, 0], 1),                 # z exactly 0 at both ends: not < 0
        ([0, 0, -1, 0, 0, 0], 1),                # one end behind, one on the plane
        ([0, 0, -1, 0, 0, 2], 1), ([0, 0, 2, 0, 0, -1], 1), ([0, 0, -1, 0, 0, -2], 0),
        ([0, 0, 2, 0, 0, 3], 1),
    ]
    out = [Problem("frustum", "identity", Tcw=T, xyz6=np.array([r[0] for r in rows], f32),
                   expect=dict(in_view=[r[1] for r in rows]))]
    # a double sum that rounds to -0.0f: -2^-150 is below half the smallest float denormal
    T2 = T.copy()
    T2[2, :] = [f32(2.0 ** -100), 0, 0, 0]
    out.append(Problem("frustum", "negative_zero", Tcw=T2,
                       xyz6=np.array([[-(2.0 ** -50), 0, 0, -(2.0 ** -50), 0, 0],
                                      [-(2.0 ** -40), 0, 0, -(2.0 ** -40), 0, 0]], f32),
                       expect=dict(in_view=[1, 0])))
    # a third row for which the order of the double accumulation matters: (a*x + b*y) + c*z
    # with a*x = 2^60, b*y = -2^60, c*z = -2^-30, t = 0: any other order loses the small term
    T3 = T.copy()
    T3[2, :] = [f32(2.0 ** 30), f32(-2.0 ** 30), f32(1.0), f32(0.0)]
    big, tiny = 2.0 ** 30, 2.0 ** -30
    out.append(Problem("frustum", "accumulation_order", Tcw=T3,
                       xyz6=np.array([[big, big, -tiny, big, big, -tiny],
                                      [big, big, tiny, big, big, -tiny],
                                      [big, big, -tiny, big, big, 0.0]], f32),
                       expect=dict(in_view=[0, 1, 1])))
    rng = np.random.default_rng(3)
    Tr = T.copy()
    Tr[2, :] = [0.6, -0.3, 0.74, -0.5]
    for n in (255, 256, 257):
        X = rng.uniform(-2, 2, (n, 6)).astype(f32)
        X[-1] = [0, 0, -5, 0, 0, -6]
        X[-2 % n] = [0, 0, 5, 0, 0, 6]
        out.append(Problem("frustum", f"n{n}", Tcw=Tr, xyz6=X))
    return out


# --------------------------------------------------------------------------
# line_frame_prepare
# --------------------------------------------------------------------------
def _depth_ramp():
    """depth[v, u] = 1 + (v * 640 + u) / 2^19: every pixel its own exact float"""
    return (1.0 + np.arange(640 * 480, dtype=np.float64) / 2.0 ** 19).astype(f32).reshape(480, 640)


def prepare_cases():
    ramp = _depth_ramp()

    def at(v, u):
        return float(ramp.reshape(-1)[v * 640 + u])
    rows = [  # end points, (depth start, depth end)
        ((100.0, 50.0, 200.0, 80.0), (at(50, 100), at(80, 200))),
        ((639.9, 479.9, 640.0, 100.0), (at(479, 639), at(101, 0))),      # x = 640 reads the next row
        ((-0.5, 10.0, -1.0, 0.0), (at(10, 0), -1.0)),                    # int(-0.5) = 0; index -1
        ((0.0, 480.0, 639.0, 479.0), (-1.0, at(479, 639))),              # past the last pixel
        ((100.7, 50.9, 200.2, 80.5), (at(50, 100), at(80, 200))),        # truncation, not rounding
        ((10.0, -0.9, 20.0, 479.99), (at(0, 10), at(479, 20))),
    ]
    kl = np.array([keyline(*r[0]) for r in rows], KL)
    out = [Problem("prepare", "lookup", cam=CAM, kl=kl, depth=ramp,
                   expect=dict(dstart=[r[1][0] for r in rows], dend=[r[1][1] for r in rows]))]
    # depth values: 0, negative, NaN, inf, denormal
    vals = [0.0, -1.0, float("nan"), float("inf"), 1e-40, 2.0 ** -126, 0.5]
    d = np.full((480, 640), 2.0, f32)
    kv = []
    for q, v in enumerate(vals):
        d[100, 10 + q] = v
        kv.append(keyline(10.0 + q, 100.0, 300.0, 200.0))
    bf = 40.0
    out.append(Problem("prepare", "depth_values", cam=CAM, kl=np.array(kv, KL), depth=d,
                       expect=dict(dstart=[-1.0, -1.0, -1.0, float("inf"), 1e-40, 2.0 ** -126, 0.5],
                                   ur_start=[-1.0, -1.0, -1.0, 13.0, float("-inf"), float("-inf"),
                                             16.0 - bf / 0.5])))
    out.append(Problem("prepare", "no_depth", cam=CAM, kl=kl, depth=None,
                       expect=dict(dstart=[-1.0] * len(rows), dend=[-1.0] * len(rows))))
    rng = np.random.default_rng(7)
    segs = np.round(rng.uniform(5, 470, (80, 4)) * 4) / 4
    k80 = np.array([keyline(*s) for s in segs], KL)
    out.append(Problem("prepare", "distorted_80", cam=TUM1, kl=k80, depth=ramp))
    out.append(Problem("prepare", "k1_zero_k2_nonzero", cam=K2_ONLY, kl=k80[:7], depth=ramp,
                       expect=dict(kl_un=k80[:7].tobytes())))
    out.append(Problem("prepare", "n1", cam=TUM1, kl=k80[:1], depth=ramp))
    return out


# --------------------------------------------------------------------------
# stereo_line_depths
# --------------------------------------------------------------------------
class Stereo:
    kind = "stereo"

    def __init__(self, name, cam=CAM):
        self.name, self.cam, self._l, self._r, self._n = name, cam, [], [], 0
        self.expect = dict(reasons={}, dstart={}, dend={})

    def __repr__(self):
        return f"stereo:{self.name}"

    def new_code(self):
        self._n += 1
        return code(self._n)

    def left(self, seg, desc, **over):
        self._l.append((keyline(*seg, **over), desc))
        return len(self._l) - 1

    def right(self, seg, desc, **over):
        self._r.append((keyline(*seg, **over), desc))
        return len(self._r) - 1

    def done(self):
        self.kl = np.array([x[0] for x in self._l], KL) if self._l else np.zeros(0, KL)
        self.desc = np.array([x[1] for x in self._l], np.uint8).reshape(len(self._l), 32)
        self.kr = np.array([x[0] for x in self._r], KL) if self._r else np.zeros(0, KL)
        self.desc_r = np.array([x[1] for x in self._r], np.uint8).reshape(len(self._r), 32)
        return self


def _shift(seg, d, dy=0.0):
    return (seg[0] - d, seg[1] + dy, seg[2] - d, seg[3] + dy)


def stereo_gates():
    """one left line per gate, a right line on either side of it. bf = 40, fx = 512: the
    disparity range is (0, 512), a disparity of 16 is a depth of 2.5."""
    b = Stereo("gates")
    e = b.expect
    seg = (300.0, 100.0, 340.0, 200.0)
    L = float(keyline(*seg)["lineLength"])
    A = float(keyline(*seg)["angle"])
    T10 = 10.0 * R.PI / 180.0

    def pair(lseg, rseg, reason, dist=0, lover=None, **rover):
        c = b.new_code()
        i = b.left(lseg, c, **(lover or {}))
        j = b.right(rseg, flip(c, dist), **rover)
        e["reasons"][(i, j)] = reason
        return i, j

    i, _ = pair(seg, _shift(seg, 16.0), R.TAKEN, dist=45)
    e["dstart"][i] = e["dend"][i] = 2.5
    pair(seg, _shift(seg, 16.0), R.DESC, dist=46)
    # the left line flat: |dy| < 0.25 length, on either side
    flat = (100.0, 300.0, 200.0, 325.0)
    Lf = float(keyline(*flat)["lineLength"])
    pair(flat, _shift(flat, 16.0), R.TAKEN, lover=dict(lineLength=100.0), lineLength=100.0)
    c = b.new_code()
    i = b.left(flat, c, lineLength=above(100.0))
    b.right(_shift(flat, 16.0), c)
    e["reasons"][(i, None)] = R.LEFT_FLAT
    assert Lf > 100.0
    # angle: > 10 degrees rejects, == the float nearest to it (below the double) does not
    a2 = R.r32(A + T10)                     # the two floats around A + 10 degrees
    while abs(A - a2) > T10:
        a2 = below(a2)
    while abs(A - above(a2)) <= T10:
        a2 = above(a2)
    pair(seg, _shift(seg, 16.0), R.TAKEN, angle=a2)
    pair(seg, _shift(seg, 16.0), R.ANGLE, angle=above(a2))
    # length: float ratio against the float 0.45f
    th = R.r32(0.45)
    Lp, Lq = _length_pair(L, th, True)
    pair(seg, _shift(seg, 16.0), R.TAKEN, lineLength=Lp)
    pair(seg, _shift(seg, 16.0), R.LENGTH, lineLength=Lq)
    # the right line flat: its length field at 4 |dy| and one float above
    pair(seg, _shift(seg, 16.0), R.TAKEN, lineLength=400.0, lover=dict(lineLength=400.0))
    pair(seg, _shift(seg, 16.0), R.RIGHT_FLAT, lineLength=above(400.0), lover=dict(lineLength=400.0))
    # row overlap: half of the shorter span (100 rows) and one row less
    pair(seg, _shift(seg, 16.0, 50.0), R.TAKEN)
    pair(seg, _shift(seg, 16.0, 51.0), R.ROW_OVERLAP)
    # disparity: exactly 0, one float above 0, exactly bf / mb = 512, one float below
    v = (600.0, 100.0, 600.0, 200.0)
    pair(v, v, R.DISPARITY)
    pair(v, _shift(v, 2.0 ** -10), R.TAKEN)
    pair(v, _shift(v, 512.0), R.DISPARITY)
    pair(v, _shift(v, 511.75), R.TAKEN)
    pair((600.0, 100.0, 620.0, 200.0), (590.0, 100.0, 625.0, 200.0), R.DISPARITY)   # end: negative
    # a NaN length: `|dy| < 0.25 NaN` is false, the line is not flat; std::min / std::max keep
    # their first argument, the ratio is NaN / NaN, which is not < 0.45f
    i, _ = pair((100.0, 50.0, 140.0, 150.0), (84.0, 50.0, 124.0, 150.0), R.TAKEN,
                lover=dict(lineLength=float("nan")))
    e["dstart"][i] = e["dend"][i] = 2.5
    pair((160.0, 50.0, 200.0, 150.0), (144.0, 50.0, 184.0, 150.0), R.TAKEN, lineLength=float("nan"))
    return b.done()


def stereo_order():
    """equal distances keep the first; a better later line that fails a later gate does not
    displace the holder; a better later line that passes does"""
    b = Stereo("order")
    seg = (300.0, 100.0, 340.0, 200.0)
    c = b.new_code()
    i = b.left(seg, c)
    b.right(_shift(seg, 16.0), flip(c, 20))              # taken: depth 2.5
    b.right(_shift(seg, 32.0), flip(c, 20, 100))         # the same distance: NOT_BETTER
    b.right(_shift(seg, 64.0, 80.0), flip(c, 10))        # better, but its rows do not overlap
    b.right(_shift(seg, 8.0), flip(c, 30))               # worse
    b.expect["reasons"].update({(i, 0): R.TAKEN, (i, 1): R.NOT_BETTER, (i, 2): R.ROW_OVERLAP,
                                (i, 3): R.NOT_BETTER})
    b.expect["dstart"][i] = b.expect["dend"][i] = 2.5
    c = b.new_code()
    i = b.left(_shift(seg, -100.0), c)
    b.right(_shift(seg, -100.0 + 16.0), flip(c, 20))
    b.right(_shift(seg, -100.0 + 32.0), flip(c, 5))      # better and passes: depth 1.25
    b.expect["reasons"].update({(i, 4): R.TAKEN, (i, 5): R.TAKEN})
    b.expect["dstart"][i] = b.expect["dend"][i] = 1.25
    return b.done()


def stereo_sizes(nl, nr, seed):
    rng = np.random.default_rng(seed)
    b = Stereo(f"nl{nl}_nr{nr}")
    codes = [b.new_code() for _ in range(max(nl, 1))]
    for q in range(nl):
        x, y = 60.0 + 7 * (q % 40), 50.0 + 200 * (q // 40)
        b.left((x, y, x + 30.0, y + 120.0), codes[q])
    for q in range(nr):
        k = (q * 7) % max(nl, 1)
        x, y = 60.0 + 7 * (k % 40), 50.0 + 200 * (k // 40)
        d = float(rng.integers(1, 40))
        b.right((x - d, y, x + 30.0 - d, y + 120.0), flip(codes[k], int(rng.integers(0, 50))))
    return b.done()


def stereo_cases():
    return [stereo_gates(), stereo_order(), stereo_sizes(80, 80, 1), stereo_sizes(80, 0, 2),
            stereo_sizes(0, 5, 3), stereo_sizes(1, 1, 4)]


# --------------------------------------------------------------------------
# seeded crowds
# --------------------------------------------------------------------------
def _mutate(rng, d, lo, hi):
    return flip(d, int(rng.integers(lo, hi)), int(rng.integers(0, 256 - hi)))


def crowd_search(seed, ncur, per, dist=(0, 44), cur_mut=24, entries=ENTRIES, win=(150, 110),
                 lens=(80.0, 100.0, 140.0, 260.0), ang=(0.55, 1.05)):
    """ncur current lines of similar direction whose start points lie in a small window,
    `per` map lines per current line placed by jittering its end points; every descriptor
    lies within a few dozen bits of one pool word (map lines `dist` bits from it, current
    lines up to cur_mut), so that the geometric gates decide most pairs. One map line for
    every projection code is mixed in."""
    rng = np.random.default_rng(seed)
    b = Search(f"crowd_s{seed}_{ncur}x{ncur * per}", entries=entries)
    pool = code(200)
    segs = []
    for j in range(ncur):
        x, y = rng.uniform(150, 150 + win[0]), rng.uniform(60, 60 + win[1])
        a = rng.uniform(*ang)
        ln = float(rng.choice(lens))
        seg = tuple(float(v) for v in np.round([x, y, x + ln * math.cos(a), y + ln * math.sin(a)], 2))
        segs.append(seg)
        b.cur(seg, _mutate(rng, pool, 0, cur_mut + 1), nobs=int(rng.random() < 0.1))
    special = [  # one of every projection code
        lambda: b.ml([0.1, 0.1, -2.0, 0.3, 0.2, -1.0]), lambda: b.ml([0.1, 0.1, 0.0, 0.3, 0.2, 2.0]),
        lambda: b.ml([0.5, 0.25, -2.0] + unproject(200.0, 180.0, 2.0)),
        lambda: b.ml(unproject(300.0, 100.0, 4.0) + [1.0, 0.5, -4.0]),
        lambda: b.ml_px(100.0, 220.0, 300.0, 220.0), lambda: b.ml_px(0.0, 100.0, 0.0, 200.0),
        lambda: b.ml_px(-100.0, -100.0, -50.0, -20.0), lambda: b.ml_px(300.0, 300.0, 380.0, 400.0, has=0),
        lambda: b.ml_px(200.0, 100.0, 200.0, 260.0, desc=_mutate(rng, pool, dist[0], dist[1] + 1)),
    ]
    n = ncur * per
    at = {int(v): k for k, v in enumerate(rng.choice(n, len(special), replace=False))}
    for i in range(n):
        if i in at:
            special[at[i]]()
            continue
        s = segs[int(rng.integers(0, ncur))]
        jit = rng.normal(0, 5.0, 4)
        if rng.random() < 0.3:
            shift = rng.normal(0, 35.0, 2)
            jit += [shift[0], shift[1], shift[0], shift[1]]
        px = [float(v) for v in np.round(np.array(s) + jit, 2)]
        z = float(rng.choice([1.0, 2.0, 4.0]))
        b.ml_px(*px, desc=_mutate(rng, pool, dist[0], dist[1] + 1), z0=z, z1=z,
                nobs=int(rng.random() < 0.5), outlier=int(rng.random() < 0.03))
    return b.done()


def crowd_stereo(seed, nl=80, nr=80):
    """left lines of similar direction, a quarter of them near the flatness bound
    |dy| = 0.25 length; right lines are left lines moved by a disparity of -20 .. 120 and
    jittered, some shortened to around 0.45 of the length"""
    rng = np.random.default_rng(seed)
    b = Stereo(f"crowd_s{seed}")
    pool = code(201)
    for q in range(nl):
        x, y = rng.uniform(200, 560), rng.uniform(20, 250)
        if rng.random() < 0.25:
            dx = rng.uniform(120, 200)
            dy = dx * rng.uniform(0.235, 0.285)
        else:
            dx, dy = rng.uniform(20, 60), rng.uniform(80, 150)
        b.left(tuple(float(v) for v in np.round([x, y, x + dx, y + dy], 2)), _mutate(rng, pool, 0, 24))
    for q in range(nr):
        k = b._l[int(rng.integers(0, nl))][0]
        s = np.array([k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"]], np.float64)
        if rng.random() < 0.2:
            s[2:] = s[:2] + (s[2:] - s[:2]) * rng.uniform(0.40, 0.50)
        d = rng.uniform(-20, 120)
        s += [-d, 0, -d, 0]
        s += rng.normal(0, 2.0, 4)
        if rng.random() < 0.3:
            s += np.tile(rng.normal(0, 40.0, 2), 2)
        b.right(tuple(float(v) for v in np.round(s, 2)), _mutate(rng, pool, 0, 44))
    return b.done()


def posed(seed, ncur, per, entries=ENTRIES):
    """a crowd under a pose that rotates about all three axes: the 3x4 product in double on
    float entries, no exact pixel values"""
    b = crowd_search(seed, ncur, per, entries=entries)
    b.name = f"posed_s{seed}_{ncur}x{ncur * per}"
    rx, ry, rz = 0.11, -0.07, 0.05
    cx, sx, cy, sy, cz, sz = (f(a) for a in (rx, ry, rz) for f in (math.cos, math.sin))
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [0.3, -0.2, 0.45]
    b.set_pose(T.astype(f32))
    return b.done()


def crowds():
    return dict(
        search=[crowd_search(1, 64, 2), crowd_search(2, 80, 1),
                crowd_search(3, 70, 8, dist=(0, 50), entries=("list", "pairs0", "pairs1")),
                # every descriptor distance is 46 .. 50: nothing passes the first pass
                crowd_search(4, 60, 4, dist=(46, 50), cur_mut=0, entries=("list", "pairs0", "pairs1"),
                             lens=(60.0, 100.0, 180.0, 260.0), ang=(0.4, 1.2)),
                # the same at the last-frame overload's capacity
                crowd_search(7, 80, 1, dist=(46, 50), cur_mut=0,
                             lens=(60.0, 100.0, 180.0, 260.0), ang=(0.4, 1.2))],
        stereo=[crowd_stereo(1), crowd_stereo(2)])


KINDS = ("search", "bf", "frustum", "prepare", "stereo")


@functools.lru_cache(maxsize=None)
def all_problems(kind):
    cases = dict(search=search_cases, bf=bf_cases, frustum=frustum_cases, prepare=prepare_cases,
                 stereo=stereo_cases)[kind]()
    return tuple(cases + crowds().get(kind, []))


def runs(kind):
    """(problem index, entry) of every comparison of a kind"""
    out = []
    for k, P in enumerate(all_problems(kind)):
        for en in (P.entries if kind == "search" else (None,)):
            out.append((k, en))
    return out

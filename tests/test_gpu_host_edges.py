"""Edge handling of the host-pointer entry points' device staging: counts of 0
and 1 on each side independently, optional arrays absent and present, and
output arrays that keep a sentinel past the returned count. A side with count
0 passes NULL arrays: nothing may read them.

Expectations come from the CPU oracle (it accepts every empty input used
here) or, for the calls the oracle does not have, from the test-only Python
references and the plain reading of the reference on an empty input: no
matches, count 0. Every case stages a handful of arrays of a few hundred bytes.
"""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from _pkg import load_oracle, load_pkg

orbpl = load_pkg()
pytestmark = pytest.mark.gpu

S = -7                       # the sentinel of int32 outputs (uint8: 0xF9, float: -7.0)
OK = orbpl.ORBPL_OK
CFG = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0,
           bf=40.0, thdepth=40.0, width=640, height=480)
SCALE = np.float32(1.2) ** np.arange(8, dtype=np.float32)
SIGMA2 = SCALE * SCALE
EYE = np.eye(4, dtype=np.float32)
RNG = np.random.default_rng(5)
DESC = RNG.integers(0, 256, (4, 32), dtype=np.uint8)
COUNTS = list(itertools.product((0, 1), (0, 1)))
# a world point 2 m ahead and the keypoint it projects to
XYZ = np.array([[0.1, 0.05, 2.0]], np.float32)
U, V = 500.0 * 0.1 / 2.0 + 320.0, 500.0 * 0.05 / 2.0 + 240.0
# a world segment 2 m ahead and the key line it projects to
XYZ6 = np.array([[-0.08, -0.16, 2.0, 0.16, -0.12, 2.0]], np.float32)
SEG = (300.0, 200.0, 360.0, 210.0)


@pytest.fixture(scope="module")
def O():
    return load_oracle()


def cams(O):
    return orbpl.make_camera(CFG), O.camera(CFG)


def p(a):
    """the array's address, NULL for an empty one"""
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def sent(n, dt=np.int32):
    return np.full(n, S).astype(dt)


def keypoints(n):
    k = np.zeros(n, orbpl.KP_DTYPE)
    k["x"], k["y"], k["size"], k["angle"], k["response"], k["class_id"] = U, V, 31.0, 10.0, 50.0, -1
    return k


def keylines(n):
    x0, y0, x1, y1 = SEG
    k = np.zeros(n, orbpl.KEYLINE_DTYPE)
    k["startPointX"] = k["sPointInOctaveX"] = x0
    k["startPointY"] = k["sPointInOctaveY"] = y0
    k["endPointX"] = k["ePointInOctaveX"] = x1
    k["endPointY"] = k["ePointInOctaveY"] = y1
    k["pt_x"], k["pt_y"] = (x0 + x1) / 2, (y0 + y1) / 2
    k["angle"] = math.atan2(y1 - y0, x1 - x0)
    k["lineLength"] = math.hypot(x1 - x0, y1 - y0)
    k["numOfPixels"], k["response"], k["size"] = 60, 0.1, 600.0
    return k


def current(n):
    return dict(Tcw=EYE, kps_un=keypoints(n), desc=DESC[:n].copy(),
                uright=np.full(n, U - 40.0 / 2.0, np.float32))


def check_ok(rc, what):
    assert rc == OK, (what, rc, orbpl.lib().orbpl_last_error().decode())


def kept(a, n):
    """the elements of an output past the first n still hold the sentinel"""
    return bool(np.all(a[n:] == np.array(S).astype(a.dtype)))


# ---------------------------------------------------------------------------
# ORBmatcher
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,nl", COUNTS)
def test_projection_last(O, n, nl):
    cam, cam_o = cams(O)
    cur = current(n)
    last = dict(Tcw=EYE, kps_un=keypoints(nl), has_mp=np.ones(nl, np.uint8),
                outlier=np.zeros(nl, np.uint8), mp_xyz=XYZ[:nl].copy(), mp_desc=DESC[:nl].copy(),
                mp_nobs=np.ones(nl, np.int32))
    em, en = O.search_by_projection_last(cam_o, SCALE, cur, last, 15.0)
    mc = orbpl.MatchCurrent(n, p(EYE), p(cur["kps_un"]), p(cur["desc"]), p(cur["uright"]))
    ml = orbpl.MatchLast(nl, p(EYE), p(last["kps_un"]), p(last["has_mp"]), p(last["outlier"]),
                         p(last["mp_xyz"]), p(last["mp_desc"]), p(last["mp_nobs"]))
    match, nm = sent(n + 2), C.c_int(S)
    check_ok(orbpl.lib().orbm_search_by_projection_last(
        C.byref(cam), p(SCALE), 8, C.byref(mc), C.byref(ml), 15.0, 0, 1, p(match), C.byref(nm)),
        "projection_last")
    assert nm.value == en and np.array_equal(match[:n], em) and kept(match, n)
    if n and nl:
        assert en == 1 and em[0] == 0        # the case does match


def track_of(nmp):
    return dict(in_view=np.ones(nmp, np.uint8), proj_x=np.full(nmp, U, np.float32),
                proj_y=np.full(nmp, V, np.float32), proj_xr=np.full(nmp, U - 20.0, np.float32),
                level=np.zeros(nmp, np.int32), view_cos=np.ones(nmp, np.float32))


@pytest.mark.parametrize("n,nmp,nobs", [(a, b, False) for a, b in COUNTS] + [(1, 1, True)])
def test_projection_local(O, n, nmp, nobs):
    cam, cam_o = cams(O)
    cur, tr = current(n), track_of(nmp)
    mpd, mpn = DESC[:nmp].copy(), np.ones(nmp, np.int32)
    cn = np.zeros(n, np.int32) if nobs else None
    em, en = O.search_by_projection_local(cam_o, SCALE, cur, tr, mpd, mpn, cn, 1.0, 0.8)
    mc = orbpl.MatchCurrent(n, p(EYE), p(cur["kps_un"]), p(cur["desc"]), p(cur["uright"]))
    match, nm = sent(n + 2), C.c_int(S)
    check_ok(orbpl.lib().orbm_search_by_projection_local(
        C.byref(cam), p(SCALE), 8, C.byref(mc), nmp, p(tr["in_view"]), p(tr["proj_x"]),
        p(tr["proj_y"]), p(tr["proj_xr"]), p(tr["level"]), p(tr["view_cos"]), p(mpd), p(mpn),
        p(cn), 1.0, 0.8, p(match), C.byref(nm)), "projection_local")
    assert nm.value == en and np.array_equal(match[:n], em) and kept(match, n)
    if n and nmp:
        assert en == 1 and em[0] == 0


@pytest.mark.parametrize("nkf,nf", COUNTS)
def test_search_by_bow(O, nkf, nf):
    kn, kv, kd = np.full(nkf, 3, np.int32), np.ones(nkf, np.uint8), DESC[:nkf].copy()
    ka = np.full(nkf, 10.0, np.float32)
    fn, fd, fa = np.full(nf, 3, np.int32), DESC[:nf].copy(), np.full(nf, 10.0, np.float32)
    em, en = O.search_by_bow(kn, kv, kd, ka, fn, fd, fa, 0.7, True)
    match, nm = sent(nf + 2), C.c_int(S)
    check_ok(orbpl.lib().orbm_search_by_bow(nkf, p(kn), p(kv), p(kd), p(ka), nf, p(fn), p(fd),
                                            p(fa), 0.7, 1, p(match), C.byref(nm)), "bow")
    assert nm.value == en and np.array_equal(match[:nf], em) and kept(match, nf)
    if nkf and nf:
        assert en == 1 and em[0] == 0


@pytest.mark.parametrize("n,nkf", [(0, 0), (0, 1), (1, 0)])
def test_projection_keyframe_with_an_empty_side(n, nkf):
    """ORBmatcher.cc:1891-2024 loops over the keyframe's map points: without
    any, or without keypoints to meet them, nothing matches."""
    cam = orbpl.make_camera(CFG)
    cur = current(n)
    has = np.zeros(n, np.uint8)
    ang, one = np.full(nkf, 10.0, np.float32), np.ones(nkf, np.uint8)
    found = np.zeros(nkf, np.uint8)
    mn, mx = np.full(nkf, 0.5, np.float32), np.full(nkf, 8.0, np.float32)
    xyz, mpd = XYZ[:nkf].copy(), DESC[:nkf].copy()
    mc = orbpl.MatchCurrent(n, p(EYE), p(cur["kps_un"]), p(cur["desc"]), None)
    match, nm = sent(n + 2), C.c_int(S)
    check_ok(orbpl.lib().orbm_search_by_projection_kf(
        C.byref(cam), p(SCALE), 8, C.byref(mc), p(has), nkf, p(ang), p(one), p(found), p(xyz),
        p(mn), p(mx), p(mpd), 10.0, 100, 1, p(match), C.byref(nm)), "projection_kf")
    assert nm.value == 0 and np.all(match[:n] == -1) and kept(match, n)


# ---------------------------------------------------------------------------
# Optimizer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,nl", COUNTS)
def test_pose_optimization(O, n, nl):
    cam, cam_o = cams(O)
    x0, y0, x1, y1 = SEG
    prob = dict(kps_un=keypoints(n), uright=np.full(n, U - 20.0, np.float32),
                has_mp=np.ones(n, np.uint8), mp_xyz=XYZ[:n].copy(),
                kl_obs=np.array([[x0, y0, x1, y1]], np.float32)[:nl],
                kl_octave=np.zeros(nl, np.int32), has_ml=np.ones(nl, np.uint8),
                ml_xyz=XYZ6[:nl].copy(), inv_sigma2=(1.0 / SIGMA2).astype(np.float32))
    eT, eo, el, en = O.pose_optimization(cam_o, prob, EYE, np.zeros(n, np.uint8),
                                         np.zeros(nl, np.uint8))
    P = orbpl.PoseProblem(n, p(prob["kps_un"]), p(prob["uright"]), p(prob["has_mp"]),
                          p(prob["mp_xyz"]), nl, p(prob["kl_obs"]), p(prob["kl_octave"]),
                          p(prob["has_ml"]), p(prob["ml_xyz"]), p(prob["inv_sigma2"]), 8)
    T = EYE.copy()
    out, lout = sent(n + 2, np.uint8), sent(nl + 2, np.uint8)
    out[:n] = 0
    lout[:nl] = 0
    nin = C.c_int(S)
    check_ok(orbpl.lib().orbpl_pose_optimization_ex(
        C.byref(cam), C.byref(P), 0, p(T), p(out) if n else None, p(lout) if nl else None,
        C.byref(nin)), "pose")
    assert nin.value == en and np.array_equal(T, eT)
    assert np.array_equal(out[:n], eo) and np.array_equal(lout[:nl], el)
    assert kept(out, n) and kept(lout, nl)


# ---------------------------------------------------------------------------
# LineMatcher
# ---------------------------------------------------------------------------
def map_lines(nml):
    return np.ones(nml, np.uint8), XYZ6[:nml].copy(), DESC[:nml].copy()


@pytest.mark.parametrize("ncur,nlast", COUNTS)
def test_line_projection_last(O, ncur, nlast):
    cam, cam_o = cams(O)
    kl, kd, lk = keylines(ncur), DESC[:ncur].copy(), keylines(nlast)
    has, xyz, ld = map_lines(nlast)
    lo = np.zeros(nlast, np.uint8)
    em, en = O.line_search_by_projection_last(cam_o, EYE, kl, kd, lk, has, lo, xyz, ld)
    match, nm = sent(ncur + 2), C.c_int(S)
    check_ok(orbpl.lib().orbl_search_by_projection_last(
        C.byref(cam), p(EYE), ncur, p(kl), p(kd), nlast, p(lk), p(has), p(lo), p(xyz), p(ld),
        p(match), C.byref(nm)), "line_projection_last")
    assert nm.value == en and np.array_equal(match[:ncur], em) and kept(match, ncur)


@pytest.mark.parametrize("ncur,nml,opt", [(a, b, False) for a, b in COUNTS] + [(1, 1, True)])
def test_line_projection_list(O, ncur, nml, opt):
    """opt: cur_nobs and wiped present, else both NULL"""
    cam, cam_o = cams(O)
    kl, kd = keylines(ncur), DESC[:ncur].copy()
    valid, xyz, md = map_lines(nml)
    cn = np.zeros(ncur, np.int32) if opt else None
    em, en, ew = O.line_search_by_projection_list(cam_o, EYE, kl, kd, cn, valid, xyz, md)
    match, nm, wiped = sent(ncur + 2), C.c_int(S), C.c_int(S)
    check_ok(orbpl.lib().orbl_search_by_projection_list(
        C.byref(cam), p(EYE), ncur, p(kl), p(kd), p(cn), nml, p(valid), p(xyz), p(md), p(match),
        C.byref(nm), C.byref(wiped) if opt else None), "line_projection_list")
    assert nm.value == en and np.array_equal(match[:ncur], em) and kept(match, ncur)
    assert wiped.value == (int(ew) if opt else S)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("ncur,nml,opt", [(a, b, False) for a, b in COUNTS] + [(1, 1, True)])
def test_line_projection_pairs(O, mode, ncur, nml, opt):
    """opt: cur_nobs, base_kl and ml_nobs present, else all three NULL"""
    cam, cam_o = cams(O)
    kl, kd = keylines(ncur), DESC[:ncur].copy()
    valid, xyz, md = map_lines(nml)
    cn = np.zeros(ncur, np.int32) if opt else None
    bk = keylines(nml) if opt else None
    mn = np.ones(nml, np.int32) if opt else None
    em, en, ew, epk, eps, epr = O.line_search_pairs(cam_o, EYE, mode, kl, kd, cn, valid, bk, xyz,
                                                    md, mn)
    match, pk, ps = sent(ncur + 2), np.zeros(nml + 2, orbpl.KEYLINE_DTYPE), sent(nml + 2)
    pk["class_id"] = S
    cap = max(1, ncur * nml)
    pairs = sent(2 * (cap + 2)).reshape(-1, 2)
    nm, wiped, npj, npr = C.c_int(S), C.c_int(S), C.c_int(S), C.c_int(S)
    check_ok(orbpl.lib().orbl_search_by_projection_pairs(
        C.byref(cam), p(EYE), mode, ncur, p(kl), p(kd), p(cn), nml, p(valid), p(bk), p(xyz), p(md),
        p(mn), p(pk), p(ps), C.byref(npj), p(pairs), cap, C.byref(npr), p(match), C.byref(nm),
        C.byref(wiped)), "line_projection_pairs")
    assert (nm.value, bool(wiped.value), npj.value, npr.value) == (en, ew, len(epk), len(epr))
    assert np.array_equal(match[:ncur], em) and kept(match, ncur)
    assert pk[:npj.value].tobytes() == epk.tobytes() and np.all(pk["class_id"][npj.value:] == S)
    assert np.array_equal(ps[:npj.value], eps) and kept(ps, npj.value)
    assert np.array_equal(pairs[:npr.value], epr) and kept(pairs, min(npr.value, cap))


@pytest.mark.parametrize("nq,nt", COUNTS)
def test_line_match_bf_knn(O, nq, nt):
    q, t = DESC[:nq].copy(), DESC[1:1 + nt].copy()
    eo, en = O.line_match_bf_knn(q, t)
    out, nm = sent(nt + 2), C.c_int(S)
    check_ok(orbpl.lib().orbl_match_bf_knn(nq, p(q), nt, p(t), p(out), C.byref(nm)), "bf_knn")
    assert nm.value == en and np.array_equal(out[:nt], eo) and kept(out, nt)


def steep_lines(n, shift):
    """the segment (300, 200)-(320, 260) moved `shift` pixels to the left"""
    k = keylines(n)
    k["startPointX"] = k["sPointInOctaveX"] = 300.0 - shift
    k["endPointX"] = k["ePointInOctaveX"] = 320.0 - shift
    k["endPointY"] = k["ePointInOctaveY"] = 260.0
    k["angle"] = math.atan2(60.0, 20.0)
    k["lineLength"] = math.hypot(20.0, 60.0)
    return k


@pytest.mark.parametrize("nl,nr", COUNTS)
def test_stereo_line_depths(O, nl, nr):
    """the right line is the left one 10 pixels to the left: both depths are
    bf / 10"""
    cam, cam_o = cams(O)
    kl, kr = steep_lines(nl, 0.0), steep_lines(nr, 10.0)
    dl, dr = DESC[:nl].copy(), DESC[:nr].copy()
    eds, ede = O.stereo_line_depths(cam_o, kl, dl, kr, dr)
    ds, de = sent(nl + 2, np.float32), sent(nl + 2, np.float32)
    check_ok(orbpl.lib().orbl_stereo_line_depths(
        C.byref(cam), p(kl), p(dl), nl, p(kr), p(dr), nr, p(ds) if nl else None,
        p(de) if nl else None), "stereo_line_depths")
    assert np.array_equal(ds[:nl], eds) and np.array_equal(de[:nl], ede)
    assert kept(ds, nl) and kept(de, nl)
    if nl:
        assert ds[0] == de[0] == (4.0 if nr else -1.0)


# ---------------------------------------------------------------------------
# Frame
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,opt", [(0, False), (0, True), (1, False), (1, True)])
def test_frame_prepare(O, n, opt):
    """opt: the depth image and bounds present, else both NULL"""
    cam, cam_o = cams(O)
    kps = keypoints(n)
    depth = np.full((480, 640), 2.0, np.float32) if opt else None
    eku, ed, eur, egc, eb = O.frame_prepare(cam_o, kps, depth)
    ku = np.zeros(n + 2, orbpl.KP_DTYPE)
    ku["class_id"] = S
    d, ur, gc, b = sent(n + 2, np.float32), sent(n + 2, np.float32), sent(n + 2), sent(4, np.float32)
    check_ok(orbpl.lib().orbpl_frame_prepare(
        C.byref(cam), p(kps), n, p(depth), p(ku) if n else None, p(d) if n else None,
        p(ur) if n else None, p(gc) if n else None, p(b) if opt else None), "frame_prepare")
    assert ku[:n].tobytes() == eku.tobytes() and np.all(ku["class_id"][n:] == S)
    assert np.array_equal(d[:n], ed) and np.array_equal(ur[:n], eur) and np.array_equal(gc[:n], egc)
    assert kept(d, n) and kept(ur, n) and kept(gc, n)
    assert np.array_equal(b, eb) if opt else kept(b, 0)


@pytest.mark.parametrize("n,opt", [(0, False), (1, False), (1, True)])
def test_line_frame_prepare(O, n, opt):
    cam, cam_o = cams(O)
    kl = keylines(n)
    depth = np.full((480, 640), 2.0, np.float32) if opt else None
    exp = O.line_frame_prepare(cam_o, kl, depth)
    ku = np.zeros(n + 2, orbpl.KEYLINE_DTYPE)
    ku["class_id"] = S
    outs = [sent(n + 2, np.float32) for _ in range(4)]
    check_ok(orbpl.lib().orbpl_line_frame_prepare(
        C.byref(cam), p(kl), n, p(depth), p(ku) if n else None,
        *[p(o) if n else None for o in outs]), "line_frame_prepare")
    assert ku[:n].tobytes() == exp[0].tobytes() and np.all(ku["class_id"][n:] == S)
    for o, e in zip(outs, exp[1:]):
        assert np.array_equal(o[:n], e) and kept(o, n)


@pytest.mark.parametrize("n", [0, 1])
def test_is_in_frustum(O, n):
    cam, cam_o = cams(O)
    mps = dict(xyz=XYZ[:n].copy(), normal=np.array([[0, 0, 1]], np.float32)[:n],
               min_dist=np.full(n, 0.5, np.float32), max_dist=np.full(n, 8.0, np.float32))
    exp = O.frame_is_in_frustum(cam_o, float(np.float32(O.lsdm(1, float(np.float32(1.2))))), 8, EYE,
                                mps)
    dts = dict(in_view=np.uint8, proj_x=np.float32, proj_y=np.float32, proj_xr=np.float32,
               level=np.int32, view_cos=np.float32)
    out = {k: sent(n + 2, dt) for k, dt in dts.items()}
    check_ok(orbpl.lib().orbpl_frame_is_in_frustum(
        C.byref(cam), float(np.float32(1.2)), 8, p(EYE), n, p(mps["xyz"]), p(mps["normal"]),
        p(mps["min_dist"]), p(mps["max_dist"]), 0.5, *[p(out[k]) if n else None for k in dts]),
        "is_in_frustum")
    for k in dts:
        assert np.array_equal(out[k][:n], exp[k]) and kept(out[k], n), k
    # and the lines' test
    ev = O.line_is_in_frustum(EYE, XYZ6[:n])
    iv = sent(n + 2, np.uint8)
    x6 = XYZ6[:n].copy()
    check_ok(orbpl.lib().orbl_frame_is_in_frustum(p(EYE), n, p(x6), p(iv) if n else None),
             "line_is_in_frustum")
    assert np.array_equal(iv[:n], ev) and kept(iv, n)


# ---------------------------------------------------------------------------
# Relocalisation: KeyFrameDatabase, PnPsolver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nkf,opt", [(0, False), (0, True), (1, False), (1, True)])
def test_detect_reloc(nkf, opt):
    """opt: common_words present, else NULL. An empty database has no
    candidates; one keyframe sharing the query's word is the reference's."""
    import _reloc_ref as R
    words, vals = np.array([3, 9], np.uint32), np.array([0.5, 0.5], np.float64)
    bows = [(words, vals)][:nkf]
    ecand, ecw, ers, _ = R.detect_reloc(bows, [[]] * nkf, np.zeros(nkf, np.float32), words, vals)
    off = np.array([0, 2], np.int32)[:nkf + 1]
    cov = np.full((max(1, nkf), 10), -1, np.int32)
    rs = sent(nkf + 2, np.float32)
    rs[:nkf] = 0
    cand, nc, cw = sent(64), sent(1), sent(nkf + 2)
    P = orbpl.KfdbProblem(nkf, p(off) if nkf else None, p(words) if nkf else None,
                          p(vals) if nkf else None, p(cov) if nkf else None,
                          p(rs) if nkf else None, 2, p(words), p(vals), p(cand), p(nc),
                          p(cw) if opt else None)
    check_ok(orbpl.lib().orbkf_detect_reloc(C.byref(P), 1, 0), "detect_reloc")
    assert nc[0] == len(ecand) and list(cand[:nc[0]]) == list(ecand) and kept(cand, nc[0])
    assert np.array_equal(rs[:nkf], ers) and kept(rs, nkf)
    assert list(cw[:nkf]) == list(ecw[:nkf]) if opt else kept(cw, 0)
    assert kept(cw, nkf)
    check_ok(orbpl.lib().orbkf_detect_reloc(None, 0, 0), "detect_reloc of nothing")


def test_pnp_iterate_without_correspondences():
    """PnPsolver::iterate (:189-199): N < mRansacMinInliers sets bNoMore and
    returns an empty pose; the solver's state stays as it was."""
    it, best = np.array([2], np.int32), np.array([5], np.int32)
    bT = np.full(16, 3.0, np.float32)
    T = sent(16, np.float32)
    res, nm, ni, dc = sent(1), sent(1), sent(1), sent(1)
    inl, bm = sent(2, np.uint8), sent(2, np.uint8)
    P = orbpl.PnpProblem(500.0, 500.0, 320.0, 240.0, 0, None, None, None, 4, 10, None, 0, None,
                         p(it), p(best), None, p(bT), p(T), p(res), p(nm), p(ni), None, p(dc))
    check_ok(orbpl.lib().orbpnp_iterate(C.byref(P), 1, 5), "pnp_iterate")
    assert (res[0], nm[0], ni[0], dc[0], it[0], best[0]) == (0, 1, 0, 0, 2, 5)
    assert np.all(T == 0) and np.all(bT == 3.0) and kept(inl, 0) and kept(bm, 0)
    check_ok(orbpl.lib().orbpnp_iterate(None, 0, 5), "pnp_iterate of nothing")


# ---------------------------------------------------------------------------
# LocalMapping
# ---------------------------------------------------------------------------
def lm_keyframe(kid, n, nl, keep):
    k = keypoints(n)
    a = [EYE.copy(), k, k.copy(), np.full(n, U - 20.0, np.float32), np.full(n, 2.0, np.float32),
         DESC[:n].copy(), np.full(n, 3, np.int32), np.zeros(n, np.uint8), XYZ[:n].copy(),
         keylines(nl), DESC[:nl].copy(), np.zeros((nl, 3), np.float64)]
    keep.append(a)
    return orbpl.LmKeyFrame(kid, p(a[0]), n, *[p(x) for x in a[1:9]], nl, *[p(x) for x in a[9:]])


@pytest.mark.parametrize("n_neigh", [0, 1])
def test_create_new_map_features_of_an_empty_keyframe(n_neigh):
    """LocalMapping::CreateNewMapPoints / CreateNewMapLines loop over the current
    keyframe's features: without any, nothing is created and every pair count
    is that of an unmatched neighbour."""
    keep = []
    cam = orbpl.make_camera(CFG)
    nb = (orbpl.LmKeyFrame * 1)(lm_keyframe(1, 1, 1, keep))
    P = orbpl.LmProblem()
    P.cur, P.n_neigh, P.neigh = lm_keyframe(0, 0, 0, keep), n_neigh, C.cast(nb, C.c_void_p)
    P.n_points = P.n_lines = S
    check_ok(orbpl.lib().orblm_create_new_map_features(C.byref(cam), p(SCALE), p(SIGMA2), 8,
                                                       C.byref(P), 1), "create_new_map_features")
    assert (P.n_points, P.n_lines) == (0, 0)
    assert all(v <= 0 for v in P.pairs) and all(v <= 0 for v in P.line_pairs)
    check_ok(orbpl.lib().orblm_create_new_map_features(C.byref(cam), p(SCALE), p(SIGMA2), 8, None,
                                                       0), "create_new_map_features of nothing")


@pytest.mark.parametrize("n1,n2,opt", [(0, 0, False), (0, 1, True), (1, 0, False), (1, 0, True)])
def test_search_for_triangulation_with_an_empty_keyframe(n1, n2, opt):
    """opt: f12_in and f12_out present, else both NULL. ORBmatcher.cc:657-815
    pairs features of KF1 with features of KF2: an empty side leaves no pairs;
    the F12 handed in is the F12 used."""
    keep = []
    cam = orbpl.make_camera(CFG)
    a, b = lm_keyframe(0, n1, 0, keep), lm_keyframe(1, n2, 0, keep)
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)
    pairs, npairs, fout = sent(2 * (n1 + 2)).reshape(-1, 2), C.c_int(S), sent(9, np.float32)
    check_ok(orbpl.lib().orbm_search_for_triangulation(
        C.byref(cam), p(SCALE), p(SIGMA2), 8, C.byref(a), C.byref(b), p(F) if opt else None, 0, 0,
        p(pairs) if n1 else None, C.byref(npairs), p(fout) if opt else None), "triangulation")
    assert npairs.value == 0 and kept(pairs, 0)
    assert np.array_equal(fout, F) if opt else kept(fout, 0)


@pytest.mark.parametrize("nl1,nl2", COUNTS)
def test_line_search_for_triangulation(nl1, nl2):
    import _localmap_ref as R
    d1, d2 = DESC[:nl1].copy(), DESC[:nl2].copy()
    exp = np.array(R.line_search_for_triangulation(d1, d2), np.int32).reshape(-1, 2)
    pairs, n = sent(2 * (nl1 + 2)).reshape(-1, 2), C.c_int(S)
    check_ok(orbpl.lib().orbl_search_for_triangulation(nl1, p(d1), nl2, p(d2),
                                                       p(pairs) if nl1 else None, C.byref(n)),
             "line_triangulation")
    assert n.value == len(exp) and np.array_equal(pairs[:n.value], exp) and kept(pairs, n.value)

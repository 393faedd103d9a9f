"""GPU parity of Frame::ComputeStereoMatches (csrc/stereo.hip) branch by
branch and at 1 to 16 pyramid levels: orbpl.stereo_matches against the oracle,
bit for bit, on the hand-made cases and shifted pairs of
tests/_stereo_cases.py (test_stereo_ref.py shows on the CPU that every case
takes the branch it was made for and that the oracle equals a sequential
restatement of the reference), and the stereo tracker off the 8-level pyramid
against the oracle's loops."""
import numpy as np
import pytest

import _stereo_cases as SC

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4   # as test_gpu_track.py


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gpu_matches(orbpl, c):
    """orbpl.stereo_matches on the device pyramids of two extractors that
    extracted the case's images."""
    exl = orbpl.ORBextractor(*SC.orb_of(c), width=c.w, height=c.h)
    exr = orbpl.ORBextractor(*SC.orb_of(c), width=c.w, height=c.h)
    try:
        exl(c.left)
        exr(c.right)
        return orbpl.stereo_matches(orbpl.make_camera(SC.cfg_of(c)), exl, exr, c.kl, c.dl, c.kr,
                                    c.dr)
    finally:
        exl.close()
        exr.close()


def _check(orbpl, oracle, c):
    ur_o, d_o = SC.run_oracle(oracle, c)
    ur_g, d_g = _gpu_matches(orbpl, c)
    bad = np.nonzero((_u32(ur_g) != _u32(ur_o)) | (_u32(d_g) != _u32(d_o)))[0]
    assert len(bad) == 0, (c.name, bad[:8], ur_g[bad[:8]], ur_o[bad[:8]])
    return ur_o, d_o


@pytest.mark.parametrize("fn", SC.DIRECTED, ids=lambda f: f.__name__[5:])
def test_directed_case_bit_exact(orbpl, oracle, fn):
    """Row bands, octave gate, disparity window, descriptor thresholds and tie
    order (also across the 256-thread stride), endu, the pinned window skip,
    the SAD curve's edges, the disparity's edges, the median cut, and right
    keypoints that enter 33 rows each (a 2.0-factor pyramid's top level: the
    host entry point sizes the row-band scratch from the keypoints)."""
    _check(orbpl, oracle, SC.directed(fn))


def test_capacity_4096_bit_exact(orbpl, oracle):
    """n = nr = 4096, deciding keypoints at indices 0, 255, 256 and 4095, a
    SAD of 58650 in the packed sort key."""
    c = SC.directed(SC.case_capacity_4096)
    ur, d = _check(orbpl, oracle, c)
    assert d[0] > 0 and d[255] > 0 and d[256] > 0 and d[4095] == -1


def test_rows_1024_bit_exact_and_1025_refused(orbpl, oracle):
    """The row table holds exactly 1024 rows: keypoints on rows 0 and 1023 of
    a 1024-row frame match the oracle; 1025 rows stay refused."""
    c = SC.directed(SC.case_rows_1024)
    _check(orbpl, oracle, c)
    tall = c._replace(h=1025, left=np.zeros((1025, c.w), np.uint8),
                      right=np.zeros((1025, c.w), np.uint8))
    with pytest.raises(orbpl.OrbplError, match="image taller than 1024 rows"):
        _gpu_matches(orbpl, tall)
    with pytest.raises(orbpl.OrbplError, match="stereo tracking supports images up to 1024 rows"):
        orbpl.Tracker(orbpl.OrbParams(*SC.orb_of(tall)), orbpl.make_camera(SC.cfg_of(tall)), 1,
                      stereo=True)


SHIFTED = [(g, s) for s in SC.SHIFT_SIZES for g in SC.SHIFT_GEOMS]


@pytest.mark.parametrize("g,s", SHIFTED, ids=[SC.shifted_id(g, s) for g, s in SHIFTED])
def test_shifted_pair_bit_exact(orbpl, oracle, g, s):
    """Oracle keypoints of a textured image and its shifted copy at 1, 2, 4,
    5, 12 and 16 levels: the kernel argument's level table holds the
    extractor's 16."""
    c = SC.shifted_case(g[0], g[1], s[0], s[1])
    ur, d = _check(orbpl, oracle, c)
    assert (d > 0).sum() >= 0.3 * len(c.kl)


def test_mismatched_extractors_refused(orbpl):
    c = SC.directed(SC.case_median_one)
    exl = orbpl.ORBextractor(300, 1.2, 8, 20, 7, width=c.w, height=c.h)
    exr = orbpl.ORBextractor(300, 1.1, 12, 20, 7, width=c.w, height=c.h)
    exl(c.left)
    exr(c.right)
    with pytest.raises(orbpl.OrbplError, match="left and right extractors differ"):
        orbpl.stereo_matches(orbpl.make_camera(SC.cfg_of(c)), exl, exr, c.kl, c.dl, c.kr, c.dr)
    exl.close()
    exr.close()


def test_octave_outside_the_pyramid_refused(orbpl):
    """The host entry point reads the level table by the keypoints' octaves
    (to size the row-band scratch) and refuses one outside the pyramid, left
    or right, before anything is launched."""
    c = SC.directed(SC.case_median_one)
    for side, octave in (("kl", c.levels), ("kr", c.levels), ("kl", -1), ("kr", -1)):
        k = getattr(c, side).copy()
        k["octave"][0] = octave
        with pytest.raises(orbpl.OrbplError, match="keypoint octave outside the pyramid"):
            _gpu_matches(orbpl, c._replace(**{side: k}))


# --- the stereo tracker off the 8-level pyramid --------------------------------
# KITTI 00 camera cut down to 496 x 152 (500 features); with lines and with the
# map model 620 x 188 and 1000 features: StereoInitialization asks for more than
# 500 keypoints, and the line constraint for 10 line inliers
TRACKER_CASES = [
    ("l3_s2.0", 3, 2.0, False, 496, 152, 500),       # top scale 4: 4 s + 3 <= 20 rows per keypoint
    ("l12_s1.1", 12, 1.1, False, 496, 152, 500),
    ("l16_s1.05", 16, 1.05, False, 496, 152, 500),
    ("l12_s1.1_lines", 12, 1.1, True, 620, 188, 1000),
]


@pytest.mark.parametrize("name,levels,factor,lines,W,H,nf", TRACKER_CASES,
                         ids=[t[0] for t in TRACKER_CASES])
def test_stereo_tracker_off_8_levels_matches_oracle(orbpl, oracle, name, levels, factor, lines, W,
                                                    H, nf):
    """ORBPL_TRACK_STEREO at 3, 12 and 16 levels, 2 streams, 3 frames, against
    oracle.LVO.step_stereo: identical counts every frame, pose within
    POSE_TOL; the oracle tracks (ok, at least 20 matches after frame 0). The
    step fills the kernel argument's 16-entry level table on the stack
    (stereo_set_levels; `make levels_check` runs it under the host
    sanitizers)."""
    from _scenes import stereo_sequence
    S, F = 2, 3
    seqs = [stereo_sequence(F, 90 + s, "KITTI00", W, H) for s in range(S)]
    cfg = seqs[0][0]
    orb = (nf, factor, levels, 20, 7)
    lvo = oracle.LVO(oracle.params(*orb), oracle.camera(cfg), S, use_lines=lines)
    tr = orbpl.Tracker(orbpl.OrbParams(*orb), orbpl.make_camera(cfg), S, stereo=True, lines=lines)
    T0 = np.stack([np.linalg.inv(sq[1][0]).astype(np.float32) for sq in seqs])
    lvo.reset(T0.reshape(S, 16))
    tr.reset(T0.reshape(S, 16))
    left = orbpl.DeviceBuffer(S * W * H)
    right = orbpl.DeviceBuffer(S * W * H)
    for f in range(F):
        left.upload(np.stack([sq[2][f][0] for sq in seqs]))
        right.upload(np.stack([sq[2][f][1] for sq in seqs]))
        tr.step_stereo_device(left.ptr, right.ptr)
        tr.synchronize()
        st, ls = tr.state(), tr.status()
        for s in range(S):
            To, so = lvo.step_stereo(s, *seqs[s][2][f])
            got = dict(nkeypoints=st["nkeypoints"][s], nmatches=st["nmatches"][s],
                       ninliers=st["ninliers"][s], nmatches_map=st["nmatches_map"][s],
                       ok=ls["ok"][s], nlines=ls["nlines"][s], line_matches=ls["line_matches"][s],
                       line_nmatches_map=ls["line_nmatches_map"][s])
            assert {k: int(v) for k, v in got.items()} == so, (f, s)
            assert np.abs(st["Tcw"][s] - To).max() < POSE_TOL, (f, s)
            assert so["ok"] == 1
            if f > 0:
                assert so["nmatches"] >= 20
                if lines:
                    assert so["line_matches"] >= 10
    tr.close()


def test_stereo_map_tracker_12_levels_matches_oracle(orbpl, oracle):
    """The map model (ORBPL_TRACK_MAP) on stereo pairs at 12 levels of 1.1:
    the 24 counts of every frame identical to oracle.MapVO, pose within
    POSE_TOL, no capacity flag."""
    from _scenes import stereo_sequence
    S, F, W, H = 2, 3, 620, 188
    seqs = [stereo_sequence(F, 90 + s, "KITTI00", W, H) for s in range(S)]
    cfg = seqs[0][0]
    orb = (1000, 1.1, 12, 20, 7)
    mvo = oracle.MapVO(oracle.params(*orb), oracle.camera(cfg), S, use_lines=False,
                       flags=oracle.TRACK_STEREO)
    tr = orbpl.Tracker(orbpl.OrbParams(*orb), orbpl.make_camera(cfg), S, map=True, stereo=True)
    T0 = np.stack([np.linalg.inv(sq[1][0]).astype(np.float32) for sq in seqs])
    mvo.reset(T0.reshape(S, 16))
    tr.reset(T0.reshape(S, 16))
    tr.set_history(F)
    fa = S * W * H
    a = orbpl.DeviceBuffer(F * fa)
    b = orbpl.DeviceBuffer(F * fa)
    for f in range(F):
        a.upload(np.stack([sq[2][f][0] for sq in seqs]), offset=f * fa)
        b.upload(np.stack([sq[2][f][1] for sq in seqs]), offset=f * fa)
        tr.step_stereo_device(a.ptr + f * fa, b.ptr + f * fa)
    tr.synchronize()
    keys = orbpl.Tracker.MAP_COUNTS
    assert tuple(keys) == tuple(oracle.MAP_COUNTS) and len(keys) == 24
    for s in range(S):
        Th, _ = tr.history(s)
        Ch = tr.map_history(s)
        for f in range(F):
            To, co = mvo.step_stereo(s, *seqs[s][2][f])
            got = [int(x) for x in Ch[f]]
            want = [co[k] for k in keys]
            assert got == want, (s, f, [(k, g, w) for k, g, w in zip(keys, got, want) if g != w])
            assert np.abs(Th[f] - To).max() < POSE_TOL, (s, f)
            assert co["ok"] == 1 and (f == 0 or co["nmatches"] >= 20)
    assert (tr.map_errors() == 0).all()
    tr.close()

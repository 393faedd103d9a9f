"""The package's pitched column packer (orbpl.PitchedProblems over _pack_rows) on
the CPU: the host arrays of PnpDeviceProblems, Sim3DeviceProblems,
Sim3MatchDeviceProblems and LmDeviceProblems for two problems of different size,
with device=None (no device buffer, no library call). Every column: the inputs
where a problem fills it, the padding value elsewhere. And the stand-alone check
of the C++ side of the same layout (csrc/host_rows.h)."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from _pkg import load_pkg

orbpl = load_pkg()
f32, i32, u8 = np.float32, np.int32, np.uint8


def check_columns(dev, want, pads):
    """dev.host has exactly the columns of `want`; a column's row s starts with
    want[name][s] and everything after it, and every further row, is the pad"""
    assert not hasattr(dev, "bufs") and not hasattr(dev, "batch")
    assert set(dev.host) == set(want)
    for name, rows in want.items():
        a = dev.host[name]
        flat = a.reshape(a.shape[0], -1)
        assert len(rows) <= len(flat), name
        for s in range(len(flat)):
            w = np.ascontiguousarray(rows[s] if s < len(rows) else [], a.dtype).reshape(-1)
            assert flat[s, :len(w)].tobytes() == w.tobytes(), (name, s)
            rest = flat[s, len(w):]
            assert rest.tobytes() == np.full(rest.shape, pads.get(name, 0), a.dtype).tobytes(), (name, s)


def test_pack_rows():
    a = orbpl._pack_rows([[1, 2, 3], None, []], 4, i32, pad=-1)
    assert a.tolist() == [[1, 2, 3, -1], [-1] * 4, [-1] * 4]
    b = orbpl._pack_rows([np.arange(6)], 3, f32, (2,))
    assert b.shape == (1, 3, 2) and b.ravel().tolist() == [0, 1, 2, 3, 4, 5]
    assert orbpl._pack_rows([], 2, u8, (32,), 1).tolist() == [[[1] * 32] * 2]       # no problem: one row
    assert orbpl._pack_rows([5, 6], None, i32).tolist() == [5, 6]
    assert orbpl._pack_rows([np.eye(4)], None, f32, (16,)).shape == (1, 16)


def test_pnp_columns_on_the_host():
    rng = np.random.default_rng(1)
    ps = []
    for n in (0, 5):
        ps.append(dict(cam=(500 + n, 501, 320, 240), p2d=rng.random((n, 2)), p3d=rng.random((n, 3)),
                       max_error=rng.random(n), min_inliers=4 + n, max_its=10 + n,
                       draws=rng.integers(0, 1000, 2 * n + 2)))
    ps[1]["state"] = dict(iterations=3, best_inliers=4, best_mask=[1, 0, 1, 1, 0], best_Tcw=rng.random((4, 4)))
    dev = orbpl.PnpDeviceProblems(ps, draw_pitch=16, device=None)
    assert (dev.ns, dev.pt_pitch, dev.draw_pitch, dev.n.tolist()) == (2, 5, 16, [0, 5])
    assert dev.host["p2d"].shape == (2, 5, 2) and dev.host["draws"].shape == (2, 16)
    st = [orbpl.pnp_new_state(0), ps[1]["state"]]
    want = {k: [p[k] for p in ps] for k in ("cam", "p2d", "p3d", "max_error", "min_inliers", "max_its", "draws")}
    want.update({k: [s[k] for s in st] for k in ("iterations", "best_inliers", "best_mask", "best_Tcw")})
    want.update(n=[0, 5], **{k: [] for k in ("Tcw", "result", "no_more", "n_inliers", "inliers", "draws_consumed")})
    check_columns(dev, want, {})
    # draws beyond the pitch are cut, and no problem at all is one row of padding
    cut = orbpl.PnpDeviceProblems([dict(ps[1], draws=np.arange(40))], draw_pitch=16, device=None)
    assert cut.host["draws"].tolist() == [list(range(16))]
    none = orbpl.PnpDeviceProblems([], device=None)
    assert none.host["p3d"].shape == (1, 1, 3) and not none.host["n"].any()


def _sim3_pair(rng, n1, n2):
    return dict(matched12=rng.integers(-2, max(n2, 1), n1), valid1=rng.integers(0, 2, n1),
                xyz1=rng.random((n1, 3)), octave1=rng.integers(0, 8, n1), valid2=rng.integers(0, 2, n2),
                xyz2=rng.random((n2, 3)), octave2=rng.integers(0, 8, n2), Tcw1=rng.random((4, 4)),
                Tcw2=rng.random((4, 4)), cam=(500 + n1, 501, 320, 240), fix_scale=n1 > 2,
                draws=rng.integers(0, 1000, 7 + n1))


def test_sim3_columns_on_the_host():
    rng = np.random.default_rng(2)
    ps = [_sim3_pair(rng, 0, 4), dict(_sim3_pair(rng, 5, 2), min_inliers=9)]
    sig = np.arange(1, 9, dtype=f32)
    dev = orbpl.Sim3DeviceProblems(ps, sig, minInliers=6, draw_pitch=16, device=None)
    assert (dev.ns, dev.pitch1, dev.pitch2, dev.nlevels) == (2, 5, 4, 8) and not hasattr(dev, "setup_batch")
    assert dev.host["xyz1"].shape == (2, 5, 3) and dev.host["X3Dc1"].shape == (2, 5, 3)
    assert dev.host["max_error1"].shape == (2, 5, 1) and dev.host["best_s"].shape == (2, 1)
    want = {k: [p[k] for p in ps] for k in ("matched12", "valid1", "xyz1", "octave1", "valid2", "xyz2",
                                            "octave2", "Tcw1", "Tcw2", "cam", "fix_scale", "draws")}
    want.update(n1=[0, 5], n2=[4, 2], min_inliers=[6, 9], level_sigma2=[sig[:1], sig[1:2]] + [[v] for v in sig[2:]])
    out = ("n", "indices1", "max_its", "iterations", "best_inliers", "best_mask", "T12", "result", "no_more",
           "n_inliers", "inliers", "draws_consumed", "X3Dc1", "X3Dc2", "P1im1", "P2im2", "max_error1",
           "max_error2", "best_T12", "best_R", "best_t", "best_s")
    want.update({k: [] for k in out})
    check_columns(dev, want, dict(matched12=-1, max_its=1))


def _sbs_keyframe(rng, n):
    kps = np.zeros(n, orbpl.KP_DTYPE)
    kps["x"], kps["octave"] = rng.random(n), rng.integers(0, 8, n)
    return dict(kps_un=kps, desc=rng.integers(0, 256, (n, 32)), valid=rng.integers(0, 2, n),
                xyz=rng.random((n, 3)), min_dist=rng.random(n), max_dist=rng.random(n),
                mp_desc=rng.integers(0, 256, (n, 32)), Tcw=rng.random((4, 4)))


def test_search_by_sim3_columns_on_the_host():
    rng = np.random.default_rng(3)
    ps = [dict(kf1=_sbs_keyframe(rng, n1), kf2=_sbs_keyframe(rng, n2), s12=1.5 + n1, R12=rng.random((3, 3)),
               t12=rng.random(3), matched12=rng.integers(-2, 3, n1)) for n1, n2 in ((2, 0), (1, 3))]
    dev = orbpl.Sim3MatchDeviceProblems(ps, device=None)
    assert (dev.ns, dev.pitch) == (2, (2, 3)) and dev.host_matched12 is dev.host["matched12"]
    assert dev.host["desc1"].shape == (2, 2, 32) and dev.host["kps_un2"].shape == (2, 3)
    want = {"%s%d" % (k, s): [p["kf%d" % s][k] for p in ps]
            for s in (1, 2) for k in ("kps_un", "desc", "valid", "xyz", "min_dist", "max_dist", "mp_desc", "Tcw")}
    want.update({k: [p[k] for p in ps] for k in ("s12", "R12", "t12", "matched12")})
    want.update(n1=[2, 1], n2=[0, 3], n_found=[], vn_match1=[], vn_match2=[], reason1=[], reason2=[])
    check_columns(dev, want, dict(matched12=-1))


def _lm_keyframe(rng, kid, n, nl):
    kps, kl = np.zeros(n, orbpl.KP_DTYPE), np.zeros(nl, orbpl.KEYLINE_DTYPE)
    kps["x"], kl["angle"] = rng.random(n), rng.random(nl)
    return dict(id=kid, Tcw=rng.random((4, 4)), kps=kps, kps_un=kps[::-1].copy(), uright=rng.random(n),
                depth=rng.random(n), desc=rng.integers(0, 256, (n, 32)), feat_node=rng.integers(0, 99, n),
                has_mp=rng.integers(0, 2, n), mp_xyz=rng.random((n, 3)), klines=kl,
                ldesc=rng.integers(0, 256, (nl, 32)), lcoef=rng.random((nl, 3)))


def test_local_mapping_columns_on_the_host():
    rng = np.random.default_rng(4)
    ps = [dict(cur=_lm_keyframe(rng, 3, 0, 0), neigh=[]),
          dict(cur=_lm_keyframe(rng, 4, 2, 1), neigh=[_lm_keyframe(rng, 5, 3, 0), _lm_keyframe(rng, 6, 1, 2)])]
    dev = orbpl.LmDeviceProblems(None, ps, device=None)
    assert (dev.ns, dev.pitch, dev.line_pitch, dev.n1, dev.nl1) == (2, 3, 2, [0, 2], [0, 1])
    kfs = [ps[0]["cur"], ps[1]["cur"]] + ps[1]["neigh"]
    assert dev.host["desc"].shape == (4, 3, 32) and dev.host["lcoef"].shape == (4, 2, 3)
    assert dev.host["lines"].shape == (2, 20) and dev.host["points"].shape == (2, 3)
    assert dev.host["pairs"].shape == (2, 10) and dev.host["neigh"].shape == (2, 10)
    want = {k: [kf[k] for kf in kfs] for k in ("kps", "kps_un", "uright", "depth", "desc", "feat_node", "has_mp",
                                               "mp_xyz", "klines", "ldesc", "lcoef")}
    want.update(kf_id=[3, 4, 5, 6], kf_n=[0, 2, 3, 1], kf_nl=[0, 1, 0, 2], kf_Tcw=[kf["Tcw"] for kf in kfs],
                cur=[0, 1], neigh=[[], [2, 3]])
    want.update({k: [] for k in ("points", "lines", "n_points", "n_lines", "kf1_point_record", "kf1_line_record",
                                 "pairs", "line_pairs")})
    check_columns(dev, want, dict(uright=-1, depth=-1, feat_node=-1, has_mp=1, neigh=-1))
    twice = orbpl.LmDeviceProblems(None, ps, device=None, repeat=2)                # the one pool, run twice
    assert twice.ns == 4 and twice.host["cur"].tolist() == [0, 1, 0, 1] and twice.host["kf_id"].shape == (4,)
    assert twice.host["neigh"][3].tolist() == [2, 3] + [-1] * 8 and twice.host["points"].shape == (4, 3)


def test_rows_check_builds_and_runs():
    """Rows and every pack struct of csrc/host_rows.h against hand-written
    values, as a program of its own under the host sanitizers"""
    if shutil.which("make") is None or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None:
        pytest.skip("no make or no hipcc (the Makefile's HIPCC)")
    csrc = Path(orbpl.__file__).resolve().parent / "csrc"
    subprocess.run(["make", "-C", str(csrc), "rows_check"], check=True, capture_output=True)
    out = subprocess.run([str(csrc.parent / "host_rows_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host_rows_check: ok" in out.stdout

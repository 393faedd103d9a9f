"""CPU: the restatement of Sim3Solver (tests/_sim3_ref.py) on its own terms -
the parameter table, the pinned Jacobi eigen-decomposition, Horn's closed
form, the constructor and the semantics of iterate() - the host C functions
against it, and the admissibility of every problem the GPU tests use."""
import copy
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _sim3_ref as ref
from _sim3_problems import (SIGMA2, TRUNCATED_POINT, big_problems, direct_problem,
                            exactly_min_inliers, identical_points, make_problem, problems,
                            pure_translation, ref_run, ref_solver, truncated_threshold)

F = np.float32


# ---------------------------------------------------------------- parameter table
@pytest.mark.parametrize("N,its", [(25, 7), (100, 300), (20, 1), (0, 1)])
def test_ransac_parameters_known_answers(orbpl, N, its):
    """SetRansacParameters(0.99, 20, 300), ComputeSim3's parameters"""
    assert ref.ransac_parameters(N, 0.99, 20, 300) == its
    assert orbpl.sim3_ransac_parameters(N, 0.99, 20, 300) == its


def test_ransac_parameters_host_equals_restatement(orbpl):
    for mn in (3, 6, 20):
        for N in list(range(0, 130)) + [500, 2048]:
            for prob, mx in ((0.99, 300), (0.5, 10)):
                assert orbpl.sim3_ransac_parameters(N, prob, mn, mx) == \
                    ref.ransac_parameters(N, prob, mn, mx), (N, mn, prob, mx)
    # fewer points than inliers: epsilon > 1, the log of a negative number
    assert ref.ransac_parameters(5, 0.99, 20, 300) == 1


# ---------------------------------------------------------------- pinned cv::eigen
def _sym(rng, traceless):
    a = rng.normal(size=(4, 4))
    a = a + a.T
    if traceless:
        a -= np.eye(4) * np.trace(a) / 4
    return a


def _check_eig(a0):
    a = [[float(x) for x in row] for row in a0]
    k, v = ref.eig_jacobi4(a)
    v = np.array(v)
    lam = np.array([a[i][i] for i in range(4)])
    w = np.linalg.eigh(np.array(a0, np.float64))[0]
    scale = max(1.0, float(np.abs(w).max()))
    assert np.abs(np.sort(lam) - w).max() <= 1e-13 * scale
    assert np.abs(v.T @ v - np.eye(4)).max() <= 1e-13
    assert np.abs(np.array(a0) @ v - v * lam).max() <= 1e-12 * scale
    assert lam[k] == lam.max() and k == int(np.argmax(lam))
    return lam, k


def test_pinned_jacobi_is_an_eigen_decomposition():
    rng = np.random.default_rng(7)
    negative_dominant = 0
    for trial in range(60):
        a = _sym(rng, traceless=trial % 2 == 0)
        lam, k = _check_eig(a)
        if trial % 2 == 0 and abs(lam.min()) > lam.max():
            negative_dominant += 1       # an SVD would pick this one
    assert negative_dominant >= 5
    # a traceless matrix whose eigenvalue of largest magnitude is negative, by construction
    q = np.linalg.qr(rng.normal(size=(4, 4)))[0]
    lam, k = _check_eig(q @ np.diag([-6.0, 1.0, 2.0, 3.0]) @ q.T)
    assert abs(lam[k] - 3.0) < 1e-12


def test_pinned_jacobi_on_N_of_real_samples():
    for p in (make_problem(30, noise=0.0, seed=301, extras=False),
              make_problem(30, 0.5, seed=302, extras=False)):
        c = ref.setup(p["pair"], SIGMA2)
        for k in range(10):
            idx = ref.sample3(p["draws"][3 * k:3 * k + 3], c["n"])
            P1 = [[c["X3Dc1"][idx[j]][r] for j in range(3)] for r in range(3)]
            P2 = [[c["X3Dc2"][idx[j]][r] for j in range(3)] for r in range(3)]
            N = ref.horn_N(P1, P2)[4]
            assert abs(sum(float(N[i][i]) for i in range(4))) < 1e-4    # traceless
            _check_eig([[float(x) for x in row] for row in N])


def test_pinned_jacobi_terminates_on_zero_and_nan():
    k, v = ref.eig_jacobi4([[0.0] * 4 for _ in range(4)])
    assert k == 0 and np.array_equal(np.array(v), np.eye(4))
    a = [[float("nan")] * 4 for _ in range(4)]
    k, v = ref.eig_jacobi4(a)
    assert k == 0 and np.array_equal(np.array(v), np.eye(4))     # nothing rotated
    a = [[1.0, float("nan"), 0, 0], [float("nan"), 2.0, 0, 0], [0, 0, 3.0, 0.5], [0, 0, 0.5, 1.0]]
    ref.eig_jacobi4(a)                                           # bounded by MAX_SWEEPS


# ---------------------------------------------------------------- ComputeSim3
def _horn_double(P1, P2, fix):
    """Horn's closed form in double with numpy.linalg.eigh on the same points"""
    P1, P2 = np.array(P1, np.float64), np.array(P2, np.float64)
    O1, O2 = P1.mean(axis=1, keepdims=True), P2.mean(axis=1, keepdims=True)
    A, B = P1 - O1, P2 - O2
    M = B @ A.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2],
                   M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    q = np.linalg.eigh(N)[1][:, 3]
    w, x, y, z = q if q[0] >= 0 else -q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    P3 = R @ B
    s = 1.0 if fix else float((A * P3).sum() / (P3 * P3).sum())
    return R, (O1 - s * R @ O2).ravel(), s


HORN_MEASURED = 1.75e-5


@pytest.mark.parametrize("fix", [False, True])
def test_compute_sim3_noise_free(fix):
    """The float ComputeSim3 against Horn's closed form in double (eigh) on the
    same three float points, 12 noise-free problems x 8 samples per scale mode:
    the largest distance in any entry of R, t or s measured is 1.75e-5 (float
    rounding in a 3-point fit; it varies with the sample's conditioning), and
    4 x that is allowed. The double solution itself is within 8.8e-6 of the
    ground truth (the inputs are rounded to float); 1e-4 is allowed."""
    worst = worst_truth = 0.0
    for seed in range(200, 212):
        p = make_problem(40, noise=0.0, fix_scale=fix, seed=seed, extras=False)
        c = ref.setup(p["pair"], SIGMA2)
        for k in range(8):
            idx = ref.sample3(p["draws"][3 * k:3 * k + 3], c["n"])
            P1 = [[c["X3Dc1"][idx[j]][r] for j in range(3)] for r in range(3)]
            P2 = [[c["X3Dc2"][idx[j]][r] for j in range(3)] for r in range(3)]
            R, t, s = ref.compute_sim3(P1, P2, fix)
            Rd, td, sd = _horn_double(P1, P2, fix)
            worst = max(worst, np.abs(np.array(R, np.float64).reshape(3, 3) - Rd).max(),
                        np.abs(np.array(t, np.float64) - td).max(), abs(float(s) - sd))
            worst_truth = max(worst_truth, np.abs(Rd - p["R12"]).max(),
                              np.abs(td - p["t12"]).max(), abs(sd - p["s12"]))
            if fix:
                assert s == F(1.0)
    print(f"fix_scale={fix}: float vs double Horn {worst:g}, double Horn vs truth {worst_truth:g}")
    assert worst <= 4 * HORN_MEASURED
    assert worst_truth <= 1e-4


def _hook(orbpl, P1, P2, fix, cam, c):
    n = c["n"]
    R, t, s, T = np.zeros(9, F), np.zeros(3, F), np.zeros(1, F), np.zeros(16, F)
    err, inl = np.zeros((max(1, n), 2), F), np.zeros(max(1, n), np.uint8)
    a = [np.ascontiguousarray(x) for x in
         (np.array(P1, F).T, np.array(P2, F).T, np.array(cam, F), c["X3Dc1"], c["X3Dc2"],
          c["P1im1"], c["P2im2"], c["max_error1"], c["max_error2"])]
    pt = orbpl._ptr
    orbpl.check(orbpl.lib().orbpl_test_sim3_hypothesis(
        pt(a[0]), pt(a[1]), int(fix), pt(a[2]), n, *[pt(x) for x in a[3:]], pt(R), pt(t), pt(s),
        pt(T), pt(err), pt(inl)), "orbpl_test_sim3_hypothesis")
    return R, t, s[0], T.reshape(4, 4), err[:n], inl[:n].astype(bool)


def test_host_core_equals_restatement_bit_for_bit(orbpl):
    """sim3_core.h, the header the kernel shares, compiled for the host:
    ComputeSim3 and CheckInliers on the first hypotheses of every problem"""
    for name, p in problems().items():
        c = ref.setup(p["pair"], SIGMA2)
        if c["n"] < 3:
            continue
        for k in range(5):
            idx = ref.sample3(p["draws"][3 * k:3 * k + 3], c["n"])
            P1 = [[c["X3Dc1"][idx[j]][r] for j in range(3)] for r in range(3)]
            P2 = [[c["X3Dc2"][idx[j]][r] for j in range(3)] for r in range(3)]
            R, t, s = ref.compute_sim3(P1, P2, p["fix_scale"])
            m, e1, e2 = ref.check_inliers(R, t, s, [F(x) for x in p["pair"]["cam"]], c)
            hR, ht, hs, hT, herr, hinl = _hook(orbpl, P1, P2, p["fix_scale"], p["pair"]["cam"], c)
            assert np.array_equal(np.array(R, F), hR, equal_nan=True), (name, k)
            assert np.array_equal(np.array(t, F), ht, equal_nan=True), (name, k)
            assert np.array_equal(F(s), hs, equal_nan=True), (name, k)
            assert np.array_equal(ref.to_T12(R, t, s), hT, equal_nan=True), (name, k)
            assert np.array_equal(e1, herr[:, 0], equal_nan=True), (name, k)
            assert np.array_equal(e2, herr[:, 1], equal_nan=True), (name, k)
            assert np.array_equal(m, hinl), (name, k)


# ---------------------------------------------------------------- the constructor
def _same_setup(got, want, what):
    assert got["n"] == want["n"], what
    for k in want:
        if k != "n":
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)


def test_setup_host_equals_restatement(orbpl):
    ps = list(problems().values()) + big_problems()[:1]
    got = orbpl.sim3_setup([p["pair"] for p in ps], SIGMA2)
    for p, g in zip(ps, got):
        want = ref.setup(p["pair"], SIGMA2)
        _same_setup(g, want, p["name"])
        if "N" in p:
            assert want["n"] == p["N"]


def test_setup_skips_each_kind_and_truncates_every_level(orbpl):
    """feature 0 no match, 1 without a good point of its own, 2 matched to a
    bad point, 3 matched to a point keyframe 2 does not observe (-2), 4..11
    accepted at levels 0..7 on side 1 and 7..0 on side 2"""
    rng = np.random.default_rng(5)
    n1, n2 = 12, 10
    xyz = lambda n: np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
                              rng.uniform(3, 6, n)], axis=1).astype(F)
    pair = dict(matched12=np.array([-1, 0, 1, -2] + list(range(2, 10)), np.int32),
                valid1=np.array([1, 0] + [1] * 10, np.uint8), xyz1=xyz(n1),
                octave1=np.array([0, 0, 0, 0] + list(range(8)), np.int32),
                valid2=np.array([1, 0] + [1] * 8, np.uint8), xyz2=xyz(n2),
                octave2=np.array([0, 0] + list(range(7, -1, -1)), np.int32),
                Tcw1=np.eye(4, dtype=F), Tcw2=np.eye(4, dtype=F), cam=(500.0, 500.0, 320.0, 240.0))
    want = ref.setup(pair, SIGMA2)
    assert list(want["indices1"]) == list(range(4, 12))
    # 9.21 * 1.2^(2 l), truncated toward zero
    trunc = [9, 13, 19, 27, 39, 57, 82, 118]
    assert list(want["max_error1"]) == trunc and list(want["max_error2"]) == trunc[::-1]
    _same_setup(orbpl.sim3_setup([pair], SIGMA2)[0], want, "kinds")
    # every accepted point is in front of both cameras
    assert (want["X3Dc1"][:, 2] > 0).all() and (want["X3Dc2"][:, 2] > 0).all()


def test_setup_refusals(orbpl):
    p = make_problem(8, seed=1)["pair"]
    for edit in (dict(matched12=np.full(len(p["matched12"]), len(p["valid2"]), np.int32)),
                 dict(matched12=np.full(len(p["matched12"]), -3, np.int32)),
                 dict(octave1=np.full(len(p["octave1"]), 8, np.int32)),
                 dict(octave2=np.full(len(p["octave2"]), -1, np.int32))):
        with pytest.raises(orbpl.OrbplError, match="failed with -1"):
            orbpl.sim3_setup([dict(p, **edit)], SIGMA2)


# ---------------------------------------------------------------- iterate(): the semantics
def test_loop_bound_is_a_conjunction():
    """a call runs min(nIterations, mRansacMaxIts - mnIterations) hypotheses"""
    p = problems()["N25_o15_fix_s112"]          # never succeeds, max_its = 40
    s = ref_solver(p)
    assert s.max_its == 40
    assert s.iterate(7, p["draws"])["draws_consumed"] == 21 and s.iterations == 7
    o = s.iterate(100, p["draws"][21:])
    assert o["draws_consumed"] == 3 * 33 and s.iterations == 40 and o["no_more"]
    assert s.hypotheses(5) == 0


def test_no_work_after_exhaustion():
    r = ref_run(problems()["N25_o15_fix_s112"])
    s = copy.deepcopy(r["solver"])
    before = s.state()
    o = s.iterate(5, np.zeros(0, np.int32))      # needs no draw
    assert o["result"] == 0 and o["no_more"] and o["draws_consumed"] == 0 and o["n_inliers"] == 0
    assert not o["T12"].any() and not o["inliers"].any()
    after = s.state()
    assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before)


def test_too_few_points_return_no_more_with_nothing_consumed():
    for N in (0, 2, 5):
        p = make_problem(N, seed=9, extras=False, min_inliers=6)
        s = ref_solver(p)
        o = s.iterate(5, p["draws"])
        assert o["no_more"] and o["result"] == 0 and o["draws_consumed"] == 0
        assert s.iterations == 0 and s.best_inliers == 0


def test_a_later_tie_replaces_the_best():
    """all inliers, min_inliers = N: the strict > never passes and every
    hypothesis ties the count; the state is the last hypothesis"""
    p = make_problem(10, noise=0.0, seed=31, extras=False, min_inliers=10, name="tie")
    s = ref_solver(p)
    s.SetRansacParameters(0.99, 10, 300)
    s.max_its = 4                                # (minInliers == N gives 1)
    o = s.iterate(2, p["draws"])
    first = s.state()
    assert o["result"] == 0 and first["best_inliers"] == 10
    s.iterate(1, p["draws"][6:])
    second = s.state()
    assert second["best_inliers"] == 10
    assert not np.array_equal(first["best_T12"], second["best_T12"])
    c = s.c
    idx = ref.sample3(p["draws"][6:9], 10)
    R, t, sc = ref.compute_sim3([[c["X3Dc1"][idx[j]][r] for j in range(3)] for r in range(3)],
                                [[c["X3Dc2"][idx[j]][r] for j in range(3)] for r in range(3)],
                                False)
    assert np.array_equal(second["best_T12"], ref.to_T12(R, t, sc))
    assert not s.margins.count_fragile


def test_success_needs_more_than_min_inliers():
    p = exactly_min_inliers()
    r = ref_run(p)
    s = r["solver"]
    assert all(o["result"] == 0 for _, o, _ in r["calls"])
    assert s.best_inliers == p["min_inliers"] == 6 and s.iterations == s.max_its
    assert r["calls"][-1][1]["no_more"] and not any(o["no_more"] for _, o, _ in r["calls"][:-1])
    assert sum(o["draws_consumed"] for _, o, _ in r["calls"]) == 3 * s.max_its


@pytest.mark.parametrize("make", [pure_translation, identical_points])
def test_first_hypothesis_with_no_inlier_becomes_the_best(make):
    """norm(vec) == 0: T12 is not a number, every point is an outlier, and 0 >=
    0 stores it"""
    p = make()
    s = ref_solver(p)
    o = s.iterate(1, p["draws"])
    st = s.state()
    assert o["result"] == 0 and st["best_inliers"] == 0 and st["iterations"] == 1
    assert np.isnan(st["best_T12"][:3]).all() and np.isnan(st["best_R"]).all()
    assert not st["best_mask"].any()


def test_truncated_threshold_makes_an_outlier():
    p = truncated_threshold()
    s = ref_solver(p)
    assert set(s.c["max_error1"]) == {13} and set(s.c["max_error2"]) == {13}
    assert ref.sample3(p["draws"][:3], 9) == [0, 8, 7]
    c = s.c
    idx = [0, 8, 7]
    R, t, sc = ref.compute_sim3([[c["X3Dc1"][idx[j]][r] for j in range(3)] for r in range(3)],
                                [[c["X3Dc2"][idx[j]][r] for j in range(3)] for r in range(3)],
                                False)
    m, e1, e2 = ref.check_inliers(R, t, sc, s.cam, c)
    k = TRUNCATED_POINT
    full = 9.210 * float(SIGMA2[1])
    assert 13.0 < e1[k] < full and 13.0 < e2[k] < full, (e1[k], e2[k], full)
    assert not m[k] and m.sum() == 8
    o = s.iterate(5, p["draws"])
    assert o["result"] == 1 and o["n_inliers"] == 8 and not o["inliers"][k]


# ---------------------------------------------------------------- admissibility
def test_every_problem_is_admissible():
    """A condition on the problems, not a measurement: in every problem the GPU
    tests use - driven by iterate(5), and by find() where they use it - no err1
    / err2 lies within a relative 1e-6 of its threshold and no count decision
    is fragile, so the labels and counts are the same under any rounding-sized
    difference."""
    runs = []
    for p in list(problems().values()) + big_problems():
        runs.append((p["name"], ref_run(p)["solver"]))
    for name in ("N100_o60_free_s121", "N257_o154_fix_s124", "N25_o15_fix_s112"):
        p = problems()[name]
        s = ref_solver(p)
        s.find(p["draws"])
        runs.append((name + " find", s))
    for name, s in runs:
        assert s.margins.min_rel >= 1e-6, (name, s.margins.min_rel)
        assert not s.margins.count_fragile, name


def _search(pair):
    from _sim3_problems import TH, ref_camera
    return ref.search_by_sim3(ref_camera(), pair["kf1"], pair["kf2"], pair["matched12"],
                              pair["s12"], pair["R12"], pair["t12"], TH)


def test_search_by_sim3_branches_are_what_they_say():
    """every hand-made pair takes the branch it is named after in the
    restatement, with margins far from rounding"""
    from _sim3_problems import hand_cases
    seen = set()
    for name, (pair, d, reason, vn, found) in hand_cases().items():
        o = _search(pair)
        assert o["reason%d" % d][0] == reason and o["vn_match%d" % d][0] == vn, name
        assert o["n_found"] == found, name
        assert o["margins"].min_rel() >= 1e-6, (name, o["margins"].min_rel())
        seen.add((d, reason))
    assert seen == {(d, r) for d in (1, 2) for r in range(8)}
    tie = _search(hand_cases()["tie_across_cells_dir1"][0])
    assert tie["margins"].hamming_tie == 1
    assert _search(hand_cases()["distance_th_high_dir2"][0])["margins"].at_th_high == 1


def test_every_matcher_scene_is_admissible():
    """no float threshold decision of any seeded scene the GPU tests use lies
    within a relative 1e-6 of its boundary; the integer decisions (octave
    gate, Hamming minimum and its ties, TH_HIGH) are exact in any
    implementation and the compared vnMatch shows how a tie was resolved"""
    from _sim3_problems import scene
    sizes = [(37, 41), (1, 1), (300, 120), (64, 65), (257, 256), (8, 200), (0, 5), (5, 0)]
    scenes = [scene(500, 1), scene(2048, 2)]
    scenes += [scene(a, 100 + k % 16, b) for k in range(40) if k % 3 != 2
               for a, b in [sizes[k % len(sizes)]]]
    for s in scenes:
        o = _search(s)
        assert o["margins"].min_rel() >= 1e-6, (s["name"], o["margins"].min_rel())


def test_sim3_check_builds_and_runs(orbpl):
    """the parameter table, orbsim3_setup, the validation and pool staging of
    orbsim3_iterate and its no-device failure path, as a program of its own
    under the host sanitizers"""
    if shutil.which("make") is None or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None:
        pytest.skip("no make or no hipcc (the Makefile's HIPCC)")
    csrc = Path(orbpl.__file__).resolve().parent / "csrc"
    subprocess.run(["make", "-C", str(csrc), "sim3_check"], check=True, capture_output=True)
    out = subprocess.run([str(csrc.parent / "sim3_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sim3_check: ok" in out.stdout or "a device is present" in out.stdout

"""CPU tests of the PnPsolver restatement (tests/_pnp_ref.py, DESIGN.md P28 /
P29): SetRansacParameters known answers (also through the C library's
orbpnp_ransac_parameters and the package's pnp_ransac_parameters), RandomInt,
the pinned Jacobi SVD against numpy.linalg, compute_pose against ground truth,
the bookkeeping known answers, and the admissibility of every problem the GPU
comparison uses. No GPU calls."""
import ctypes as C

import numpy as np
import pytest

import _pnp_ref as ref
from _pnp_problems import (DEFAULTS, all_outliers, big_problem, make_problem, problems, ref_run,
                           ten_of_twenty)

# worked by hand from PnPsolver.cc:121-157 with (0.99, 10, 300, 4, 0.5, 5.991):
# N = 100: int(100 * 0.5f) = 50; eps 0.5; ceil(log(0.01) / log(1 - 0.125)) = ceil(34.49) = 35
# N = 15:  int(7.5) = 7 -> 10; eps = 10/15; ceil(log(0.01) / log(1 - 0.2963)) = ceil(13.1) = 14
# N = 10:  min = 10 = N -> nIterations = 1
KNOWN = [(100, 50, np.float32(0.5), 35), (15, 10, np.float32(10) / np.float32(15), 14),
         (10, 10, np.float32(1.0), 1)]


@pytest.mark.parametrize("N,mn,eps,its", KNOWN)
def test_ransac_parameters_known_answers(orbpl, N, mn, eps, its):
    got = ref.ransac_parameters(N, *DEFAULTS)
    assert (got[0], got[1]) == (mn, its) and got[2] == eps
    pk = orbpl.pnp_ransac_parameters(N, *DEFAULTS)
    assert (pk[0], pk[1]) == (mn, its) and pk[2] == eps
    # the C library, with mvMaxError
    sigma2 = (np.arange(N) % 8 + 1).astype(np.float32)
    o_mn, o_its = np.zeros(1, np.int32), np.zeros(1, np.int32)
    o_eps, me = np.zeros(1, np.float32), np.zeros(N, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = orbpl.lib().orbpnp_ransac_parameters(N, DEFAULTS[0], DEFAULTS[1], DEFAULTS[2],
                                              DEFAULTS[3], DEFAULTS[4], DEFAULTS[5], p(sigma2),
                                              p(o_mn), p(o_its), p(o_eps), p(me))
    assert rc == 0
    assert (int(o_mn[0]), int(o_its[0])) == (mn, its) and o_eps[0] == eps
    assert np.array_equal(me, sigma2 * np.float32(5.991))
    assert np.array_equal(ref.ransac_parameters(N, *DEFAULTS, sigma2=sigma2)[3], me)


def test_ransac_parameters_degenerate_counts(orbpl):
    """N = 0 divides by zero in float: the quotient is not a finite int, which
    the project pins to INT_MIN, so mRansacMaxIts = max(1, INT_MIN) = 1"""
    o_mn, o_its, o_eps = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert orbpl.lib().orbpnp_ransac_parameters(0, 0.99, 10, 300, 4, 0.5, 5.991, None, p(o_mn),
                                                p(o_its), p(o_eps), None) == 0
    assert (int(o_mn[0]), int(o_its[0])) == (10, 1)
    assert ref.ransac_parameters(0, *DEFAULTS)[:2] == (10, 1)
    assert orbpl.pnp_ransac_parameters(0, *DEFAULTS)[:2] == (10, 1)


def test_too_few_points_return_no_more_with_nothing_consumed():
    p = make_problem(8, seed=1)
    s = ref.PnPsolver(p["cam"], p["p2d"], p["sigma2"], p["p3d"])
    s.SetRansacParameters(*DEFAULTS)
    assert s.min_inliers == 10
    o = s.iterate(5, p["draws"])
    assert o["no_more"] and o["result"] == 0 and o["draws_consumed"] == 0 and s.iterations == 0


def test_random_int_formula():
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand(0)
    raws = [0, ref.RAND_MAX] + [libc.rand() for _ in range(3)]
    for size in (1, 4, 97, 100, 2048):
        assert ref.random_int(0, size) == 0
        assert ref.random_int(ref.RAND_MAX, size) == size - 1
        for raw in raws:
            assert 0 <= raw <= ref.RAND_MAX
            # raw / 2^31 and the product are exact enough in double for these sizes
            assert ref.random_int(raw, size) == (raw * size) >> 31
    # the minimal set: swap-with-back removal
    assert ref.sample4([0, 0, 0, 0], 10) == [0, 9, 8, 7]
    assert ref.sample4([ref.RAND_MAX] * 4, 10) == [9, 8, 7, 6]
    assert ref.sample4([0, ref.RAND_MAX, 0, ref.RAND_MAX], 5) == [0, 3, 4, 1]


def _recon(U, s, V):
    return (np.array(U) * np.array(s)) @ np.array(V).T


@pytest.mark.parametrize("shape,sym", [((3, 3), True), ((12, 12), True), ((3, 3), False),
                                       ((6, 3), False), ((6, 4), False), ((6, 5), False)])
def test_pinned_jacobi_is_an_svd(shape, sym):
    rng = np.random.default_rng(shape[0] * 10 + shape[1] + sym)
    for trial in range(4):
        A = rng.normal(size=shape)
        if sym:
            A = A + A.T
            if trial == 3:               # positive semi-definite of rank n - 4 or n - 1, as MtM is
                B = rng.normal(size=(shape[0], max(1, shape[0] - 4)))
                A = B @ B.T
        U, s, V = ref.svd_jacobi(A.tolist())
        want = np.linalg.svd(A, compute_uv=False)
        scale = want[0]
        assert np.all(np.diff(s) <= 0)
        assert np.abs(np.array(s) - want).max() <= 1e-12 * scale
        assert np.abs(_recon(U, s, V) - A).max() <= 1e-12 * scale
        Vn = np.array(V)
        assert np.abs(Vn.T @ Vn - np.eye(shape[1])).max() <= 1e-12
        if sym:
            ev = np.sort(np.abs(np.linalg.eigvalsh(A)))[::-1]
            assert np.abs(np.array(s) - ev).max() <= 1e-12 * scale


def test_svd_solve_is_least_squares():
    rng = np.random.default_rng(5)
    for n in (3, 4, 5):
        A, b = rng.normal(size=(6, n)), rng.normal(size=6)
        x = ref.svd_solve(A.tolist(), b.tolist())
        assert np.abs(np.array(x) - np.linalg.lstsq(A, b, rcond=None)[0]).max() <= 1e-12
    # a rank-deficient system takes the minimum-norm solution
    A = rng.normal(size=(6, 4))
    A[:, 3] = A[:, 0]
    b = rng.normal(size=6)
    x = ref.svd_solve(A.tolist(), b.tolist())
    assert np.abs(np.array(x) - np.linalg.pinv(A) @ b).max() <= 1e-10


@pytest.mark.parametrize("N", [4, 15, 200])
def test_compute_pose_noise_free(N):
    """float32 inputs of a noise-free problem: the pose is the ground truth up
    to the inputs' rounding (2^-24 relative on pixels of <= 640 and metres of <=
    6, amplified by the 4-point geometry: 1e-3 is loose for N = 4, the others
    are far below)"""
    p = make_problem(N, noise=0.0, seed=50 + N)
    cam = tuple(float(np.float32(c)) for c in p["cam"])
    R, t = ref.compute_pose(cam, p["p3d"].astype(np.float64), p["p2d"].astype(np.float64))
    got = np.concatenate([np.array(R), np.array(t)])
    want = np.concatenate([p["Tcw"][:3, :3].ravel(), p["Tcw"][:3, 3]])
    assert np.abs(got - want).max() < (1e-3 if N == 4 else 1e-5)


def test_ten_inliers_of_twenty_runs_to_exhaustion():
    p = ten_of_twenty()
    r = ref_run(p)
    s, (off, o, st) = r["solver"], r["calls"][0]
    assert (s.min_inliers, s.max_its) == (10, 35)
    assert len(r["calls"]) == 1
    assert o["result"] == 2 and o["no_more"] and o["n_inliers"] == 10
    assert o["draws_consumed"] == 4 * 35 and st["iterations"] == 35
    assert np.array_equal(o["inliers"], ~p["outlier"])
    assert np.array_equal(o["Tcw"], st["best_Tcw"])      # mBestTcw, a 4-point pose


def test_all_outliers_exhaust_and_a_later_call_runs_exactly_n():
    p = all_outliers()
    s = ref.PnPsolver(p["cam"], p["p2d"], p["sigma2"], p["p3d"])
    s.SetRansacParameters(*DEFAULTS)
    o = s.iterate(5, p["draws"])
    assert o["draws_consumed"] == 4 * s.max_its and s.max_its == 35
    assert o["result"] == 0 and o["no_more"] and o["n_inliers"] == 0
    o2 = s.iterate(5, p["draws"][o["draws_consumed"]:])
    assert o2["draws_consumed"] == 20 and s.iterations == 40
    assert o2["result"] == 0 and o2["no_more"]


def test_every_problem_is_admissible():
    """no error2 within a relative 1e-6 of its threshold and no fragile count
    decision (Margins) in any problem of the GPU comparison: none is dropped"""
    for p in list(problems().values()) + [big_problem()]:
        m = ref_run(p)["solver"].margins
        assert m.min_rel > 1e-6, (p["name"], m.min_rel)
        assert not m.count_fragile, p["name"]

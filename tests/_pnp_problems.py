"""Seeded synthetic PnP problems for the PnPsolver tests: TUM1 intrinsics,
points 0.5-5 m in front of a random pose, inlier noise <= 0.5 px, outliers
displaced >= 30 px, sigma2 from the 8-level 1.2 pyramid. Every problem is a
dict(cam, p2d, sigma2, p3d, Tcw (ground truth), draws, name); draws are raw
rand() values in [0, RAND_MAX]."""
import numpy as np

RAND_MAX = 2147483647
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], np.float32)
DEFAULTS = (0.99, 10, 300, 4, 0.5, 5.991)     # Tracking::Relocalization's parameters
N_DRAWS = 4 * 320


def _rot(rng):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(-0.6, 0.6)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def make_problem(N, outlier_share=0.0, noise=0.5, seed=0, n_outliers=None, name=None):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = TUM1
    R, t = _rot(rng), rng.uniform(-1.0, 1.0, 3)
    u = rng.uniform(20, 620, N)
    v = rng.uniform(20, 460, N)
    z = rng.uniform(0.5, 5.0, N)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    Xw = (Xc - t) @ R                       # R^T (Xc - t)
    ang = rng.uniform(0, 2 * np.pi, N)
    rad = rng.uniform(0, noise, N)
    p2d = np.stack([u + rad * np.cos(ang), v + rad * np.sin(ang)], axis=1)
    n_out = int(round(outlier_share * N)) if n_outliers is None else n_outliers
    out = rng.permutation(N)[:n_out]
    oa = rng.uniform(0, 2 * np.pi, n_out)
    orad = rng.uniform(30, 100, n_out)
    p2d[out] += np.stack([orad * np.cos(oa), orad * np.sin(oa)], axis=1)
    is_out = np.zeros(N, bool)
    is_out[out] = True
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(cam=TUM1, p2d=p2d.astype(np.float32), p3d=Xw.astype(np.float32),
                sigma2=SIGMA2[rng.integers(0, 8, N)], Tcw=T, outlier=is_out,
                draws=rng.integers(0, RAND_MAX + 1, N_DRAWS, dtype=np.int64).astype(np.int32),
                name=name or f"N{N}_o{n_out}_s{seed}")


def identical_points(N=20, seed=5):
    """every world point the same: no pose exists, every loop must end"""
    p = make_problem(N, seed=seed, name=f"identical_N{N}")
    p["p3d"] = np.tile(p["p3d"][:1], (N, 1))
    return p


def all_outliers(N=40, seed=7):
    """image points unrelated to the world points"""
    p = make_problem(N, seed=seed, name=f"all_outliers_N{N}")
    rng = np.random.default_rng(seed + 1000)
    p["p2d"] = np.stack([rng.uniform(20, 620, N), rng.uniform(20, 460, N)],
                        axis=1).astype(np.float32)
    p["sigma2"] = np.full(N, SIGMA2[0], np.float32)
    return p


def ten_of_twenty(seed=12):
    """N = 20 with exactly 10 noise-free inliers: min_inliers = 10, so Refine()'s
    strict > can never pass"""
    return make_problem(20, noise=0.0, seed=seed, n_outliers=10, name="ten_of_twenty")


def problems():
    """the driven problems of the GPU comparison (name -> problem)"""
    ps = [make_problem(8, seed=1), make_problem(10, noise=0.0, seed=2),
          make_problem(15, noise=0.0, seed=3)]
    for N, s in ((63, 20), (64, 21), (65, 22), (200, 23)):
        ps.append(make_problem(N, 0.3, seed=s))
        ps.append(make_problem(N, 0.5, seed=s + 10))
    ps += [ten_of_twenty(), all_outliers(), identical_points()]
    return {p["name"]: p for p in ps}


def big_problem():
    return make_problem(2048, seed=40, name="N2048_all_inliers")


_RUNS = {}


def ref_run(p, n_iterations=5, params=DEFAULTS, max_calls=80):
    """The restatement driven like Tracking::Relocalization drives the solver:
    SetRansacParameters(params), then iterate(n_iterations) until a pose or
    bNoMore. Call c uses p["draws"] from the draws the earlier calls consumed
    on. Returns dict(solver, calls=[(draw offset, output, state after)]);
    computed once per problem and shared by the tests."""
    key = (p["name"], n_iterations, params)
    if key in _RUNS:
        return _RUNS[key]
    import _pnp_ref as ref
    s = ref.PnPsolver(p["cam"], p["p2d"], p["sigma2"], p["p3d"])
    s.SetRansacParameters(*params)
    calls, off = [], 0
    for _ in range(max_calls):
        o = s.iterate(n_iterations, p["draws"][off:])
        calls.append((off, o, s.state()))
        off += o["draws_consumed"]
        if o["result"] or o["no_more"]:
            break
    _RUNS[key] = dict(solver=s, calls=calls)
    return _RUNS[key]
